// AdamW and Lion whose moments live as 8-bit codes with one fp32 scale (absmax) per block of 256 elements: the state layout of
// bitsandbytes' AdamW8bit / Lion8bit (block-wise dynamic quantisation, Dettmers et al. 2022): 1 B per moment and parameter and one
// fp32 scale per 256, 16 / 14 B/param.  The rule is written out at uwu_adamw8_step (include/uwu_hip.h): dequantise, adamw_elem /
// lion_elem (optimizer_shared.h: the very functions adamw_kernel and lion_kernel call) on the fp32 values, the block's new
// absmax, the nearest table entry of value / absmax.  Two things the package does are NOT reproduced: it applies the weight decay
// after the update (here first, as adamw_kernel does: O(lr^2 wd) per step apart), and after quantising the first moment it moves a
// code whose sign differs from the value's to the neighbouring entry (its sign-preservation fix-up); here the code is the
// nearest entry and nothing else.
//
// One 256-element block is one wave at 4 elements per lane: p and g move as 16-byte accesses, the codes as one dword per lane,
// the block maximum is a DPP wave reduction, so the loop has no barrier.  Blocks are counted from the buffer's start; a launch
// covers whole blocks (the last may be partial: those lanes take the element-wise path).  Both tables are staged in LDS once per
// workgroup; the search is a binary search over the staged table (8 dependent reads, a 9th for the upper neighbour) and assumes
// nothing about the table but that it increases (see Q8Table for the order it is staged in).  Per parameter: 10 B read + 6 B written for AdamW (+ 2 B shadow, + 4 B zeroed g).
#include "optimizer_shared.h"

// A staged table: T in index order (dequantisation, the upper neighbour) and E, the same entries in the level order of the binary
// search over T[1..255] (E[1] = T[128], E[2] = T[64], E[3] = T[192], ...; E[0] = T[0]).  Searched in index order, level k reads
// only entries whose index is an odd multiple of 2^(8-k): 8 distinct entries in ONE of the 32 LDS banks at level 4, 16 in two banks
// at level 5 -- most of a wave's lanes queue behind each other.  In level order a level's entries are consecutive dwords.
struct Q8Table {
  float T[256], E[256];
};

__device__ __forceinline__ void q8_stage(Q8Table& Q, const float* __restrict__ q) {  // 256 threads; the caller synchronises
  const int i = threadIdx.x;
  Q.T[i] = q[i];
  const int k = 32 - __builtin_clz(i | 1);  // the level of E[i], 1..8
  const int r = i - (1 << (k - 1));         // its place within the level
  Q.E[i] = q[i ? (2 * r + 1) << (8 - k) : 0];
}

__device__ __forceinline__ uint32_t q8_nearest(const Q8Table& Q, float x) {
  int i = 1;  // after 8 levels i - 256 = the number of entries T[1..255] that are <= x = the index of the last entry <= x
  float tlo = Q.E[0];
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const float t = Q.E[i];
    const bool c = t <= x;
    tlo = c ? t : tlo;
    i = 2 * i + (c ? 1 : 0);
  }
  const int lo = i - 256, hi = lo < 255 ? lo + 1 : 255;
  return (Q.T[hi] - x) < (x - tlo) ? hi : lo;  // a tie stays at the lower index
}

// the 4 elements of one lane: vector accesses when all 4 lie inside the buffer, element by element in the ragged last block
struct Q8Lane {
  int64_t e;
  int valid;
};

__device__ __forceinline__ void q8_load(const Q8Lane& L, const float* p, const float* g, f32x4& pv, f32x4& gv) {
  if (L.valid == 4) {
    pv = load4(p + L.e);
    gv = load4(g + L.e);
  } else {
    pv = f32x4{0.f, 0.f, 0.f, 0.f};
    gv = pv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < L.valid) {
        pv[j] = p[L.e + j];
        gv[j] = g[L.e + j];
      }
    }
  }
}

__device__ __forceinline__ uint32_t q8_load_codes(const Q8Lane& L, const uint8_t* c8) {
  if (L.valid == 4) return *reinterpret_cast<const uint32_t*>(c8 + L.e);
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < L.valid) c |= (uint32_t)c8[L.e + j] << (8 * j);
  return c;
}

__device__ __forceinline__ void q8_store_codes(const Q8Lane& L, uint8_t* c8, uint32_t c) {
  if (L.valid == 4) {
    *reinterpret_cast<uint32_t*>(c8 + L.e) = c;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < L.valid) c8[L.e + j] = (uint8_t)(c >> (8 * j));
  }
}

__device__ __forceinline__ void q8_store(const Q8Lane& L, float* p, float* g, bf16_t* pbf, f32x4 pv, int zero_grad) {
  if (L.valid == 4) {
    store4(p + L.e, pv);
    if (pbf) store4(pbf + L.e, pv);
    if (zero_grad) store4(g + L.e, f32x4{0.f, 0.f, 0.f, 0.f});
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < L.valid) {
        p[L.e + j] = pv[j];
        if (pbf) pbf[L.e + j] = (bf16_t)pv[j];
        if (zero_grad) g[L.e + j] = 0.f;
      }
    }
  }
}

__device__ __forceinline__ Q8Lane q8_lane(int64_t blk, int lane, int64_t n) {
  Q8Lane L;
  L.e = blk * 256 + 4 * lane;
  const int64_t left = n - L.e;
  L.valid = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
  return L;
}

// value / absmax quantised against the staged table, 4 codes packed in lane order; absmax == 0: the code nearest to 0
__device__ __forceinline__ uint32_t q8_quantise4(const Q8Table& Q, f32x4 x, float amax) {
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) c |= q8_nearest(Q, amax > 0.f ? x[j] / amax : 0.f) << (8 * j);
  return c;
}

__global__ void __launch_bounds__(256) adamw8_kernel(float* __restrict__ p, float* __restrict__ g, uint8_t* __restrict__ m8,
                                                     uint8_t* __restrict__ v8, float* __restrict__ am, float* __restrict__ av,
                                                     const float* __restrict__ qm, const float* __restrict__ qv,
                                                     bf16_t* __restrict__ pbf, int64_t n, int64_t blk0, int64_t blk1, float omb1,
                                                     float b2, float omb2, float eps, float decay, float step_size,
                                                     float inv_bc2_sqrt, float pre_scale, const float* __restrict__ clip,
                                                     int zero_grad) {
  __shared__ Q8Table Qm, Qv;
  q8_stage(Qm, qm);
  q8_stage(Qv, qv);
  __syncthreads();
  const float gscale = grad_scale(pre_scale, clip);
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t blk = blk0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); blk < blk1; blk += stride) {  // wave-uniform
    const Q8Lane L = q8_lane(blk, lane, n);
    f32x4 pv, gv, mv, vv;
    q8_load(L, p, g, pv, gv);
    const uint32_t mc = q8_load_codes(L, m8), vc = q8_load_codes(L, v8);
    const float am_old = am[blk], av_old = av[blk];
    float mmax = 0.f, vmax = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pp = pv[j], mm = j < L.valid ? Qm.T[(mc >> (8 * j)) & 255] * am_old : 0.f;
      float vn = j < L.valid ? Qv.T[(vc >> (8 * j)) & 255] * av_old : 0.f;
      adamw_elem(pp, gv[j], mm, vn, gscale, decay, omb1, b2, omb2, eps, step_size, inv_bc2_sqrt);  // the unrounded new moments
      pv[j] = pp;
      mv[j] = mm;
      vv[j] = vn;
      mmax = fmaxf(mmax, fabsf(mm));
      vmax = fmaxf(vmax, vn);
    }
    mmax = wave_max(mmax);
    vmax = wave_max(vmax);
    q8_store_codes(L, m8, q8_quantise4(Qm, mv, mmax));
    q8_store_codes(L, v8, q8_quantise4(Qv, vv, vmax));
    if (lane == 0) {
      am[blk] = mmax;
      av[blk] = vmax;
    }
    q8_store(L, p, g, pbf, pv, zero_grad);
  }
}

__global__ void __launch_bounds__(256) lion8_kernel(float* __restrict__ p, float* __restrict__ g, uint8_t* __restrict__ m8,
                                                    float* __restrict__ am, const float* __restrict__ qm,
                                                    bf16_t* __restrict__ pbf, int64_t n, int64_t blk0, int64_t blk1, float lr,
                                                    float b1, float omb1, float b2, float omb2, float decay, float pre_scale,
                                                    const float* __restrict__ clip, int zero_grad) {
  __shared__ Q8Table Qm;
  q8_stage(Qm, qm);
  __syncthreads();
  const float gscale = grad_scale(pre_scale, clip);
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t blk = blk0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); blk < blk1; blk += stride) {  // wave-uniform
    const Q8Lane L = q8_lane(blk, lane, n);
    f32x4 pv, gv, mv;
    q8_load(L, p, g, pv, gv);
    const uint32_t mc = q8_load_codes(L, m8);
    const float am_old = am[blk];
    float mmax = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pp = pv[j], mm = j < L.valid ? Qm.T[(mc >> (8 * j)) & 255] * am_old : 0.f;
      lion_elem(pp, gv[j] * gscale, mm, decay, lr, b1, omb1, b2, omb2);
      pv[j] = pp;
      mv[j] = mm;
      mmax = fmaxf(mmax, fabsf(mm));
    }
    mmax = wave_max(mmax);
    q8_store_codes(L, m8, q8_quantise4(Qm, mv, mmax));
    if (lane == 0) am[blk] = mmax;
    q8_store(L, p, g, pbf, pv, zero_grad);
  }
}

// the element range [e0, e1) of a buffer of n elements as whole 256-element blocks
static inline bool q8_range_ok(int64_t n, int64_t e0, int64_t e1) {
  return n > 0 && e0 >= 0 && e0 < e1 && e1 <= n && (e0 & 255) == 0 && ((e1 & 255) == 0 || e1 == n);
}

extern "C" int uwu_adamw8_step(float* p, float* g, void* state1, void* state2, float* absmax1, float* absmax2,
                               const float* qmap1, const float* qmap2, void* p_bf16, int64_t n, int64_t e0, int64_t e1,
                               double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                               float pre_scale, const float* clip, int zero_grad, void* stream) {
  UWU_CHECK_ARG(p && g && state1 && state2 && absmax1 && absmax2 && qmap1 && qmap2, "uwu_adamw8_step: null pointer");
  UWU_CHECK_ARG((((uintptr_t)p | (uintptr_t)g) & 15) == 0, "uwu_adamw8_step: p and g must be 16-byte aligned");
  UWU_CHECK_ARG((((uintptr_t)state1 | (uintptr_t)state2 | (uintptr_t)absmax1 | (uintptr_t)absmax2 | (uintptr_t)qmap1 |
                  (uintptr_t)qmap2) & 3) == 0,
                "uwu_adamw8_step: codes, absmax and tables must be 4-byte aligned");
  UWU_CHECK_ARG(p_bf16 == nullptr || ((uintptr_t)p_bf16 & 7) == 0, "uwu_adamw8_step: bf16 shadow must be 8-byte aligned");
  UWU_CHECK_ARG(q8_range_ok(n, e0, e1),
                "uwu_adamw8_step: bad range [%lld, %lld) of %lld: e0 must be a multiple of 256, e1 a multiple of 256 or n",
                (long long)e0, (long long)e1, (long long)n);
  UWU_CHECK_ARG(step >= 1, "uwu_adamw8_step: step counts from 1");
  // bias corrections, 1 - beta and 1 - lr*wd in double on the host, as python does
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  const int64_t blk0 = e0 >> 8, blk1 = (e1 + 255) >> 8;
  hipLaunchKernelGGL(adamw8_kernel, dim3(ew_grid(blk1 - blk0, 4)), dim3(256), 0, (hipStream_t)stream, p, g, (uint8_t*)state1,
                     (uint8_t*)state2, absmax1, absmax2, qmap1, qmap2, (bf16_t*)p_bf16, n, blk0, blk1, (float)(1.0 - beta1),
                     (float)beta2, (float)(1.0 - beta2), (float)eps, (float)(1.0 - lr * weight_decay), (float)(lr / bc1),
                     (float)(1.0 / sqrt(bc2)), pre_scale, clip, zero_grad);
  UWU_LAUNCH_CHECK("uwu_adamw8_step");
  return UWU_OK;
}

extern "C" int uwu_lion8_step(float* p, float* g, void* state1, float* absmax1, const float* qmap1, void* p_bf16, int64_t n,
                              int64_t e0, int64_t e1, double lr, double beta1, double beta2, double weight_decay,
                              float pre_scale, const float* clip, int zero_grad, void* stream) {
  UWU_CHECK_ARG(p && g && state1 && absmax1 && qmap1, "uwu_lion8_step: null pointer");
  UWU_CHECK_ARG((((uintptr_t)p | (uintptr_t)g) & 15) == 0, "uwu_lion8_step: p and g must be 16-byte aligned");
  UWU_CHECK_ARG((((uintptr_t)state1 | (uintptr_t)absmax1 | (uintptr_t)qmap1) & 3) == 0,
                "uwu_lion8_step: codes, absmax and table must be 4-byte aligned");
  UWU_CHECK_ARG(p_bf16 == nullptr || ((uintptr_t)p_bf16 & 7) == 0, "uwu_lion8_step: bf16 shadow must be 8-byte aligned");
  UWU_CHECK_ARG(q8_range_ok(n, e0, e1),
                "uwu_lion8_step: bad range [%lld, %lld) of %lld: e0 must be a multiple of 256, e1 a multiple of 256 or n",
                (long long)e0, (long long)e1, (long long)n);
  const int64_t blk0 = e0 >> 8, blk1 = (e1 + 255) >> 8;
  hipLaunchKernelGGL(lion8_kernel, dim3(ew_grid(blk1 - blk0, 4)), dim3(256), 0, (hipStream_t)stream, p, g, (uint8_t*)state1,
                     absmax1, qmap1, (bf16_t*)p_bf16, n, blk0, blk1, (float)lr, (float)beta1, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), (float)(1.0 - lr * weight_decay), pre_scale, clip, zero_grad);
  UWU_LAUNCH_CHECK("uwu_lion8_step");
  return UWU_OK;
}
