// Single-head scaled-dot-product attention at head dim 512, forward only: the mid-block attention of the AutoencoderKL
// (one head as wide as the feature map has channels, T = (H/8) (W/8) tokens; uwudiff_amd/vae.py).  The other attention kernels
// cannot be instantiated here: attn_fwd_mfma stages whole K / V^T tiles of 64 keys twice (256 KB at d = 512) and attn_fwd_simple
// keeps d / 2 values per lane.
//
//   bf16: attn512_fwd_mfma -- flash-style, online softmax, no T x T tensor anywhere.  One workgroup of four waves owns 64
//         queries (16 per wave) and walks the keys 32 at a time.  Everything is computed TRANSPOSED so the probabilities
//         never leave their registers: S^T = K Q^T puts (query = lane % 16, keys 4 (lane / 16) .. + 3) into each lane,
//         which is exactly the B-operand layout of O^T += V^T P^T on v_mfma_f32_16x16x16_bf16, and the softmax statistics of
//         a query live in the lanes that hold its output column.  Per wave: Q as 32 B-fragments (64 VGPRs), O^T as 32
//         accumulators (128 VGPRs).  LDS: K [32][512 + 8] row-major and V^T [512][32 + 4] (transposed while it is
//         written), 70 KB, single stage; the next tile's global loads are issued before the current tile's MFMAs and held
//         in 64 VGPRs.  Keys past T are zero rows with -inf scores, queries past T are computed and not stored.
//   fp32: attn512_fwd_valu -- the exact-fp32 parity path.  A row is spread over 16 lanes (32 head dims each, interleaved
//         in 4-element chunks so a K / V row is read as contiguous 256 B per 16 lanes); partial dot products meet in a DPP
//         row sum.  16 rows per workgroup, 8 keys per step staged in LDS as fp32.
#include "common.h"

namespace {

struct Attn512Args {
  const void *q, *k, *v;
  void* o;
  int B, T, ldq, ldk, ldv, ldo;
  float scale;
};

constexpr int DH = 512;
constexpr int M_QW = 16, M_NW = 4, M_QB = M_QW * M_NW;  // queries per wave / waves / queries per workgroup
constexpr int M_KT = 32;                                // keys per step
constexpr int M_KLD = DH + 8;                           // K row stride in LDS (elements): 1040 B, 16-byte aligned rows
constexpr int M_VLD = M_KT + 4;                         // V^T row stride (elements): 72 B, 8-byte aligned rows
constexpr int M_LDS = (M_KT * M_KLD + DH * M_VLD) * 2;  // 70144 B

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // (a native vector: HIP's uint4 struct turns `c ? *p : zero` into a select of addresses)

__device__ __forceinline__ s16x4 pack_bf16x4(f32x4 v) {
  bf16x4 o = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
  return __builtin_bit_cast(s16x4, o);
}

__global__ void __launch_bounds__(256) attn512_fwd_mfma(const Attn512Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* Ks = reinterpret_cast<bf16_t*>(smem);  // [M_KT][M_KLD]
  bf16_t* Vt = Ks + M_KT * M_KLD;                // [DH][M_VLD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int b = blockIdx.y;
  const bf16_t* Q = static_cast<const bf16_t*>(a.q) + (int64_t)b * a.T * a.ldq;
  const bf16_t* K = static_cast<const bf16_t*>(a.k) + (int64_t)b * a.T * a.ldk;
  const bf16_t* V = static_cast<const bf16_t*>(a.v) + (int64_t)b * a.T * a.ldv;
  const int tq = blockIdx.x * M_QB + wave * M_QW + n;
  const bool qok = tq < a.T;

  // Q^T fragments (B operand): query n, head dims 16 ks + 4 g .. + 3
  s16x4 qf[DH / 16];
#pragma unroll
  for (int ks = 0; ks < DH / 16; ++ks)
    qf[ks] = qok ? *reinterpret_cast<const s16x4*>(Q + (int64_t)tq * a.ldq + 16 * ks + 4 * g) : s16x4{0, 0, 0, 0};

  f32x4 o[DH / 16];
#pragma unroll
  for (int dt = 0; dt < DH / 16; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, lsum = 0.f;
  const float sc = a.scale * 1.4426950408889634f;

  // staging: K tile = 32 rows x 64 chunks of 16 B, chunk c = tid + 256 i (a wave reads one row);
  //          V tile = 16 key pairs x 64 chunks, lane -> (pair = lane % 16, chunk = lane / 16 + 4 wave + 16 i): the 64 lanes of a
  //          transposed 4-byte LDS write hit 64 different banks
  u32x4 kr[8], vr[8];
  const u32x4 z4 = {0u, 0u, 0u, 0u};
#define ATTN512_GLOAD(t_)                                                                                                  \
  {                                                                                                                        \
    const int k0 = (t_) * M_KT;                                                                                            \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                                        \
      const int c = tid + 256 * i, row = c >> 6, col8 = c & 63;                                                            \
      kr[i] = (k0 + row < a.T) ? *reinterpret_cast<const u32x4*>(K + (int64_t)(k0 + row) * a.ldk + 8 * col8) : z4;         \
    }                                                                                                                      \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                                        \
      const int key = k0 + 2 * (lane & 15) + (i & 1), col8 = (lane >> 4) + 4 * wave + 16 * (i >> 1);                       \
      vr[i] = (key < a.T) ? *reinterpret_cast<const u32x4*>(V + (int64_t)key * a.ldv + 8 * col8) : z4;                     \
    }                                                                                                                      \
  }
  // word e of a V chunk: head dims 8 col8 + 2 e, + 1 of key 2 pair (lo) and key 2 pair + 1 (hi) -> V^T[dim][2 pair, 2 pair + 1]
#define ATTN512_VT(lo_, hi_, e_)                                                                            \
  *reinterpret_cast<unsigned*>(vdst + (2 * (e_)) * M_VLD) = ((lo_) & 0xFFFFu) | ((hi_) << 16);              \
  *reinterpret_cast<unsigned*>(vdst + (2 * (e_) + 1) * M_VLD) = ((lo_) >> 16) | ((hi_) & 0xFFFF0000u);
#define ATTN512_LSTORE()                                                                                    \
  {                                                                                                         \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                         \
      const int c = tid + 256 * i, row = c >> 6, col8 = c & 63;                                             \
      *reinterpret_cast<u32x4*>(Ks + row * M_KLD + 8 * col8) = kr[i];                                       \
    }                                                                                                       \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                         \
      bf16_t* vdst = Vt + 8 * ((lane >> 4) + 4 * wave + 16 * i) * M_VLD + 2 * (lane & 15);                  \
      const u32x4 lo = vr[2 * i], hi = vr[2 * i + 1];                                                       \
      ATTN512_VT(lo.x, hi.x, 0) ATTN512_VT(lo.y, hi.y, 1) ATTN512_VT(lo.z, hi.z, 2) ATTN512_VT(lo.w, hi.w, 3) \
    }                                                                                                       \
  }

  const int nt = (a.T + M_KT - 1) / M_KT;
  ATTN512_GLOAD(0)
  ATTN512_LSTORE()
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    ATTN512_GLOAD(t + 1)  // (past the last tile: every key >= T, no load is issued)
    // S^T[key 16 kt + 4 g + i][query n]
    f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < DH / 16; ++ks)
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const s16x4 kf = *reinterpret_cast<const s16x4*>(Ks + (16 * kt + n) * M_KLD + 16 * ks + 4 * g);
        s[kt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(kf, qf[ks], s[kt], 0, 0, 0);
      }
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = t * M_KT + 16 * kt + 4 * g + i;
        s[kt][i] = key < a.T ? s[kt][i] * sc : -INFINITY;
        mx = fmaxf(mx, s[kt][i]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);  // finite: every tile holds at least one key
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    float ps = 0.f;
    s16x4 pf[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[kt][i] = __builtin_amdgcn_exp2f(s[kt][i] - mn);
        ps += s[kt][i];
      }
      pf[kt] = pack_bf16x4(s[kt]);
    }
    lsum = lsum * alpha + ps;
    // O^T[head dim 16 dt + 4 g + i][query n] = alpha O^T + sum_key V^T[dim][key] P^T[key][query]
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) {
      o[dt] = o[dt] * alpha;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const s16x4 vf = *reinterpret_cast<const s16x4*>(Vt + (16 * dt + n) * M_VLD + 16 * kt + 4 * g);
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(vf, pf[kt], o[dt], 0, 0, 0);
      }
    }
    __syncthreads();  // every wave has read this tile
    ATTN512_LSTORE()
    __syncthreads();
  }
  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  if (qok) {
    const float inv = 1.f / lsum;
    bf16_t* O = static_cast<bf16_t*>(a.o) + ((int64_t)b * a.T + tq) * a.ldo + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) store4(O + 16 * dt, o[dt] * inv);
  }
}

constexpr int F_LANES = 16, F_ROWS = 16, F_KT = 8, F_PER = DH / F_LANES;  // 32 head dims per lane

__global__ void __launch_bounds__(256) attn512_fwd_valu(const Attn512Args a) {
  __shared__ __attribute__((aligned(16))) float Ks[F_KT * DH];
  __shared__ __attribute__((aligned(16))) float Vs[F_KT * DH];
  const int tid = threadIdx.x, j = tid & 15, r = tid >> 4;
  const int b = blockIdx.y;
  const int t = blockIdx.x * F_ROWS + r;
  const bool valid = t < a.T;
  const float* q = static_cast<const float*>(a.q) + (int64_t)b * a.T * a.ldq;
  const float* k = static_cast<const float*>(a.k) + (int64_t)b * a.T * a.ldk;
  const float* v = static_cast<const float*>(a.v) + (int64_t)b * a.T * a.ldv;
  float qr[F_PER], oa[F_PER];
#pragma unroll
  for (int i = 0; i < F_PER / 4; ++i) {  // this lane's chunk i: head dims 4 (j + 16 i) .. + 3
    const f32x4 qv = valid ? load4(q + (int64_t)t * a.ldq + 4 * (j + 16 * i)) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qr[4 * i + e] = qv[e] * a.scale;
      oa[4 * i + e] = 0.f;
    }
  }
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < a.T; k0 += F_KT) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < F_KT * DH / 4 / 256; ++i) {
      const int c = tid + 256 * i, row = c >> 7, col = (c & 127) * 4;
      f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = kv;
      if (k0 + row < a.T) {
        kv = load4(k + (int64_t)(k0 + row) * a.ldk + col);
        vv = load4(v + (int64_t)(k0 + row) * a.ldv + col);
      }
      store4(Ks + row * DH + col, kv);
      store4(Vs + row * DH + col, vv);
    }
    __syncthreads();
    float s[F_KT];
    float tmax = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < F_KT; ++jj) {
      float p = 0.f;
#pragma unroll
      for (int i = 0; i < F_PER / 4; ++i) {
        const f32x4 kv = load4(Ks + jj * DH + 4 * (j + 16 * i));
        p += qr[4 * i] * kv[0] + qr[4 * i + 1] * kv[1] + qr[4 * i + 2] * kv[2] + qr[4 * i + 3] * kv[3];
      }
      p = row16_sum(p);
      s[jj] = (k0 + jj < a.T) ? p : -INFINITY;
      tmax = fmaxf(tmax, s[jj]);
    }
    const float mn = fmaxf(m, tmax);
    const float alpha = __expf(m - mn);  // m = -inf on the first tile -> 0
    l *= alpha;
#pragma unroll
    for (int i = 0; i < F_PER; ++i) oa[i] *= alpha;
#pragma unroll
    for (int jj = 0; jj < F_KT; ++jj) {
      const float p = __expf(s[jj] - mn);
      l += p;
#pragma unroll
      for (int i = 0; i < F_PER / 4; ++i) {
        const f32x4 vv = load4(Vs + jj * DH + 4 * (j + 16 * i));
#pragma unroll
        for (int e = 0; e < 4; ++e) oa[4 * i + e] += p * vv[e];
      }
    }
    m = mn;
  }
  if (valid) {
    const float inv = 1.f / l;
    float* o = static_cast<float*>(a.o) + ((int64_t)b * a.T + t) * a.ldo;
#pragma unroll
    for (int i = 0; i < F_PER / 4; ++i)
      store4(o + 4 * (j + 16 * i), f32x4{oa[4 * i] * inv, oa[4 * i + 1] * inv, oa[4 * i + 2] * inv, oa[4 * i + 3] * inv});
  }
}

}  // namespace

extern "C" int uwu_attention_d512_fwd(const void* q, const void* k, const void* v, void* o, int B, int T, int ldq, int ldk,
                                      int ldv, int ldo, float scale, int dtype, void* stream) {
  UWU_CHECK_ARG(q && k && v && o, "attention_d512_fwd: null pointer");
  UWU_CHECK_ARG(B > 0 && B <= 65535 && T > 0, "attention_d512_fwd: bad shape B=%d T=%d", B, T);
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "attention_d512_fwd: bad dtype %d", dtype);
  UWU_CHECK_ARG(scale > 0.f, "attention_d512_fwd: scale must be positive");
  const int epc = dtype == UWU_BF16 ? 8 : 4;  // 16-byte rows
  UWU_CHECK_ARG(ldq >= DH && ldk >= DH && ldv >= DH && ldo >= DH && ldq % epc == 0 && ldk % epc == 0 && ldv % epc == 0 &&
                    ldo % epc == 0,
                "attention_d512_fwd: row strides must be >= 512 and multiples of %d", epc);
  UWU_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) == 0, "attention_d512_fwd: misaligned tensor");
  UWU_CHECK_ARG((int64_t)B * T * (int64_t)(ldq > ldk ? ldq : ldk) < ((int64_t)1 << 40), "attention_d512_fwd: tensor too large");
  Attn512Args a{q, k, v, o, B, T, ldq, ldk, ldv, ldo, scale};
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  if (dtype == UWU_BF16) {
    static unsigned char done[UWU_MAX_DEV];
    if (!uwu_func_lds(reinterpret_cast<const void*>(attn512_fwd_mfma), M_LDS, done)) {
      uwu_set_error("attention_d512_fwd: the device cannot give a workgroup %d bytes of LDS", M_LDS);
      return UWU_ELAUNCH;
    }
    hipLaunchKernelGGL(attn512_fwd_mfma, dim3(cdiv(T, M_QB), B), dim3(256), M_LDS, st, a);
  } else {
    hipLaunchKernelGGL(attn512_fwd_valu, dim3(cdiv(T, F_ROWS), B), dim3(256), 0, st, a);
  }
  UWU_LAUNCH_CHECK("attention_d512_fwd");
  // algorithmic work: QK^T + PV = 4 T^2 d; q, k, v, o once
  prof.done(UWU_PROF_ATTN_FWD, dtype == UWU_BF16 ? 0 : 1, 4.0 * B * (double)T * T * DH, (double)(dtype == UWU_BF16 ? 2 : 4) * B * DH * 4.0 * T);
  return UWU_OK;
}
