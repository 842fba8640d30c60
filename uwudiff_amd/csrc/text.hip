// The CLIP text transformer's own kernels (uwudiff_amd/text_model.py): causal attention over at most
// 128 tokens at head width 64, token + position embedding, bias + quick_gelu / erf-GELU, pooling at the eos token.  Forward
// only: the text encoders are frozen.  Everything else of the model (packed q/k/v, out_proj, fc1, fc2 GEMMs, the affine
// pre-LayerNorm with fused residual) runs on uwu_gemm and uwu_add_ln_modulate_fwd.
//
//   uwu_attention_causal_fwd
//     bf16: attn_causal_mfma -- one workgroup of four waves per (batch, head).  K [Tp][64 + 8] and V^T [64][128 + 8] of the head
//           are staged once in LDS (rows of keys the key mask hides, and rows past T, are staged as zeros: T is padded to the
//           MFMA tile here, never in memory).  Q is not staged: a query row is used by exactly one wave, once, so its two
//           B-fragments go from global memory straight to registers.  A wave owns query tiles w and 7 - w (16 queries each;
//           under the causal mask tile qt meets qt + 1 key tiles, so every wave gets 9).  As in attention_d512.hip everything
//           is computed TRANSPOSED: S^T = K Q^T on v_mfma_f32_16x16x32_bf16 leaves (query = lane % 16, keys 16 kt + 4 (lane /
//           16) .. + 3) in each lane, which is the B-operand layout of O^T += V^T P^T once two key tiles share one K = 32
//           step (k slot 8 g + j <-> key 16 (2 kp + j / 4) + 4 g + j % 4; V^T is read with the same permutation, two
//           ds_read_b64).  Key tiles above the diagonal are skipped in both products.  A score row is at most 128 wide: 32
//           registers per lane, plain max / exp / sum, the two cross-lane steps of each through ds_bpermute.  The DIAGONAL
//           tile's share of P V runs on the VALU with a select per (query, key): a matrix product would multiply a hidden
//           key's V row by a probability of exactly 0, which is NaN for a NaN, and pass it to queries that must not see it.
//           LDS banks: K rows are 144 B apart, so the 16 rows of a ds_read_b128 group start on 16 different 16-byte slots;
//           V^T rows are 272 B apart (4 r + 2 g dwords: no two lanes of a ds_read_b64 half on one bank); the transposed V
//           writes put consecutive lanes on consecutive keys.
//     fp32: attn_causal_valu -- the exact-fp32 parity path in the manner of attention_simple.hip (two lanes per query row, K / V
//           tiles of 32 keys staged as fp32), with the causal bound and the key mask applied as selects.
#include <math.h>

#include "common.h"

namespace {

struct CausalArgs {
  const void *q, *k, *v;
  const int64_t* mask;
  void* o;
  int B, T, H, ldq, ldk, ldv, ldo;
  float scale;
};

constexpr int CD = 64;          // head width
constexpr int CT_MAX = 128;     // longest sequence
constexpr int C_KLD = CD + 8;   // K row stride in LDS (elements): 144 B
constexpr int C_VLD = CT_MAX + 8;  // V^T row stride (elements): 272 B

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) attn_causal_mfma(const CausalArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[CT_MAX * C_KLD];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[CD * C_VLD];
  __shared__ __attribute__((aligned(16))) int kvis[CT_MAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / a.H, h = blockIdx.x - b * a.H;
  const int T = a.T, Tp16 = (T + 15) & ~15, Tp32 = (T + 31) & ~31;
  const bf16_t* Q = static_cast<const bf16_t*>(a.q) + (int64_t)b * T * a.ldq + h * CD;
  const bf16_t* K = static_cast<const bf16_t*>(a.k) + (int64_t)b * T * a.ldk + h * CD;
  const bf16_t* V = static_cast<const bf16_t*>(a.v) + (int64_t)b * T * a.ldv + h * CD;
  const int64_t* mk = a.mask ? a.mask + (int64_t)b * T : nullptr;
  const u32x4 z4 = {0u, 0u, 0u, 0u};

  if (tid < CT_MAX) kvis[tid] = (tid < T && (!mk || mk[tid] != 0)) ? 1 : 0;
  // K: Tp16 rows x 8 chunks of 16 B, a row per 8 consecutive lanes
  for (int c = tid; c < Tp16 * 8; c += 256) {
    const int row = c >> 3, col8 = c & 7;
    const bool ok = row < T && (!mk || mk[row] != 0);
    *reinterpret_cast<u32x4*>(Ks + row * C_KLD + 8 * col8) = ok ? *reinterpret_cast<const u32x4*>(K + (int64_t)row * a.ldk + 8 * col8) : z4;
  }
  // V^T: Tp32 keys x 8 chunks, consecutive lanes on consecutive keys (the 2-byte transposed writes of a wave are contiguous)
  for (int c = tid; c < Tp32 * 8; c += 256) {
    const int key = c % Tp32, col8 = c / Tp32;
    const bool ok = key < T && (!mk || mk[key] != 0);
    const u32x4 raw = ok ? *reinterpret_cast<const u32x4*>(V + (int64_t)key * a.ldv + 8 * col8) : z4;
    const bf16x8 v8 = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
    for (int j = 0; j < 8; ++j) Vt[(8 * col8 + j) * C_VLD + key] = v8[j];
  }
  __syncthreads();

  const float sc = a.scale * 1.4426950408889634f;
  const int nqt = Tp16 >> 4;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    const int qt = pass == 0 ? wave : 7 - wave;  // wave-uniform
    if (qt >= nqt) continue;
    const int tq = 16 * qt + n;
    const bool qok = tq < T;
    bf16x8 qf[2];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc)
      qf[kc] = __builtin_bit_cast(bf16x8, qok ? *reinterpret_cast<const u32x4*>(Q + (int64_t)tq * a.ldq + 32 * kc + 8 * g) : z4);

    // S^T[key 16 kt + 4 g + r][query n], key tiles 0 .. qt
    f32x4 s[8];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      s[kt] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (kt <= qt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + (16 * kt + n) * C_KLD + 32 * kc + 8 * g);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kc], acc, 0, 0, 0);
        }
        const i32x4 vis = *reinterpret_cast<const i32x4*>(kvis + 16 * kt + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = 16 * kt + 4 * g + r;
          s[kt][r] = (key <= tq && vis[r]) ? acc[r] * sc : -INFINITY;  // a select: a NaN score of a hidden key goes nowhere
          mx = fmaxf(mx, s[kt][r]);
        }
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (mx == -INFINITY) mx = 0.f;  // no visible key (the precondition key_mask[b, 0] != 0 broken): a zero row, not NaN
    float lsum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[kt][r] = __builtin_amdgcn_exp2f(s[kt][r] - mx);  // exp2(-inf) = 0 for hidden keys and skipped tiles
        lsum += s[kt][r];
      }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);

    // O^T[d 16 dt + 4 g + r][query n] += V^T P^T over the key tiles BELOW the diagonal one, two per K = 32 step
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 pd = {0.f, 0.f, 0.f, 0.f};  // the diagonal tile's probabilities: keys 16 qt + 4 g + r
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
      if (kt == qt) pd = s[kt];
    const bf16x4 zb = {(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
#pragma unroll
    for (int kp = 0; kp < 4; ++kp) {
      if (2 * kp < qt) {
        const bool second = 2 * kp + 1 < qt;  // else the step's upper half is the diagonal tile: P = 0 there and V is not read
        const bf16x4 plo = {(bf16_t)s[2 * kp][0], (bf16_t)s[2 * kp][1], (bf16_t)s[2 * kp][2], (bf16_t)s[2 * kp][3]};
        const bf16x4 phi = {(bf16_t)s[2 * kp + 1][0], (bf16_t)s[2 * kp + 1][1], (bf16_t)s[2 * kp + 1][2], (bf16_t)s[2 * kp + 1][3]};
        const bf16x4 ph = second ? phi : zb;
        const bf16x8 pf = {plo[0], plo[1], plo[2], plo[3], ph[0], ph[1], ph[2], ph[3]};
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16_t* vrow = Vt + (16 * dt + n) * C_VLD + 32 * kp + 4 * g;
          const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vrow);
          const bf16x4 hi = second ? *reinterpret_cast<const bf16x4*>(vrow + 16) : zb;
          const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
        }
      }
    }
    // The diagonal tile on the VALU.  Inside it a key is visible to some of the tile's queries and hidden from others, and a
    // matrix product shares the V operand among all 16: a hidden key's probability is exactly 0, but 0 * NaN is NaN.  Here a
    // hidden (query, key) pair is skipped by a select, so what a V row holds reaches only the queries that see it.  fp32
    // probabilities, V^T read four keys at a time (the 16 lanes of a query group read the same address: a broadcast).
#pragma unroll
    for (int jg = 0; jg < 4; ++jg) {
      float pj[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) pj[r] = __shfl(pd[r], n + 16 * jg, 64);  // P[query n][key 16 qt + 4 jg + r]
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r2 = 0; r2 < 4; ++r2) {
          const bf16x4 vv = *reinterpret_cast<const bf16x4*>(Vt + (16 * dt + 4 * g + r2) * C_VLD + 16 * qt + 4 * jg);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (16 * qt + 4 * jg + r <= tq) o[dt][r2] = fmaf(pj[r], (float)vv[r], o[dt][r2]);
        }
    }
    if (qok) {
      const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
      bf16_t* O = static_cast<bf16_t*>(a.o) + ((int64_t)b * T + tq) * a.ldo + h * CD + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x4 ov = {(bf16_t)(o[dt][0] * inv), (bf16_t)(o[dt][1] * inv), (bf16_t)(o[dt][2] * inv), (bf16_t)(o[dt][3] * inv)};
        *reinterpret_cast<bf16x4*>(O + 16 * dt) = ov;
      }
    }
  }
}

// exact fp32: 64 query rows per workgroup (two lanes per row, 32 head dims each), keys walked 32 at a time up to the block's
// last row; online softmax as attn_fwd_simple
constexpr int V_ROWS = 64, V_TILE = 32, V_HALF = CD / 2;

__global__ void __launch_bounds__(128) attn_causal_valu(const CausalArgs a) {
  __shared__ __attribute__((aligned(16))) float Ks[V_TILE * CD];
  __shared__ __attribute__((aligned(16))) float Vs[V_TILE * CD];
  __shared__ int kvis[V_TILE];
  const int T = a.T;
  const int b = blockIdx.y / a.H, h = blockIdx.y - b * a.H;
  const int r = threadIdx.x >> 1, half = threadIdx.x & 1;
  const int t = blockIdx.x * V_ROWS + r;
  const bool valid = t < T;
  const float* q = static_cast<const float*>(a.q) + (int64_t)b * T * a.ldq + h * CD;
  const float* k = static_cast<const float*>(a.k) + (int64_t)b * T * a.ldk + h * CD;
  const float* v = static_cast<const float*>(a.v) + (int64_t)b * T * a.ldv + h * CD;
  const int64_t* mk = a.mask ? a.mask + (int64_t)b * T : nullptr;
  float qr[V_HALF], oa[V_HALF];
#pragma unroll
  for (int i = 0; i < V_HALF; i += 4) {
    const f32x4 qv = valid ? load4(q + (int64_t)t * a.ldq + half * V_HALF + i) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qr[i + e] = qv[e] * a.scale;
      oa[i + e] = 0.f;
    }
  }
  float m = -INFINITY, l = 0.f;
  const int kend = min(T, (int)(blockIdx.x + 1) * V_ROWS);  // no row of this block sees a key at or past kend
  for (int k0 = 0; k0 < kend; k0 += V_TILE) {
    __syncthreads();
    for (int c = threadIdx.x; c < V_TILE * CD / 4; c += 128) {
      const int row = (c * 4) / CD, col = c * 4 - row * CD, key = k0 + row;
      const bool ok = key < T && (!mk || mk[key] != 0);
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      store4(Ks + row * CD + col, ok ? load4(k + (int64_t)key * a.ldk + col) : z);
      store4(Vs + row * CD + col, ok ? load4(v + (int64_t)key * a.ldv + col) : z);
    }
    if (threadIdx.x < V_TILE) {
      const int key = k0 + threadIdx.x;
      kvis[threadIdx.x] = (key < T && (!mk || mk[key] != 0)) ? 1 : 0;
    }
    __syncthreads();
    float s[V_TILE];
    float tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < V_TILE; ++j) {
      float p = 0.f;
      const float* kr = Ks + j * CD + half * V_HALF;
#pragma unroll
      for (int i = 0; i < V_HALF; i += 4) {
        const f32x4 kv = load4(kr + i);
        p += qr[i] * kv[0] + qr[i + 1] * kv[1] + qr[i + 2] * kv[2] + qr[i + 3] * kv[3];
      }
      p += __shfl_xor(p, 1, 64);
      s[j] = (k0 + j <= t && kvis[j]) ? p : -INFINITY;
      tmax = fmaxf(tmax, s[j]);
    }
    float mn = fmaxf(m, tmax);
    if (mn == -INFINITY) mn = 0.f;  // nothing visible yet (rows of a later 64-row block never get here with key 0 hidden)
    const float alpha = expf(m - mn);
    l *= alpha;
#pragma unroll
    for (int i = 0; i < V_HALF; ++i) oa[i] *= alpha;
#pragma unroll
    for (int j = 0; j < V_TILE; ++j) {
      if (s[j] == -INFINITY) continue;  // a hidden key's V row is never multiplied (it may hold anything)
      const float p = expf(s[j] - mn);
      l += p;
      const float* vr = Vs + j * CD + half * V_HALF;
#pragma unroll
      for (int i = 0; i < V_HALF; i += 4) {
        const f32x4 vv = load4(vr + i);
        oa[i] += p * vv[0];
        oa[i + 1] += p * vv[1];
        oa[i + 2] += p * vv[2];
        oa[i + 3] += p * vv[3];
      }
    }
    m = mn;
  }
  if (valid) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    float* o = static_cast<float*>(a.o) + ((int64_t)b * T + t) * a.ldo + h * CD + half * V_HALF;
#pragma unroll
    for (int i = 0; i < V_HALF; i += 4) store4(o + i, f32x4{oa[i] * inv, oa[i + 1] * inv, oa[i + 2] * inv, oa[i + 3] * inv});
  }
}

// ---- token + position embedding ---------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) text_embed_kernel(const int64_t* __restrict__ ids, const T* __restrict__ tok,
                                                         const T* __restrict__ pos, T* __restrict__ out, int64_t rows, int Tn,
                                                         int D, int vocab) {
  const int per = D / 8;
  const int64_t total = rows * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / per;
    const int c = (int)(i - row * per) * 8;
    int64_t id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const f32x8 a = load8(tok + id * D + c), p = load8(pos + (row % Tn) * D + c);
    store8(out + row * D + c, a + p);
  }
}

// ---- bias + activation ------------------------------------------------------------------------------------------------
// fp32 tensors: x + bias and the activation are evaluated in double (the exact-parity mode: 1 + erf cancels for v < -3, and the
// left tails amplify a rounding of v by |v f'(v) / f(v)| ~ 1.702 |v|)
template <int KIND>
__device__ __forceinline__ float act_one(float x, float b, float) {
  const double d = (double)x + (double)b;
  if (KIND == UWU_ACT_QUICK_GELU) return (float)(d / (1.0 + exp(-1.702 * d)));
  return (float)(0.5 * d * erfc(-d * 0.70710678118654752440));
}
// bf16 tensors: fp32 arithmetic; erfc, not 1 + erf, keeps the left tail's relative error far below a bf16 rounding
template <int KIND>
__device__ __forceinline__ float act_one(float x, float b, bf16_t) {
  const float v = x + b;
  if (KIND == UWU_ACT_QUICK_GELU) return v / (1.f + expf(-1.702f * v));
  return 0.5f * v * erfcf(-v * 0.70710678118654752440f);
}

template <typename T, int KIND>
__global__ void __launch_bounds__(256) bias_act_kernel(const T* __restrict__ x, const float* __restrict__ bias, T* __restrict__ y,
                                                       int64_t M, int N, int ld) {
  const int per = N / 8;
  const int64_t total = M * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / per;
    const int c = (int)(i - row * per) * 8;
    f32x8 v = load8(x + row * ld + c);
    const f32x8 bv = bias ? load8(bias + c) : f32x8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = act_one<KIND>(v[e], bv[e], T{});
    store8(y + row * ld + c, v);
  }
}

// ---- pooling at the eos token -----------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) text_pool_kernel(const int64_t* __restrict__ ids, const T* __restrict__ h, T* __restrict__ pooled,
                                                        int Tn, int D, int64_t eos_id) {
  __shared__ int pos_s;
  const int b = blockIdx.x;
  if (threadIdx.x < 64) {  // first position of the largest key: the id itself (eos_id == 2), or [id == eos_id]
    int64_t best = INT64_MIN;
    int bp = 0;
    for (int t = threadIdx.x; t < Tn; t += 64) {
      const int64_t id = ids[(int64_t)b * Tn + t];
      const int64_t key = eos_id == 2 ? id : (int64_t)(id == eos_id);
      if (key > best) {
        best = key;
        bp = t;
      }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int64_t ob = __shfl_xor(best, off, 64);
      const int op = __shfl_xor(bp, off, 64);
      if (ob > best || (ob == best && op < bp)) {
        best = ob;
        bp = op;
      }
    }
    if (threadIdx.x == 0) pos_s = bp;
  }
  __syncthreads();
  const T* src = h + ((int64_t)b * Tn + pos_s) * D;
  for (int c = threadIdx.x * 8; c < D; c += 256 * 8) store8(pooled + (int64_t)b * D + c, load8(src + c));
}

}  // namespace

extern "C" int uwu_attention_causal_fwd(const void* q, const void* k, const void* v, const int64_t* key_mask, void* o, int B, int T,
                                        int H, int d, int ldq, int ldk, int ldv, int ldo, float scale, int dtype, void* stream) {
  UWU_CHECK_ARG(q && k && v && o, "attention_causal_fwd: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "attention_causal_fwd: bad dtype %d", dtype);
  UWU_CHECK_ARG(d == CD, "attention_causal_fwd: head dim %d (built for 64)", d);
  UWU_CHECK_ARG(T >= 1 && T <= CT_MAX, "attention_causal_fwd: T = %d outside [1, 128]", T);
  UWU_CHECK_ARG(B > 0 && H > 0 && (int64_t)B * H <= 0x7FFFFFFF / 64, "attention_causal_fwd: bad B = %d, H = %d", B, H);
  const int hd = H * CD;
  UWU_CHECK_ARG(ldq >= hd && ldk >= hd && ldv >= hd && ldo >= hd, "attention_causal_fwd: row stride < H*d");
  const int al = dtype == UWU_BF16 ? 8 : 4;
  UWU_CHECK_ARG(ldq % al == 0 && ldk % al == 0 && ldv % al == 0 && ldo % al == 0,
                "attention_causal_fwd: row strides must be multiples of %d elements", al);
  UWU_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) == 0 && ((uintptr_t)key_mask & 7) == 0,
                "attention_causal_fwd: misaligned pointer (16-byte q / k / v / o, 8-byte key_mask)");
  UWU_CHECK_ARG(scale > 0.f && isfinite(scale), "attention_causal_fwd: scale must be positive");
  CausalArgs a{q, k, v, key_mask, o, B, T, H, ldq, ldk, ldv, ldo, scale};
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  if (dtype == UWU_BF16)
    hipLaunchKernelGGL(attn_causal_mfma, dim3(B * H), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(attn_causal_valu, dim3(cdiv(T, V_ROWS), B * H), dim3(128), 0, st, a);
  // algorithmic work of the causal half: 4 d T (T + 1) / 2 per head; q, k, v, o once
  prof.done(UWU_PROF_ATTN_FWD, dtype == UWU_BF16 ? 0 : 1, 2.0 * B * H * CD * T * (T + 1.0), 4.0 * B * H * CD * T * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("attention_causal_fwd");
  return UWU_OK;
}

extern "C" int uwu_text_embed(const int64_t* ids, const void* tok_table, const void* pos_table, void* out, int B, int T, int D,
                              int vocab, int dtype, void* stream) {
  UWU_CHECK_ARG(ids && tok_table && pos_table && out, "text_embed: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "text_embed: bad dtype %d", dtype);
  UWU_CHECK_ARG(B > 0 && T > 0 && vocab > 0 && D > 0 && D % 8 == 0, "text_embed: bad shape B = %d, T = %d, D = %d, vocab = %d", B, T, D, vocab);
  UWU_CHECK_ARG((((uintptr_t)tok_table | (uintptr_t)pos_table | (uintptr_t)out) & 15) == 0 && ((uintptr_t)ids & 7) == 0,
                "text_embed: misaligned pointer");
  const int64_t rows = (int64_t)B * T;
  const int grid = ew_grid(rows * (D / 8), 256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == UWU_BF16)
    hipLaunchKernelGGL(text_embed_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, ids, (const bf16_t*)tok_table, (const bf16_t*)pos_table,
                       (bf16_t*)out, rows, T, D, vocab);
  else
    hipLaunchKernelGGL(text_embed_kernel<float>, dim3(grid), dim3(256), 0, st, ids, (const float*)tok_table, (const float*)pos_table,
                       (float*)out, rows, T, D, vocab);
  UWU_LAUNCH_CHECK("text_embed");
  return UWU_OK;
}

extern "C" int uwu_bias_act_fwd(const void* x, const float* bias, void* y, int M, int N, int ld, int kind, int dtype, void* stream) {
  UWU_CHECK_ARG(x && y, "bias_act_fwd: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "bias_act_fwd: bad dtype %d", dtype);
  UWU_CHECK_ARG(kind == UWU_ACT_QUICK_GELU || kind == UWU_ACT_GELU_ERF, "bias_act_fwd: bad kind %d", kind);
  UWU_CHECK_ARG(M > 0 && N > 0 && N % 8 == 0 && ld >= N && ld % 8 == 0, "bias_act_fwd: bad shape M = %d, N = %d, ld = %d", M, N, ld);
  UWU_CHECK_ARG((((uintptr_t)x | (uintptr_t)y | (uintptr_t)bias) & 15) == 0, "bias_act_fwd: misaligned pointer");
  const int grid = ew_grid((int64_t)M * (N / 8), 256);
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
#define UWU_BA_LAUNCH(TYPE, KIND) \
  hipLaunchKernelGGL((bias_act_kernel<TYPE, KIND>), dim3(grid), dim3(256), 0, st, (const TYPE*)x, bias, (TYPE*)y, (int64_t)M, N, ld)
  if (dtype == UWU_BF16) {
    if (kind == UWU_ACT_QUICK_GELU) UWU_BA_LAUNCH(bf16_t, UWU_ACT_QUICK_GELU);
    else UWU_BA_LAUNCH(bf16_t, UWU_ACT_GELU_ERF);
  } else {
    if (kind == UWU_ACT_QUICK_GELU) UWU_BA_LAUNCH(float, UWU_ACT_QUICK_GELU);
    else UWU_BA_LAUNCH(float, UWU_ACT_GELU_ERF);
  }
#undef UWU_BA_LAUNCH
  prof.done(UWU_PROF_OTHER, dtype == UWU_BF16 ? 0 : 1, 0.0, 2.0 * M * N * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("bias_act_fwd");
  return UWU_OK;
}

extern "C" int uwu_text_pool(const int64_t* ids, const void* h, void* pooled, int B, int T, int D, int eos_id, int dtype, void* stream) {
  UWU_CHECK_ARG(ids && h && pooled, "text_pool: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "text_pool: bad dtype %d", dtype);
  UWU_CHECK_ARG(B > 0 && T > 0 && D > 0 && D % 8 == 0, "text_pool: bad shape B = %d, T = %d, D = %d", B, T, D);
  UWU_CHECK_ARG((((uintptr_t)h | (uintptr_t)pooled) & 15) == 0 && ((uintptr_t)ids & 7) == 0, "text_pool: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == UWU_BF16)
    hipLaunchKernelGGL(text_pool_kernel<bf16_t>, dim3(B), dim3(256), 0, st, ids, (const bf16_t*)h, (bf16_t*)pooled, T, D, (int64_t)eos_id);
  else
    hipLaunchKernelGGL(text_pool_kernel<float>, dim3(B), dim3(256), 0, st, ids, (const float*)h, (float*)pooled, T, D, (int64_t)eos_id);
  UWU_LAUNCH_CHECK("text_pool");
  return UWU_OK;
}
