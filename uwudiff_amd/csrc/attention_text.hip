// Self-attention of the frozen encoders at head width 64 (uwudiff_amd/text_model.py, uwudiff_amd/vision_model.py; DESIGN.md
// sections 4.23, 4.25 and 4.29), forward only.  Three entry points, two bf16 MFMA kernels (one of them in two instantiations) and
// one exact-fp32 kernel between them.
//
//   uwu_attention_causal_fwd      o = softmax(scale Q K^T + causal mask + M) V, T <= 128 (the CLIP text transformer)
//   uwu_attention_relbias_fwd     o = softmax(scale Q K^T + rel_bias[h, j - i + T - 1] + M) V, T <= 512 (the T5 encoder)
//   uwu_attention_bidir_fwd       o = softmax(scale Q K^T + M) V, T <= 1024 (the CLIP image tower: T = 50, 197, 257, 577)
//
// M hides the keys key_mask marks as padding.  PRECONDITION: key 0 of every sequence is visible (causal), at least one
// key of every sequence is visible (relative bias, bidirectional).  A row that sees no key at all comes out as zeros, never NaN.  Where the
// causal precondition is broken the fp32 path carries its running maximum over wholly hidden tiles by the rule the relative-bias
// path always had (a hidden tile leaves it alone); before the two were one kernel it reset the maximum to 0 there, so such rows
// may differ from earlier builds in the last bits.  Every input that meets the precondition gives the same bits as before.
//
// What the bf16 kernels share (the helpers below): in both everything is computed TRANSPOSED.  S^T = K Q^T on
// v_mfma_f32_16x16x32_bf16 leaves (query = lane % 16, keys 16 kt + 4 (lane / 16) .. + 3) in each lane, which is the B-operand
// layout of O^T += V^T P^T once two key tiles share one K = 32 step (k slot 8 g + j <-> key 16 (2 kp + j / 4) + 4 g + j % 4; V^T
// is read with the same permutation, two ds_read_b64).  K rows and V^T rows are staged in LDS; rows of keys the key mask hides,
// and rows past T, are staged as zeros: T is padded to the MFMA tile here, never in memory.  Q is not staged: a query row is used
// by exactly one wave, so its two B-fragments go from global memory straight to registers.  A hidden key's score is replaced
// by -inf with a select, so a NaN under it goes nowhere.  LDS banks: K rows are 144 B apart, so the 16 rows of a ds_read_b128
// group start on 16 different 16-byte slots; the transposed V writes put consecutive lanes on consecutive keys.
// What they do not share, on purpose: the schedule and the softmax.
//
//     attn_causal_mfma -- one workgroup of four waves per (batch, head).  K [Tp][64 + 8] and V^T [64][128 + 8] of the head are
//           staged once.  A wave owns query tiles w and 7 - w (16 queries each; under the causal mask tile qt meets qt + 1 key
//           tiles, so every wave gets 9).  Key tiles above the diagonal are skipped in both products.  A score row is at most
//           128 wide: 32 registers per lane, plain max / exp / sum, the two cross-lane steps of each through ds_bpermute.  The
//           DIAGONAL tile's share of P V runs on the VALU with a select per (query, key): a matrix product would multiply a
//           hidden key's V row by a probability of exactly 0, which is NaN for a NaN, and pass it to queries that must not see
//           it.  V^T rows are 272 B apart (4 r + 2 g dwords: no two lanes of a ds_read_b64 half on one bank).
//     attn_relbias_mfma -- a workgroup of four waves per (64 queries, batch, head); a wave owns one tile of 16 queries.  Keys are
//           walked 64 at a time with an online softmax: the chunk's K [64][64 + 8] and V^T [64][64 + 8] are staged, the head's
//           bias row (2 T - 1 floats, times log2 e) is staged once with 64 zeros of margin on either side so that the padded
//           queries and keys index inside it.  Tiling over query blocks was chosen over staging all 512 keys once per (batch,
//           head) because K + V^T of 512 keys take 140 KB -- one workgroup of four waves per CU, every load latency exposed,
//           and 768 workgroups for 256 CUs at B H = 768 whatever T is -- while 23 KB let several workgroups share a CU and
//           T = 512 brings eight times as many of them; the K / V re-reads hit the L2.  Every query sees the same keys, so no
//           tile needs the VALU path the causal kernel has for its diagonal.
//     attn_relbias_mfma<false> -- the same kernel without the bias (uwu_attention_bidir_fwd): no bias row is staged and none is
//           added to the scores.  The bias row was the only thing in the kernel whose size depends on T, so this instantiation
//           takes any T the grid can hold; the entry point stops at BT_MAX = 1024.
//     attn_text_valu<CAUSAL> -- the exact-fp32 parity path of both in the manner of attention_simple.hip: two lanes per query
//           row, K / V tiles of 32 keys staged as fp32, online softmax; the causal bound and the key mask are selects, the bias
//           is read per (query, key) from global memory, or not at all (BIAS = false: the bidirectional entry point).
#include <math.h>

#include "common.h"

namespace {

struct AttnArgs {
  const void *q, *k, *v;
  const int64_t* mask;
  void* o;
  int B, T, H, ldq, ldk, ldv, ldo;
  float scale;
  const float* bias;  // [H, 2 T - 1]; nullptr for causal attention
};

constexpr int HD = 64;             // head width
constexpr int CT_MAX = 128;        // longest causal sequence
constexpr int C_KLD = HD + 8;      // causal: K row stride in LDS (elements): 144 B
constexpr int C_VLD = CT_MAX + 8;  // causal: V^T row stride (elements): 272 B
constexpr int RT_MAX = 512;        // longest relative-bias sequence (T5_T_MAX in text.hip is the same number)
constexpr int BT_MAX = 1024;       // longest bidirectional sequence without a bias (ViT-L/14 at 336 x 336 has 577 tokens)
constexpr int R_QB = 64;           // relative bias: queries per workgroup
constexpr int R_KC = 64;           // keys per chunk
constexpr int R_LD = HD + 8;       // row stride of both LDS tiles (elements): 144 B
constexpr int R_BM = 64;           // margin of the staged bias row on either side
constexpr int R_BN = 2 * RT_MAX - 1 + 2 * R_BM + 1;  // 1152 floats

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- what the two MFMA kernels share ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool key_visible(const int64_t* mk, int key, int T) { return key < T && (!mk || mk[key] != 0); }

// 16 B of key `key` (head dims 8 col8 .. + 7) into LDS row `row`; zeros unless `ok` (the key is visible)
template <int LD>
__device__ __forceinline__ void stage_k(bf16_t* Ks, int row, int col8, const bf16_t* K, int ldk, int key, bool ok) {
  const u32x4 z4 = {0u, 0u, 0u, 0u};
  *reinterpret_cast<u32x4*>(Ks + row * LD + 8 * col8) = ok ? *reinterpret_cast<const u32x4*>(K + (int64_t)key * ldk + 8 * col8) : z4;
}

// the same 16 B of V, transposed: eight 2-byte writes into column `row` of V^T
template <int LD>
__device__ __forceinline__ void stage_vt(bf16_t* Vt, int row, int col8, const bf16_t* V, int ldv, int key, bool ok) {
  const u32x4 z4 = {0u, 0u, 0u, 0u};
  const u32x4 raw = ok ? *reinterpret_cast<const u32x4*>(V + (int64_t)key * ldv + 8 * col8) : z4;
  const bf16x8 v8 = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
  for (int j = 0; j < 8; ++j) Vt[(8 * col8 + j) * LD + row] = v8[j];
}

// the two B-fragments of query tq (lane group g holds head dims 32 kc + 8 g .. + 7); zeros for a query past T
__device__ __forceinline__ void load_q(bf16x8 (&qf)[2], const bf16_t* Q, int tq, int ldq, int g, bool qok) {
  const u32x4 z4 = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int kc = 0; kc < 2; ++kc)
    qf[kc] = __builtin_bit_cast(bf16x8, qok ? *reinterpret_cast<const u32x4*>(Q + (int64_t)tq * ldq + 32 * kc + 8 * g) : z4);
}

// S^T[key 16 kt + 4 g + r][query n] of the staged key tile kt, unscaled
template <int LD>
__device__ __forceinline__ f32x4 score_tile(const bf16_t* Ks, int kt, int n, int g, const bf16x8 (&qf)[2]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + (16 * kt + n) * LD + 32 * kc + 8 * g);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kc], acc, 0, 0, 0);
  }
  return acc;
}

// the A-fragment of V^T for head dims 16 dt + n and the K = 32 step kp; without `second` the step's upper key tile is not read
template <int LD>
__device__ __forceinline__ bf16x8 vt_frag(const bf16_t* Vt, int dt, int n, int kp, int g, bool second) {
  const bf16x4 zb = {(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
  const bf16_t* vrow = Vt + (16 * dt + n) * LD + 32 * kp + 4 * g;
  const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vrow);
  const bf16x4 hi = second ? *reinterpret_cast<const bf16x4*>(vrow + 16) : zb;
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// O^T[d 16 dt + 4 g + r][query n] / lsum -> row O of the output; no visible key at all: a zero row, not NaN
__device__ __forceinline__ void store_o(bf16_t* O, const f32x4 (&o)[4], float lsum) {
  const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const bf16x4 ov = {(bf16_t)(o[dt][0] * inv), (bf16_t)(o[dt][1] * inv), (bf16_t)(o[dt][2] * inv), (bf16_t)(o[dt][3] * inv)};
    *reinterpret_cast<bf16x4*>(O + 16 * dt) = ov;
  }
}

// ---- causal, bf16 ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) attn_causal_mfma(const AttnArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[CT_MAX * C_KLD];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[HD * C_VLD];
  __shared__ __attribute__((aligned(16))) int kvis[CT_MAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / a.H, h = blockIdx.x - b * a.H;
  const int T = a.T, Tp16 = (T + 15) & ~15, Tp32 = (T + 31) & ~31;
  const bf16_t* Q = static_cast<const bf16_t*>(a.q) + (int64_t)b * T * a.ldq + h * HD;
  const bf16_t* K = static_cast<const bf16_t*>(a.k) + (int64_t)b * T * a.ldk + h * HD;
  const bf16_t* V = static_cast<const bf16_t*>(a.v) + (int64_t)b * T * a.ldv + h * HD;
  const int64_t* mk = a.mask ? a.mask + (int64_t)b * T : nullptr;

  if (tid < CT_MAX) kvis[tid] = key_visible(mk, tid, T) ? 1 : 0;
  // K: Tp16 rows x 8 chunks of 16 B, a row per 8 consecutive lanes
  for (int c = tid; c < Tp16 * 8; c += 256) stage_k<C_KLD>(Ks, c >> 3, c & 7, K, a.ldk, c >> 3, key_visible(mk, c >> 3, T));
  // V^T: Tp32 keys x 8 chunks, consecutive lanes on consecutive keys (the 2-byte transposed writes of a wave are contiguous)
  for (int c = tid; c < Tp32 * 8; c += 256) stage_vt<C_VLD>(Vt, c % Tp32, c / Tp32, V, a.ldv, c % Tp32, key_visible(mk, c % Tp32, T));
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
    load_q(qf, Q, tq, a.ldq, g, qok);

    // S^T[key 16 kt + 4 g + r][query n], key tiles 0 .. qt
    f32x4 s[8];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      s[kt] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (kt <= qt) {
        const f32x4 acc = score_tile<C_KLD>(Ks, kt, n, g, qf);
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
        for (int dt = 0; dt < 4; ++dt)
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vt_frag<C_VLD>(Vt, dt, n, kp, g, second), pf, o[dt], 0, 0, 0);
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
    if (qok) store_o(static_cast<bf16_t*>(a.o) + ((int64_t)b * T + tq) * a.ldo + h * HD + 4 * g, o, lsum);
  }
}

// ---- relative bias (BIAS), or bidirectional with no bias at all, bf16 ---------------------------------------------------------------
template <bool BIAS>
__global__ void __launch_bounds__(256) attn_relbias_mfma(const AttnArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[R_KC * R_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[HD * R_LD];
  __shared__ __attribute__((aligned(16))) float bs[BIAS ? R_BN : 4];  // without a bias: not used
  __shared__ __attribute__((aligned(16))) int kvis[R_KC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int b = blockIdx.y / a.H, h = blockIdx.y - b * a.H;
  const int T = a.T;
  const int q0 = blockIdx.x * R_QB;
  const bf16_t* Q = static_cast<const bf16_t*>(a.q) + (int64_t)b * T * a.ldq + h * HD;
  const bf16_t* K = static_cast<const bf16_t*>(a.k) + (int64_t)b * T * a.ldk + h * HD;
  const bf16_t* V = static_cast<const bf16_t*>(a.v) + (int64_t)b * T * a.ldv + h * HD;
  const int64_t* mk = a.mask ? a.mask + (int64_t)b * T : nullptr;
  const float LOG2E = 1.4426950408889634f;

  // bs[R_BM + o] = log2(e) rel_bias[h, o] for 0 <= o < 2 T - 1, zero around it
  if constexpr (BIAS) {
    const float* bias = a.bias + (int64_t)h * (2 * T - 1);
    for (int c = tid; c < R_BN; c += 256) {
      const int o = c - R_BM;
      bs[c] = (o >= 0 && o < 2 * T - 1) ? bias[o] * LOG2E : 0.f;
    }
  }
  const int tq = q0 + 16 * wave + n;  // this lane's query
  const bool qok = tq < T;
  const bool wave_on = q0 + 16 * wave < T;  // wave-uniform
  bf16x8 qf[2];
  load_q(qf, Q, tq, a.ldq, g, qok);
  // bias index of (query tq, key j): R_BM + j - tq + T - 1 >= R_BM + T - 1 - (q0 + 63) >= 1 as q0 < T, <= R_BM + 2 T + 61
  const int boff = R_BM + T - 1 - tq + 4 * g;

  const float sc = a.scale * LOG2E;
  float m = -INFINITY, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int k0 = 0; k0 < T; k0 += R_KC) {
    __syncthreads();  // the previous chunk's reads are done (first pass: nothing yet)
    if (tid < R_KC) kvis[tid] = key_visible(mk, k0 + tid, T) ? 1 : 0;
    // K: 64 rows x 8 chunks of 16 B, a row per 8 consecutive lanes
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i;
      stage_k<R_LD>(Ks, c >> 3, c & 7, K, a.ldk, k0 + (c >> 3), key_visible(mk, k0 + (c >> 3), T));
    }
    // V^T: 64 keys x 8 chunks, consecutive lanes on consecutive keys (the 2-byte transposed writes of a wave are contiguous)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i;
      stage_vt<R_LD>(Vt, c & 63, c >> 6, V, a.ldv, k0 + (c & 63), key_visible(mk, k0 + (c & 63), T));
    }
    __syncthreads();
    if (!wave_on) continue;  // no query of this wave is inside the sequence; it still stages
    const int nkt = min(4, (T - k0 + 15) >> 4);  // key tiles of this chunk that hold a key below T (wave-uniform)

    // S^T[key k0 + 16 kt + 4 g + r][query n] in log2 units
    f32x4 s[4];
    float cmax = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      s[kt] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (kt < nkt) {
        const f32x4 acc = score_tile<R_LD>(Ks, kt, n, g, qf);
        const i32x4 vis = *reinterpret_cast<const i32x4*>(kvis + 16 * kt + 4 * g);
        const float* br = BIAS ? bs + boff + k0 + 16 * kt : nullptr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (BIAS)
            s[kt][r] = vis[r] ? fmaf(acc[r], sc, br[r]) : -INFINITY;  // a select: nothing of a hidden key goes further
          else
            s[kt][r] = vis[r] ? acc[r] * sc : -INFINITY;
          cmax = fmaxf(cmax, s[kt][r]);
        }
      }
    }
    cmax = fmaxf(cmax, __shfl_xor(cmax, 16, 64));
    cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
    const float mn = fmaxf(m, cmax);
    const float ms = mn == -INFINITY ? 0.f : mn;  // no visible key so far: exp2(-inf - 0) = 0 below, never inf - inf
    const float alpha = __builtin_amdgcn_exp2f(m - ms);
    m = mn;
    l *= alpha;  // a partial sum per lane: alpha is the same in the four lanes of a query, they are added at the end
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[kt][r] = __builtin_amdgcn_exp2f(s[kt][r] - ms);
        l += s[kt][r];
      }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
    // O^T[d 16 dt + 4 g + r][query n] += V^T P^T, two key tiles per K = 32 step
#pragma unroll
    for (int kp = 0; kp < 2; ++kp) {
      if (2 * kp < nkt) {
        const bf16x8 pf = {(bf16_t)s[2 * kp][0],     (bf16_t)s[2 * kp][1],     (bf16_t)s[2 * kp][2],     (bf16_t)s[2 * kp][3],
                           (bf16_t)s[2 * kp + 1][0], (bf16_t)s[2 * kp + 1][1], (bf16_t)s[2 * kp + 1][2], (bf16_t)s[2 * kp + 1][3]};
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vt_frag<R_LD>(Vt, dt, n, kp, g, true), pf, o[dt], 0, 0, 0);
      }
    }
  }
  if (!wave_on) return;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (qok) store_o(static_cast<bf16_t*>(a.o) + ((int64_t)b * T + tq) * a.ldo + h * HD + 4 * g, o, l);
}

// ---- exact fp32, all three ---------------------------------------------------------------------------------------------------------------
// 64 query rows per workgroup (two lanes per row, 32 head dims each), keys walked 32 at a time -- all of them, or under the causal
// mask up to the block's last row; online softmax as attn_fwd_simple
constexpr int V_ROWS = 64, V_TILE = 32, V_HALF = HD / 2;

template <bool CAUSAL, bool BIAS = !CAUSAL>
__global__ void __launch_bounds__(128) attn_text_valu(const AttnArgs a) {
  __shared__ __attribute__((aligned(16))) float Ks[V_TILE * HD];
  __shared__ __attribute__((aligned(16))) float Vs[V_TILE * HD];
  __shared__ int kvis[V_TILE];
  const int T = a.T;
  const int b = blockIdx.y / a.H, h = blockIdx.y - b * a.H;
  const int r = threadIdx.x >> 1, half = threadIdx.x & 1;
  const int t = blockIdx.x * V_ROWS + r;
  const bool valid = t < T;
  const float* q = static_cast<const float*>(a.q) + (int64_t)b * T * a.ldq + h * HD;
  const float* k = static_cast<const float*>(a.k) + (int64_t)b * T * a.ldk + h * HD;
  const float* v = static_cast<const float*>(a.v) + (int64_t)b * T * a.ldv + h * HD;
  const int64_t* mk = a.mask ? a.mask + (int64_t)b * T : nullptr;
  const float* bias = nullptr;
  if constexpr (BIAS) bias = a.bias + (int64_t)h * (2 * T - 1) + (T - 1 - t);  // + key; read for valid rows and keys below T only
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
  int kend = T;
  if constexpr (CAUSAL) kend = min(T, (int)(blockIdx.x + 1) * V_ROWS);  // no row of this block sees a key at or past kend
  for (int k0 = 0; k0 < kend; k0 += V_TILE) {
    __syncthreads();
    for (int c = threadIdx.x; c < V_TILE * HD / 4; c += 128) {
      const int row = (c * 4) / HD, col = c * 4 - row * HD, key = k0 + row;
      const bool ok = key_visible(mk, key, T);
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      store4(Ks + row * HD + col, ok ? load4(k + (int64_t)key * a.ldk + col) : z);
      store4(Vs + row * HD + col, ok ? load4(v + (int64_t)key * a.ldv + col) : z);
    }
    if (threadIdx.x < V_TILE) kvis[threadIdx.x] = key_visible(mk, k0 + threadIdx.x, T) ? 1 : 0;
    __syncthreads();
    float s[V_TILE];
    float tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < V_TILE; ++j) {
      float p = 0.f;
      const float* kr = Ks + j * HD + half * V_HALF;
#pragma unroll
      for (int i = 0; i < V_HALF; i += 4) {
        const f32x4 kv = load4(kr + i);
        p += qr[i] * kv[0] + qr[i + 1] * kv[1] + qr[i + 2] * kv[2] + qr[i + 3] * kv[3];
      }
      p += __shfl_xor(p, 1, 64);
      if constexpr (CAUSAL)
        s[j] = (k0 + j <= t && kvis[j]) ? p : -INFINITY;
      else if constexpr (BIAS)
        s[j] = (valid && kvis[j]) ? p + bias[k0 + j] : -INFINITY;
      else
        s[j] = (valid && kvis[j]) ? p : -INFINITY;
      tmax = fmaxf(tmax, s[j]);
    }
    const float mx = fmaxf(m, tmax);
    const float mn = mx == -INFINITY ? 0.f : mx;  // nothing visible yet: the exponents below are taken against 0
    const float alpha = expf(m - mn);
    l *= alpha;
#pragma unroll
    for (int i = 0; i < V_HALF; ++i) oa[i] *= alpha;
#pragma unroll
    for (int j = 0; j < V_TILE; ++j) {
      if (s[j] == -INFINITY) continue;  // a hidden key's V row is never multiplied (it may hold anything)
      const float p = expf(s[j] - mn);
      l += p;
      const float* vr = Vs + j * HD + half * V_HALF;
#pragma unroll
      for (int i = 0; i < V_HALF; i += 4) {
        const f32x4 vv = load4(vr + i);
        oa[i] += p * vv[0];
        oa[i + 1] += p * vv[1];
        oa[i + 2] += p * vv[2];
        oa[i + 3] += p * vv[3];
      }
    }
    m = mx;  // not mn: a wholly hidden tile (tmax = -inf) leaves the maximum alone, and it stays -inf until a key is seen
  }
  if (valid) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    float* o = static_cast<float*>(a.o) + ((int64_t)b * T + t) * a.ldo + h * HD + half * V_HALF;
#pragma unroll
    for (int i = 0; i < V_HALF; i += 4) store4(o + i, f32x4{oa[i] * inv, oa[i + 1] * inv, oa[i + 2] * inv, oa[i + 3] * inv});
  }
}

// what the entry points refuse; `fn` opens every message.  rel_bias may be null only where the entry point has none
int check_args(const char* fn, const AttnArgs& a, bool has_bias, int d, int dtype, int t_max, int64_t bh_max) {
  UWU_CHECK_ARG(a.q && a.k && a.v && a.o && (!has_bias || a.bias), "%s: null pointer", fn);
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "%s: bad dtype %d", fn, dtype);
  UWU_CHECK_ARG(d == HD, "%s: head dim %d (built for 64)", fn, d);
  UWU_CHECK_ARG(a.T >= 1 && a.T <= t_max, "%s: T = %d outside [1, %d]", fn, a.T, t_max);
  UWU_CHECK_ARG(a.B > 0 && a.H > 0 && (int64_t)a.B * a.H <= bh_max, "%s: bad B = %d, H = %d%s", fn, a.B, a.H,
                bh_max == 65535 ? " (B * H <= 65535)" : "");
  const int hd = a.H * HD;
  UWU_CHECK_ARG(a.ldq >= hd && a.ldk >= hd && a.ldv >= hd && a.ldo >= hd, "%s: row stride < H*d", fn);
  const int al = dtype == UWU_BF16 ? 8 : 4;
  UWU_CHECK_ARG(a.ldq % al == 0 && a.ldk % al == 0 && a.ldv % al == 0 && a.ldo % al == 0, "%s: row strides must be multiples of %d elements",
                fn, al);
  UWU_CHECK_ARG((((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.o) & 15) == 0 && ((uintptr_t)a.mask & 7) == 0 &&
                    ((uintptr_t)a.bias & 3) == 0,
                "%s: misaligned pointer (16-byte q / k / v / o, 8-byte key_mask%s)", fn, has_bias ? ", 4-byte rel_bias" : "");
  UWU_CHECK_ARG(a.scale > 0.f && isfinite(a.scale), "%s: scale must be positive", fn);
  return UWU_OK;
}

}  // namespace

extern "C" int uwu_attention_causal_fwd(const void* q, const void* k, const void* v, const int64_t* key_mask, void* o, int B, int T,
                                        int H, int d, int ldq, int ldk, int ldv, int ldo, float scale, int dtype, void* stream) {
  const AttnArgs a{q, k, v, key_mask, o, B, T, H, ldq, ldk, ldv, ldo, scale, nullptr};
  if (const int e = check_args("attention_causal_fwd", a, false, d, dtype, CT_MAX, 0x7FFFFFFF / 64)) return e;
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  if (dtype == UWU_BF16)
    hipLaunchKernelGGL(attn_causal_mfma, dim3(B * H), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(attn_text_valu<true>, dim3(cdiv(T, V_ROWS), B * H), dim3(128), 0, st, a);
  // algorithmic work of the causal half: 4 d T (T + 1) / 2 per head; q, k, v, o once
  prof.done(UWU_PROF_ATTN_FWD, dtype == UWU_BF16 ? 0 : 1, 2.0 * B * H * HD * T * (T + 1.0), 4.0 * B * H * HD * T * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("attention_causal_fwd");
  return UWU_OK;
}

extern "C" int uwu_attention_relbias_fwd(const void* q, const void* k, const void* v, const float* rel_bias, const int64_t* key_mask,
                                         void* o, int B, int T, int H, int d, int ldq, int ldk, int ldv, int ldo, float scale, int dtype,
                                         void* stream) {
  const AttnArgs a{q, k, v, key_mask, o, B, T, H, ldq, ldk, ldv, ldo, scale, rel_bias};
  if (const int e = check_args("attention_relbias_fwd", a, true, d, dtype, RT_MAX, 65535)) return e;
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  if (dtype == UWU_BF16)
    hipLaunchKernelGGL(attn_relbias_mfma<true>, dim3(cdiv(T, R_QB), B * H), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((attn_text_valu<false, true>), dim3(cdiv(T, V_ROWS), B * H), dim3(128), 0, st, a);
  prof.done(UWU_PROF_ATTN_FWD, dtype == UWU_BF16 ? 0 : 1, 4.0 * B * H * HD * T * (double)T, 4.0 * B * H * HD * T * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("attention_relbias_fwd");
  return UWU_OK;
}

extern "C" int uwu_attention_bidir_fwd(const void* q, const void* k, const void* v, const int64_t* key_mask, void* o, int B, int T,
                                       int H, int d, int ldq, int ldk, int ldv, int ldo, float scale, int dtype, void* stream) {
  UWU_CHECK_ARG(d != 80, "attention_bidir_fwd: head dim 80 is not built (ViT-H/14, apple/DFN5B-CLIP-ViT-H-14-378 included): built for 64");
  const AttnArgs a{q, k, v, key_mask, o, B, T, H, ldq, ldk, ldv, ldo, scale, nullptr};
  if (const int e = check_args("attention_bidir_fwd", a, false, d, dtype, BT_MAX, 65535)) return e;
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  if (dtype == UWU_BF16)
    hipLaunchKernelGGL(attn_relbias_mfma<false>, dim3(cdiv(T, R_QB), B * H), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((attn_text_valu<false, false>), dim3(cdiv(T, V_ROWS), B * H), dim3(128), 0, st, a);
  prof.done(UWU_PROF_ATTN_FWD, dtype == UWU_BF16 ? 0 : 1, 4.0 * B * H * HD * T * (double)T, 4.0 * B * H * HD * T * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("attention_bidir_fwd");
  return UWU_OK;
}
