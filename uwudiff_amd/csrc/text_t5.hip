// The T5 v1.1 encoder's own kernels (uwudiff_amd/text_model.py T5EncoderModel): bidirectional attention
// with a learned relative-position bias over at most 512 tokens at head width 64, RMS normalisation with the residual add fused
// in, the tanh-GELU gate of the feed-forward, the gather that turns the bucket table into a bias per offset, and the token
// embedding (T5 has no position table).  Forward only: the text encoders are frozen.  The projections (packed q/k/v, o, wi_0 |
// wi_1, wo) run on uwu_gemm.
//
//   uwu_attention_relbias_fwd     o = softmax(scale Q K^T + rel_bias[h, j - i + T - 1] + M) V
//     bf16: attn_relbias_mfma -- a workgroup of four waves per (64 queries, batch, head); a wave owns one tile of 16 queries.  Keys
//           are walked 64 at a time with an online softmax: the chunk's K [64][64 + 8] and V^T [64][64 + 8] are staged in LDS
//           (rows of keys the key mask hides, and rows past T, as zeros: T is padded to the tile here, never in memory), the
//           head's bias row (2 T - 1 floats, times log2 e) is staged once with 64 zeros of margin on either side so that the
//           padded queries and keys index inside it.  Tiling over query blocks was chosen over staging all 512 keys once per
//           (batch, head) because K + V^T of 512 keys take 140 KB -- one workgroup of four waves per CU, every load latency
//           exposed, and 768 workgroups for 256 CUs at B H = 768 whatever T is -- while 23 KB let several workgroups share a CU
//           and T = 512 brings eight times as many of them; the K / V re-reads hit the L2.  As in text.hip everything is
//           computed TRANSPOSED: S^T = K Q^T on v_mfma_f32_16x16x32_bf16 leaves (query = lane % 16, keys 16 kt + 4 (lane / 16)
//           .. + 3) in each lane, which is the B-operand layout of O^T += V^T P^T once two key tiles share one K = 32 step.
//           Q goes from global memory straight to registers (a query row is used by one wave).  A hidden key's score is
//           replaced by -inf with a select and its K / V rows are never read, so what they hold goes nowhere; every query sees
//           the same keys, so no tile needs the VALU path the causal kernel has for its diagonal.
//     fp32: attn_relbias_valu -- the exact-fp32 parity path in the manner of attn_causal_valu (two lanes per query row, K / V
//           tiles of 32 keys staged as fp32), the bias read per (query, key) from global memory.
#include <math.h>

#include "common.h"

namespace {

struct RelArgs {
  const void *q, *k, *v;
  const float* bias;
  const int64_t* mask;
  void* o;
  int B, T, H, ldq, ldk, ldv, ldo;
  float scale;
};

constexpr int RD = 64;            // head width
constexpr int RT_MAX = 512;       // longest sequence
constexpr int R_QB = 64;          // queries per workgroup
constexpr int R_KC = 64;          // keys per chunk
constexpr int R_LD = RD + 8;      // row stride of both LDS tiles (elements): 144 B
constexpr int R_BM = 64;          // margin of the staged bias row on either side
constexpr int R_BN = 2 * RT_MAX - 1 + 2 * R_BM + 1;  // 1152 floats

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) attn_relbias_mfma(const RelArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[R_KC * R_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[RD * R_LD];
  __shared__ __attribute__((aligned(16))) float bs[R_BN];
  __shared__ __attribute__((aligned(16))) int kvis[R_KC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int b = blockIdx.y / a.H, h = blockIdx.y - b * a.H;
  const int T = a.T;
  const int q0 = blockIdx.x * R_QB;
  const bf16_t* Q = static_cast<const bf16_t*>(a.q) + (int64_t)b * T * a.ldq + h * RD;
  const bf16_t* K = static_cast<const bf16_t*>(a.k) + (int64_t)b * T * a.ldk + h * RD;
  const bf16_t* V = static_cast<const bf16_t*>(a.v) + (int64_t)b * T * a.ldv + h * RD;
  const int64_t* mk = a.mask ? a.mask + (int64_t)b * T : nullptr;
  const float* bias = a.bias + (int64_t)h * (2 * T - 1);
  const u32x4 z4 = {0u, 0u, 0u, 0u};
  const float LOG2E = 1.4426950408889634f;

  // bs[R_BM + o] = log2(e) rel_bias[h, o] for 0 <= o < 2 T - 1, zero around it
  for (int c = tid; c < R_BN; c += 256) {
    const int o = c - R_BM;
    bs[c] = (o >= 0 && o < 2 * T - 1) ? bias[o] * LOG2E : 0.f;
  }
  const int tq = q0 + 16 * wave + n;  // this lane's query
  const bool qok = tq < T;
  const bool wave_on = q0 + 16 * wave < T;  // wave-uniform
  bf16x8 qf[2];
#pragma unroll
  for (int kc = 0; kc < 2; ++kc)
    qf[kc] = __builtin_bit_cast(bf16x8, qok ? *reinterpret_cast<const u32x4*>(Q + (int64_t)tq * a.ldq + 32 * kc + 8 * g) : z4);
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
    if (tid < R_KC) kvis[tid] = (k0 + tid < T && (!mk || mk[k0 + tid] != 0)) ? 1 : 0;
    // K: 64 rows x 8 chunks of 16 B, a row per 8 consecutive lanes
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i;
      const int row = c >> 3, col8 = c & 7, key = k0 + row;
      const bool ok = key < T && (!mk || mk[key] != 0);
      *reinterpret_cast<u32x4*>(Ks + row * R_LD + 8 * col8) = ok ? *reinterpret_cast<const u32x4*>(K + (int64_t)key * a.ldk + 8 * col8) : z4;
    }
    // V^T: 64 keys x 8 chunks, consecutive lanes on consecutive keys (the 2-byte transposed writes of a wave are contiguous)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i;
      const int row = c & 63, col8 = c >> 6, key = k0 + row;
      const bool ok = key < T && (!mk || mk[key] != 0);
      const u32x4 raw = ok ? *reinterpret_cast<const u32x4*>(V + (int64_t)key * a.ldv + 8 * col8) : z4;
      const bf16x8 v8 = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
      for (int j = 0; j < 8; ++j) Vt[(8 * col8 + j) * R_LD + row] = v8[j];
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
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + (16 * kt + n) * R_LD + 32 * kc + 8 * g);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kc], acc, 0, 0, 0);
        }
        const i32x4 vis = *reinterpret_cast<const i32x4*>(kvis + 16 * kt + 4 * g);
        const float* br = bs + boff + k0 + 16 * kt;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[kt][r] = vis[r] ? fmaf(acc[r], sc, br[r]) : -INFINITY;  // a select: nothing of a hidden key goes further
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
    // O^T[d 16 dt + 4 g + r][query n] += V^T P^T, two key tiles per K = 32 step: k slot 8 g + j <-> key 16 (2 kp + j / 4) + 4 g + j % 4
#pragma unroll
    for (int kp = 0; kp < 2; ++kp) {
      if (2 * kp < nkt) {
        const bf16x8 pf = {(bf16_t)s[2 * kp][0],     (bf16_t)s[2 * kp][1],     (bf16_t)s[2 * kp][2],     (bf16_t)s[2 * kp][3],
                           (bf16_t)s[2 * kp + 1][0], (bf16_t)s[2 * kp + 1][1], (bf16_t)s[2 * kp + 1][2], (bf16_t)s[2 * kp + 1][3]};
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16_t* vrow = Vt + (16 * dt + n) * R_LD + 32 * kp + 4 * g;
          const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vrow);
          const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vrow + 16);
          const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
        }
      }
    }
  }
  if (!wave_on) return;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (qok) {
    const float inv = l > 0.f ? 1.f / l : 0.f;  // no visible key at all: a zero row, not NaN
    bf16_t* O = static_cast<bf16_t*>(a.o) + ((int64_t)b * T + tq) * a.ldo + h * RD + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const bf16x4 ov = {(bf16_t)(o[dt][0] * inv), (bf16_t)(o[dt][1] * inv), (bf16_t)(o[dt][2] * inv), (bf16_t)(o[dt][3] * inv)};
      *reinterpret_cast<bf16x4*>(O + 16 * dt) = ov;
    }
  }
}

// exact fp32: 64 query rows per workgroup (two lanes per row, 32 head dims each), all keys walked 32 at a time; online softmax
constexpr int V_ROWS = 64, V_TILE = 32, V_HALF = RD / 2;

__global__ void __launch_bounds__(128) attn_relbias_valu(const RelArgs a) {
  __shared__ __attribute__((aligned(16))) float Ks[V_TILE * RD];
  __shared__ __attribute__((aligned(16))) float Vs[V_TILE * RD];
  __shared__ int kvis[V_TILE];
  const int T = a.T;
  const int b = blockIdx.y / a.H, h = blockIdx.y - b * a.H;
  const int r = threadIdx.x >> 1, half = threadIdx.x & 1;
  const int t = blockIdx.x * V_ROWS + r;
  const bool valid = t < T;
  const float* q = static_cast<const float*>(a.q) + (int64_t)b * T * a.ldq + h * RD;
  const float* k = static_cast<const float*>(a.k) + (int64_t)b * T * a.ldk + h * RD;
  const float* v = static_cast<const float*>(a.v) + (int64_t)b * T * a.ldv + h * RD;
  const int64_t* mk = a.mask ? a.mask + (int64_t)b * T : nullptr;
  const float* bias = a.bias + (int64_t)h * (2 * T - 1) + (T - 1 - t);  // + key; read for valid rows and keys below T only
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
  for (int k0 = 0; k0 < T; k0 += V_TILE) {
    __syncthreads();
    for (int c = threadIdx.x; c < V_TILE * RD / 4; c += 128) {
      const int row = (c * 4) / RD, col = c * 4 - row * RD, key = k0 + row;
      const bool ok = key < T && (!mk || mk[key] != 0);
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      store4(Ks + row * RD + col, ok ? load4(k + (int64_t)key * a.ldk + col) : z);
      store4(Vs + row * RD + col, ok ? load4(v + (int64_t)key * a.ldv + col) : z);
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
      const float* kr = Ks + j * RD + half * V_HALF;
#pragma unroll
      for (int i = 0; i < V_HALF; i += 4) {
        const f32x4 kv = load4(kr + i);
        p += qr[i] * kv[0] + qr[i + 1] * kv[1] + qr[i + 2] * kv[2] + qr[i + 3] * kv[3];
      }
      p += __shfl_xor(p, 1, 64);
      const bool see = valid && kvis[j];
      s[j] = see ? p + bias[k0 + j] : -INFINITY;
      tmax = fmaxf(tmax, s[j]);
    }
    float mn = fmaxf(m, tmax);
    if (mn == -INFINITY) mn = 0.f;  // nothing visible yet
    const float alpha = expf(m - mn);
    l *= alpha;
#pragma unroll
    for (int i = 0; i < V_HALF; ++i) oa[i] *= alpha;
#pragma unroll
    for (int j = 0; j < V_TILE; ++j) {
      if (s[j] == -INFINITY) continue;  // a hidden key's V row is never multiplied (it may hold anything)
      const float p = expf(s[j] - mn);
      l += p;
      const float* vr = Vs + j * RD + half * V_HALF;
#pragma unroll
      for (int i = 0; i < V_HALF; i += 4) {
        const f32x4 vv = load4(vr + i);
        oa[i] += p * vv[0];
        oa[i + 1] += p * vv[1];
        oa[i + 2] += p * vv[2];
        oa[i + 3] += p * vv[3];
      }
    }
    if (tmax != -INFINITY) m = mn;
  }
  if (valid) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    float* o = static_cast<float*>(a.o) + ((int64_t)b * T + t) * a.ldo + h * RD + half * V_HALF;
#pragma unroll
    for (int i = 0; i < V_HALF; i += 4) store4(o + i, f32x4{oa[i] * inv, oa[i + 1] * inv, oa[i + 2] * inv, oa[i + 3] * inv});
  }
}

// ---- x_out = x_in + y;  n_out = x_out * rsqrt(mean(x_out^2) + eps) * weight -----------------------------------------------
// one workgroup per row; the row is read twice (the second time what this thread itself wrote or read: a cache hit).  The
// statistics are those of x_out AS STORED (for bf16 the rounded sum), so n_out is the norm of the tensor the next layer reads.
template <typename T>
__global__ void __launch_bounds__(256) add_rmsnorm_kernel(const T* x_in, const T* y, const float* __restrict__ w,
                                                          T* x_out, T* __restrict__ n_out, int D, float eps) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const T* xi = x_in + row * D;
  T* xo = x_out + row * D;
  float ss = 0.f;
  for (int c = threadIdx.x * 8; c < D; c += 256 * 8) {
    f32x8 v = load8(xi + c);
    if (y) {
      v = v + load8(y + row * D + c);
      store8(xo + c, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = to_f32(from_f32<T>(v[e]));
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = fmaf(v[e], v[e], ss);
  }
  const float tot = block_sum<4>(ss, red);
  const float rstd = 1.f / sqrtf(tot / (float)D + eps);
  const T* src = y ? xo : xi;
  for (int c = threadIdx.x * 8; c < D; c += 256 * 8) {
    const f32x8 v = load8(src + c), g = load8(w + c);
    f32x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = v[e] * rstd * g[e];
    store8(n_out + row * D + c, r);
  }
}

// ---- out = gelu_new(u[:, :F]) * u[:, F:2F] ---------------------------------------------------------------------------------
// gelu_new(x) = 0.5 x (1 + tanh(z)) = x / (1 + exp(-2 z)), z = sqrt(2 / pi) (x + 0.044715 x^3): the second form has no
// cancellation in the left tail.  fp32 tensors in double, bf16 tensors in fp32 (as uwu_bias_act_fwd).
__device__ __forceinline__ float gate_one(float x, float gte, float) {
  const double d = (double)x;
  const double z2 = 2.0 * 0.79788456080286535588 * (d + 0.044715 * d * d * d);
  return (float)(d / (1.0 + exp(-z2)) * (double)gte);
}
__device__ __forceinline__ float gate_one(float x, float gte, bf16_t) {
  const float z2 = 2.f * 0.7978845608028654f * fmaf(0.044715f * (x * x), x, x);
  const float t = expf(-fabsf(z2));  // never overflows: sigmoid(z2) = 1 / (1 + t) on the right, t / (1 + t) on the left
  return x * ((z2 >= 0.f ? 1.f : t) / (1.f + t)) * gte;
}

template <typename T>
__global__ void __launch_bounds__(256) gated_act_kernel(const T* __restrict__ u, T* __restrict__ out, int64_t M, int F, int ldu, int ldo) {
  const int per = F / 8;
  const int64_t total = M * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / per;
    const int c = (int)(i - row * per) * 8;
    const f32x8 x = load8(u + row * ldu + c), gt = load8(u + row * ldu + F + c);
    f32x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = gate_one(x[e], gt[e], T{});
    store8(out + row * ldo + c, r);
  }
}

// ---- out[h, o] = weight[bucket[o], h] --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rel_bias_kernel(const float* __restrict__ w, const int* __restrict__ bucket, float* __restrict__ out,
                                                       int nb, int H, int n) {
  const int total = H * n;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int h = i / n, o = i - h * n;
    int bk = bucket[o];
    bk = bk < 0 ? 0 : (bk >= nb ? nb - 1 : bk);  // nothing outside the table is ever read
    out[i] = w[bk * H + h];
  }
}

// ---- out[row, :] = table[ids[row], :] --------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) token_embed_kernel(const int64_t* __restrict__ ids, const T* __restrict__ tok, T* __restrict__ out,
                                                          int64_t rows, int D, int vocab) {
  const int per = D / 8;
  const int64_t total = rows * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / per;
    const int c = (int)(i - row * per) * 8;
    int64_t id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    store8(out + row * D + c, load8(tok + id * D + c));
  }
}

}  // namespace

extern "C" int uwu_attention_relbias_fwd(const void* q, const void* k, const void* v, const float* rel_bias, const int64_t* key_mask,
                                         void* o, int B, int T, int H, int d, int ldq, int ldk, int ldv, int ldo, float scale, int dtype,
                                         void* stream) {
  UWU_CHECK_ARG(q && k && v && o && rel_bias, "attention_relbias_fwd: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "attention_relbias_fwd: bad dtype %d", dtype);
  UWU_CHECK_ARG(d == RD, "attention_relbias_fwd: head dim %d (built for 64)", d);
  UWU_CHECK_ARG(T >= 1 && T <= RT_MAX, "attention_relbias_fwd: T = %d outside [1, 512]", T);
  UWU_CHECK_ARG(B > 0 && H > 0 && (int64_t)B * H <= 65535, "attention_relbias_fwd: bad B = %d, H = %d (B * H <= 65535)", B, H);
  const int hd = H * RD;
  UWU_CHECK_ARG(ldq >= hd && ldk >= hd && ldv >= hd && ldo >= hd, "attention_relbias_fwd: row stride < H*d");
  const int al = dtype == UWU_BF16 ? 8 : 4;
  UWU_CHECK_ARG(ldq % al == 0 && ldk % al == 0 && ldv % al == 0 && ldo % al == 0,
                "attention_relbias_fwd: row strides must be multiples of %d elements", al);
  UWU_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) == 0 && ((uintptr_t)key_mask & 7) == 0 &&
                    ((uintptr_t)rel_bias & 3) == 0,
                "attention_relbias_fwd: misaligned pointer (16-byte q / k / v / o, 8-byte key_mask, 4-byte rel_bias)");
  UWU_CHECK_ARG(scale > 0.f && isfinite(scale), "attention_relbias_fwd: scale must be positive");
  RelArgs a{q, k, v, rel_bias, key_mask, o, B, T, H, ldq, ldk, ldv, ldo, scale};
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  if (dtype == UWU_BF16)
    hipLaunchKernelGGL(attn_relbias_mfma, dim3(cdiv(T, R_QB), B * H), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(attn_relbias_valu, dim3(cdiv(T, V_ROWS), B * H), dim3(128), 0, st, a);
  prof.done(UWU_PROF_ATTN_FWD, dtype == UWU_BF16 ? 0 : 1, 4.0 * B * H * RD * T * (double)T, 4.0 * B * H * RD * T * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("attention_relbias_fwd");
  return UWU_OK;
}

extern "C" int uwu_add_rmsnorm_fwd(const void* x_in, const void* y, const float* weight, void* x_out, void* n_out, int M, int D, float eps,
                                   int dtype, void* stream) {
  UWU_CHECK_ARG(x_in && weight && n_out && (!y || x_out), "add_rmsnorm_fwd: null pointer (x_out is required with y)");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "add_rmsnorm_fwd: bad dtype %d", dtype);
  UWU_CHECK_ARG(M > 0 && D > 0 && D % 8 == 0, "add_rmsnorm_fwd: bad shape M = %d, D = %d (D a multiple of 8)", M, D);
  UWU_CHECK_ARG(eps >= 0.f && isfinite(eps), "add_rmsnorm_fwd: bad eps");
  UWU_CHECK_ARG((((uintptr_t)x_in | (uintptr_t)y | (uintptr_t)weight | (uintptr_t)x_out | (uintptr_t)n_out) & 15) == 0,
                "add_rmsnorm_fwd: misaligned pointer");
  UWU_CHECK_ARG(n_out != x_in && n_out != x_out && n_out != y, "add_rmsnorm_fwd: n_out must not alias an input or x_out");
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  if (dtype == UWU_BF16)
    hipLaunchKernelGGL(add_rmsnorm_kernel<bf16_t>, dim3(M), dim3(256), 0, st, (const bf16_t*)x_in, (const bf16_t*)y, weight, (bf16_t*)x_out,
                       (bf16_t*)n_out, D, eps);
  else
    hipLaunchKernelGGL(add_rmsnorm_kernel<float>, dim3(M), dim3(256), 0, st, (const float*)x_in, (const float*)y, weight, (float*)x_out,
                       (float*)n_out, D, eps);
  prof.done(UWU_PROF_LN_FWD, dtype == UWU_BF16 ? 0 : 1, 0.0, (y ? 4.0 : 2.0) * M * D * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("add_rmsnorm_fwd");
  return UWU_OK;
}

extern "C" int uwu_gated_act_fwd(const void* u, void* out, int M, int F, int ldu, int ldo, int kind, int dtype, void* stream) {
  UWU_CHECK_ARG(u && out, "gated_act_fwd: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "gated_act_fwd: bad dtype %d", dtype);
  UWU_CHECK_ARG(kind == UWU_GATE_GELU_TANH, "gated_act_fwd: bad kind %d", kind);
  UWU_CHECK_ARG(M > 0 && F > 0 && F % 8 == 0 && ldu >= 2 * (int64_t)F && ldu % 8 == 0 && ldo >= F && ldo % 8 == 0,
                "gated_act_fwd: bad shape M = %d, F = %d, ldu = %d, ldo = %d", M, F, ldu, ldo);
  UWU_CHECK_ARG((((uintptr_t)u | (uintptr_t)out) & 15) == 0, "gated_act_fwd: misaligned pointer");
  const int esz = dtype == UWU_BF16 ? 2 : 4;
  const uintptr_t ub = (uintptr_t)u, ue = ub + ((uintptr_t)(M - 1) * ldu + 2 * (uintptr_t)F) * esz;
  const uintptr_t ob = (uintptr_t)out, oe = ob + ((uintptr_t)(M - 1) * ldo + F) * esz;
  UWU_CHECK_ARG(oe <= ub || ue <= ob, "gated_act_fwd: out overlaps u");
  const int grid = ew_grid((int64_t)M * (F / 8), 256);
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  if (dtype == UWU_BF16)
    hipLaunchKernelGGL(gated_act_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)u, (bf16_t*)out, (int64_t)M, F, ldu, ldo);
  else
    hipLaunchKernelGGL(gated_act_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)u, (float*)out, (int64_t)M, F, ldu, ldo);
  prof.done(UWU_PROF_OTHER, dtype == UWU_BF16 ? 0 : 1, 0.0, 3.0 * M * F * esz);
  UWU_LAUNCH_CHECK("gated_act_fwd");
  return UWU_OK;
}

extern "C" int uwu_t5_rel_bias(const float* weight, const int32_t* bucket, float* out, int num_buckets, int H, int n, void* stream) {
  UWU_CHECK_ARG(weight && bucket && out, "t5_rel_bias: null pointer");
  UWU_CHECK_ARG(num_buckets > 0 && H > 0 && n > 0 && n % 2 == 1 && n <= 2 * RT_MAX - 1 && (int64_t)H * n <= 0x7FFFFFFF,
                "t5_rel_bias: bad shape num_buckets = %d, H = %d, n = %d (n = 2 T - 1, T <= 512)", num_buckets, H, n);
  UWU_CHECK_ARG((((uintptr_t)weight | (uintptr_t)bucket | (uintptr_t)out) & 3) == 0, "t5_rel_bias: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  hipLaunchKernelGGL(rel_bias_kernel, dim3(ew_grid((int64_t)H * n, 256)), dim3(256), 0, st, weight, bucket, out, num_buckets, H, n);
  prof.done(UWU_PROF_OTHER, 1, 0.0, 8.0 * H * n + 4.0 * n);
  UWU_LAUNCH_CHECK("t5_rel_bias");
  return UWU_OK;
}

extern "C" int uwu_token_embed(const int64_t* ids, const void* tok_table, void* out, int B, int T, int D, int vocab, int dtype, void* stream) {
  UWU_CHECK_ARG(ids && tok_table && out, "token_embed: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "token_embed: bad dtype %d", dtype);
  UWU_CHECK_ARG(B > 0 && T > 0 && vocab > 0 && D > 0 && D % 8 == 0, "token_embed: bad shape B = %d, T = %d, D = %d, vocab = %d", B, T, D, vocab);
  UWU_CHECK_ARG((((uintptr_t)tok_table | (uintptr_t)out) & 15) == 0 && ((uintptr_t)ids & 7) == 0, "token_embed: misaligned pointer");
  const int64_t rows = (int64_t)B * T;
  const int grid = ew_grid(rows * (D / 8), 256);
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  if (dtype == UWU_BF16)
    hipLaunchKernelGGL(token_embed_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, ids, (const bf16_t*)tok_table, (bf16_t*)out, rows, D, vocab);
  else
    hipLaunchKernelGGL(token_embed_kernel<float>, dim3(grid), dim3(256), 0, st, ids, (const float*)tok_table, (float*)out, rows, D, vocab);
  prof.done(UWU_PROF_OTHER, dtype == UWU_BF16 ? 0 : 1, 0.0, 2.0 * rows * D * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("token_embed");
  return UWU_OK;
}
