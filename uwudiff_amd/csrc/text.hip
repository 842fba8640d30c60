// The text encoders' own kernels apart from attention (uwudiff_amd/text_model.py; DESIGN.md sections 4.23 and 4.25).  Forward
// only: the text encoders are frozen.  Attention is in attention_text.hip; the projections and feed-forward GEMMs run on uwu_gemm.
//
//   the CLIP text transformer: token + position embedding (uwu_text_embed), bias + quick_gelu / erf-GELU (uwu_bias_act_fwd),
//     pooling at the eos token (uwu_text_pool); its affine pre-LayerNorm with fused residual is uwu_add_ln_modulate_fwd
//   the T5 v1.1 encoder: the token embedding alone, T5 has no position table (uwu_token_embed), RMS normalisation with the
//     residual add fused in (uwu_add_rmsnorm_fwd), the tanh-GELU gate of the feed-forward (uwu_gated_act_fwd), the gather that
//     turns the bucket table into a bias per offset (uwu_t5_rel_bias)
#include <math.h>

#include "common.h"

namespace {

constexpr int T5_T_MAX = 512;  // RT_MAX of attention_text.hip, the longest sequence uwu_attention_relbias_fwd takes: keep the two equal

// ---- out[row, :] = tok[ids[row], :] (+ pos[row % Tn, :]) --------------------------------------------------------------------
template <typename T, bool POS>
__global__ void __launch_bounds__(256) embed_kernel(const int64_t* __restrict__ ids, const T* __restrict__ tok, const T* __restrict__ pos,
                                                    T* __restrict__ out, int64_t rows, int Tn, int D, int vocab) {
  const int per = D / 8;
  const int64_t total = rows * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / per;
    const int c = (int)(i - row * per) * 8;
    int64_t id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    f32x8 a = load8(tok + id * D + c);
    if constexpr (POS) a = a + load8(pos + (row % Tn) * D + c);
    store8(out + row * D + c, a);
  }
}

// what both embedding entry points refuse; `pos` is null for the one without a position table
int check_embed(const char* fn, const int64_t* ids, const void* tok, const void* pos, bool has_pos, const void* out, int B, int T, int D,
                int vocab, int dtype) {
  UWU_CHECK_ARG(ids && tok && out && (!has_pos || pos), "%s: null pointer", fn);
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "%s: bad dtype %d", fn, dtype);
  UWU_CHECK_ARG(B > 0 && T > 0 && vocab > 0 && D > 0 && D % 8 == 0, "%s: bad shape B = %d, T = %d, D = %d, vocab = %d", fn, B, T, D, vocab);
  UWU_CHECK_ARG((((uintptr_t)tok | (uintptr_t)pos | (uintptr_t)out) & 15) == 0 && ((uintptr_t)ids & 7) == 0, "%s: misaligned pointer", fn);
  return UWU_OK;
}

template <bool POS>
void launch_embed(const int64_t* ids, const void* tok, const void* pos, void* out, int B, int T, int D, int vocab, int dtype, void* stream) {
  const int64_t rows = (int64_t)B * T;
  const int grid = ew_grid(rows * (D / 8), 256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == UWU_BF16)
    hipLaunchKernelGGL((embed_kernel<bf16_t, POS>), dim3(grid), dim3(256), 0, st, ids, (const bf16_t*)tok, (const bf16_t*)pos, (bf16_t*)out,
                       rows, T, D, vocab);
  else
    hipLaunchKernelGGL((embed_kernel<float, POS>), dim3(grid), dim3(256), 0, st, ids, (const float*)tok, (const float*)pos, (float*)out, rows,
                       T, D, vocab);
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

}  // namespace

extern "C" int uwu_text_embed(const int64_t* ids, const void* tok_table, const void* pos_table, void* out, int B, int T, int D,
                              int vocab, int dtype, void* stream) {
  if (const int e = check_embed("text_embed", ids, tok_table, pos_table, true, out, B, T, D, vocab, dtype)) return e;
  launch_embed<true>(ids, tok_table, pos_table, out, B, T, D, vocab, dtype, stream);
  UWU_LAUNCH_CHECK("text_embed");
  return UWU_OK;
}

extern "C" int uwu_token_embed(const int64_t* ids, const void* tok_table, void* out, int B, int T, int D, int vocab, int dtype, void* stream) {
  if (const int e = check_embed("token_embed", ids, tok_table, nullptr, false, out, B, T, D, vocab, dtype)) return e;
  UwuProfScope prof(stream);
  launch_embed<false>(ids, tok_table, nullptr, out, B, T, D, vocab, dtype, stream);
  prof.done(UWU_PROF_OTHER, dtype == UWU_BF16 ? 0 : 1, 0.0, 2.0 * B * T * D * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("token_embed");
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
  UWU_CHECK_ARG(num_buckets > 0 && H > 0 && n > 0 && n % 2 == 1 && n <= 2 * T5_T_MAX - 1 && (int64_t)H * n <= 0x7FFFFFFF,
                "t5_rel_bias: bad shape num_buckets = %d, H = %d, n = %d (n = 2 T - 1, T <= 512)", num_buckets, H, n);
  UWU_CHECK_ARG((((uintptr_t)weight | (uintptr_t)bucket | (uintptr_t)out) & 3) == 0, "t5_rel_bias: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  hipLaunchKernelGGL(rel_bias_kernel, dim3(ew_grid((int64_t)H * n, 256)), dim3(256), 0, st, weight, bucket, out, num_buckets, H, n);
  prof.done(UWU_PROF_OTHER, 1, 0.0, 8.0 * H * n + 4.0 * n);
  UWU_LAUNCH_CHECK("t5_rel_bias");
  return UWU_OK;
}
