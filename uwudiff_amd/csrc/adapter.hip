// LyCORIS-style adapters on the frozen UNet: the merge of every adapted tensor into the
// effective weights (one launch) and the adapter gradients of one layer from its fp32 weight gradient.
//
//   merge: W_eff = W + dW_adapter, written as fp32 (where an fp32 effective copy exists) and as bf16 (the GEMM shadow);
//          one pass over the adapted elements, the factors come from L1 / L2.
//   grad:  LoRA  d_up += s dW down^T, d_down += s up^T dW;  LoKr  dw1[i,j] += s <dW block (i,j), w2>,
//          dw2 += s sum_ij w1[i,j] dW block (i,j) (through w2 = w2_a w2_b for the low-rank form).  dW is read once; the
//          partial sums of the workgroups go to a workspace and a second launch adds them in a fixed order: no float
//          atomics, the result is bit-identical run to run.
//   dora:  weight decomposition on top of LoRA / LoKr (section 4.39): W' = m (W + dW) / (||W + dW|| + eps) per row or column --
//          the norms of every decomposed tensor (one launch), the merge with the factor m / n (one launch), and per layer the
//          stage in front of `grad` that turns dL/dW' into dL/d(W + dW) in place and adds dL/dm.  Fixed-order fp64 sums.
//   conv:  the same on a 3x3 convolution weight stored [Cout_store, 9, Cin_store] (section 4.41): LoCon, its Tucker form and LoKr
//          with the adapter tensors tap-major -- T = mid . down of every Tucker segment (one launch) and the merge of every
//          convolution (one launch); per layer the LoRA / LoKr gradient kernels above through a column map, plus the Tucker chain.
#include "common.h"

namespace {

constexpr int AD_NF = 13;  // int64 fields per segment row (see uwu_hip.h)
constexpr int AD_MERGE_ELEMS = 4096;  // elements per workgroup: 256 threads x 4 x 4
constexpr int AD_MAX_RANK = 128;

__device__ __forceinline__ float ad_delta(const int64_t* __restrict__ row, const float* __restrict__ p, int e) {
  const int kind = (int)row[0];
  const int cols = (int)row[2];
  if (kind == UWU_ADAPTER_NORM) return p[row[6] + e];
  const int i = e / cols, j = e - i * cols;
  const float scale = __int_as_float((int)row[12]);
  const int r = (int)row[9];
  if (kind == UWU_ADAPTER_LORA) {
    const float* up = p + row[6] + (int64_t)i * r;
    const float* down = p + row[7] + j;
    float acc = 0.f;
    for (int t = 0; t < r; ++t) acc += up[t] * down[(int64_t)t * cols];
    return acc * scale;
  }
  const int out_k = (int)row[10], in_n = (int)row[11], in_m = cols / in_n;
  const int i1 = i / out_k, k = i - i1 * out_k, j1 = j / in_n, l = j - j1 * in_n;
  const float w1 = p[row[6] + (int64_t)i1 * in_m + j1];
  float w2;
  if (kind == UWU_ADAPTER_LOKR) {
    w2 = p[row[7] + (int64_t)k * in_n + l];
  } else {  // low-rank w2 = w2_a [out_k, r] . w2_b [r, in_n], formed before the Kronecker product
    const float* a = p + row[7] + (int64_t)k * r;
    const float* b = p + row[8] + l;
    w2 = 0.f;
    for (int t = 0; t < r; ++t) w2 += a[t] * b[(int64_t)t * in_n];
  }
  return (w1 * w2) * scale;
}

__global__ void __launch_bounds__(256) adapter_merge_kernel(const float* __restrict__ base, const float* __restrict__ p,
                                                            const int64_t* __restrict__ table,
                                                            const int64_t* __restrict__ blk_start, int nseg,
                                                            float* __restrict__ eff, bf16_t* __restrict__ shadow) {
  // the segment of this workgroup: blk_start is the exclusive prefix sum of the workgroups per segment
  const int64_t bid = blockIdx.x;
  int lo = 0, hi = nseg;  // blk_start[lo] <= bid < blk_start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blk_start[mid] <= bid) lo = mid;
    else hi = mid;
  }
  const int64_t* row = table + (int64_t)lo * AD_NF;
  const int n = (int)(row[1] * row[2]);
  const int64_t boff = row[3], eoff = row[4], soff = row[5];
  const int e0 = (int)(bid - blk_start[lo]) * AD_MERGE_ELEMS;
#pragma unroll
  for (int it = 0; it < AD_MERGE_ELEMS / 1024; ++it) {
    const int e = e0 + it * 1024 + 4 * threadIdx.x;
    if (e >= n) break;
    if (e + 4 <= n) {  // offsets are multiples of 64 elements: 16-byte aligned fp32, 8-byte aligned bf16
      f32x4 v = load4(base + boff + e);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] += ad_delta(row, p, e + q);
      if (eoff >= 0) store4(eff + eoff + e, v);
      if (shadow && soff >= 0) store4(shadow + soff + e, v);
    } else {
      for (int q = e; q < n; ++q) {
        const float v = base[boff + q] + ad_delta(row, p, q);
        if (eoff >= 0) eff[eoff + q] = v;
        if (shadow && soff >= 0) shadow[soff + q] = (bf16_t)v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- LoRA
constexpr int LR_RT = 32, LR_CT = 256;  // dW tile of one workgroup: 32 rows x 256 columns, staged in LDS

// partials: du_part[ct][n][r] = sum_{c in tile ct} dW[n,c] down[t,c];  dd_part[rt][t][k] = sum_{i in tile rt} up[i,t] dW[i,k]
// CONV (section 4.41): dw is a stored convolution gradient [>= N rows, 9 cin_store]; column j = t cin + c of the [N, K = 9 cin]
// problem is read from column t cin_store + c (row stride ld), so padded rows and channels are never touched.
template <bool CONV>
__global__ void __launch_bounds__(256) lora_grad_partial_kernel(const float* __restrict__ dw, int N, int K,
                                                                const float* __restrict__ up,
                                                                const float* __restrict__ down, int r,
                                                                float* __restrict__ du_part,
                                                                float* __restrict__ dd_part, int ld, int cin,
                                                                int cin_store) {
  __shared__ float tile[LR_RT][LR_CT + 1];
  const int ct = blockIdx.x, rt = blockIdx.y, tid = threadIdx.x;
  const int i0 = rt * LR_RT, j0 = ct * LR_CT;
  const int nr = min(LR_RT, N - i0), nc = min(LR_CT, K - j0);
  if constexpr (CONV) {
    const int t = (j0 + tid) / cin;
    const int src = t * cin_store + (j0 + tid - t * cin);
    for (int i = 0; i < LR_RT; ++i) tile[i][tid] = (i < nr && tid < nc) ? dw[(int64_t)(i0 + i) * ld + src] : 0.f;
  } else {
    for (int i = 0; i < LR_RT; ++i) tile[i][tid] = (i < nr && tid < nc) ? dw[(int64_t)(i0 + i) * K + j0 + tid] : 0.f;
  }
  __syncthreads();
  if (tid < nc) {
    for (int t = 0; t < r; ++t) {
      float acc = 0.f;
      for (int i = 0; i < nr; ++i) acc += up[(int64_t)(i0 + i) * r + t] * tile[i][tid];
      dd_part[((int64_t)rt * r + t) * K + j0 + tid] = acc;
    }
  }
  for (int o = tid; o < nr * r; o += 256) {
    const int i = o / r, t = o - i * r;
    const float* dn = down + (int64_t)t * K + j0;
    float acc = 0.f;
    for (int c = 0; c < nc; ++c) acc += tile[i][c] * dn[c];
    du_part[((int64_t)ct * N + i0 + i) * r + t] = acc;
  }
}

__global__ void __launch_bounds__(256) lora_grad_reduce_kernel(const float* __restrict__ du_part,
                                                               const float* __restrict__ dd_part, int N, int K, int r,
                                                               int nct, int nrt, float scale, float* __restrict__ gu,
                                                               float* __restrict__ gd, int gd_accumulate) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nu = (int64_t)N * r, nd = (int64_t)r * K;
  if (o < nu) {
    float acc = 0.f;
    for (int c = 0; c < nct; ++c) acc += du_part[(int64_t)c * nu + o];
    gu[o] += scale * acc;
  } else if (o < nu + nd) {
    const int64_t q = o - nu;
    float acc = 0.f;
    for (int c = 0; c < nrt; ++c) acc += dd_part[(int64_t)c * nd + q];
    if (gd_accumulate) gd[q] += scale * acc;
    else gd[q] = scale * acc;  // (Tucker: dT, a workspace)
  }
}

// ---------------------------------------------------------------------------------------------------------------- LoKr
constexpr int LK_GROUP = 2048;  // w2 elements per workgroup (8 per thread)

// w2 = w2_a . w2_b (low-rank form), [out_k, in_n]
__global__ void __launch_bounds__(256) lokr_form_w2_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           int out_k, int in_n, int r, float* __restrict__ w2) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)out_k * in_n) return;
  const int k = (int)(e / in_n), l = (int)(e - (int64_t)k * in_n);
  float acc = 0.f;
  for (int t = 0; t < r; ++t) acc += a[(int64_t)k * r + t] * b[(int64_t)t * in_n + l];
  w2[e] = acc;
}

// workgroup (g, i): the w2 elements [g*2048, (g+1)*2048) of every Kronecker block (i, j), j = 0..in_m-1.
//   p1[(i*G + g)*in_m + j] = sum_{e in group} dW[i,k,j,l] w2[e]      (partial of dw1[i,j])
//   p2[i*W2 + e]           = sum_j w1[i,j] dW[i,k,j,l]                (partial of dw2[e])
// CONV (section 4.41): w2 is [out_k, 9, in_n]; its element (k, t, l) of block (i, j) is dW[i out_k + k][t cin_store + j in_n + l]
// of the stored convolution gradient (K: its row stride 9 cin_store).
template <bool CONV>
__global__ void __launch_bounds__(256) lokr_grad_partial_kernel(const float* __restrict__ dw, int K, int out_k,
                                                                int in_n, int in_m, const float* __restrict__ w1,
                                                                const float* __restrict__ w2, float* __restrict__ p1,
                                                                float* __restrict__ p2, int cin_store) {
  __shared__ float red[4];
  const int g = blockIdx.x, i = blockIdx.y, G = gridDim.x, tid = threadIdx.x;
  const int W2 = CONV ? 9 * out_k * in_n : out_k * in_n;
  float acc[8], w2v[8];
  int64_t roff[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = g * LK_GROUP + q * 256 + tid;
    acc[q] = 0.f;
    w2v[q] = 0.f;
    roff[q] = -1;
    if (e < W2) {
      if constexpr (CONV) {
        const int k = e / (9 * in_n), tl = e - k * 9 * in_n, t = tl / in_n;
        roff[q] = (int64_t)(i * out_k + k) * K + t * cin_store + (tl - t * in_n);
      } else {
        const int k = e / in_n, l = e - k * in_n;
        roff[q] = (int64_t)(i * out_k + k) * K + l;
      }
      w2v[q] = w2[e];
    }
  }
  for (int j = 0; j < in_m; ++j) {
    const float w1v = w1[(int64_t)i * in_m + j];
    float dot = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (roff[q] >= 0) {
        const float v = dw[roff[q] + (int64_t)j * in_n];
        acc[q] += w1v * v;
        dot += v * w2v[q];
      }
    }
    dot = block_sum<4>(dot, red);
    if (tid == 0) p1[((int64_t)i * G + g) * in_m + j] = dot;
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = g * LK_GROUP + q * 256 + tid;
    if (e < W2) p2[(int64_t)i * W2 + e] = acc[q];
  }
}

// dw1[i,j] += s sum_g p1;  dw2[e] (+)= s sum_i p2 -- into the gradient (full w2) or into the workspace (low-rank form)
__global__ void __launch_bounds__(256) lokr_grad_reduce_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                               int out_l, int in_m, int W2, int G, float scale,
                                                               float* __restrict__ g1, float* __restrict__ g2,
                                                               int g2_accumulate) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n1 = (int64_t)out_l * in_m;
  if (o < n1) {
    const int i = (int)(o / in_m), j = (int)(o - (int64_t)i * in_m);
    float acc = 0.f;
    for (int g = 0; g < G; ++g) acc += p1[((int64_t)i * G + g) * in_m + j];
    g1[o] += scale * acc;
  } else if (o < n1 + W2) {
    const int64_t e = o - n1;
    float acc = 0.f;
    for (int i = 0; i < out_l; ++i) acc += p2[(int64_t)i * W2 + e];
    if (g2_accumulate) g2[e] += scale * acc;
    else g2[e] = scale * acc;
  }
}

// low-rank chain: d_w2a[k,t] += sum_l dw2[k,l] w2_b[t,l];  d_w2b[t,l] += sum_k w2_a[k,t] dw2[k,l]
__global__ void __launch_bounds__(256) lokr_grad_lowrank_kernel(const float* __restrict__ dw2, const float* __restrict__ a,
                                                                const float* __restrict__ b, int out_k, int in_n, int r,
                                                                float* __restrict__ ga, float* __restrict__ gb) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t na = (int64_t)out_k * r, nb = (int64_t)r * in_n;
  if (o < na) {
    const int k = (int)(o / r), t = (int)(o - (int64_t)k * r);
    float acc = 0.f;
    for (int l = 0; l < in_n; ++l) acc += dw2[(int64_t)k * in_n + l] * b[(int64_t)t * in_n + l];
    ga[o] += acc;
  } else if (o < na + nb) {
    const int64_t q = o - na;
    const int t = (int)(q / in_n), l = (int)(q - (int64_t)t * in_n);
    float acc = 0.f;
    for (int k = 0; k < out_k; ++k) acc += a[(int64_t)k * r + t] * dw2[(int64_t)k * in_n + l];
    gb[q] += acc;
  }
}

// workspace of uwu_adapter_grad in floats (mirrored by uwudiff_amd/adapters.py: grad_ws_elems)
int64_t ad_grad_ws_elems(int kind, int64_t N, int64_t K, int r, int out_k, int in_n) {
  if (kind == UWU_ADAPTER_LORA) {
    const int64_t nct = (K + LR_CT - 1) / LR_CT, nrt = (N + LR_RT - 1) / LR_RT;
    return nct * N * r + nrt * r * K;
  }
  const int64_t out_l = N / out_k, in_m = K / in_n, W2 = (int64_t)out_k * in_n;
  const int64_t G = (W2 + LK_GROUP - 1) / LK_GROUP;
  return out_l * G * in_m + out_l * W2 + 2 * W2;
}

// ---------------------------------------------------------------------------------------------------------------- DoRA
// Weight decomposition: W' = m V / n, V = base + delta, n = ||V row or column||_2 + eps.
// A decomposed segment row has 16 fields: the 13 of the merge, then dora_off (m in p), norm_off (n in norms), orient
// (1: one magnitude per row, wd_on_out; 0: one per column).
constexpr int AD_DNF = 16;
constexpr int AD_ROWS_WG = 4;    // row orientation: one wave per row, four rows per workgroup
constexpr int AD_COLS_WG = 64;   // column orientation: one lane per column, the four waves stride the rows
constexpr int AD_COL_RT = 256;   // rows per workgroup of the column-orientation gradient stage
constexpr double AD_EPS = 1.1920928955078125e-07;  // 2^-23 = torch.finfo(torch.float32).eps

// V = base + delta with the sum rounded on its own (never contracted into delta's last multiplication): the norm pass, the
// merge and both passes of the gradient stage must see the same V bit for bit -- the gradient's bracket cancels on it
__device__ __forceinline__ float ad_v(float b, const int64_t* __restrict__ row, const float* __restrict__ p, int e) {
  return __fadd_rn(b, ad_delta(row, p, e));
}

struct AdSeg {
  int64_t f[AD_DNF];
};

__device__ __forceinline__ double wave_sum_f64(double v) {  // xor butterfly: a fixed order, the sum in every lane
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct AdSums {
  double ss, t;  // <V, V> and <G, V> (t: only with G)
};

// the sums over the row `i`; one wave, the result in every lane
__device__ __forceinline__ AdSums ad_row_sums(const int64_t* __restrict__ row, const float* __restrict__ base,
                                              const float* __restrict__ p, const float* __restrict__ G, int i, int cols,
                                              int lane) {
  const int e0 = i * cols;
  AdSums a = {0.0, 0.0};
  if ((cols & 3) == 0) {
    for (int j = 4 * lane; j < cols; j += 4 * UWU_WAVE) {
      f32x4 v = load4(base + e0 + j);
      f32x4 w = {0.f, 0.f, 0.f, 0.f};
      if (G) w = load4(G + e0 + j);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double x = (double)ad_v(v[q], row, p, e0 + j + q);
        a.ss += x * x;
        a.t += x * (double)w[q];
      }
    }
  } else {
    for (int j = lane; j < cols; j += UWU_WAVE) {
      const double x = (double)ad_v(base[e0 + j], row, p, e0 + j);
      a.ss += x * x;
      if (G) a.t += x * (double)G[e0 + j];
    }
  }
  a.ss = wave_sum_f64(a.ss);
  if (G) a.t = wave_sum_f64(a.t);
  return a;
}

// the sums over the rows [i0, i1) of column j: the four waves take every fourth row, their sums are added in wave order
// through `red` [2][4][64].  Valid where j < cols; every thread of the workgroup must call it.
__device__ __forceinline__ AdSums ad_col_sums(const int64_t* __restrict__ row, const float* __restrict__ base,
                                              const float* __restrict__ p, const float* __restrict__ G, int i0, int i1,
                                              int cols, int j, double (*red)[4][AD_COLS_WG]) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  AdSums a = {0.0, 0.0};
  if (j < cols) {
    for (int i = i0 + w; i < i1; i += 4) {
      const int e = i * cols + j;
      const double x = (double)ad_v(base[e], row, p, e);
      a.ss += x * x;
      if (G) a.t += x * (double)G[e];
    }
  }
  red[0][w][lane] = a.ss;
  red[1][w][lane] = a.t;
  __syncthreads();
  a.ss = ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
  a.t = ((red[1][0][lane] + red[1][1][lane]) + red[1][2][lane]) + red[1][3][lane];
  return a;
}

__device__ __forceinline__ int ad_find_segment(const int64_t* __restrict__ blk_start, int nseg, int64_t bid) {
  int lo = 0, hi = nseg;  // blk_start[lo] <= bid < blk_start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blk_start[mid] <= bid) lo = mid;
    else hi = mid;
  }
  return lo;
}

// norms[norm_off + a] = ||V[a, :]|| + eps (orient 1) or ||V[:, a]|| + eps (orient 0) of every decomposed segment.  The sum of
// squares is added in double in an order the shape alone fixes: lane partials, then the butterfly (rows); wave partials,
// then wave order (columns).
__global__ void __launch_bounds__(256) adapter_dora_norms_kernel(const float* __restrict__ base, const float* __restrict__ p,
                                                                 const int64_t* __restrict__ table,
                                                                 const int64_t* __restrict__ blk_start, int nseg,
                                                                 float* __restrict__ norms) {
  __shared__ double red[2][4][AD_COLS_WG];
  const int64_t bid = blockIdx.x;
  const int lo = ad_find_segment(blk_start, nseg, bid);
  const int64_t* row = table + (int64_t)lo * AD_DNF;
  const int rows = (int)row[1], cols = (int)row[2];
  const int b = (int)(bid - blk_start[lo]);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* bs = base + row[3];
  float* out = norms + row[14];
  if (row[15]) {
    const int i = b * AD_ROWS_WG + w;
    if (i >= rows) return;
    const AdSums a = ad_row_sums(row, bs, p, nullptr, i, cols, lane);
    if (lane == 0) out[i] = (float)(sqrt(a.ss) + AD_EPS);
  } else {
    const int j = b * AD_COLS_WG + lane;
    const AdSums a = ad_col_sums(row, bs, p, nullptr, 0, rows, cols, j, red);
    if (w == 0 && j < cols) out[j] = (float)(sqrt(a.ss) + AD_EPS);
  }
}

// W' = (base + delta) m / n: the merge kernel with one more factor per row or column
__global__ void __launch_bounds__(256) adapter_dora_merge_kernel(const float* __restrict__ base, const float* __restrict__ p,
                                                                 const int64_t* __restrict__ table,
                                                                 const int64_t* __restrict__ blk_start, int nseg,
                                                                 const float* __restrict__ norms, float* __restrict__ eff,
                                                                 bf16_t* __restrict__ shadow) {
  const int64_t bid = blockIdx.x;
  const int lo = ad_find_segment(blk_start, nseg, bid);
  const int64_t* row = table + (int64_t)lo * AD_DNF;
  const int cols = (int)row[2];
  const int n = (int)(row[1] * row[2]);
  const int64_t boff = row[3], eoff = row[4], soff = row[5];
  const float* m = p + row[13];
  const float* nr = norms + row[14];
  const bool by_row = row[15] != 0;
  const int e0 = (int)(bid - blk_start[lo]) * AD_MERGE_ELEMS;
#pragma unroll
  for (int it = 0; it < AD_MERGE_ELEMS / 1024; ++it) {
    const int e = e0 + it * 1024 + 4 * threadIdx.x;
    if (e >= n) break;
    if (e + 4 <= n) {
      f32x4 v = load4(base + boff + e);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = (e + q) / cols;
        const int a = by_row ? i : e + q - i * cols;
        v[q] = ad_v(v[q], row, p, e + q) * (m[a] / nr[a]);
      }
      if (eoff >= 0) store4(eff + eoff + e, v);
      if (shadow && soff >= 0) store4(shadow + soff + e, v);
    } else {
      for (int q = e; q < n; ++q) {
        const int i = q / cols;
        const int a = by_row ? i : q - i * cols;
        const float v = ad_v(base[boff + q], row, p, q) * (m[a] / nr[a]);
        if (eoff >= 0) eff[eoff + q] = v;
        if (shadow && soff >= 0) shadow[soff + q] = (bf16_t)v;
      }
    }
  }
}

// dV = s (G - V t / (n u)), s = m / n, dm = t / n with the n of the merge.  Where one element carries its row or column,
// G - V t / (n u) is the difference of two nearly equal numbers (for a single element: G eps / n), and the fp32 n no longer
// tells u = n - eps apart from n.  So u^2 = <V, V> is summed again next to t, and the term is evaluated in double as
//   (G - V a) + V a eps / n,  a = t / u^2   (a = 0 where u = 0)
// whose first part cancels exactly where it must.
struct AdCoef {
  double a, b;  // a = t / u^2, b = a eps / n
  float s, dm;
};
__device__ __forceinline__ AdCoef ad_dora_coeffs(float n, float m, AdSums sums) {
  AdCoef c;
  c.a = sums.ss > 0.0 ? sums.t / sums.ss : 0.0;
  c.b = c.a * (AD_EPS / (double)n);
  c.s = m / n;
  c.dm = (float)(sums.t / (double)n);
  return c;
}
__device__ __forceinline__ float ad_dora_dv(AdCoef c, float g, float v) {
  const double va = (double)v * c.a;
  return c.s * (float)(((double)g - va) + (double)v * c.b);
}

// row orientation: one wave per row.  t = <G row, V row>, then the row of G is rewritten; V is recomputed both times (the
// second read of base and G is served by the cache this wave has just filled).
__global__ void __launch_bounds__(256) adapter_dora_grad_row_kernel(float* __restrict__ G, const float* __restrict__ base,
                                                                    const float* __restrict__ p, float* __restrict__ g,
                                                                    const float* __restrict__ norms, AdSeg seg) {
  const int64_t* row = seg.f;
  const int rows = (int)row[1], cols = (int)row[2];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * AD_ROWS_WG + w;
  if (i >= rows) return;
  const AdCoef c = ad_dora_coeffs(norms[row[14] + i], p[row[13] + i], ad_row_sums(row, base, p, G, i, cols, lane));
  const int e0 = i * cols;
  if ((cols & 3) == 0) {
    for (int j = 4 * lane; j < cols; j += 4 * UWU_WAVE) {
      const f32x4 v = load4(base + e0 + j);
      f32x4 gv = load4(G + e0 + j);
#pragma unroll
      for (int q = 0; q < 4; ++q) gv[q] = ad_dora_dv(c, gv[q], ad_v(v[q], row, p, e0 + j + q));
      store4(G + e0 + j, gv);
    }
  } else {
    for (int j = lane; j < cols; j += UWU_WAVE)
      G[e0 + j] = ad_dora_dv(c, G[e0 + j], ad_v(base[e0 + j], row, p, e0 + j));
  }
  if (lane == 0) g[row[13] + i] += c.dm;
}

// column orientation, stage 1: part[rt][j] = the two sums over the 256 rows of tile rt
__global__ void __launch_bounds__(256) adapter_dora_grad_col_partial_kernel(const float* __restrict__ G,
                                                                            const float* __restrict__ base,
                                                                            const float* __restrict__ p,
                                                                            AdSums* __restrict__ part, AdSeg seg) {
  __shared__ double red[2][4][AD_COLS_WG];
  const int64_t* row = seg.f;
  const int rows = (int)row[1], cols = (int)row[2];
  const int j = blockIdx.x * AD_COLS_WG + (threadIdx.x & 63);
  const int i0 = blockIdx.y * AD_COL_RT, i1 = min(rows, i0 + AD_COL_RT);
  const AdSums a = ad_col_sums(row, base, p, G, i0, i1, cols, j, red);
  if (threadIdx.x < 64 && j < cols) part[(int64_t)blockIdx.y * cols + j] = a;
}

// stage 2: the sums of column j = the tile partials added in tile order (every workgroup of a column group computes the same sum), then the
// workgroup's 256 x 64 tile of G is rewritten; the first row tile adds dm
__global__ void __launch_bounds__(256) adapter_dora_grad_col_apply_kernel(float* __restrict__ G,
                                                                          const float* __restrict__ base,
                                                                          const float* __restrict__ p, float* __restrict__ g,
                                                                          const float* __restrict__ norms,
                                                                          const AdSums* __restrict__ part, int nrt,
                                                                          AdSeg seg) {
  const int64_t* row = seg.f;
  const int rows = (int)row[1], cols = (int)row[2];
  const int w = threadIdx.x >> 6;
  const int j = blockIdx.x * AD_COLS_WG + (threadIdx.x & 63);
  if (j >= cols) return;
  AdSums sums = {0.0, 0.0};
  for (int q = 0; q < nrt; ++q) {
    const AdSums a = part[(int64_t)q * cols + j];
    sums.ss += a.ss;
    sums.t += a.t;
  }
  const AdCoef c = ad_dora_coeffs(norms[row[14] + j], p[row[13] + j], sums);
  const int i0 = blockIdx.y * AD_COL_RT, i1 = min(rows, i0 + AD_COL_RT);
  for (int i = i0 + w; i < i1; i += 4) {
    const int e = i * cols + j;
    G[e] = ad_dora_dv(c, G[e], ad_v(base[e], row, p, e));
  }
  if (blockIdx.y == 0 && w == 0) g[row[13] + j] += c.dm;
}

// workspace of uwu_adapter_dora_grad in floats (mirrored by uwudiff_amd/adapters.py: dora_grad_ws_elems)
int64_t ad_dora_grad_ws_elems(int64_t N, int64_t K, int wd_on_out) {
  return wd_on_out ? 0 : 4 * ((N + AD_COL_RT - 1) / AD_COL_RT) * K;
}

// the host copy of a decomposed segment table: every row is checked before anything is launched
const char* ad_dora_check_rows(const int64_t* t, int nseg) {
  for (int s = 0; s < nseg; ++s) {
    const int64_t* r = t + (int64_t)s * AD_DNF;
    if (r[0] != UWU_ADAPTER_LORA && r[0] != UWU_ADAPTER_LOKR && r[0] != UWU_ADAPTER_LOKR_LOWRANK) return "kind";
    if (r[1] < 1 || r[2] < 1 || r[1] * r[2] >= (1ll << 31)) return "shape";
    if (r[0] != UWU_ADAPTER_LOKR && (r[9] < 1 || r[9] > AD_MAX_RANK)) return "rank outside [1, 128]";
    if (r[0] != UWU_ADAPTER_LORA && (r[10] < 1 || r[11] < 1 || r[1] % r[10] || r[2] % r[11])) return "LoKr factors";
    if (r[3] < 0 || r[3] % 64 || (r[4] >= 0 && r[4] % 64) || (r[5] >= 0 && r[5] % 64)) return "misaligned base / eff / shadow offset";
    if (r[6] < 0 || r[7] < 0 || r[8] < 0 || r[13] < 0 || r[14] < 0) return "negative offset";
    if (r[15] != 0 && r[15] != 1) return "orientation";
  }
  return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------- conv
// Convolution adapters.  The stored weight is [cout_store, 9, cin_store]; the adapter tensors are
// tap-major in the true sizes, so plain LoRA is the 2-D problem [cout, 9 cin] read through a column map, Tucker is LoRA
// with down := T = mid . dn (formed first), and LoKr's w2 carries the taps between its two axes.  A segment row has 17
// fields: the 13 of the merge, then cout, cin, cin_store, t_off (T in the workspace).
constexpr int AD_CNF = 17;

__device__ __forceinline__ float ad_conv_delta(const int64_t* __restrict__ row, const float* __restrict__ p,
                                               const float* __restrict__ tws, int e) {
  const int kind = (int)row[0];
  const int cols = (int)row[2];
  const int cout = (int)row[13], cin = (int)row[14], cs = (int)row[15];
  const int o = e / cols, j = e - o * cols;
  const int t = j / cs, c = j - t * cs;
  if (o >= cout || c >= cin) return 0.f;  // padding: base + 0 stays the zero it holds
  const float scale = __int_as_float((int)row[12]);
  const int r = (int)row[9];
  if (kind == UWU_ADAPTER_CONV_LORA || kind == UWU_ADAPTER_CONV_TUCKER) {
    const float* up = p + row[6] + (int64_t)o * r;
    const float* down = (kind == UWU_ADAPTER_CONV_TUCKER ? tws + row[16] : p + row[7]) + t * cin + c;
    const int64_t ld = 9 * (int64_t)cin;
    float acc = 0.f;
    for (int i = 0; i < r; ++i) acc += up[i] * down[i * ld];
    return acc * scale;
  }
  const int out_k = (int)row[10], in_n = (int)row[11], in_m = cin / in_n;
  const int a = o / out_k, k = o - a * out_k, b = c / in_n, l = c - b * in_n;
  const float w1 = p[row[6] + (int64_t)a * in_m + b];
  float w2;
  if (kind == UWU_ADAPTER_CONV_LOKR) {
    w2 = p[row[7] + ((int64_t)k * 9 + t) * in_n + l];
  } else {  // w2 = w2_a [out_k, r] . w2_b [r, 9, in_n]
    const float* wa = p + row[7] + (int64_t)k * r;
    const float* wb = p + row[8] + t * in_n + l;
    w2 = 0.f;
    for (int i = 0; i < r; ++i) w2 += wa[i] * wb[(int64_t)i * 9 * in_n];
  }
  return (w1 * w2) * scale;
}

// T[(i, t), c] = sum_j mid[(i, t), j] dn[j, c] of every Tucker segment: one thread per element of T
__global__ void __launch_bounds__(256) adapter_conv_form_kernel(const float* __restrict__ p, const int64_t* __restrict__ table,
                                                                const int64_t* __restrict__ form_start, int nseg,
                                                                float* __restrict__ tws) {
  const int64_t bid = blockIdx.x;
  const int lo = ad_find_segment(form_start, nseg, bid);
  const int64_t* row = table + (int64_t)lo * AD_CNF;
  const int r = (int)row[9], cin = (int)row[14];
  const int e = (int)(bid - form_start[lo]) * 256 + threadIdx.x;
  if (row[0] != UWU_ADAPTER_CONV_TUCKER || e >= 9 * r * cin) return;
  const int it = e / cin, c = e - it * cin;
  const float* mid = p + row[8] + (int64_t)it * r;
  const float* dn = p + row[7] + c;
  float acc = 0.f;
  for (int j = 0; j < r; ++j) acc += mid[j] * dn[(int64_t)j * cin];
  tws[row[16] + e] = acc;
}

__global__ void __launch_bounds__(256) adapter_conv_merge_kernel(const float* __restrict__ base, const float* __restrict__ p,
                                                                 const int64_t* __restrict__ table,
                                                                 const int64_t* __restrict__ blk_start, int nseg,
                                                                 const float* __restrict__ tws, float* __restrict__ eff,
                                                                 bf16_t* __restrict__ shadow) {
  const int64_t bid = blockIdx.x;
  const int lo = ad_find_segment(blk_start, nseg, bid);
  const int64_t* row = table + (int64_t)lo * AD_CNF;
  const int n = (int)(row[1] * row[2]);
  const int64_t boff = row[3], eoff = row[4], soff = row[5];
  const int e0 = (int)(bid - blk_start[lo]) * AD_MERGE_ELEMS;
#pragma unroll
  for (int it = 0; it < AD_MERGE_ELEMS / 1024; ++it) {
    const int e = e0 + it * 1024 + 4 * threadIdx.x;
    if (e >= n) break;
    if (e + 4 <= n) {
      f32x4 v = load4(base + boff + e);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] += ad_conv_delta(row, p, tws, e + q);
      if (eoff >= 0) store4(eff + eoff + e, v);
      if (shadow && soff >= 0) store4(shadow + soff + e, v);
    } else {
      for (int q = e; q < n; ++q) {
        const float v = base[boff + q] + ad_conv_delta(row, p, tws, q);
        if (eoff >= 0) eff[eoff + q] = v;
        if (shadow && soff >= 0) shadow[soff + q] = (bf16_t)v;
      }
    }
  }
}

bool ad_is_conv_kind(int64_t k) { return k >= UWU_ADAPTER_CONV_LORA && k <= UWU_ADAPTER_CONV_LOKR_LOWRANK; }
bool ad_conv_is_lokr(int64_t k) { return k == UWU_ADAPTER_CONV_LOKR || k == UWU_ADAPTER_CONV_LOKR_LOWRANK; }

// the host copy of a convolution segment table: every row is checked before anything is launched
const char* ad_conv_check_rows(const int64_t* t, int nseg, int64_t tws_elems) {
  for (int s = 0; s < nseg; ++s) {
    const int64_t* r = t + (int64_t)s * AD_CNF;
    if (!ad_is_conv_kind(r[0])) return "kind";
    if (r[1] < 1 || r[2] < 1 || r[1] * r[2] >= (1ll << 31)) return "shape";
    if (r[15] < 1 || r[2] != 9 * r[15] || r[13] < 1 || r[13] > r[1] || r[14] < 1 || r[14] > r[15]) return "channels";
    if (r[0] != UWU_ADAPTER_CONV_LOKR && (r[9] < 1 || r[9] > AD_MAX_RANK)) return "rank outside [1, 128]";
    if (ad_conv_is_lokr(r[0]) && (r[10] < 1 || r[11] < 1 || r[13] % r[10] || r[14] % r[11])) return "LoKr factors";
    if (r[3] < 0 || r[3] % 64 || (r[4] >= 0 && r[4] % 64) || (r[5] >= 0 && r[5] % 64)) return "misaligned base / eff / shadow offset";
    if (r[6] < 0 || r[7] < 0 || r[8] < 0) return "negative offset";
    if (r[0] == UWU_ADAPTER_CONV_TUCKER && (r[16] < 0 || r[16] + 9 * r[9] * r[14] > tws_elems)) return "T outside the workspace";
  }
  return nullptr;
}

// workspace of uwu_adapter_conv_grad in floats (mirrored by uwudiff_amd/adapters.py: conv_grad_ws_elems)
int64_t ad_conv_grad_ws_elems(int kind, int64_t cout, int64_t cin, int r, int out_k, int in_n) {
  const int64_t K = 9 * cin;
  if (!ad_conv_is_lokr(kind)) {
    const int64_t nct = (K + LR_CT - 1) / LR_CT, nrt = (cout + LR_RT - 1) / LR_RT;
    return nct * cout * r + nrt * r * K + (kind == UWU_ADAPTER_CONV_TUCKER ? 2 * r * K : 0);
  }
  const int64_t out_l = cout / out_k, in_m = cin / in_n, W2 = 9 * (int64_t)out_k * in_n;
  const int64_t G = (W2 + LK_GROUP - 1) / LK_GROUP;
  return out_l * G * in_m + out_l * W2 + 2 * W2;
}

}  // namespace

extern "C" int uwu_adapter_conv_merge(const float* base, const float* p, const int64_t* table, const int64_t* table_host,
                                      const int64_t* blk_start, const int64_t* form_start, int nseg, int64_t nblocks,
                                      int64_t nform, float* tws, int64_t tws_elems, float* eff, void* shadow, void* stream) {
  UWU_CHECK_ARG(base && p && table && table_host && blk_start && nseg > 0 && nblocks > 0 && nblocks < (1ll << 31) &&
                    nform >= 0 && nform < (1ll << 31) && tws_elems >= 0,
                "adapter_conv_merge: bad args (nseg=%d nblocks=%lld nform=%lld)", nseg, (long long)nblocks, (long long)nform);
  UWU_CHECK_ARG(eff || shadow, "adapter_conv_merge: no output");
  const char* why = ad_conv_check_rows(table_host, nseg, tws ? tws_elems : 0);
  UWU_CHECK_ARG(!why, "adapter_conv_merge: bad segment table: %s", why);
  int64_t want = 0, wantf = 0;
  for (int s = 0; s < nseg; ++s) {
    const int64_t* r = table_host + (int64_t)s * AD_CNF;
    want += (r[1] * r[2] + AD_MERGE_ELEMS - 1) / AD_MERGE_ELEMS;
    if (r[0] == UWU_ADAPTER_CONV_TUCKER) wantf += (9 * r[9] * r[14] + 255) / 256;
  }
  UWU_CHECK_ARG(want == nblocks && wantf == nform && (nform == 0 || form_start),
                "adapter_conv_merge: nblocks %lld / nform %lld, the table needs %lld / %lld", (long long)nblocks,
                (long long)nform, (long long)want, (long long)wantf);
  hipStream_t st = (hipStream_t)stream;
  if (nform > 0)
    hipLaunchKernelGGL(adapter_conv_form_kernel, dim3((unsigned)nform), dim3(256), 0, st, p, table, form_start, nseg, tws);
  hipLaunchKernelGGL(adapter_conv_merge_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, base, p, table, blk_start, nseg,
                     tws, eff, (bf16_t*)shadow);
  UWU_LAUNCH_CHECK("adapter_conv_merge");
  return UWU_OK;
}

extern "C" int uwu_adapter_conv_grad(const float* dw, int64_t cout_store, int64_t cin_store, int64_t cout, int64_t cin,
                                     int kind, const float* p, float* g, int64_t pa, int64_t pb, int64_t pc, int r, int out_k,
                                     int in_n, float scale, float* ws, int64_t ws_elems, void* stream) {
  UWU_CHECK_ARG(dw && p && g && ws && cout >= 1 && cout <= cout_store && cin >= 1 && cin <= cin_store &&
                    cout_store < (1 << 24) && cin_store < (1 << 24) && cout_store * 9 * cin_store < (1ll << 31),
                "adapter_conv_grad: bad args");
  UWU_CHECK_ARG(ad_is_conv_kind(kind), "adapter_conv_grad: bad kind %d", kind);
  UWU_CHECK_ARG(pa >= 0 && pb >= 0 && pc >= 0, "adapter_conv_grad: negative offset");
  const bool lokr = ad_conv_is_lokr(kind);
  UWU_CHECK_ARG(kind == UWU_ADAPTER_CONV_LOKR || (r >= 1 && r <= AD_MAX_RANK), "adapter_conv_grad: rank %d outside [1, %d]", r,
                AD_MAX_RANK);
  UWU_CHECK_ARG(!lokr || (out_k >= 1 && in_n >= 1 && cout % out_k == 0 && cin % in_n == 0),
                "adapter_conv_grad: LoKr shape %lldx%lld / (%d, %d)", (long long)cout, (long long)cin, out_k, in_n);
  const int64_t need = ad_conv_grad_ws_elems(kind, cout, cin, r, out_k, in_n);
  UWU_CHECK_ARG(ws_elems >= need, "adapter_conv_grad: workspace %lld < %lld floats", (long long)ws_elems, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  const int N = (int)cout, K = (int)(9 * cin), ld = (int)(9 * cin_store);
  if (!lokr) {
    const bool tucker = kind == UWU_ADAPTER_CONV_TUCKER;
    const int nct = (K + LR_CT - 1) / LR_CT, nrt = (N + LR_RT - 1) / LR_RT;
    float* du = ws;
    float* dd = du + (int64_t)nct * N * r;
    float* T = dd + (int64_t)nrt * r * K;  // Tucker: T [r, 9, cin], then dT
    float* dT = T + (int64_t)r * K;
    const float* down = p + pb;
    if (tucker) {  // T [(i, t), c] = mid [(i, t), j] . dn [j, c]: the low-rank product of LoKr with out_k = 9 r, in_n = cin
      hipLaunchKernelGGL(lokr_form_w2_kernel, dim3((unsigned)(((int64_t)r * K + 255) / 256)), dim3(256), 0, st, p + pc, p + pb,
                         9 * r, (int)cin, r, T);
      down = T;
    }
    hipLaunchKernelGGL(lora_grad_partial_kernel<true>, dim3(nct, nrt), dim3(256), 0, st, dw, N, K, p + pa, down, r, du, dd, ld,
                       (int)cin, (int)cin_store);
    const int64_t nout = (int64_t)N * r + (int64_t)r * K;
    hipLaunchKernelGGL(lora_grad_reduce_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, du, dd, N, K, r, nct,
                       nrt, scale, g + pa, tucker ? dT : g + pb, tucker ? 0 : 1);
    if (tucker) {  // d_mid[(i, t), j] += sum_c dT[(i, t), c] dn[j, c];  d_dn[j, c] += sum_(i, t) mid[(i, t), j] dT[(i, t), c]
      const int64_t n2 = (int64_t)9 * r * r + (int64_t)r * cin;
      hipLaunchKernelGGL(lokr_grad_lowrank_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, dT, p + pc, p + pb,
                         9 * r, (int)cin, r, g + pc, g + pb);
    }
    UWU_LAUNCH_CHECK("adapter_conv_grad");
    return UWU_OK;
  }
  const bool low = kind == UWU_ADAPTER_CONV_LOKR_LOWRANK;
  const int out_l = (int)(cout / out_k), in_m = (int)(cin / in_n);
  const int W2 = 9 * out_k * in_n;
  const int G = (W2 + LK_GROUP - 1) / LK_GROUP;
  float* p1 = ws;
  float* p2 = p1 + (int64_t)out_l * G * in_m;
  float* w2f = p2 + (int64_t)out_l * W2;  // low-rank: the formed w2, then dw2
  float* dw2 = w2f + W2;
  const float* w2 = p + pb;
  if (low) {
    hipLaunchKernelGGL(lokr_form_w2_kernel, dim3((W2 + 255) / 256), dim3(256), 0, st, p + pb, p + pc, out_k, 9 * in_n, r, w2f);
    w2 = w2f;
  }
  hipLaunchKernelGGL(lokr_grad_partial_kernel<true>, dim3(G, out_l), dim3(256), 0, st, dw, ld, out_k, in_n, in_m, p + pa, w2,
                     p1, p2, (int)cin_store);
  const int64_t nout = (int64_t)out_l * in_m + W2;
  hipLaunchKernelGGL(lokr_grad_reduce_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, p1, p2, out_l, in_m, W2,
                     G, scale, g + pa, low ? dw2 : g + pb, low ? 0 : 1);
  if (low) {
    const int64_t n2 = (int64_t)out_k * r + (int64_t)r * 9 * in_n;
    hipLaunchKernelGGL(lokr_grad_lowrank_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, dw2, p + pb, p + pc,
                       out_k, 9 * in_n, r, g + pb, g + pc);
  }
  UWU_LAUNCH_CHECK("adapter_conv_grad");
  return UWU_OK;
}

extern "C" int uwu_adapter_merge(const float* base, const float* p, const int64_t* table, const int64_t* blk_start,
                                 int nseg, int64_t nblocks, float* eff, void* shadow, void* stream) {
  UWU_CHECK_ARG(base && p && table && blk_start && nseg > 0 && nblocks > 0 && nblocks < (1ll << 31),
                "adapter_merge: bad args (nseg=%d nblocks=%lld)", nseg, (long long)nblocks);
  UWU_CHECK_ARG(eff || shadow, "adapter_merge: no output");
  hipLaunchKernelGGL(adapter_merge_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, base, p, table,
                     blk_start, nseg, eff, (bf16_t*)shadow);
  UWU_LAUNCH_CHECK("adapter_merge");
  return UWU_OK;
}

extern "C" int uwu_adapter_grad(const float* dw, int64_t N, int64_t K, int kind, const float* p, float* g, int64_t pa,
                                int64_t pb, int64_t pc, int r, int out_k, int in_n, float scale, float* ws,
                                int64_t ws_elems, void* stream) {
  UWU_CHECK_ARG(dw && p && g && ws && N > 0 && K > 0 && N < (1 << 30) && K < (1 << 30) && N * K < (1ll << 31),
                "adapter_grad: bad args");
  hipStream_t st = (hipStream_t)stream;
  if (kind == UWU_ADAPTER_LORA) {
    UWU_CHECK_ARG(r >= 1 && r <= AD_MAX_RANK, "adapter_grad: LoRA rank %d outside [1, %d]", r, AD_MAX_RANK);
    const int nct = (int)((K + LR_CT - 1) / LR_CT), nrt = (int)((N + LR_RT - 1) / LR_RT);
    const int64_t need = (int64_t)nct * N * r + (int64_t)nrt * r * K;
    UWU_CHECK_ARG(ws_elems >= need, "adapter_grad: workspace %lld < %lld floats", (long long)ws_elems, (long long)need);
    float* du = ws;
    float* dd = ws + (int64_t)nct * N * r;
    hipLaunchKernelGGL(lora_grad_partial_kernel<false>, dim3(nct, nrt), dim3(256), 0, st, dw, (int)N, (int)K, p + pa, p + pb,
                       r, du, dd, 0, 0, 0);
    const int64_t nout = N * r + (int64_t)r * K;
    hipLaunchKernelGGL(lora_grad_reduce_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, du, dd, (int)N,
                       (int)K, r, nct, nrt, scale, g + pa, g + pb, 1);
    UWU_LAUNCH_CHECK("adapter_grad");
    return UWU_OK;
  }
  UWU_CHECK_ARG(kind == UWU_ADAPTER_LOKR || kind == UWU_ADAPTER_LOKR_LOWRANK, "adapter_grad: bad kind %d", kind);
  UWU_CHECK_ARG(out_k >= 1 && in_n >= 1 && N % out_k == 0 && K % in_n == 0, "adapter_grad: LoKr shape %lldx%lld / (%d, %d)",
                (long long)N, (long long)K, out_k, in_n);
  const bool low = kind == UWU_ADAPTER_LOKR_LOWRANK;
  UWU_CHECK_ARG(!low || (r >= 1 && r <= AD_MAX_RANK), "adapter_grad: LoKr rank %d outside [1, %d]", r, AD_MAX_RANK);
  const int out_l = (int)(N / out_k), in_m = (int)(K / in_n);
  const int W2 = out_k * in_n;
  const int G = (W2 + LK_GROUP - 1) / LK_GROUP;
  const int64_t need = ad_grad_ws_elems(kind, N, K, r, out_k, in_n);
  UWU_CHECK_ARG(ws_elems >= need, "adapter_grad: workspace %lld < %lld floats", (long long)ws_elems, (long long)need);
  float* p1 = ws;
  float* p2 = p1 + (int64_t)out_l * G * in_m;
  float* w2f = p2 + (int64_t)out_l * W2;  // low-rank: the formed w2, then dw2
  float* dw2 = w2f + W2;
  const float* w2 = p + pb;
  if (low) {
    hipLaunchKernelGGL(lokr_form_w2_kernel, dim3((W2 + 255) / 256), dim3(256), 0, st, p + pb, p + pc, out_k, in_n, r, w2f);
    w2 = w2f;
  }
  hipLaunchKernelGGL(lokr_grad_partial_kernel<false>, dim3(G, out_l), dim3(256), 0, st, dw, (int)K, out_k, in_n, in_m, p + pa,
                     w2, p1, p2, 0);
  const int64_t nout = (int64_t)out_l * in_m + W2;
  hipLaunchKernelGGL(lokr_grad_reduce_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, p1, p2, out_l, in_m,
                     W2, G, scale, g + pa, low ? dw2 : g + pb, low ? 0 : 1);
  if (low) {
    const int64_t n2 = (int64_t)out_k * r + (int64_t)r * in_n;
    hipLaunchKernelGGL(lokr_grad_lowrank_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, dw2, p + pb, p + pc,
                       out_k, in_n, r, g + pb, g + pc);
  }
  UWU_LAUNCH_CHECK("adapter_grad");
  return UWU_OK;
}

extern "C" int uwu_adapter_dora_norms(const float* base, const float* p, const int64_t* table, const int64_t* table_host,
                                      const int64_t* blk_start, int nseg, int64_t nblocks, float* norms, void* stream) {
  UWU_CHECK_ARG(base && p && table && table_host && blk_start && norms && nseg > 0 && nblocks > 0 && nblocks < (1ll << 31),
                "adapter_dora_norms: bad args (nseg=%d nblocks=%lld)", nseg, (long long)nblocks);
  const char* why = ad_dora_check_rows(table_host, nseg);
  UWU_CHECK_ARG(!why, "adapter_dora_norms: bad segment table: %s", why);
  int64_t want = 0;
  for (int s = 0; s < nseg; ++s) {
    const int64_t* r = table_host + (int64_t)s * AD_DNF;
    want += r[15] ? (r[1] + AD_ROWS_WG - 1) / AD_ROWS_WG : (r[2] + AD_COLS_WG - 1) / AD_COLS_WG;
  }
  UWU_CHECK_ARG(want == nblocks, "adapter_dora_norms: nblocks %lld, the table needs %lld", (long long)nblocks, (long long)want);
  hipLaunchKernelGGL(adapter_dora_norms_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, base, p, table,
                     blk_start, nseg, norms);
  UWU_LAUNCH_CHECK("adapter_dora_norms");
  return UWU_OK;
}

extern "C" int uwu_adapter_dora_merge(const float* base, const float* p, const int64_t* table, const int64_t* table_host,
                                      const int64_t* blk_start, int nseg, int64_t nblocks, const float* norms, float* eff,
                                      void* shadow, void* stream) {
  UWU_CHECK_ARG(base && p && table && table_host && blk_start && norms && nseg > 0 && nblocks > 0 && nblocks < (1ll << 31),
                "adapter_dora_merge: bad args (nseg=%d nblocks=%lld)", nseg, (long long)nblocks);
  UWU_CHECK_ARG(eff || shadow, "adapter_dora_merge: no output");
  const char* why = ad_dora_check_rows(table_host, nseg);
  UWU_CHECK_ARG(!why, "adapter_dora_merge: bad segment table: %s", why);
  int64_t want = 0;
  for (int s = 0; s < nseg; ++s) {
    const int64_t* r = table_host + (int64_t)s * AD_DNF;
    want += (r[1] * r[2] + AD_MERGE_ELEMS - 1) / AD_MERGE_ELEMS;
  }
  UWU_CHECK_ARG(want == nblocks, "adapter_dora_merge: nblocks %lld, the table needs %lld", (long long)nblocks, (long long)want);
  hipLaunchKernelGGL(adapter_dora_merge_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, base, p, table,
                     blk_start, nseg, norms, eff, (bf16_t*)shadow);
  UWU_LAUNCH_CHECK("adapter_dora_merge");
  return UWU_OK;
}

extern "C" int uwu_adapter_dora_grad(float* dw, const float* base, int64_t N, int64_t K, int kind, const float* p, float* g,
                                     int64_t pa, int64_t pb, int64_t pc, int r, int out_k, int in_n, float scale,
                                     int64_t dora_off, const float* norms, int wd_on_out, float* ws, int64_t ws_elems,
                                     void* stream) {
  UWU_CHECK_ARG(dw && base && p && g && norms && N > 0 && K > 0 && N * K < (1ll << 31), "adapter_dora_grad: bad args");
  const AdSeg seg = {{kind, N, K, 0, -1, -1, pa, pb, pc, r, out_k, in_n, (int64_t)__builtin_bit_cast(uint32_t, scale),
                      dora_off, 0, wd_on_out}};
  const char* why = ad_dora_check_rows(seg.f, 1);
  UWU_CHECK_ARG(!why, "adapter_dora_grad: bad segment: %s", why);
  UWU_CHECK_ARG(K % 4 != 0 || (((uintptr_t)dw | (uintptr_t)base) & 15) == 0,
                "adapter_dora_grad: misaligned dw / base (16 bytes where K is a multiple of 4)");
  const int64_t need = ad_dora_grad_ws_elems(N, K, wd_on_out);
  UWU_CHECK_ARG(ws_elems >= need && (need == 0 || (ws && ((uintptr_t)ws & 7) == 0)),
                "adapter_dora_grad: workspace %lld < %lld floats, null or not 8-byte aligned", (long long)ws_elems,
                (long long)need);
  hipStream_t st = (hipStream_t)stream;
  if (wd_on_out) {
    hipLaunchKernelGGL(adapter_dora_grad_row_kernel, dim3((unsigned)((N + AD_ROWS_WG - 1) / AD_ROWS_WG)), dim3(256), 0, st, dw,
                       base, p, g, norms, seg);
  } else {
    const int nrt = (int)((N + AD_COL_RT - 1) / AD_COL_RT);
    const dim3 grid((unsigned)((K + AD_COLS_WG - 1) / AD_COLS_WG), (unsigned)nrt);
    hipLaunchKernelGGL(adapter_dora_grad_col_partial_kernel, grid, dim3(256), 0, st, dw, base, p, (AdSums*)ws, seg);
    hipLaunchKernelGGL(adapter_dora_grad_col_apply_kernel, grid, dim3(256), 0, st, dw, base, p, g, norms, (const AdSums*)ws,
                       nrt, seg);
  }
  UWU_LAUNCH_CHECK("adapter_dora_grad");
  return UWU_OK;
}
