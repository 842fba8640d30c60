// transformers.optimization.Adafactor (Shazeer & Stern, "Adafactor: Adaptive Learning Rates with Sublinear Memory Cost") on a
// flat buffer.  The rule is per TENSOR, so the kernels walk a device table of the tensors the flat store holds (uwu_hip.h:
// UWU_ADAFACTOR_FIELDS) and a launch list of the tensors that are ready, with prefix-summed workgroup starts as
// uwu_adapter_merge has them.  Per tensor W (seen as [R, C], or 1-D), g = grad * pre_scale * clip[1], step t:
//   beta2t = 1 - t^decay_rate ; U = g^2 + eps0
//   factored:   row[i] = beta2t row[i] + (1 - beta2t) mean_j U[i,j] ; col[j] = beta2t col[j] + (1 - beta2t) mean_i U[i,j]
//               u[i,j] = (rsqrt(row[i] / mean_i row[i]) * rsqrt(col[j])) * g[i,j]        (never row * col: it underflows)
//   unfactored: v = beta2t v + (1 - beta2t) U ; u = rsqrt(v) * g
//   u /= max(1, RMS(u) / clip_threshold) ; u *= alpha        alpha = lr_t * (scale_parameter ? max(eps1, RMS(W)) : 1)
//   beta1: m = beta1 m + (1 - beta1) u ; u = m
//   W -= weight_decay * alpha * W ; W -= u
//
// Four launches per call sequence, whatever the number of tensors:
//   adafactor_stats_kernel    one workgroup per tile: partial row and column sums of U (and of W^2) -> workspace; 1-D: v itself
//   adafactor_moments_kernel  one thread per row / column: the tile partials added in tile order, the moment updated, and one
//                             partial of sum_i row[i] per workgroup
//   adafactor_norm_kernel     one workgroup per tile: a partial of sum u^2 (needs every row[i], col[j] and mean(row) of the tensor)
//   adafactor_apply_kernel    one workgroup per tile: u again, the clip, alpha, m, the decay, W, the bf16 shadow, the zeroed gradient
// No atomics.  A tile's place in its tensor, the order of every sum and so every bit of a tensor's result depend on the tensor's
// shape alone, not on the launch it was part of: workgroup b of a launch serves tile b - start[s] of the s-th listed tensor.
// Per-tensor scalars (mean(row), sum u^2, sum W^2) are partials in double, one per workgroup, which every consuming workgroup
// adds up again in the same fixed order; nothing is read back.
#include "optimizer_shared.h"

namespace {

constexpr int AF_K = 128;      // rows of a factored tile each thread walks
constexpr int AF_1D = 4096;    // elements per tile of a 1-D tensor (16 per thread)
constexpr int AF_F = UWU_ADAFACTOR_FIELDS;

// The tiling of one tensor: a function of (R, C) alone.  A factored tile is tr rows x tc columns with tc = the power of two
// >= C, at most 256, and tr = (256 / tc) * AF_K: thread t owns column t % tc and the rows t / tc + k * (256 / tc).  A [1280, 4]
// tensor gets 4-column tiles 8192 rows tall (every lane loads), a [320, 11520] one 256-column tiles with coalesced rows.
struct AfGeo {
  int tc, tc_log2, rt;
  int64_t tr, ntc, ntr, tiles, nrb, mblocks, ws_floats, ws_doubles;
};

__host__ __device__ inline AfGeo af_geo(int64_t R, int64_t C) {
  AfGeo g;
  if (R == 0) {
    g.tc = 256, g.tc_log2 = 8, g.rt = 1, g.tr = 0, g.ntr = 0, g.nrb = 0, g.mblocks = 0;
    g.ntc = g.tiles = (C + AF_1D - 1) / AF_1D;
    g.ws_floats = 0;
    g.ws_doubles = 2 * g.tiles;
    return g;
  }
  int l = 0;
  while (((int64_t)1 << l) < C && l < 8) ++l;
  g.tc_log2 = l, g.tc = 1 << l, g.rt = 256 >> l;
  g.tr = (int64_t)g.rt * AF_K;
  g.ntc = (C + g.tc - 1) >> l;
  g.ntr = (R + g.tr - 1) / g.tr;
  g.tiles = g.ntc * g.ntr;
  g.nrb = (R + 255) / 256;
  g.mblocks = g.nrb + (C + 255) / 256;
  g.ws_floats = g.ntc * R + g.ntr * C;      // row partials [ntc, R], then column partials [ntr, C]
  g.ws_doubles = 2 * g.tiles + g.nrb;       // sum W^2 per tile, sum u^2 per tile, sum row per moments workgroup
  return g;
}

// largest s with start[s] <= b, given start[0] <= b < start[n] (tensors without workgroups repeat a start)
__device__ __forceinline__ int af_find(const int64_t* __restrict__ start, int n, int64_t b) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

struct AfTile {
  const int64_t* row;  // the tensor's table row
  int64_t id, tile, off, R, C;
  AfGeo geo;
};

__device__ __forceinline__ AfTile af_tile(const int64_t* __restrict__ table, const int64_t* __restrict__ launch, int nready,
                                          const int64_t* __restrict__ start) {
  AfTile a;
  const int s = af_find(start, nready, blockIdx.x);
  a.id = launch[s];
  a.tile = (int64_t)blockIdx.x - start[s];
  a.row = table + a.id * AF_F;
  a.off = a.row[0], a.R = a.row[1], a.C = a.row[2];
  a.geo = af_geo(a.R, a.C);
  return a;
}

// partials [0, n) added in a fixed order: thread t takes t, t + 256, ..., then the LDS tree
__device__ __forceinline__ double af_sum_partials(const double* __restrict__ part, int64_t n, double* red) {
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) a += part[i];
  return block_sum_f64(a, red);
}

// u of one element before the clip: the package's (r_factor * c_factor) * grad; 1-D: rf = rsqrt(v), cf = 1
__device__ __forceinline__ float af_update(float g, float gscale, float rf, float cf) {
  const float gs = gscale * g;
  return (rf * cf) * gs;
}

// Walks this workgroup's tile: fn(e, u) per element inside the tensor, e its index in the flat buffer, u from af_update.
// mean(row) is summed first (factored), so the call is a workgroup-wide one: every thread makes it.
template <typename Fn>
__device__ __forceinline__ void af_for_each_update(const AfTile& a, const float* __restrict__ g, const float* __restrict__ rowst,
                                                   const float* __restrict__ colst, const float* __restrict__ v,
                                                   const double* __restrict__ dws, float gscale, double* red, Fn fn) {
  const int t = threadIdx.x;
  if (a.R == 0) {
    const float* vv = v + a.row[5];
    const int64_t e0 = a.tile * AF_1D;
#pragma unroll 4
    for (int k = 0; k < AF_1D / 256; ++k) {
      const int64_t i = e0 + k * 256 + t;
      if (i < a.C) fn(a.off + i, af_update(g[a.off + i], gscale, rsqrtf(vv[i]), 1.f));
    }
    return;
  }
  const double rsum = af_sum_partials(dws + a.row[7] + 2 * a.geo.tiles, a.geo.nrb, red);
  const float rowmean = (float)(rsum / (double)a.R);
  const int64_t trow = a.tile / a.geo.ntc, tcol = a.tile - trow * a.geo.ntc;
  const int cx = t & (a.geo.tc - 1), ry = t >> a.geo.tc_log2;
  const int64_t c = tcol * a.geo.tc + cx, r0 = trow * a.geo.tr;
  if (c >= a.C) return;
  const float cf = rsqrtf(colst[a.row[4] + c]);
  const float* rs = rowst + a.row[3];
  const int64_t rows = a.R - r0 < a.geo.tr ? a.R - r0 : a.geo.tr;
#pragma unroll 4
  for (int64_t lr = ry; lr < rows; lr += a.geo.rt) {
    const int64_t r = r0 + lr, e = a.off + r * a.C + c;
    fn(e, af_update(g[e], gscale, rsqrtf(rs[r] / rowmean), cf));
  }
}

__global__ void __launch_bounds__(256) adafactor_stats_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                              float* __restrict__ v, float* __restrict__ fws,
                                                              double* __restrict__ dws, const int64_t* __restrict__ table,
                                                              const int64_t* __restrict__ launch, int nready, float beta2t,
                                                              float omb2t, float eps0, int scale_parameter, float pre_scale,
                                                              const float* __restrict__ clip) {
  __shared__ double red[256];
  __shared__ float colbuf[256];
  __shared__ float rowbuf[512];
  const int t = threadIdx.x;
  const AfTile a = af_tile(table, launch, nready, launch + nready);
  const float gscale = grad_scale(pre_scale, clip);
  double wsq = 0.0;
  if (a.R == 0) {  // unfactored: the moment itself.  Rounded first: gs, gs*gs, gs*gs + eps0, omb2t*U; fused: beta2t*v + (.)
    float* vv = v + a.row[5];
    const int64_t e0 = a.tile * AF_1D;
#pragma unroll 4
    for (int k = 0; k < AF_1D / 256; ++k) {
      const int64_t i = e0 + k * 256 + t;
      if (i < a.C) {
        const float gs = gscale * g[a.off + i];
        const float u = gs * gs + eps0;
        vv[i] = __builtin_fmaf(beta2t, vv[i], omb2t * u);
        if (scale_parameter) {
          const double pp = (double)p[a.off + i];
          wsq = __builtin_fma(pp, pp, wsq);
        }
      }
    }
  } else {
    const AfGeo& geo = a.geo;
    const int64_t trow = a.tile / geo.ntc, tcol = a.tile - trow * geo.ntc;
    const int cx = t & (geo.tc - 1), ry = t >> geo.tc_log2;
    const int64_t c = tcol * geo.tc + cx, r0 = trow * geo.tr;
    const bool cin = c < a.C;
    const int sw = geo.tc < 64 ? geo.tc : 64;  // lanes that share a row inside one wave
    const int nseg = geo.tc >> 6;              // waves that share a row: 0 (tc < 64), 1, 2 or 4
    float* rowpart = fws + a.row[6] + tcol * a.R;
    const int64_t rows = a.R - r0 < geo.tr ? a.R - r0 : geo.tr;
    const int kmax = (int)((rows + geo.rt - 1) / geo.rt);  // the same for every thread: the shuffles below need all lanes
    float colacc = 0.f;
    for (int k0 = 0; k0 < kmax; k0 += 4) {  // four rows at a time: their loads are in flight together
      float u[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t lr = (int64_t)(k0 + j) * geo.rt + ry;
        u[j] = 0.f;  // outside the tensor: nothing is read, nothing is added
        if (cin && lr < rows) {
          const int64_t e = a.off + (r0 + lr) * a.C + c;
          const float gs = gscale * g[e];
          u[j] = gs * gs + eps0;
          if (scale_parameter) {
            const double pp = (double)p[e];
            wsq = __builtin_fma(pp, pp, wsq);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t lr = (int64_t)(k0 + j) * geo.rt + ry;
        colacc += u[j];
        float rsum = u[j];
        for (int o = sw >> 1; o > 0; o >>= 1) rsum += __shfl_xor(rsum, o);  // a butterfly: the same tree on every run
        if ((t & (sw - 1)) == 0 && lr < rows) {
          if (nseg <= 1) rowpart[r0 + lr] = rsum;
          else rowbuf[lr * nseg + (cx >> 6)] = rsum;
        }
      }
    }
    __syncthreads();
    if (nseg > 1)
      for (int64_t lr = t; lr < rows; lr += 256) {
        float s = rowbuf[lr * nseg];
        for (int j = 1; j < nseg; ++j) s += rowbuf[lr * nseg + j];
        rowpart[r0 + lr] = s;
      }
    colbuf[t] = colacc;
    __syncthreads();
    if (t < geo.tc && cin) {  // (t < tc: this thread's column is c)
      float s = colbuf[t];
      for (int y = 1; y < geo.rt; ++y) s += colbuf[y * geo.tc + t];
      fws[a.row[6] + geo.ntc * a.R + trow * a.C + c] = s;
    }
  }
  if (scale_parameter) {
    wsq = block_sum_f64(wsq, red);
    if (t == 0) dws[a.row[7] + a.tile] = wsq;
  }
}

// Workgroup b of a factored tensor: b < nrb takes rows [256 b, 256 b + 256), the others columns.  The tile partials are added in
// tile order; mean = sum / count (rounded), omb2t*mean rounded, beta2t*moment + (.) fused.
__global__ void __launch_bounds__(256) adafactor_moments_kernel(float* __restrict__ rowst, float* __restrict__ colst,
                                                                const float* __restrict__ fws, double* __restrict__ dws,
                                                                const int64_t* __restrict__ table,
                                                                const int64_t* __restrict__ launch, int nready, float beta2t,
                                                                float omb2t) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const AfTile a = af_tile(table, launch, nready, launch + 2 * nready + 1);
  const AfGeo& geo = a.geo;
  const int64_t b = a.tile;
  const float* rowpart = fws + a.row[6];
  const float* colpart = rowpart + geo.ntc * a.R;
  if (b < geo.nrb) {
    const int64_t i = b * 256 + t;
    double acc = 0.0;
    if (i < a.R) {
      float s = rowpart[i];
      for (int64_t k = 1; k < geo.ntc; ++k) s += rowpart[k * a.R + i];
      const float mean = s / (float)a.C;
      float* r = rowst + a.row[3] + i;
      const float rn = __builtin_fmaf(beta2t, *r, omb2t * mean);
      *r = rn;
      acc = (double)rn;
    }
    acc = block_sum_f64(acc, red);
    if (t == 0) dws[a.row[7] + 2 * geo.tiles + b] = acc;
  } else {
    const int64_t j = (b - geo.nrb) * 256 + t;
    if (j < a.C) {
      float s = colpart[j];
      for (int64_t k = 1; k < geo.ntr; ++k) s += colpart[k * a.C + j];
      const float mean = s / (float)a.R;
      float* cc = colst + a.row[4] + j;
      *cc = __builtin_fmaf(beta2t, *cc, omb2t * mean);
    }
  }
}

__global__ void __launch_bounds__(256) adafactor_norm_kernel(const float* __restrict__ g, const float* __restrict__ rowst,
                                                             const float* __restrict__ colst, const float* __restrict__ v,
                                                             double* __restrict__ dws, const int64_t* __restrict__ table,
                                                             const int64_t* __restrict__ launch, int nready, float pre_scale,
                                                             const float* __restrict__ clip) {
  __shared__ double red[256];
  const AfTile a = af_tile(table, launch, nready, launch + nready);
  double usq = 0.0;
  af_for_each_update(a, g, rowst, colst, v, dws, grad_scale(pre_scale, clip), red, [&](int64_t, float u) {
    usq = __builtin_fma((double)u, (double)u, usq);
  });
  usq = block_sum_f64(usq, red);
  if (threadIdx.x == 0) dws[a.row[7] + a.geo.tiles + a.tile] = usq;
}

// Rounded first: u / denom, (.) * alpha, omb1*u, wd_alpha*W; fused: beta1*m + (.), W - wd_alpha*W.  denom and alpha are formed in
// double from the double sums and rounded once.
__global__ void __launch_bounds__(256) adafactor_apply_kernel(float* __restrict__ p, float* __restrict__ g,
                                                              bf16_t* __restrict__ pbf, float* __restrict__ m,
                                                              const float* __restrict__ rowst, const float* __restrict__ colst,
                                                              const float* __restrict__ v, float* __restrict__ rms,
                                                              const double* __restrict__ dws, const int64_t* __restrict__ table,
                                                              const int64_t* __restrict__ launch, int nready, double lr_t,
                                                              double eps1, double clip_threshold, int scale_parameter,
                                                              float beta1, float omb1, double weight_decay, float pre_scale,
                                                              const float* __restrict__ clip, int zero_grad) {
  __shared__ double red[256];
  const AfTile a = af_tile(table, launch, nready, launch + nready);
  const double numel = (double)(a.R ? a.R * a.C : a.C);
  const double usum = af_sum_partials(dws + a.row[7] + a.geo.tiles, a.geo.tiles, red);
  const double ratio = sqrt(usum / numel) / clip_threshold;
  const float denom = (float)(ratio > 1.0 || ratio != ratio ? ratio : 1.0);  // max(1, .) that keeps a NaN, as clamp_ does
  double alpha = lr_t;
  if (scale_parameter) {
    const double rms_w = sqrt(af_sum_partials(dws + a.row[7], a.geo.tiles, red) / numel);
    alpha = lr_t * (rms_w > eps1 || rms_w != rms_w ? rms_w : eps1);
    if (a.tile == 0 && threadIdx.x == 0) rms[a.id] = (float)rms_w;
  }
  const float alphaf = (float)alpha, wda = (float)(weight_decay * alpha);
  af_for_each_update(a, g, rowst, colst, v, dws, grad_scale(pre_scale, clip), red, [&](int64_t e, float u) {
    u = u / denom;
    u = u * alphaf;
    if (m) {
      const float mn = __builtin_fmaf(beta1, m[e], omb1 * u);
      m[e] = mn;
      u = mn;
    }
    float pp = p[e];
    if (wda != 0.f) pp = __builtin_fmaf(-wda, pp, pp);
    pp = pp - u;
    flat_write_back(p, pbf, g, e, pp, zero_grad);
  });
}

// Everything a launch is about to index, checked on the host copy of the table before anything is launched.  The listed tensors
// come in table order, and in that order their ranges in the flat buffer, in the state and in both workspaces ascend without
// overlap (the table is built that way); a tensor is R x C with R * C < 2^31, or 1-D (R = 0) with C < 2^31.
int af_check(const UwuAdafactorDesc* d, const int64_t* lh, const int64_t* ld, int nready, const char* who, int64_t* tiles,
             int64_t* mblocks) {
  UWU_CHECK_ARG(d && lh && ld, "%s: null pointer", who);
  UWU_CHECK_ARG(d->p && d->g && d->row && d->col && d->v && d->rms && d->fws && d->dws && d->table_host && d->table,
                "%s: null pointer in the descriptor", who);
  UWU_CHECK_ARG((((uintptr_t)d->p | (uintptr_t)d->g) & 15) == 0 && ((uintptr_t)d->p_bf16 & 7) == 0 && ((uintptr_t)d->dws & 7) == 0,
                "%s: p and g must be 16-byte aligned, the shadow and the double workspace 8-byte aligned", who);
  UWU_CHECK_ARG(d->ntensors > 0 && nready > 0 && nready <= d->ntensors, "%s: %d of %d tensors", who, nready, d->ntensors);
  int64_t prev = -1, end_p = 0, end_r = 0, end_c = 0, end_v = 0, end_f = 0, end_d = 0, nt = 0, nm = 0;
  for (int s = 0; s < nready; ++s) {
    const int64_t id = lh[s];
    UWU_CHECK_ARG(id > prev && id < d->ntensors, "%s: launch list entry %d names tensor %lld (not ascending, or outside the table)",
                  who, s, (long long)id);
    prev = id;
    const int64_t* r = d->table_host + id * AF_F;
    const int64_t off = r[0], R = r[1], C = r[2];
    UWU_CHECK_ARG(R >= 0 && C >= 1 && C < (1ll << 31) && (R == 0 || C <= ((1ll << 31) - 1) / R),
                  "%s: tensor %lld is %lld x %lld (needs R * C < 2^31)", who, (long long)id, (long long)R, (long long)C);
    const int64_t numel = R ? R * C : C;
    UWU_CHECK_ARG(off >= 0 && off % 4 == 0, "%s: tensor %lld starts at element %lld (needs a multiple of 4)", who, (long long)id,
                  (long long)off);
    UWU_CHECK_ARG(off >= end_p && numel <= d->n && off <= d->n - numel,
                  "%s: tensor %lld [%lld, %lld) overlaps its predecessor or leaves the buffer of %lld elements", who, (long long)id,
                  (long long)off, (long long)(off + numel), (long long)d->n);
    end_p = off + numel;
    const AfGeo geo = af_geo(R, C);
    if (R) {
      UWU_CHECK_ARG(r[3] >= end_r && r[3] <= d->n_row - R && r[4] >= end_c && r[4] <= d->n_col - C,
                    "%s: tensor %lld: row / column state outside its buffers", who, (long long)id);
      end_r = r[3] + R, end_c = r[4] + C;
    } else {
      UWU_CHECK_ARG(r[5] >= end_v && r[5] <= d->n_v - C, "%s: tensor %lld: unfactored state outside its buffer", who, (long long)id);
      end_v = r[5] + C;
    }
    UWU_CHECK_ARG(r[6] >= end_f && r[6] <= d->n_fws - geo.ws_floats && r[7] >= end_d && r[7] <= d->n_dws - geo.ws_doubles,
                  "%s: tensor %lld: workspace outside its buffers", who, (long long)id);
    end_f = r[6] + geo.ws_floats, end_d = r[7] + geo.ws_doubles;
    UWU_CHECK_ARG(lh[nready + s] == nt && lh[2 * nready + 1 + s] == nm, "%s: launch list: workgroup starts of entry %d are wrong", who,
                  s);
    nt += geo.tiles, nm += geo.mblocks;
  }
  UWU_CHECK_ARG(lh[2 * nready] == nt && lh[3 * nready + 1] == nm && nt > 0 && nt < (1ll << 31) && nm < (1ll << 31),
                "%s: launch list: workgroup totals are wrong", who);
  *tiles = nt, *mblocks = nm;
  return UWU_OK;
}

}  // namespace

extern "C" int64_t uwu_adafactor_tiles(int64_t R, int64_t C) { return R >= 0 && C >= 1 ? af_geo(R, C).tiles : 0; }
extern "C" int64_t uwu_adafactor_moment_blocks(int64_t R, int64_t C) { return R >= 0 && C >= 1 ? af_geo(R, C).mblocks : 0; }
extern "C" int64_t uwu_adafactor_ws_floats(int64_t R, int64_t C) { return R >= 0 && C >= 1 ? af_geo(R, C).ws_floats : 0; }
extern "C" int64_t uwu_adafactor_ws_doubles(int64_t R, int64_t C) { return R >= 0 && C >= 1 ? af_geo(R, C).ws_doubles : 0; }

extern "C" int uwu_adafactor_stats(const UwuAdafactorDesc* d, const int64_t* launch_host, const int64_t* launch, int nready,
                                   double beta2t, double eps0, int scale_parameter, float pre_scale, const float* clip,
                                   void* stream) {
  int64_t tiles, mblocks;
  if (int rc = af_check(d, launch_host, launch, nready, "adafactor_stats", &tiles, &mblocks)) return rc;
  UWU_CHECK_ARG(beta2t >= 0.0 && beta2t < 1.0 && eps0 >= 0.0, "adafactor_stats: beta2t %g outside [0, 1) or eps0 %g < 0", beta2t, eps0);
  // 1 - beta2t in double on the host, as the package does with python floats
  hipLaunchKernelGGL(adafactor_stats_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, d->p, d->g, d->v, d->fws,
                     d->dws, d->table, launch, nready, (float)beta2t, (float)(1.0 - beta2t), (float)eps0, scale_parameter,
                     pre_scale, clip);
  if (mblocks > 0)
    hipLaunchKernelGGL(adafactor_moments_kernel, dim3((unsigned)mblocks), dim3(256), 0, (hipStream_t)stream, d->row, d->col,
                       d->fws, d->dws, d->table, launch, nready, (float)beta2t, (float)(1.0 - beta2t));
  UWU_LAUNCH_CHECK("adafactor_stats");
  return UWU_OK;
}

extern "C" int uwu_adafactor_norm(const UwuAdafactorDesc* d, const int64_t* launch_host, const int64_t* launch, int nready,
                                  float pre_scale, const float* clip, void* stream) {
  int64_t tiles, mblocks;
  if (int rc = af_check(d, launch_host, launch, nready, "adafactor_norm", &tiles, &mblocks)) return rc;
  hipLaunchKernelGGL(adafactor_norm_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, d->g, d->row, d->col, d->v,
                     d->dws, d->table, launch, nready, pre_scale, clip);
  UWU_LAUNCH_CHECK("adafactor_norm");
  return UWU_OK;
}

extern "C" int uwu_adafactor_apply(const UwuAdafactorDesc* d, const int64_t* launch_host, const int64_t* launch, int nready,
                                   double lr_t, double eps1, double clip_threshold, int scale_parameter, int use_beta1,
                                   double beta1, double weight_decay, float pre_scale, const float* clip, int zero_grad,
                                   void* stream) {
  int64_t tiles, mblocks;
  if (int rc = af_check(d, launch_host, launch, nready, "adafactor_apply", &tiles, &mblocks)) return rc;
  UWU_CHECK_ARG(clip_threshold > 0.0, "adafactor_apply: clip_threshold %g must be positive", clip_threshold);
  UWU_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0, "adafactor_apply: beta1 %g outside [0, 1)", beta1);
  UWU_CHECK_ARG(!use_beta1 || d->m, "adafactor_apply: beta1 given without the first moment's buffer");
  UWU_CHECK_ARG(!use_beta1 || ((uintptr_t)d->m & 15) == 0, "adafactor_apply: exp_avg must be 16-byte aligned");
  hipLaunchKernelGGL(adafactor_apply_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, d->p, d->g,
                     (bf16_t*)d->p_bf16, use_beta1 ? d->m : nullptr, d->row, d->col, d->v, d->rms, d->dws, d->table, launch,
                     nready, lr_t, eps1, clip_threshold, scale_parameter, (float)beta1, (float)(1.0 - beta1), weight_decay,
                     pre_scale, clip, zero_grad);
  UWU_LAUNCH_CHECK("adafactor_apply");
  return UWU_OK;
}
