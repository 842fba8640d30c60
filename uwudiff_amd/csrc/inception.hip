// The InceptionV3 feature extractor's kernels and the FID statistics (uwudiff_amd/inception.py, uwudiff_amd/metrics.py; DESIGN.md
// section 4.37).  Forward only: the extractor is frozen.
//
//   uwu_conv2d_fwd        y = [relu](conv(x, w) + bias) on channels-last activations as an implicit GEMM on the MFMA units: kernel
//                         1x1 / 3x3 / 5x5 / 1x7 / 7x1 / 1x3 / 3x1, stride 1 | 2, zero padding (ph, pw), a row stride and a channel
//                         offset on both sides (a branch reads a slice of a buffer and writes into its slice of the concatenation)
//   uwu_inception_stem    pictures [B, 3, H, W] (uint8, or floats in [0, 1]) -> the A operand [B Ho Wo, 32] of Conv2d_1a_3x3 (3x3,
//                         stride 2, no padding), the input rule (v - 128) / 128 fused in
//   uwu_relu_rows         ReLU in place on a channel slice (behind uwu_gemm, which has no ReLU epilogue, on the routed 1x1 layers)
//   uwu_pool2d_fwd        max 3x3 / 2, max 3x3 / 1 pad 1, average 3x3 / 1 pad 1 over the pixels inside the image
//   uwu_global_avgpool    [B, HW, C] -> fp32 [B, C]
//   uwu_fid_stats_accum   n += B, sum[D] += column sums, outer[D, D] += F^T F in float64, every element owned by one thread
#include <math.h>

#include <type_traits>

#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------- convolution
// One workgroup of four waves (2 x 2) computes 64 or 128 output pixels x 64 or 96 output channels.  The reduction runs tap by tap, 32
// input channels at a time: every thread fetches 8 consecutive channels of its pixel row(s) and of its weight row(s) straight from
// global memory into registers (zeros for a tap outside the image, a row past M, a channel past C or a weight row past Cout: this
// is the M tail and the 48 / 80 channel case), PF such fetches are in flight while a step multiplies out of one of two LDS stages.
// The product is taken as W . X^T so that a lane's four accumulator registers are four consecutive output channels of one pixel:
// one vector store in the epilogue.
//   MT  64-pixel row groups per workgroup: 2 where 128-pixel workgroups still give two per CU, else 1
//   NT  16-channel subtiles per wave: 2 (64 channels per workgroup), or 3 (96) where Cout is a multiple of 96 and not of 64, so that
//       the 96-channel layers do not run a half-empty second tile
//   PF  fetches in flight: the 64-pixel workgroups run where a layer gives a CU only a few workgroups and the latency of a fetch,
//       not the MFMAs, bounds a step, so they keep 4; the 128-pixel ones keep 1 (more would cost them a wave of occupancy)
constexpr int CV_BM = 64, CV_BK = 32;

template <typename T>
struct Pack8 {
  uint4 q[sizeof(T) / 2];
};

template <typename T>
__device__ __forceinline__ Pack8<T> ld_pack8(const T* p, bool ok) {
  Pack8<T> r;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 2); ++i) r.q[i] = ok ? reinterpret_cast<const uint4*>(p)[i] : uint4{0u, 0u, 0u, 0u};
  return r;
}

struct Conv2dP {
  int H, W, C, Cout, KH, KW, stride, ph, pw, Ho, Wo, ldx, ldy, relu;
  int64_t M;
};

template <typename T, int MT, int NT, int PF>
__global__ void __launch_bounds__(256) conv2d_kernel(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias,
                                                      T* __restrict__ y, Conv2dP p) {
  static_assert(PF == 1 || PF == 2 || PF == 4, "the step loop is unrolled by four");
  constexpr int BM = CV_BM * MT, BN = 32 * NT, WR = (BN + 63) / 64;  // WR: weight rows a thread fetches (the second only below BN)
  constexpr int LDS_LD = CV_BK + 16 / (int)sizeof(T);  // 16 bytes of padding per row: the 16 rows a lane group reads hit distinct banks
  __shared__ __attribute__((aligned(16))) T Xs[2][BM * LDS_LD];  // two stages: one barrier per step
  __shared__ __attribute__((aligned(16))) T Ws[2][WR * 64 * LDS_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int r = tid >> 2, seg = (tid & 3) * 8;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;

  // this thread's pixel rows (r, r + 64) and weight rows (r, r + 64), fixed for the whole reduction
  bool m_ok[MT];
  int iy0[MT], ix0[MT];
  int64_t img[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int64_t m = m0 + r + t * 64;
    m_ok[t] = m < p.M;
    iy0[t] = ix0[t] = 0;
    img[t] = 0;
    if (m_ok[t]) {
      const int64_t b = m / ((int64_t)p.Ho * p.Wo);
      const int rem = (int)(m - b * p.Ho * p.Wo), oy = rem / p.Wo, ox = rem - oy * p.Wo;
      iy0[t] = oy * p.stride - p.ph;
      ix0[t] = ox * p.stride - p.pw;
      img[t] = b * p.H;
    }
  }
  const int taps = p.KH * p.KW, kc = (p.C + CV_BK - 1) / CV_BK, steps = taps * kc;
  bool n_ok[WR];
  const T* wrow[WR];
#pragma unroll
  for (int u = 0; u < WR; ++u) {
    n_ok[u] = r + u * 64 < BN && n0 + r + u * 64 < p.Cout;
    wrow[u] = w + (int64_t)(n_ok[u] ? n0 + r + u * 64 : 0) * taps * p.C;
  }

  auto fetch = [&](int tap, int c0, Pack8<T>* xv, Pack8<T>* wv) {
    const int ky = tap / p.KW, kx = tap - ky * p.KW;
    const int c = c0 + seg;
    const bool c_ok = c < p.C;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int iy = iy0[t] + ky, ix = ix0[t] + kx;
      const bool x_ok = m_ok[t] && c_ok && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      xv[t] = ld_pack8<T>(x + (x_ok ? ((img[t] + iy) * p.W + ix) * p.ldx + c : 0), x_ok);
    }
#pragma unroll
    for (int u = 0; u < WR; ++u) wv[u] = ld_pack8<T>(wrow[u] + (n_ok[u] && c_ok ? (int64_t)tap * p.C + c : 0), n_ok[u] && c_ok);
  };

  f32x4 acc[NT][2 * MT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < 2 * MT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  Pack8<T> xv[PF][MT], wv[PF][WR];
  int tap = 0, c0 = 0;
  auto advance = [&]() {
    c0 += CV_BK;
    if (c0 >= p.C) {
      c0 = 0;
      ++tap;
    }
  };
#pragma unroll
  for (int i = 0; i < PF; ++i)
    if (i < steps) {
      fetch(tap, c0, xv[i], wv[i]);
      advance();
    }
  const int fr = lane & 15, fk = lane >> 4;
  const bool live = n0 + wn * 16 * NT < p.Cout;  // wave-uniform: in a partial channel tile a wave may own no column at all
  auto step = [&](int s, auto idx_c) {
    constexpr int STAGE = decltype(idx_c)::value & 1, SLOT = decltype(idx_c)::value % PF;
    // stage STAGE was last read in step s - 2, and every wave has passed the barrier of step s - 1 since
    T* xs = Xs[STAGE];
    T* ws = Ws[STAGE];
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 2); ++i) {
#pragma unroll
      for (int t = 0; t < MT; ++t) reinterpret_cast<uint4*>(xs + (r + t * 64) * LDS_LD + seg)[i] = xv[SLOT][t].q[i];
#pragma unroll
      for (int u = 0; u < WR; ++u) reinterpret_cast<uint4*>(ws + (r + u * 64) * LDS_LD + seg)[i] = wv[SLOT][u].q[i];
    }
    __syncthreads();
    if (s + PF < steps) {
      fetch(tap, c0, xv[SLOT], wv[SLOT]);
      advance();
    }
    if (!live) return;
    if constexpr (sizeof(T) == 2) {
      bf16x8 a[NT], b[2 * MT];
#pragma unroll
      for (int i = 0; i < NT; ++i) a[i] = *reinterpret_cast<const bf16x8*>(ws + (wn * 16 * NT + i * 16 + fr) * LDS_LD + fk * 8);
#pragma unroll
      for (int j = 0; j < 2 * MT; ++j) b[j] = *reinterpret_cast<const bf16x8*>(xs + (wm * 32 * MT + j * 16 + fr) * LDS_LD + fk * 8);
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < 2 * MT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    } else {
#pragma unroll
      for (int kk = 0; kk < CV_BK / 4; ++kk) {
        float a[NT], b[2 * MT];
#pragma unroll
        for (int i = 0; i < NT; ++i) a[i] = ws[(wn * 16 * NT + i * 16 + fr) * LDS_LD + kk * 4 + fk];
#pragma unroll
        for (int j = 0; j < 2 * MT; ++j) b[j] = xs[(wm * 32 * MT + j * 16 + fr) * LDS_LD + kk * 4 + fk];
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
          for (int j = 0; j < 2 * MT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
  };
  for (int s = 0; s < steps; s += 4) {
    step(s, std::integral_constant<int, 0>{});
    if (s + 1 < steps) step(s + 1, std::integral_constant<int, 1>{});
    if (s + 2 < steps) step(s + 2, std::integral_constant<int, 2>{});
    if (s + 3 < steps) step(s + 3, std::integral_constant<int, 3>{});
  }

  // accumulator register e of lane l: output channel 4 (l >> 4) + e of the 16-channel subtile, pixel l & 15 of the 16-pixel subtile
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int co = n0 + wn * 16 * NT + i * 16 + (lane >> 4) * 4;
    if (co >= p.Cout) continue;  // Cout is a multiple of 8: the four channels are inside together
    const f32x4 bv = bias ? *reinterpret_cast<const f32x4*>(bias + co) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 2 * MT; ++j) {
      const int64_t mo = m0 + wm * 32 * MT + j * 16 + (lane & 15);
      if (mo >= p.M) continue;
      f32x4 v = acc[i][j] + bv;
      if (p.relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      store4(y + mo * p.ldy + co, v);
    }
  }
}

// ---------------------------------------------------------------------------------------------- stem operand
// one thread per output element; column (c, ky, kx) = 9 c + 3 ky + kx of row (b, oy, ox), the order of conv.weight.view(32, 27)
template <typename TI, typename TO>
__global__ void __launch_bounds__(256) inception_stem_kernel(const TI* __restrict__ img, TO* __restrict__ out, int64_t rows, int H, int W, int Ho,
                                                              int Wo) {
  const int64_t total = rows * 32;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i >> 5;
    const int col = (int)(i & 31);
    float v = 0.f;  // columns 27 .. 31
    if (col < 27) {
      const int64_t b = row / ((int64_t)Ho * Wo);
      const int rem = (int)(row - b * Ho * Wo), oy = rem / Wo, ox = rem - oy * Wo;
      const int c = col / 9, t = col - c * 9, ky = t / 3, kx = t - ky * 3;
      const TI raw = img[((b * 3 + c) * H + 2 * oy + ky) * (int64_t)W + 2 * ox + kx];
      float u;
      if constexpr (sizeof(TI) == 1) u = (float)raw;
      else u = truncf(fminf(fmaxf((float)raw, 0.f), 1.f) * 255.f);  // NaN -> 0; the product is rounded to fp32, then truncated
      v = (u - 128.f) / 128.f;  // exact: an integer in [-128, 127] over a power of two
    }
    out[i] = from_f32<TO>(v);
  }
}

// ---------------------------------------------------------------------------------------------- pooling
enum { POOL_MAX_S2 = 0, POOL_MAX_S1P1 = 1, POOL_AVG_S1P1 = 2 };

template <typename T, int MODE>
__global__ void __launch_bounds__(256) pool2d_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t Mo, int H, int W, int C, int Ho, int Wo,
                                                      int ldx, int ldy) {
  constexpr int S = MODE == POOL_MAX_S2 ? 2 : 1, PAD = MODE == POOL_MAX_S2 ? 0 : 1;
  const int per = C / 8;
  const int64_t total = Mo * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t mo = i / per;
    const int c = (int)(i - mo * per) * 8;
    const int64_t b = mo / ((int64_t)Ho * Wo);
    const int rem = (int)(mo - b * Ho * Wo), oy = rem / Wo, ox = rem - oy * Wo;
    f32x8 a;
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = MODE == POOL_AVG_S1P1 ? 0.f : -INFINITY;
    int cnt = 0;
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * S - PAD + ky;
      if (iy < 0 || iy >= H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * S - PAD + kx;
        if (ix < 0 || ix >= W) continue;
        const f32x8 v = load8(x + ((b * H + iy) * W + ix) * ldx + c);
        ++cnt;
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = MODE == POOL_AVG_S1P1 ? a[e] + v[e] : fmaxf(a[e], v[e]);
      }
    }
    if constexpr (MODE == POOL_AVG_S1P1) {
      const float d = (float)cnt;  // 4, 6 or 9: the pixels inside the image (count_include_pad = False)
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = a[e] / d;
    }
    store8(y + mo * ldy + c, a);
  }
}

// y = max(y, 0) on channels yoff .. yoff + N of every row, 8 elements per thread
template <typename T>
__global__ void __launch_bounds__(256) relu_rows_kernel(T* __restrict__ y, int64_t M, int N, int ldy) {
  const int per = N / 8;
  const int64_t total = M * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t m = i / per;
    T* q = y + m * ldy + (int)(i - m * per) * 8;
    f32x8 v = load8(q);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
    store8(q, v);
  }
}

// consecutive threads take consecutive channels; the HW pixels are added in ascending order in fp32
template <typename T>
__global__ void __launch_bounds__(256) global_avgpool_kernel(const T* __restrict__ x, float* __restrict__ out, int64_t total, int HW, int C,
                                                              int ldx) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / C;
    const int c = (int)(i - b * C);
    float s = 0.f;
    for (int q = 0; q < HW; ++q) s += to_f32(x[(b * HW + q) * ldx + c]);
    out[i] = s / (float)HW;
  }
}

// ---------------------------------------------------------------------------------------------- FID statistics
// outer += F^T F: a workgroup owns a 64 x 64 tile of `outer`, a thread 4 x 4 of it; the B rows are added in ascending order in
// float64 (a product of two floats is exact there), then the tile is added to memory once.  No atomics anywhere: the same batches
// in the same order give the same bits.
__global__ void __launch_bounds__(256) fid_outer_kernel(const float* __restrict__ f, double* __restrict__ outer, int B, int D) {
  __shared__ double Fi[16][64], Fj[16][64];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  for (int b0 = 0; b0 < B; b0 += 16) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + q * 256, rb = e >> 6, cc = e & 63;
      const bool ok = b0 + rb < B;
      Fi[rb][cc] = ok ? (double)f[(int64_t)(b0 + rb) * D + i0 + cc] : 0.0;
      Fj[rb][cc] = ok ? (double)f[(int64_t)(b0 + rb) * D + j0 + cc] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int rb = 0; rb < 16; ++rb) {
      double a[4], b[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[e] = Fi[rb][ti * 4 + e];
        b[e] = Fj[rb][tj * 4 + e];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) outer[(int64_t)(i0 + ti * 4 + u) * D + j0 + tj * 4 + v] += acc[u][v];
}

__global__ void __launch_bounds__(256) fid_sum_kernel(const float* __restrict__ f, double* __restrict__ n, double* __restrict__ sum, int B, int D) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d == 0) n[0] += (double)B;
  if (d >= D) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += (double)f[(int64_t)b * D + d];
  sum[d] += s;
}

bool conv2d_family(int KH, int KW) {
  return (KH == 1 && (KW == 1 || KW == 3 || KW == 7)) || (KW == 1 && (KH == 3 || KH == 7)) || (KH == KW && (KH == 3 || KH == 5));
}

}  // namespace

extern "C" int uwu_conv2d_ok(int B, int H, int W, int C, int Cout, int KH, int KW, int stride, int ph, int pw, int ldx, int xoff, int ldy,
                             int yoff, int dtype) {
  if (dtype != UWU_F32 && dtype != UWU_BF16) return 0;
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || Cout <= 0 || !conv2d_family(KH, KW) || (stride != 1 && stride != 2)) return 0;
  if (ph < 0 || pw < 0 || ph >= KH || pw >= KW || H + 2 * ph < KH || W + 2 * pw < KW) return 0;
  if (C % 8 || Cout % 8 || ldx % 8 || ldy % 8 || xoff % 8 || yoff % 8 || xoff < 0 || yoff < 0) return 0;
  if ((int64_t)xoff + C > ldx || (int64_t)yoff + Cout > ldy) return 0;
  const int64_t Ho = (H + 2 * ph - KH) / stride + 1, Wo = (W + 2 * pw - KW) / stride + 1;
  if ((int64_t)B * Ho * Wo > 0x7FFFFFFF - CV_BM || (int64_t)KH * KW * C > 0x7FFFFFFF / 4) return 0;
  if ((int64_t)B * Ho * Wo / CV_BM + 1 > 0x7FFFFFFF || (Cout + 63) / 64 > 65535) return 0;
  return 1;
}

extern "C" size_t uwu_conv2d_ws_bytes(int B, int H, int W, int C, int Cout, int KH, int KW, int stride, int ph, int pw, int ldx, int xoff,
                                      int ldy, int yoff, int dtype) {
  return 0;  // both dtypes run the implicit kernel: no column matrix exists
}

extern "C" int uwu_conv2d_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int Cout, int KH, int KW,
                              int stride, int ph, int pw, int ldx, int xoff, int ldy, int yoff, int relu, int dtype, void* ws,
                              size_t ws_bytes, void* stream) {
  UWU_CHECK_ARG(x && w && y, "conv2d_fwd: null pointer");
  UWU_CHECK_ARG(uwu_conv2d_ok(B, H, W, C, Cout, KH, KW, stride, ph, pw, ldx, xoff, ldy, yoff, dtype),
                "conv2d_fwd: shape not built: B = %d, H = %d, W = %d, C = %d, Cout = %d, kernel %d x %d, stride %d, padding (%d, %d), ldx = %d "
                "(offset %d), ldy = %d (offset %d), dtype %d (kernels 1x1 3x3 5x5 1x7 7x1 1x3 3x1, stride 1 | 2, padding below the kernel "
                "size, channels, strides and offsets multiples of 8, a slice inside its row)",
                B, H, W, C, Cout, KH, KW, stride, ph, pw, ldx, xoff, ldy, yoff, dtype);
  const size_t es = dtype == UWU_BF16 ? 2 : 4;
  UWU_CHECK_ARG((((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)bias) & 15) == 0, "conv2d_fwd: misaligned pointer");
  Conv2dP p;
  p.H = H, p.W = W, p.C = C, p.Cout = Cout, p.KH = KH, p.KW = KW, p.stride = stride, p.ph = ph, p.pw = pw;
  p.Ho = (H + 2 * ph - KH) / stride + 1, p.Wo = (W + 2 * pw - KW) / stride + 1;
  p.ldx = ldx, p.ldy = ldy, p.relu = relu != 0;
  p.M = (int64_t)B * p.Ho * p.Wo;
  // 128 pixels per workgroup (each weight fragment feeds twice the products) where that still leaves two workgroups per CU; among
  // those, 96 channels per workgroup where that divides Cout and 64 does not
  const bool wide = dtype == UWU_BF16 && (p.M + 127) / 128 * ((Cout + 63) / 64) >= 2 * (int64_t)uwu_dev_cus();
  const bool n96 = wide && Cout % 96 == 0 && Cout % 64 != 0;
  const int bm = wide ? 2 * CV_BM : CV_BM, bn = n96 ? 96 : 64;
  const dim3 grid((unsigned)((p.M + bm - 1) / bm), (unsigned)((Cout + bn - 1) / bn));
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
#define UWU_CONV_LAUNCH(T, MT, NT, PF) \
  hipLaunchKernelGGL((conv2d_kernel<T, MT, NT, PF>), grid, dim3(256), 0, st, (const T*)x + xoff, (const T*)w, bias, (T*)y + yoff, p)
  if (n96) UWU_CONV_LAUNCH(bf16_t, 2, 3, 1);
  else if (wide) UWU_CONV_LAUNCH(bf16_t, 2, 2, 1);
  else if (dtype == UWU_BF16) UWU_CONV_LAUNCH(bf16_t, 1, 2, 4);
  else UWU_CONV_LAUNCH(float, 1, 2, 2);
#undef UWU_CONV_LAUNCH
  prof.done(UWU_PROF_OTHER, dtype == UWU_BF16 ? 0 : 1, 2.0 * p.M * Cout * KH * KW * C,
            ((double)B * H * W * C + (double)p.M * Cout + (double)Cout * KH * KW * C) * es);
  UWU_LAUNCH_CHECK("conv2d_fwd");
  return UWU_OK;
}

extern "C" int uwu_inception_stem(const void* images, int in_u8, void* out, int B, int H, int W, int dtype, void* stream) {
  UWU_CHECK_ARG(images && out, "inception_stem: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "inception_stem: bad dtype %d", dtype);
  UWU_CHECK_ARG(B > 0 && H >= 3 && W >= 3 && (int64_t)B * H * W <= 0x7FFFFFFF / 8, "inception_stem: bad shape B = %d, H = %d, W = %d", B, H, W);
  UWU_CHECK_ARG(((uintptr_t)out & 15) == 0 && (in_u8 || ((uintptr_t)images & 3) == 0), "inception_stem: misaligned pointer");
  const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
  const int64_t rows = (int64_t)B * Ho * Wo;
  const int grid = ew_grid(rows * 32, 256);
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
#define UWU_STEM_LAUNCH(TI, TO) \
  hipLaunchKernelGGL((inception_stem_kernel<TI, TO>), dim3(grid), dim3(256), 0, st, (const TI*)images, (TO*)out, rows, H, W, Ho, Wo)
  if (in_u8) {
    if (dtype == UWU_BF16) UWU_STEM_LAUNCH(uint8_t, bf16_t);
    else UWU_STEM_LAUNCH(uint8_t, float);
  } else {
    if (dtype == UWU_BF16) UWU_STEM_LAUNCH(float, bf16_t);
    else UWU_STEM_LAUNCH(float, float);
  }
#undef UWU_STEM_LAUNCH
  prof.done(UWU_PROF_OTHER, dtype == UWU_BF16 ? 0 : 1, 0.0, 3.0 * B * H * W * (in_u8 ? 1 : 4) + (double)rows * 32 * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("inception_stem");
  return UWU_OK;
}

extern "C" int uwu_pool2d_fwd(const void* x, void* y, int B, int H, int W, int C, int mode, int ldx, int xoff, int ldy, int yoff, int dtype,
                              void* stream) {
  UWU_CHECK_ARG(x && y, "pool2d_fwd: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "pool2d_fwd: bad dtype %d", dtype);
  UWU_CHECK_ARG(mode == UWU_POOL_MAX_S2 || mode == UWU_POOL_MAX_S1P1 || mode == UWU_POOL_AVG_S1P1, "pool2d_fwd: bad mode %d", mode);
  UWU_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && (mode != UWU_POOL_MAX_S2 || (H >= 3 && W >= 3)),
                "pool2d_fwd: bad shape B = %d, H = %d, W = %d, C = %d (C a multiple of 8; the stride-2 pool needs H, W >= 3)", B, H, W, C);
  UWU_CHECK_ARG(ldx % 8 == 0 && ldy % 8 == 0 && xoff % 8 == 0 && yoff % 8 == 0 && xoff >= 0 && yoff >= 0 && (int64_t)xoff + C <= ldx &&
                    (int64_t)yoff + C <= ldy,
                "pool2d_fwd: strides and offsets must be multiples of 8 and the slices inside their rows: ldx = %d (offset %d), ldy = %d "
                "(offset %d), C = %d", ldx, xoff, ldy, yoff, C);
  UWU_CHECK_ARG((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "pool2d_fwd: misaligned pointer");
  const int Ho = mode == UWU_POOL_MAX_S2 ? (H - 3) / 2 + 1 : H, Wo = mode == UWU_POOL_MAX_S2 ? (W - 3) / 2 + 1 : W;
  const int64_t Mo = (int64_t)B * Ho * Wo;
  UWU_CHECK_ARG((int64_t)B * H * W <= 0x7FFFFFFF, "pool2d_fwd: too many pixels");
  const int grid = ew_grid(Mo * (C / 8), 256);
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
#define UWU_POOL_LAUNCH(T, MODE) \
  hipLaunchKernelGGL((pool2d_kernel<T, MODE>), dim3(grid), dim3(256), 0, st, (const T*)x + xoff, (T*)y + yoff, Mo, H, W, C, Ho, Wo, ldx, ldy)
  if (dtype == UWU_BF16) {
    if (mode == UWU_POOL_MAX_S2) UWU_POOL_LAUNCH(bf16_t, POOL_MAX_S2);
    else if (mode == UWU_POOL_MAX_S1P1) UWU_POOL_LAUNCH(bf16_t, POOL_MAX_S1P1);
    else UWU_POOL_LAUNCH(bf16_t, POOL_AVG_S1P1);
  } else {
    if (mode == UWU_POOL_MAX_S2) UWU_POOL_LAUNCH(float, POOL_MAX_S2);
    else if (mode == UWU_POOL_MAX_S1P1) UWU_POOL_LAUNCH(float, POOL_MAX_S1P1);
    else UWU_POOL_LAUNCH(float, POOL_AVG_S1P1);
  }
#undef UWU_POOL_LAUNCH
  prof.done(UWU_PROF_OTHER, dtype == UWU_BF16 ? 0 : 1, 0.0, ((double)B * H * W * C + (double)Mo * C) * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("pool2d_fwd");
  return UWU_OK;
}

extern "C" int uwu_relu_rows(void* y, int64_t M, int N, int ldy, int yoff, int dtype, void* stream) {
  UWU_CHECK_ARG(y, "relu_rows: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "relu_rows: bad dtype %d", dtype);
  UWU_CHECK_ARG(M > 0 && N > 0 && N % 8 == 0 && ldy % 8 == 0 && yoff % 8 == 0 && yoff >= 0 && (int64_t)yoff + N <= ldy && M <= 0x7FFFFFFF,
                "relu_rows: bad shape M = %lld, N = %d, ldy = %d (offset %d): N, ldy and the offset multiples of 8, the slice inside its row",
                (long long)M, N, ldy, yoff);
  UWU_CHECK_ARG(((uintptr_t)y & 15) == 0, "relu_rows: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  const int grid = ew_grid(M * (N / 8), 256);
  if (dtype == UWU_BF16) hipLaunchKernelGGL(relu_rows_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, (bf16_t*)y + yoff, M, N, ldy);
  else hipLaunchKernelGGL(relu_rows_kernel<float>, dim3(grid), dim3(256), 0, st, (float*)y + yoff, M, N, ldy);
  prof.done(UWU_PROF_OTHER, dtype == UWU_BF16 ? 0 : 1, 0.0, 2.0 * M * N * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("relu_rows");
  return UWU_OK;
}

extern "C" int uwu_global_avgpool(const void* x, float* out, int B, int HW, int C, int ldx, int dtype, void* stream) {
  UWU_CHECK_ARG(x && out, "global_avgpool: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "global_avgpool: bad dtype %d", dtype);
  UWU_CHECK_ARG(B > 0 && HW > 0 && C > 0 && ldx >= C && (int64_t)B * HW <= 0x7FFFFFFF, "global_avgpool: bad shape B = %d, HW = %d, C = %d, ldx = %d",
                B, HW, C, ldx);
  UWU_CHECK_ARG(((uintptr_t)out & 3) == 0 && ((uintptr_t)x & (dtype == UWU_BF16 ? 1 : 3)) == 0, "global_avgpool: misaligned pointer");
  const int64_t total = (int64_t)B * C;
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  if (dtype == UWU_BF16)
    hipLaunchKernelGGL(global_avgpool_kernel<bf16_t>, dim3(ew_grid(total, 256)), dim3(256), 0, st, (const bf16_t*)x, out, total, HW, C, ldx);
  else
    hipLaunchKernelGGL(global_avgpool_kernel<float>, dim3(ew_grid(total, 256)), dim3(256), 0, st, (const float*)x, out, total, HW, C, ldx);
  prof.done(UWU_PROF_OTHER, dtype == UWU_BF16 ? 0 : 1, (double)B * HW * C, (double)B * HW * C * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("global_avgpool");
  return UWU_OK;
}

extern "C" int uwu_fid_stats_accum(const float* features, double* acc, int B, int D, void* stream) {
  UWU_CHECK_ARG(features && acc, "fid_stats_accum: null pointer");
  UWU_CHECK_ARG(B > 0 && D > 0 && D % 64 == 0 && D <= 8192, "fid_stats_accum: bad shape B = %d, D = %d (D a multiple of 64, at most 8192)", B, D);
  UWU_CHECK_ARG(((uintptr_t)features & 3) == 0 && ((uintptr_t)acc & 7) == 0, "fid_stats_accum: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  hipLaunchKernelGGL(fid_sum_kernel, dim3(cdiv(D, 256)), dim3(256), 0, st, features, acc, acc + 1, B, D);
  hipLaunchKernelGGL(fid_outer_kernel, dim3(D / 64, D / 64), dim3(256), 0, st, features, acc + 1 + D, B, D);
  prof.done(UWU_PROF_OTHER, 1, 2.0 * B * D * D, 16.0 * D * D + 4.0 * B * D);
  UWU_LAUNCH_CHECK("fid_stats_accum");
  return UWU_OK;
}
