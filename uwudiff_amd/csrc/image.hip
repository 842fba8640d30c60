// Training images (reference src/duwu/data/utils.py:25-58, resize_and_crop_image) for a batch on the device: Pillow's 8-bit resampler
// restated (include/uwu_hip.h states the rule), the crop, ToTensor and Normalize(0.5, 0.5).  The coefficient tables are made on the
// host in double with libm's sin -- a device sin need not round like it -- and everything after them is integer arithmetic, so the
// result equals Image.resize byte for byte.
//
// Two launches per group of pictures, through a uint8 workspace:
//   resample_h_kernel  source rows row0 .. row0 + nrows - 1 (the rows the window's output rows touch), output columns left ..
//                      left + Wt - 1 only -> mid [nrows, stride] uint8, RGB interleaved, stride = Wt * 3 rounded up to 4
//   resample_v_kernel  mid -> out [3, Ht, Wt]; a lane takes four consecutive bytes of a mid row (one dword load per tap)
// The picture descriptors travel as kernel arguments, so the entry point copies nothing and waits for nothing.
#include <math.h>

#include <vector>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int IMG_GROUP = 16;  // pictures per launch (their descriptors are kernel arguments: 16 x 72 bytes)

// ---------------------------------------------------------------------------------------- host: the coefficient rule
double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
double lanczos_filter(double x) { return (-3.0 <= x && x < 3.0) ? sinc_filter(x) * sinc_filter(x / 3) : 0.0; }
double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

struct Filter {
  double (*fn)(double);
  double support;
};
bool filter_of(int id, Filter* f) {
  switch (id) {
    case UWU_FILTER_BILINEAR: *f = {bilinear_filter, 1.0}; return true;
    case UWU_FILTER_BICUBIC: *f = {bicubic_filter, 2.0}; return true;
    case UWU_FILTER_LANCZOS: *f = {lanczos_filter, 3.0}; return true;
  }
  return false;
}

struct Axis {
  double scale, fs, support;
  int in, ksize;
  Axis(int in_size, int out_size, double S) : in(in_size) {
    scale = (double)in_size / out_size;
    fs = scale < 1.0 ? 1.0 : scale;
    support = S * fs;
    ksize = (int)ceil(support) * 2 + 1;
  }
  void bounds(int xx, double* center, int* xmin, int* n) const {
    *center = (xx + 0.5) * scale;
    int lo = (int)(*center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(*center + support + 0.5);
    if (hi > in) hi = in;
    *xmin = lo;
    *n = hi - lo;
  }
};

// the source rows [row0, row0 + nrows) that output rows top .. top + Ht - 1 read (bounds are non-decreasing in the output index)
void row_span(int sh, int nh, int top, int Ht, double S, int* row0, int* nrows) {
  if (nh == sh) {
    *row0 = top;
    *nrows = Ht;
    return;
  }
  const Axis ax(sh, nh, S);
  double c;
  int lo, n0, hi, n1;
  ax.bounds(top, &c, &lo, &n0);
  ax.bounds(top + Ht - 1, &c, &hi, &n1);
  *row0 = lo;
  *nrows = hi + n1 - lo;
}

inline int mid_stride(int Wt) { return (Wt * 3 + 3) & ~3; }
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// ---------------------------------------------------------------------------------------- device
struct ImgDesc {
  const unsigned char* src;  // the picture: [sh, sw, 3]
  unsigned char* mid;        // [nrows, stride]
  const int32_t* ch;         // horizontal coeffs [Wt, kh]; nullptr: the pass is skipped (mid = the window's columns of src)
  const int32_t* bh;         // horizontal bounds [Wt, 2]
  const int32_t* cv;         // vertical coeffs [Ht, kv]; nullptr: skipped (out row y = mid row y)
  const int32_t* bv;         // vertical bounds [Ht, 2]
  int sw, kh, kv, row0, nrows, left;
};
struct ImgGroup {
  ImgDesc im[IMG_GROUP];
};

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// One source row of one output column: the taps' three channels, int32 accumulators.  K is the column's coefficient row, in LDS or
// in global memory (inlined once for each).  The taps are 3 n consecutive bytes from s, at any alignment: four taps at a time are
// 12 bytes = three dwords of that byte stream, each cut out of two aligned dwords (v_alignbyte_b32), so four aligned loads serve
// twelve multiply-adds; group g reads the aligned dwords 3 g .. 3 g + 3 from s rounded down to 4, that is up to 16 + 12 g bytes
// from there, and runs only where that stays below `end` (the end of the source buffer).  The last n % 4 taps, and the groups that
// would cross `end`, go byte by byte.
template <typename K>
__device__ __forceinline__ void h_pixel(const unsigned char* __restrict__ s, const unsigned char* end, K k, int n,
                                        unsigned char* __restrict__ m) {
  int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
  const unsigned shift = (unsigned)((uintptr_t)s & 3);
  const unsigned* q = reinterpret_cast<const unsigned*>(s - shift);
  const int64_t room = (end - (s - shift)) - 16;
  const int groups = room < 0 ? 0 : (int)min((int64_t)(n >> 2), room / 12 + 1);
  unsigned q0 = groups ? q[0] : 0u;
  for (int g = 0; g < groups; ++g) {
    const unsigned q1 = q[3 * g + 1], q2 = q[3 * g + 2], q3 = q[3 * g + 3];
    const unsigned w0 = __builtin_amdgcn_alignbyte(q1, q0, shift), w1 = __builtin_amdgcn_alignbyte(q2, q1, shift),
                   w2 = __builtin_amdgcn_alignbyte(q3, q2, shift);  // bytes 0-3, 4-7, 8-11 of the group: R G B R | G B R G | B R G B
    q0 = q3;
    const int c0 = k[4 * g], c1 = k[4 * g + 1], c2 = k[4 * g + 2], c3 = k[4 * g + 3];
    a0 += (int)(w0 & 255u) * c0 + (int)(w0 >> 24) * c1 + (int)((w1 >> 16) & 255u) * c2 + (int)((w2 >> 8) & 255u) * c3;
    a1 += (int)((w0 >> 8) & 255u) * c0 + (int)(w1 & 255u) * c1 + (int)(w1 >> 24) * c2 + (int)((w2 >> 16) & 255u) * c3;
    a2 += (int)((w0 >> 16) & 255u) * c0 + (int)((w1 >> 8) & 255u) * c1 + (int)(w2 & 255u) * c2 + (int)(w2 >> 24) * c3;
  }
  for (int t = 4 * groups; t < n; ++t) {
    const int c = k[t];
    a0 += (int)s[3 * t] * c;
    a1 += (int)s[3 * t + 1] * c;
    a2 += (int)s[3 * t + 2] * c;
  }
  m[0] = (unsigned char)clip8(a0), m[1] = (unsigned char)clip8(a1), m[2] = (unsigned char)clip8(a2);
}

// 64 output columns x 4 source rows per pass of a workgroup; blockIdx.y strides over the rows, blockIdx.z is the picture.  The 64
// columns' coefficient rows are copied to LDS once (a workgroup reuses them for every row it walks): read from global memory, lane x
// takes K[x][t], 64 addresses ksize * 4 bytes apart -- 64 cache lines per load.  In LDS the same addresses fall on distinct banks,
// because ksize is odd.  A table wider than H_LDS_TAPS (a reduction beyond 21-fold with Lanczos) is read from global memory.
constexpr int H_LDS_TAPS = 127;
__global__ void __launch_bounds__(256) resample_h_kernel(const ImgGroup g, const unsigned char* __restrict__ src_end, int Wt, int stride) {
  __shared__ int32_t kl[64 * H_LDS_TAPS];
  const ImgDesc& d = g.im[blockIdx.z];
  const int x0 = blockIdx.x * 64, lx = threadIdx.x & 63, x = x0 + lx;
  const bool staged = d.ch && d.kh <= H_LDS_TAPS;  // (the same in every lane of the workgroup)
  if (staged) {
    const int cnt = min(64, Wt - x0) * d.kh;
    const int32_t* from = d.ch + (int64_t)x0 * d.kh;
    for (int i = threadIdx.x; i < cnt; i += 256) kl[i] = from[i];
    __syncthreads();
  }
  if (x >= Wt) return;
  int xmin = d.left + x, n = 1;
  if (d.ch) {
    n = min(max(d.bh[2 * x + 1], 0), min(d.kh, d.sw));
    xmin = min(max(d.bh[2 * x], 0), d.sw - n);
  }
  for (int r = blockIdx.y * 4 + (threadIdx.x >> 6); r < d.nrows; r += gridDim.y * 4) {
    const unsigned char* s = d.src + ((int64_t)(d.row0 + r) * d.sw + xmin) * 3;
    unsigned char* m = d.mid + (int64_t)r * stride + 3 * x;
    if (!d.ch)
      m[0] = s[0], m[1] = s[1], m[2] = s[2];
    else if (staged)
      h_pixel(s, src_end, kl + lx * d.kh, n, m);
    else
      h_pixel(s, src_end, d.ch + (int64_t)x * d.kh, n, m);
  }
}

template <bool NORM>
__device__ __forceinline__ float level(int u) {
  const float v = (float)u / 255.f;  // ToTensor; IEEE division (the chain of torch operations, not u * (2 / 255) - 1)
  return NORM ? (v - 0.5f) / 0.5f : v;
}

// a lane owns bytes 4 j .. 4 j + 3 of output row y of the mid layout (byte i is channel i % 3 of column i / 3)
template <typename T, bool NORM>
__global__ void __launch_bounds__(256) resample_v_kernel(const ImgGroup g, T* __restrict__ out, int b0, int Ht, int Wt, int stride) {
  const ImgDesc& d = g.im[blockIdx.z];
  const int n4 = stride >> 2;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= Ht * n4) return;
  const int y = idx / n4, j = idx - y * n4;
  int a[4];
  if (d.cv) {
    const int n = min(max(d.bv[2 * y + 1], 0), min(d.kv, d.nrows));
    const int r0 = min(max(d.bv[2 * y] - d.row0, 0), d.nrows - n);
    const int32_t* k = d.cv + (int64_t)y * d.kv;
    const unsigned char* m = d.mid + (int64_t)r0 * stride + 4 * j;
    a[0] = a[1] = a[2] = a[3] = 1 << (PRECISION_BITS - 1);
    for (int t = 0; t < n; ++t) {
      const unsigned v = *reinterpret_cast<const unsigned*>(m + (int64_t)t * stride);
      const int c = k[t];
      a[0] += (int)(v & 255u) * c;
      a[1] += (int)((v >> 8) & 255u) * c;
      a[2] += (int)((v >> 16) & 255u) * c;
      a[3] += (int)(v >> 24) * c;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = clip8(a[i]);
  } else {
    const unsigned v = *reinterpret_cast<const unsigned*>(d.mid + (int64_t)y * stride + 4 * j);
    a[0] = v & 255u, a[1] = (v >> 8) & 255u, a[2] = (v >> 16) & 255u, a[3] = v >> 24;
  }
  T* o = out + (int64_t)(b0 + blockIdx.z) * 3 * Ht * Wt + (int64_t)y * Wt;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = 4 * j + i, x = e / 3, c = e - 3 * x;
    if (x < Wt) o[(int64_t)c * Ht * Wt + x] = from_f32<T>(level<NORM>(a[i]));
  }
}

const char* check_meta(int B, const int32_t* meta, int Ht, int Wt) {
  for (int b = 0; b < B; ++b) {
    const int32_t* m = meta + 6 * b;
    const int sh = m[0], sw = m[1], nh = m[2], nw = m[3], top = m[4], left = m[5];
    if (sh < 1 || sw < 1 || nh < 1 || nw < 1) return "a picture or its resized size has a side < 1";
    if (nh < Ht || nw < Wt) return "a resized size is smaller than the target";
    if (top < 0 || left < 0 || top > nh - Ht || left > nw - Wt) return "a window leaves the resized picture";
  }
  return nullptr;
}

}  // namespace

extern "C" int uwu_resample_ksize(int in_size, int out_size, int filter) {
  Filter f;
  UWU_CHECK_ARG(filter_of(filter, &f), "resample_ksize: bad filter %d", filter);
  UWU_CHECK_ARG(in_size >= 1 && out_size >= 1, "resample_ksize: bad sizes in=%d out=%d", in_size, out_size);
  return Axis(in_size, out_size, f.support).ksize;
}

extern "C" int uwu_resample_coeffs(int in_size, int out_size, int filter, int first, int count, int32_t* coeffs, int32_t* bounds) {
  Filter f;
  UWU_CHECK_ARG(filter_of(filter, &f), "resample_coeffs: bad filter %d", filter);
  UWU_CHECK_ARG(in_size >= 1 && out_size >= 1, "resample_coeffs: bad sizes in=%d out=%d", in_size, out_size);
  UWU_CHECK_ARG(first >= 0 && count >= 1 && first <= out_size - count, "resample_coeffs: outputs %d .. %d + %d leave 0 .. %d", first, first,
                count, out_size);
  UWU_CHECK_ARG(coeffs && bounds, "resample_coeffs: null pointer");
  const Axis ax(in_size, out_size, f.support);
  std::vector<double> w((size_t)ax.ksize);
  for (int i = 0; i < count; ++i) {
    double center;
    int xmin, n;
    ax.bounds(first + i, &center, &xmin, &n);
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      w[x] = f.fn((x + xmin - center + 0.5) / ax.fs);
      ww += w[x];
    }
    int32_t* k = coeffs + (size_t)i * ax.ksize;
    for (int x = 0; x < ax.ksize; ++x) {
      if (x >= n) {
        k[x] = 0;
        continue;
      }
      const double v = ww != 0.0 ? w[x] / ww : w[x];
      k[x] = v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS));
    }
    bounds[2 * i] = xmin;
    bounds[2 * i + 1] = n;
  }
  return UWU_OK;
}

extern "C" size_t uwu_image_resize_crop_ws_bytes(int B, const int32_t* meta, int Ht, int Wt, int filter) {
  Filter f;
  if (B < 1 || Ht < 1 || Wt < 1 || !meta || !filter_of(filter, &f) || check_meta(B, meta, Ht, Wt)) return 0;
  size_t total = 0;
  for (int b = 0; b < B; ++b) {
    int row0, nrows;
    row_span(meta[6 * b], meta[6 * b + 2], meta[6 * b + 4], Ht, f.support, &row0, &nrows);
    total += align16((size_t)nrows * mid_stride(Wt));
  }
  return total;
}

extern "C" int uwu_image_resize_crop(const void* src, int64_t src_bytes, const int64_t* src_off, const int32_t* meta, const int32_t* tables,
                                     int64_t tables_len, const int64_t* tab_off, void* out, int dtype, int B, int Ht, int Wt, int filter,
                                     int normalize, void* ws, size_t ws_bytes, void* stream) {
  Filter f;
  UWU_CHECK_ARG(filter_of(filter, &f), "image_resize_crop: bad filter %d", filter);
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "image_resize_crop: bad dtype %d", dtype);
  UWU_CHECK_ARG(normalize == 0 || normalize == 1, "image_resize_crop: normalize must be 0 or 1, got %d", normalize);
  UWU_CHECK_ARG(B >= 1 && Ht >= 1 && Wt >= 1, "image_resize_crop: bad shape B=%d Ht=%d Wt=%d", B, Ht, Wt);
  UWU_CHECK_ARG((int64_t)Ht * mid_stride(Wt) < ((int64_t)1 << 31), "image_resize_crop: target %d x %d too large", Ht, Wt);
  UWU_CHECK_ARG(src && out && ws && tables && src_off && meta && tab_off, "image_resize_crop: null pointer");
  UWU_CHECK_ARG((((uintptr_t)src | (uintptr_t)out | (uintptr_t)ws | (uintptr_t)tables) & 15) == 0,
                "image_resize_crop: device pointers must be 16-byte aligned");
  const char* bad = check_meta(B, meta, Ht, Wt);
  UWU_CHECK_ARG(!bad, "image_resize_crop: %s", bad);
  const size_t need = uwu_image_resize_crop_ws_bytes(B, meta, Ht, Wt, filter);
  UWU_CHECK_ARG(ws_bytes >= need, "image_resize_crop: workspace of %zu bytes, %zu needed", ws_bytes, need);
  const int stride = mid_stride(Wt);
  std::vector<ImgDesc> descs((size_t)B);
  size_t ws_at = 0;
  int max_rows = 1;
  for (int b = 0; b < B; ++b) {
    const int32_t* m = meta + 6 * b;
    const int sh = m[0], sw = m[1], nh = m[2], nw = m[3], top = m[4], left = m[5];
    const int64_t bytes = (int64_t)sh * sw * 3;
    UWU_CHECK_ARG(src_off[b] >= 0 && src_off[b] <= src_bytes - bytes, "image_resize_crop: picture %d (%d x %d at byte %lld) leaves the %lld bytes of src",
                  b, sh, sw, (long long)src_off[b], (long long)src_bytes);
    ImgDesc& d = descs[b];
    d.src = (const unsigned char*)src + src_off[b];
    d.sw = sw;
    d.left = left;
    d.ch = d.bh = d.cv = d.bv = nullptr;
    d.kh = d.kv = 0;
    const int64_t* t = tab_off + 4 * b;
    if (nw != sw) {
      d.kh = Axis(sw, nw, f.support).ksize;
      UWU_CHECK_ARG(t[0] >= 0 && t[0] <= tables_len - (int64_t)Wt * d.kh && t[1] >= 0 && t[1] <= tables_len - 2 * (int64_t)Wt,
                    "image_resize_crop: the horizontal tables of picture %d leave the %lld elements of tables", b, (long long)tables_len);
      d.ch = tables + t[0];
      d.bh = tables + t[1];
    }
    if (nh != sh) {
      d.kv = Axis(sh, nh, f.support).ksize;
      UWU_CHECK_ARG(t[2] >= 0 && t[2] <= tables_len - (int64_t)Ht * d.kv && t[3] >= 0 && t[3] <= tables_len - 2 * (int64_t)Ht,
                    "image_resize_crop: the vertical tables of picture %d leave the %lld elements of tables", b, (long long)tables_len);
      d.cv = tables + t[2];
      d.bv = tables + t[3];
    }
    row_span(sh, nh, top, Ht, f.support, &d.row0, &d.nrows);
    d.mid = (unsigned char*)ws + ws_at;
    ws_at += align16((size_t)d.nrows * stride);
    if (d.nrows > max_rows) max_rows = d.nrows;
  }
  // every check has passed: launch
  const int vgrid = cdiv((int64_t)Ht * (stride >> 2), 256);
  for (int b0 = 0; b0 < B; b0 += IMG_GROUP) {
    const int nb = B - b0 < IMG_GROUP ? B - b0 : IMG_GROUP;
    ImgGroup g;
    int rows = 1;
    for (int i = 0; i < IMG_GROUP; ++i) {
      g.im[i] = descs[b0 + (i < nb ? i : 0)];
      if (i < nb && g.im[i].nrows > rows) rows = g.im[i].nrows;
    }
    const int ygrid = cdiv(rows, 4) < 256 ? cdiv(rows, 4) : 256;
    hipLaunchKernelGGL(resample_h_kernel, dim3(cdiv(Wt, 64), ygrid, nb), dim3(256), 0, (hipStream_t)stream, g,
                       (const unsigned char*)src + src_bytes, Wt, stride);
    UWU_LAUNCH_CHECK("image_resize_crop (horizontal)");
    const dim3 vg(vgrid, 1, nb);
#define UWU_V(T, NORM) hipLaunchKernelGGL((resample_v_kernel<T, NORM>), vg, dim3(256), 0, (hipStream_t)stream, g, (T*)out, b0, Ht, Wt, stride)
    if (dtype == UWU_F32) {
      if (normalize) UWU_V(float, true); else UWU_V(float, false);
    } else {
      if (normalize) UWU_V(bf16_t, true); else UWU_V(bf16_t, false);
    }
#undef UWU_V
    UWU_LAUNCH_CHECK("image_resize_crop (vertical)");
  }
  return UWU_OK;
}
