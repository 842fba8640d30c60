// Fast-math probe: how far are the rotation factors of csrc/rope.hip from their exact values?  The rope kernels compute
//   ef = __expf(f);  th = p * ef;  __sincosf(th, &sn, &cs);  factors cs - sn and cs + sn
// with the hardware exp / sin / cos.  This evaluates exactly those expressions on a grid of log-frequencies
// f in [ln(pi) - 1, ln(10 pi)] (the shipped init spans ln(pi) .. ln(10 pi); - 1 leaves room below) and positions p in [-1, 1],
// and prints, per octave of |theta| = |p| e^f, the worst |fast - fp64| of either factor, fp64 = cos / sin of (double)p * exp((double)f)
// on the host.  tests/test_edge_kernels_gpu.py takes E_FAST(|theta|) = twice the worst of the octave (the grid samples, it does
// not enumerate); profiles/edge_kernels_accuracy_mi355x.txt keeps the table.
//   hipcc --offload-arch=gfx950 -O3 -o probe_fastmath tools/probes/probe_fastmath.hip && ./probe_fastmath
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(e)                                                                        \
  do {                                                                                  \
    hipError_t err_ = (e);                                                              \
    if (err_ != hipSuccess) {                                                           \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(err_));      \
      return 1;                                                                         \
    }                                                                                   \
  } while (0)

constexpr int NF = 4096, NP = 4097;  // NP odd: p = 0 and p = +-1 are grid points

__host__ __device__ inline float grid_f(int i, float f_lo, float f_hi) { return f_lo + (f_hi - f_lo) * ((float)i / (float)(NF - 1)); }
__host__ __device__ inline float grid_p(int j) { return -1.f + 2.f * ((float)j / (float)(NP - 1)); }

__global__ void __launch_bounds__(256) fast_kernel(float f_lo, float f_hi, float* __restrict__ minus, float* __restrict__ plus,
                                                   float* __restrict__ fs, float* __restrict__ ps) {
  const int64_t total = (int64_t)NF * NP, step = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += step) {
    const int i = (int)(idx / NP), j = (int)(idx - (int64_t)i * NP);
    const float f = grid_f(i, f_lo, f_hi), p = grid_p(j);
    const float ef = __expf(f);
    const float th = p * ef;
    float sn, cs;
    __sincosf(th, &sn, &cs);
    minus[idx] = cs - sn;
    plus[idx] = cs + sn;
    if (j == 0) fs[i] = f;  // the inputs as the device saw them (the host reads these, not its own restatement)
    if (i == 0) ps[j] = p;
  }
}

int main() {
  const float f_lo = logf(3.14159265358979f) - 1.f, f_hi = logf(31.4159265358979f);
  const size_t total = (size_t)NF * NP;
  float *d_minus, *d_plus, *d_f, *d_p;
  CHECK(hipMalloc(&d_minus, total * sizeof(float)));
  CHECK(hipMalloc(&d_plus, total * sizeof(float)));
  CHECK(hipMalloc(&d_f, NF * sizeof(float)));
  CHECK(hipMalloc(&d_p, NP * sizeof(float)));
  fast_kernel<<<2048, 256>>>(f_lo, f_hi, d_minus, d_plus, d_f, d_p);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  float* minus = (float*)malloc(total * sizeof(float));
  float* plus = (float*)malloc(total * sizeof(float));
  float* fs = (float*)malloc(NF * sizeof(float));
  float* ps = (float*)malloc(NP * sizeof(float));
  if (!minus || !plus || !fs || !ps) return 1;
  CHECK(hipMemcpy(minus, d_minus, total * sizeof(float), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(plus, d_plus, total * sizeof(float), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(fs, d_f, NF * sizeof(float), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(ps, d_p, NP * sizeof(float), hipMemcpyDeviceToHost));

  // octave b: 2^(b-3) <= |theta| < 2^(b-2) for b = 1..7 (up to 32); b = 0 takes everything below 1/4
  constexpr int NB = 8;
  double worst[NB] = {0}, at_th[NB] = {0};
  long count[NB] = {0};
  double max_th = 0;
  for (int i = 0; i < NF; ++i) {
    const double e = exp((double)fs[i]);
    for (int j = 0; j < NP; ++j) {
      const double th = (double)ps[j] * e, a = fabs(th);
      const size_t idx = (size_t)i * NP + j;
      const double c = cos(th), s = sin(th);
      const double err = fmax(fabs((double)minus[idx] - (c - s)), fabs((double)plus[idx] - (c + s)));
      int b = 0;
      for (double lim = 0.25; b < NB - 1 && a >= lim; lim *= 2) ++b;
      ++count[b];
      if (!(err <= worst[b])) worst[b] = err, at_th[b] = th;  // (a NaN lands here and is printed)
      if (a > max_th) max_th = a;
    }
  }
  printf("probe_fastmath: ef = __expf(f); __sincosf(p * ef); factors cs - sn, cs + sn against host fp64\n");
  printf("grid: %d f in [%.6f, %.6f] x %d p in [-1, 1]; max |theta| %.4f\n", NF, fs[0], fs[NF - 1], NP, max_th);
  printf("%-22s %12s %14s %12s %14s\n", "|theta| in", "points", "worst |err|", "/ 2^-9", "at theta");
  for (int b = 0; b < NB; ++b) {
    char range[32];
    snprintf(range, sizeof range, "[%g, %g)", b == 0 ? 0.0 : ldexp(1.0, b - 3), ldexp(1.0, b - 2));
    printf("%-22s %12ld %14.3e %12.5f %14.6f\n", range, count[b], worst[b], worst[b] / ldexp(1.0, -9), at_th[b]);
  }
  free(minus), free(plus), free(fs), free(ps);
  CHECK(hipFree(d_minus));
  CHECK(hipFree(d_plus));
  CHECK(hipFree(d_f));
  CHECK(hipFree(d_p));
  return 0;
}
