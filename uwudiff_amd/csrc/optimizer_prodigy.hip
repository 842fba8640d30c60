// prodigyopt.Prodigy (Mishchenko & Defazio, "Prodigy: An Expeditiously Adaptive Parameter-Free Learner") on a flat buffer:
// three kernels round two global sums, 40 + 18 B/param with the shadow and the zeroed gradient.
// One step of the package, with g = grad * pre_scale * clip[1]:
//   beta3 = beta3 or sqrt(beta2) ; bc = sqrt(1 - beta2^(k+1)) / (1 - beta1^(k+1)) if use_bias_correction else 1
//   dlr   = d * lr * bc                                                  (the OLD d)
//   if weight_decay != 0 and not decouple:  g += weight_decay * p
//   d_numerator = beta3 * d_numerator + (d/d0) * dlr * sum_i g_i (p0_i - p_i)
//   exp_avg     = beta1 * exp_avg    + d * (1-beta1) * g
//   exp_avg_sq  = beta2 * exp_avg_sq + d*d * (1-beta2) * g*g
//   s           = beta3 * s + (d/d0) * (d if safeguard_warmup else dlr) * g
//   d_denom     = sum_i |s_i|
//   if d_denom == 0:  return         (p, the shadow and k keep their values)
//   d_hat = d_coef * d_numerator / d_denom ; if d == d0: d = max(d, d_hat)
//   d_max = max(d_max, d_hat) ; d = min(d_max, d * growth_rate)
//   if weight_decay != 0 and decouple:  p *= 1 - weight_decay * dlr
//   p -= dlr * exp_avg / (sqrt(exp_avg_sq) + d * eps)                    (the OLD dlr, the NEW d)
//   k += 1
// lr == 0 skips the moments, s and both sums, as the package does (d_numerator still decays, d_denom is then 0: the return).
//
// The two sums are global, so a step is three launches: `prodigy_stats_kernel` per chunk (moments + one partial of each sum per
// workgroup), `prodigy_finalize_kernel` (one workgroup: the scalar recurrence) and `prodigy_apply_kernel` (the update).  The
// scalars never leave the device: they live in a block of UWU_PRODIGY_SCALARS doubles (the UWU_PRODIGY_* indices of uwu_hip.h).
#include "optimizer_shared.h"

// d * lr * bc from the block's d and k: the statistics pass and the finalize pass both call this, so they use the same dlr
__device__ __forceinline__ double prodigy_dlr(double d, double k, double lr, double beta1, double beta2, int use_bc) {
  double bc = 1.0;
  if (use_bc) bc = sqrt(1.0 - pow(beta2, k + 1.0)) / (1.0 - pow(beta1, k + 1.0));
  return d * lr * bc;
}

struct ProdigyCoef {
  double gscale, wd_coupled, b1, c1, b2, c2, b3, cs;
};

// one element in double: the products, p0 - p and the sums carry no fp32 rounding; each stored moment is rounded to fp32 once.
// Fused (in double): gscale*g + (.), num + (p0 - p)*g, b1*m + (.), b2*v + (.), b3*s + (.).  Rounded to double first: wd*p, p0 - p,
// c1*g, c2*g, (c2*g)*g, cs*g.
__device__ __forceinline__ void prodigy_elem(float p, float g, float p0, float& m, float& v, float& s, const ProdigyCoef& c,
                                             double& num, double& den) {
  const double pd = (double)p;
  const double gd = __builtin_fma(c.gscale, (double)g, c.wd_coupled * pd);
  num = __builtin_fma((double)p0 - pd, gd, num);
  m = (float)__builtin_fma(c.b1, (double)m, c.c1 * gd);
  v = (float)__builtin_fma(c.b2, (double)v, gd * (c.c2 * gd));
  s = (float)__builtin_fma(c.b3, (double)s, c.cs * gd);
  den += fabs((double)s);  // of the value as stored
}

// 24 B read + 12 B written per parameter (+ 4 B for the zeroed gradient).  ws[2 * (slot0 + blockIdx.x)] and the word after it
// receive this workgroup's partials of g.(p0 - p) and |s|: a slot of its own, no atomics.
__global__ void __launch_bounds__(256) prodigy_stats_kernel(const float* __restrict__ p, float* __restrict__ g,
                                                            const float* __restrict__ p0, float* __restrict__ m,
                                                            float* __restrict__ v, float* __restrict__ s, int64_t n,
                                                            const double* __restrict__ scal, double* __restrict__ ws,
                                                            int64_t slot0, double lr, double beta1, double omb1, double beta2,
                                                            double omb2, double beta3, double wd_coupled, double d0,
                                                            int use_bc, int safeguard, float pre_scale,
                                                            const float* __restrict__ clip, int zero_grad) {
  __shared__ double red[256];
  double num = 0.0, den = 0.0;
  if (lr > 0.0) {
    const double d = scal[UWU_PRODIGY_D];
    const double dlr = prodigy_dlr(d, scal[UWU_PRODIGY_K], lr, beta1, beta2, use_bc);
    ProdigyCoef c;
    c.gscale = (double)grad_scale(pre_scale, clip);  // the fp32 factor uwu_adamw_step multiplies by
    c.wd_coupled = wd_coupled;
    c.b1 = beta1;
    c.c1 = d * omb1;
    c.b2 = beta2;
    c.c2 = d * d * omb2;
    c.b3 = beta3;
    c.cs = (d / d0) * (safeguard ? d : dlr);
    for_each_group<4>(n, 0, [&](int64_t e) {
      const f32x4 pv = load4(p + e), gv = load4(g + e), qv = load4(p0 + e);
      f32x4 mv = load4(m + e), vv = load4(v + e), sv = load4(s + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float mm = mv[j], vn = vv[j], ss = sv[j];
        prodigy_elem(pv[j], gv[j], qv[j], mm, vn, ss, c, num, den);
        mv[j] = mm;
        vv[j] = vn;
        sv[j] = ss;
      }
      store4(m + e, mv);
      store4(v + e, vv);
      store4(s + e, sv);
      if (zero_grad) store4(g + e, f32x4{0.f, 0.f, 0.f, 0.f});
    }, [&](int64_t i) {
      prodigy_elem(p[i], g[i], p0[i], m[i], v[i], s[i], c, num, den);
      if (zero_grad) g[i] = 0.f;
    });
  } else if (zero_grad) {  // lr == 0: no statistics; the gradient is consumed all the same
    for_each_group<4>(n, 0, [&](int64_t e) { store4(g + e, f32x4{0.f, 0.f, 0.f, 0.f}); }, [&](int64_t i) { g[i] = 0.f; });
  }
  num = block_sum_f64(num, red);
  den = block_sum_f64(den, red);
  if (threadIdx.x == 0) {
    ws[2 * (slot0 + blockIdx.x)] = num;
    ws[2 * (slot0 + blockIdx.x) + 1] = den;
  }
}

// One workgroup: the partials of all chunks added in slot order, then the scalar recurrence; thread 0 writes the block.
__global__ void __launch_bounds__(256) prodigy_finalize_kernel(double* __restrict__ scal, const double* __restrict__ ws,
                                                               int64_t nslots, double lr, double beta1, double beta2,
                                                               double beta3, double d0, double d_coef, double growth_rate,
                                                               int use_bc) {
  __shared__ double red[256];
  double num = 0.0, den = 0.0;
  for (int64_t i = threadIdx.x; i < nslots; i += 256) {
    num += ws[2 * i];
    den += ws[2 * i + 1];
  }
  num = block_sum_f64(num, red);
  den = block_sum_f64(den, red);
  if (threadIdx.x != 0) return;
  double d = scal[UWU_PRODIGY_D], d_max = scal[UWU_PRODIGY_D_MAX];
  const double dlr = prodigy_dlr(d, scal[UWU_PRODIGY_K], lr, beta1, beta2, use_bc);
  const double d_numerator = __builtin_fma(beta3, scal[UWU_PRODIGY_D_NUMERATOR], (d / d0) * dlr * num);
  scal[UWU_PRODIGY_D_NUMERATOR] = d_numerator;
  scal[UWU_PRODIGY_D_DENOM] = den;
  scal[UWU_PRODIGY_DLR] = dlr;
  if (den == 0.0) {
    scal[UWU_PRODIGY_SKIPPED] = 1.0;
    return;
  }
  const double d_hat = d_coef * d_numerator / den;
  if (d == d0) d = fmax(d, d_hat);
  d_max = fmax(d_max, d_hat);
  d = fmin(d_max, d * growth_rate);
  scal[UWU_PRODIGY_D] = d;
  scal[UWU_PRODIGY_D_MAX] = d_max;
  scal[UWU_PRODIGY_D_HAT] = d_hat;
  scal[UWU_PRODIGY_K] = scal[UWU_PRODIGY_K] + 1.0;
  scal[UWU_PRODIGY_SKIPPED] = 0.0;
}

// 12 B read + 4 B written per parameter (+ 2 B for the shadow): the decoupled decay and the update with the step's dlr (the old d)
// and the new d, in fp32; nothing at all when the step returned early.
// Fused: decay*p - (.).  Rounded first: sqrt(v) + d*eps, the quotient, dlr*quotient.
__device__ __forceinline__ float prodigy_apply_elem(float p, float m, float v, float decay, float dlr, float deps) {
  const float upd = dlr * (m / (sqrtf(v) + deps));
  return __builtin_fmaf(p, decay, -upd);
}

__global__ void __launch_bounds__(256) prodigy_apply_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                            const float* __restrict__ v, bf16_t* __restrict__ pbf, int64_t n,
                                                            const double* __restrict__ scal, double eps, double wd_decoupled) {
  if (scal[UWU_PRODIGY_SKIPPED] != 0.0) return;
  const double dlr_d = scal[UWU_PRODIGY_DLR];
  // 1 - wd*dlr is one fused multiply-add in double, rounded to fp32 once
  const float dlr = (float)dlr_d, deps = (float)(scal[UWU_PRODIGY_D] * eps);
  const float decay = (float)__builtin_fma(-wd_decoupled, dlr_d, 1.0);
  for_each_group<4>(n, 0, [&](int64_t e) {
    f32x4 pv = load4(p + e);
    const f32x4 mv = load4(m + e), vv = load4(v + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) pv[j] = prodigy_apply_elem(pv[j], mv[j], vv[j], decay, dlr, deps);
    store4(p + e, pv);
    if (pbf) store4(pbf + e, pv);
  }, [&](int64_t i) {
    const float pp = prodigy_apply_elem(p[i], m[i], v[i], decay, dlr, deps);
    p[i] = pp;
    if (pbf) pbf[i] = (bf16_t)pp;
  });
}

extern "C" int uwu_prodigy_stats_blocks(int64_t n) { return n > 0 ? ew_grid(n / 4, 256) : 0; }

extern "C" int uwu_prodigy_stats(const float* p, float* g, const float* p0, float* exp_avg, float* exp_avg_sq, float* s,
                                 int64_t n, const double* scalars, double* ws, int64_t ws_slots, int64_t slot0, double lr,
                                 double beta1, double beta2, double beta3, double weight_decay, int decouple, double d0,
                                 int use_bias_correction, int safeguard_warmup, float pre_scale, const float* clip,
                                 int zero_grad, void* stream) {
  UWU_CHECK_ARG(p && g && p0 && exp_avg && exp_avg_sq && s && scalars && ws, "prodigy_stats: null pointer");
  UWU_CHECK_ARG(n > 0, "prodigy_stats: n must be positive");
  UWU_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)p0 | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)s) & 15) == 0,
                "prodigy_stats: buffers must be 16-byte aligned");
  UWU_CHECK_ARG((((uintptr_t)scalars | (uintptr_t)ws) & 7) == 0, "prodigy_stats: scalars and workspace must be 8-byte aligned");
  UWU_CHECK_ARG(lr >= 0.0 && d0 > 0.0, "prodigy_stats: lr must be >= 0 and d0 > 0");
  const int grid = ew_grid(n / 4, 256);
  UWU_CHECK_ARG(slot0 >= 0 && ws_slots >= 0 && slot0 <= ws_slots - grid,
                "prodigy_stats: workspace too small (%lld slots from %lld needed, %lld given)", (long long)grid,
                (long long)slot0, (long long)ws_slots);
  // 1 - beta in double on the host, as the package does with python floats (see uwu_lion_step)
  hipLaunchKernelGGL(prodigy_stats_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, p0, exp_avg, exp_avg_sq, s, n,
                     scalars, ws, slot0, lr, beta1, 1.0 - beta1, beta2, 1.0 - beta2, beta3,
                     (weight_decay != 0.0 && !decouple) ? weight_decay : 0.0, d0, use_bias_correction, safeguard_warmup,
                     pre_scale, clip, zero_grad);
  UWU_LAUNCH_CHECK("prodigy_stats");
  return UWU_OK;
}

extern "C" int uwu_prodigy_finalize(double* scalars, const double* ws, int64_t nslots, double lr, double beta1, double beta2,
                                    double beta3, double d0, double d_coef, double growth_rate, int use_bias_correction,
                                    void* stream) {
  UWU_CHECK_ARG(scalars && ws, "prodigy_finalize: null pointer");
  UWU_CHECK_ARG((((uintptr_t)scalars | (uintptr_t)ws) & 7) == 0, "prodigy_finalize: scalars and workspace must be 8-byte aligned");
  UWU_CHECK_ARG(nslots > 0, "prodigy_finalize: no partials (nslots must be positive)");
  UWU_CHECK_ARG(lr >= 0.0 && d0 > 0.0, "prodigy_finalize: lr must be >= 0 and d0 > 0");
  hipLaunchKernelGGL(prodigy_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scalars, ws, nslots, lr, beta1, beta2,
                     beta3, d0, d_coef, growth_rate, use_bias_correction);
  UWU_LAUNCH_CHECK("prodigy_finalize");
  return UWU_OK;
}

extern "C" int uwu_prodigy_apply(float* p, const float* exp_avg, const float* exp_avg_sq, void* p_bf16, int64_t n,
                                 const double* scalars, double eps, double weight_decay, int decouple, void* stream) {
  UWU_CHECK_ARG(p && exp_avg && exp_avg_sq && scalars, "prodigy_apply: null pointer");
  UWU_CHECK_ARG(n > 0, "prodigy_apply: n must be positive");
  UWU_CHECK_ARG((((uintptr_t)p | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0,
                "prodigy_apply: buffers must be 16-byte aligned");
  UWU_CHECK_ARG(((uintptr_t)scalars & 7) == 0, "prodigy_apply: scalars must be 8-byte aligned");
  UWU_CHECK_ARG(p_bf16 == nullptr || ((uintptr_t)p_bf16 & 7) == 0, "prodigy_apply: bf16 shadow must be 8-byte aligned");
  hipLaunchKernelGGL(prodigy_apply_kernel, dim3(ew_grid(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, p, exp_avg, exp_avg_sq,
                     (bf16_t*)p_bf16, n, scalars, eps, (weight_decay != 0.0 && decouple) ? weight_decay : 0.0);
  UWU_LAUNCH_CHECK("prodigy_apply");
  return UWU_OK;
}

