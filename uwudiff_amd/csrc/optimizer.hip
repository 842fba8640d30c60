// Flat-buffer optimizer kernels: global grad norm (+clip coefficient), fused AdamW / Lion / AdamWFP16 with bf16 shadow
// refresh, the weight average (update, exchange with the weights), dtype casts.  HBM-bound: AdamW moves 28 B/param, Lion and
// AdamWFP16 20 B/param (+2 B/param for the bf16 shadow, +4 B/param for the zeroed gradient), the average's update 12 B/param.
// Schedule-free AdamW (next to the weight average, whose exchange kernel it uses) moves AdamW's 28 B/param; its average 12 B/param.
// Prodigy is in optimizer_prodigy.hip, the 8-bit block-wise AdamW / Lion in optimizer_8bit.hip, Adafactor in
// optimizer_adafactor.hip; optimizer_shared.h holds the traversal every kernel here runs on, the AdamW and Lion rules and the
// rounding contract all of them keep.
// Reference: src/duwu/trainer/trainer.py:52-74 (torch.optim.AdamW + Lightning gradient_clip_val),
// src/duwu/trainer/optimizers.py (AdamWFP16), lion_pytorch.Lion (configs/demo_training*.yaml, commented alternative).
#include "optimizer_shared.h"

// stage 1: per-block partial sums (deterministic order), stage 2: one block folds the partials
__global__ void __launch_bounds__(256) sqnorm_partial_kernel(const float* __restrict__ g, int64_t n,
                                                             float* __restrict__ partial) {
  __shared__ float red[4];
  float a = 0.f;  // every square is rounded, then added
  for_each_group<4>(n, 0, [&](int64_t e) {
    const f32x4 v = load4(g + e);
    a += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }, [&](int64_t i) { a += g[i] * g[i]; });
  float t = block_sum<4>(a, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ void __launch_bounds__(256) sqnorm_final_kernel(const float* __restrict__ partial, int np,
                                                           float pre_scale, float max_norm,
                                                           float* __restrict__ out) {
  __shared__ float red[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < np; i += 256) a += partial[i];
  float t = block_sum<4>(a, red);
  if (threadIdx.x == 0) {
    float sq = t * pre_scale * pre_scale;
    out[0] = sq;
    float coef = 1.f;
    if (max_norm > 0.f) {
      // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
      coef = fminf(max_norm / (sqrtf(sq) + 1e-6f), 1.f);
    }
    out[1] = coef;
  }
}

// adamw_elem (optimizer_shared.h) over the flat buffer.  1 - lr*wd is one fused multiply-add and 1 - b1, 1 - b2 are fp32
// differences, all formed here on the device.
__global__ void __launch_bounds__(256) adamw_kernel(float* __restrict__ p, float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    bf16_t* __restrict__ pbf, int64_t n, float lr, float b1,
                                                    float b2, float eps, float wd, float step_size,
                                                    float inv_bc2_sqrt, float pre_scale,
                                                    const float* __restrict__ clip, int zero_grad) {
  const float gscale = grad_scale(pre_scale, clip);
  const float decay = __builtin_fmaf(-lr, wd, 1.f), omb1 = 1.f - b1, omb2 = 1.f - b2;
  float* const s[2] = {m, v};
  flat_step(p, g, s, pbf, n, zero_grad, [=](float& pp, float gg, float(&ss)[2]) {
    adamw_elem(pp, gg, ss[0], ss[1], gscale, decay, omb1, b2, omb2, eps, step_size, inv_bc2_sqrt);
  });
}

// lion_elem (optimizer_shared.h) over the flat buffer; the scaled gradient is rounded before the rule sees it
__global__ void __launch_bounds__(256) lion_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                   bf16_t* __restrict__ pbf, int64_t n, float lr, float b1, float omb1,
                                                   float b2, float omb2, float decay, float pre_scale,
                                                   const float* __restrict__ clip, int zero_grad) {
  const float gscale = grad_scale(pre_scale, clip);
  float* const s[1] = {m};
  flat_step(p, g, s, pbf, n, zero_grad,
            [=](float& pp, float gg, float(&ss)[1]) { lion_elem(pp, gg * gscale, ss[0], decay, lr, b1, omb1, b2, omb2); });
}

// AdamWFP16 (optimizers.py:96-120 as called from :78-92): both moments live in fp16, the update is computed in fp32 from
// the widened moments and uses the UNROUNDED new moments; no first-moment bias correction, no weight decay here.
//   m = float(m16)*b1 + (1-b1) g ; v = float(v16)*b2 + (1-b2) g^2 ; p -= lr*sqrt(1-b2^step) * m / (sqrt(v) + eps)
//   m16 = half(m) ; v16 = half(v)   -- v_cvt_f16_f32: round to nearest even, subnormals kept, overflow -> inf (what
//   torch.Tensor.half() does).  Nothing is clamped: a v that underflowed to 0 or sits at inf is the reference's behaviour.
// Fused: omb1*g + (.), b2*v + (.), p - step_size*(.).  Rounded first: b1*m, omb2*g, (omb2*g)*g, sqrt(v) + eps, the quotient.
// The new moments are rounded to fp32 and then to fp16, two roundings, as optimizers.py does.  Left to itself the compiler merges a
// lone multiply-add and its conversion into one v_fma_mixlo_f16, which rounds once: in the scalar path only, and visible where m
// sits half-way between two fp16 values.  adamw16_kernel is therefore compiled without the mixed-precision fma instructions.
typedef _Float16 f16_t;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
#if defined(__HIP_DEVICE_COMPILE__)  // (a device feature: the host pass of the same source does not know it)
#define UWU_NO_FMA_MIX __attribute__((target("no-fma-mix-insts")))
#else
#define UWU_NO_FMA_MIX
#endif

__device__ __forceinline__ void adamw16_elem(float& p, float g, f16_t& m16, f16_t& v16, float b1, float omb1, float b2,
                                             float omb2, float eps, float step_size) {
  const float m = __builtin_fmaf(omb1, g, b1 * (float)m16);
  const float v = __builtin_fmaf(b2, (float)v16, g * (omb2 * g));
  const float denom = sqrtf(v) + eps;
  p = __builtin_fmaf(-step_size, m / denom, p);
  m16 = (f16_t)m;
  v16 = (f16_t)v;
}

// 8 elements per lane: the fp16 state goes through 16-byte accesses like the fp32 buffers (two of them per 8 elements).
// m16 / v16 are only 8-byte aligned (chunk offsets are multiples of 4 elements): `head` (0 or up to 4) leading elements
// are peeled off as scalars so that the body's fp16 accesses start on a 16-byte boundary; p and g stay 16-byte aligned.
// The peeled head and the tail together are fewer than 12 elements.
UWU_NO_FMA_MIX
__global__ void __launch_bounds__(256) adamw16_kernel(float* __restrict__ p, float* __restrict__ g,
                                                      f16_t* __restrict__ m16, f16_t* __restrict__ v16,
                                                      bf16_t* __restrict__ pbf, int64_t n, int head, float b1, float omb1,
                                                      float b2, float omb2, float eps, float step_size,
                                                      float pre_scale, const float* __restrict__ clip, int zero_grad) {
  const float gscale = grad_scale(pre_scale, clip);
  const bool pbf16B = (((uintptr_t)(pbf + head)) & 15) == 0;  // wave-uniform
  for_each_group<8>(n, head, [&](int64_t e) {
    f32x8 pv = load8(p + e), gv = load8(g + e);
    f16x8 mv = *reinterpret_cast<const f16x8*>(m16 + e), vv = *reinterpret_cast<const f16x8*>(v16 + e);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float pp = pv[j];
      f16_t mm = mv[j], vn = vv[j];
      adamw16_elem(pp, gv[j] * gscale, mm, vn, b1, omb1, b2, omb2, eps, step_size);
      pv[j] = pp;
      mv[j] = mm;
      vv[j] = vn;
    }
    store8(p + e, pv);
    *reinterpret_cast<f16x8*>(m16 + e) = mv;
    *reinterpret_cast<f16x8*>(v16 + e) = vv;
    if (pbf) {
      if (pbf16B) {
        store8(pbf + e, pv);
      } else {
        store4(pbf + e, f32x4{pv[0], pv[1], pv[2], pv[3]});
        store4(pbf + e + 4, f32x4{pv[4], pv[5], pv[6], pv[7]});
      }
    }
    if (zero_grad) store8(g + e, f32x8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f});
  }, [&](int64_t i) {
    float pp = p[i];
    adamw16_elem(pp, g[i] * gscale, m16[i], v16[i], b1, omb1, b2, omb2, eps, step_size);
    p[i] = pp;
    if (pbf) pbf[i] = (bf16_t)pp;
    if (zero_grad) g[i] = 0.f;
  });
}

// p *= factor over one tensor's range (AdamWFP16's accumulated weight decay, optimizers.py:117-118), shadow refreshed
__global__ void __launch_bounds__(256) param_decay_kernel(float* __restrict__ p, bf16_t* __restrict__ pbf, int64_t n,
                                                          int head, float factor) {
  const bool pbf8B = (((uintptr_t)(pbf + head)) & 7) == 0;  // wave-uniform
  for_each_group<4>(n, head, [&](int64_t e) {
    f32x4 pv = load4(p + e);
    pv *= factor;
    store4(p + e, pv);
    if (pbf) {
      if (pbf8B) {
        store4(pbf + e, pv);
      } else {  // a tensor may start on any even byte of the shadow
#pragma unroll
        for (int j = 0; j < 4; ++j) pbf[e + j] = (bf16_t)pv[j];
      }
    }
  }, [&](int64_t i) {
    const float pp = p[i] * factor;
    p[i] = pp;
    if (pbf) pbf[i] = (bf16_t)pp;
  });
}

// Weight averaging (uwudiff_amd/averaging.py; torch.optim.swa_utils.AveragedModel as Lightning's WeightAveraging drives it):
//   avg = keep * avg + take * p      one multiply and one fused multiply-add per element, 8 B read + 4 B written per parameter
__device__ __forceinline__ float ema_elem(float avg, float p, float keep, float take) {
  return __builtin_fmaf(keep, avg, take * p);
}

__global__ void __launch_bounds__(256) ema_update_kernel(float* __restrict__ avg, const float* __restrict__ p, int64_t n,
                                                         float keep, float take) {
  for_each_group<4>(n, 0, [&](int64_t e) {
    f32x4 av = load4(avg + e), pv = load4(p + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) av[j] = ema_elem(av[j], pv[j], keep, take);
    store4(avg + e, av);
  }, [&](int64_t i) { avg[i] = ema_elem(avg[i], p[i], keep, take); });
}

// The average put in place of the weights without moving a pointer: p <- avg (and the bf16 shadow of the new p, rounded as
// cast_kernel rounds), avg <- the old p when `exchange`.  The fp32 words travel as integers: every bit pattern survives.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }

__global__ void __launch_bounds__(256) ema_swap_kernel(uint32_t* __restrict__ avg, uint32_t* __restrict__ p,
                                                       bf16_t* __restrict__ pbf, int64_t n, int exchange) {
  for_each_group<4>(n, 0, [&](int64_t e) {
    const u32x4 av = *reinterpret_cast<const u32x4*>(avg + e);
    if (exchange) {
      const u32x4 pv = *reinterpret_cast<const u32x4*>(p + e);
      *reinterpret_cast<u32x4*>(avg + e) = pv;
    }
    *reinterpret_cast<u32x4*>(p + e) = av;
    if (pbf) store4(pbf + e, f32x4{bits_f32(av[0]), bits_f32(av[1]), bits_f32(av[2]), bits_f32(av[3])});
  }, [&](int64_t i) {
    const uint32_t a = avg[i];
    if (exchange) avg[i] = p[i];
    p[i] = a;
    if (pbf) pbf[i] = from_f32<bf16_t>(bits_f32(a));
  });
}

// schedulefree.AdamWScheduleFree (Defazio et al., "The Road Less Scheduled"; the rule at uwu_sfadamw_step in include/uwu_hip.h):
//   v = b2*v + (1-b2) g^2 ; gn = g / (sqrt(v/bc2) + eps) + wd*y ; y = lerp(y, z, c) + a*gn ; z = z - lr_t*gn
// torch.lerp's two branches, chosen by the weight alone (uniform over the launch): at w = 1 the second gives `end` exactly.
__device__ __forceinline__ float lerp2(float start, float end, float w, float omw) {
  const float d = end - start;
  return w < 0.5f ? __builtin_fmaf(w, d, start) : __builtin_fmaf(-d, omw, end);
}

// fp32 roundings on each output's path, counted for the tests' bounds (each hyper-parameter's own rounding to fp32 counts as one;
// a fused multiply-add rounds once where the count takes the product and the sum apart):
//   v:  the g^2 term carries gscale (1) and g*gscale (1) twice, omb2 (1) and its two products (2) = 7, v*b2 carries b2 (1) and the
//       product (1); the sum adds 1 to both:                                              K_v = 8 on |v|
//   gn: denom = sqrt(v*inv_bc2) + eps: (8 + inv_bc2 1 + product 1) / 2 = 5, sqrt 1, the sum 1 = 7 (eps's own rounding is on the
//       smaller term); g/denom = 2 + 7 + the division 1 = 10; wd*y = 2 on a term lr_t*wd times |y|; the sum 1:  11 on |gn|
//   z:  lr_t (1) + gn (11) + the fma (1) = 13 on lr_t*|gn|, 1 on |z|:                     K_z = 16 on |z| + lr_t*|gn|
//   y:  lerp = z - y (1), c (1), product (1), sum (1) on at most |y| + |z|; a (1) + gn (11) + the fma (1) = 13 on |a|*|gn|,
//       |a| <= lr_t:                                                                      K_y = 16 on |y| + |z| + lr_t*|gn|
//   (16 = 13 and the division and square root taken as 2 units each instead of 1, should the build not round them correctly)
// Fused: b2*v + (.), wd*y + (.), a*gn + lerp, z - lr_t*gn and the lerp's own.  Rounded first: omb2*g, (omb2*g)*g, v*inv_bc2,
// sqrt(.) + eps, the quotient.
__device__ __forceinline__ void sfadamw_elem(float& y, float g, float& z, float& v, float b2, float omb2, float inv_bc2,
                                             float eps, float wd, float c, float omc, float a, float neg_lr) {
  const float vn = __builtin_fmaf(v, b2, (omb2 * g) * g);
  const float gn = __builtin_fmaf(wd, y, g / (sqrtf(vn * inv_bc2) + eps));
  y = __builtin_fmaf(a, gn, lerp2(y, z, c, omc));
  z = __builtin_fmaf(neg_lr, gn, z);
  v = vn;
}

__global__ void __launch_bounds__(256) sfadamw_kernel(float* __restrict__ y, float* __restrict__ g, float* __restrict__ z,
                                                      float* __restrict__ v, bf16_t* __restrict__ pbf, int64_t n, float b2,
                                                      float omb2, float inv_bc2, float eps, float wd, float c, float omc,
                                                      float a, float neg_lr, float pre_scale,
                                                      const float* __restrict__ clip, int zero_grad) {
  const float gscale = grad_scale(pre_scale, clip);
  float* const s[2] = {z, v};
  flat_step(y, g, s, pbf, n, zero_grad, [=](float& yy, float gg, float(&ss)[2]) {
    sfadamw_elem(yy, gg * gscale, ss[0], ss[1], b2, omb2, inv_bc2, eps, wd, c, omc, a, neg_lr);
  });
}

// out = lerp(y, z, w), out of place: the averaged weights x of the schedule-free rule at w = 1 - 1/beta1.  8 B read + 4 B written.
__global__ void __launch_bounds__(256) sf_average_kernel(const float* __restrict__ y, const float* __restrict__ z,
                                                         float* __restrict__ out, int64_t n, float w, float omw) {
  for_each_group<4>(n, 0, [&](int64_t e) {
    f32x4 yv = load4(y + e), zv = load4(z + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) yv[j] = lerp2(yv[j], zv[j], w, omw);
    store4(out + e, yv);
  }, [&](int64_t i) { out[i] = lerp2(y[i], z[i], w, omw); });
}

template <typename TS, typename TD>
__global__ void __launch_bounds__(256) cast_kernel(const TS* __restrict__ s, TD* __restrict__ d, int64_t n) {
  for_each_group<4>(n, 0, [&](int64_t e) { store4(d + e, load4(s + e)); }, [&](int64_t i) { d[i] = from_f32<TD>(to_f32(s[i])); });
}

extern "C" int uwu_grad_sqnorm_clip(const float* g, int64_t n, float pre_scale, float max_norm, float* partial,
                                    float* out, void* stream) {
  UWU_CHECK_ARG(g && partial && out && n > 0, "grad_sqnorm_clip: bad args");
  UWU_CHECK_ARG(((uintptr_t)g & 15) == 0, "grad_sqnorm_clip: g must be 16-byte aligned");
  int grid = ew_grid(n / 4, 256);
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, g, n, partial);
  UWU_LAUNCH_CHECK("sqnorm_partial");
  hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, grid, pre_scale,
                     max_norm, out);
  UWU_LAUNCH_CHECK("sqnorm_final");
  return UWU_OK;
}

extern "C" int uwu_adamw_step(float* p, float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int step, float pre_scale,
                              const float* clip, int zero_grad, void* stream) {
  UWU_CHECK_ARG(p && g && m && v && n > 0 && step >= 1, "adamw_step: bad args");
  UWU_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0,
                "adamw_step: buffers must be 16-byte aligned");
  UWU_CHECK_ARG(p_bf16 == nullptr || ((uintptr_t)p_bf16 & 7) == 0, "adamw_step: bf16 shadow must be 8-byte aligned");
  // bias corrections in double on the host, as torch does with python floats
  double bc1 = 1.0 - pow((double)beta1, (double)step);
  double bc2 = 1.0 - pow((double)beta2, (double)step);
  float step_size = (float)((double)lr / bc1);
  float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
  hipLaunchKernelGGL(adamw_kernel, dim3(ew_grid(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                     (bf16_t*)p_bf16, n, lr, beta1, beta2, eps, weight_decay, step_size, inv_bc2_sqrt, pre_scale,
                     clip, zero_grad);
  UWU_LAUNCH_CHECK("adamw_step");
  return UWU_OK;
}

extern "C" int uwu_lion_step(float* p, float* g, float* m, void* p_bf16, int64_t n, double lr, double beta1, double beta2,
                             double weight_decay, float pre_scale, const float* clip, int zero_grad, void* stream) {
  UWU_CHECK_ARG(p && g && m && n > 0, "lion_step: bad args");
  UWU_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0, "lion_step: buffers must be 16-byte aligned");
  UWU_CHECK_ARG(p_bf16 == nullptr || ((uintptr_t)p_bf16 & 7) == 0, "lion_step: bf16 shadow must be 8-byte aligned");
  // 1 - beta and 1 - lr*wd in double on the host, as lion_pytorch does with python floats
  hipLaunchKernelGGL(lion_kernel, dim3(ew_grid(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, (bf16_t*)p_bf16,
                     n, (float)lr, (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                     (float)(1.0 - lr * weight_decay), pre_scale, clip, zero_grad);
  UWU_LAUNCH_CHECK("lion_step");
  return UWU_OK;
}

extern "C" int uwu_adamw_fp16_step(float* p, float* g, void* m16, void* v16, void* p_bf16, int64_t n, double lr,
                                   double beta1, double beta2, double eps, int step, float pre_scale, const float* clip,
                                   int zero_grad, void* stream) {
  UWU_CHECK_ARG(p && g && m16 && v16 && n > 0 && step >= 1, "adamw_fp16_step: bad args");
  UWU_CHECK_ARG((((uintptr_t)p | (uintptr_t)g) & 15) == 0, "adamw_fp16_step: p and g must be 16-byte aligned");
  UWU_CHECK_ARG((((uintptr_t)m16 | (uintptr_t)v16) & 7) == 0, "adamw_fp16_step: fp16 moments must be 8-byte aligned");
  UWU_CHECK_ARG((((uintptr_t)m16 ^ (uintptr_t)v16) & 15) == 0,
                "adamw_fp16_step: both fp16 moments must sit at the same offset within 16 bytes");
  UWU_CHECK_ARG(p_bf16 == nullptr || ((uintptr_t)p_bf16 & 7) == 0, "adamw_fp16_step: bf16 shadow must be 8-byte aligned");
  // the peel moves the fp16 state by 8 bytes and p / g by 16: everything the body touches 16 bytes at a time stays aligned
  int head = ((uintptr_t)m16 & 15) ? 4 : 0;
  if (head > n) head = (int)n;
  // optimizers.py:111-115: value = -lr * (1 - beta2**step) ** 0.5 as a python float
  const double step_size = lr * sqrt(1.0 - pow(beta2, (double)step));
  hipLaunchKernelGGL(adamw16_kernel, dim3(ew_grid(n / 8, 256)), dim3(256), 0, (hipStream_t)stream, p, g, (f16_t*)m16,
                     (f16_t*)v16, (bf16_t*)p_bf16, n, head, (float)beta1, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), (float)eps, (float)step_size, pre_scale, clip, zero_grad);
  UWU_LAUNCH_CHECK("adamw_fp16_step");
  return UWU_OK;
}

extern "C" int uwu_param_decay(float* p, void* p_bf16, int64_t n, double factor, void* stream) {
  UWU_CHECK_ARG(p && n > 0, "param_decay: bad args");
  UWU_CHECK_ARG(((uintptr_t)p & 3) == 0 && ((uintptr_t)p_bf16 & 1) == 0, "param_decay: misaligned buffers");
  // a tensor of the flat buffer may start anywhere: peel up to 3 elements to reach a 16-byte boundary of p
  int head = (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
  if (head > n) head = (int)n;
  hipLaunchKernelGGL(param_decay_kernel, dim3(ew_grid(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, p,
                     (bf16_t*)p_bf16, n, head, (float)factor);
  UWU_LAUNCH_CHECK("param_decay");
  return UWU_OK;
}

extern "C" int uwu_ema_update(float* avg, const float* p, int64_t n, float keep, float take, void* stream) {
  UWU_CHECK_ARG(avg && p && n > 0, "ema_update: bad args");
  UWU_CHECK_ARG((((uintptr_t)avg | (uintptr_t)p) & 15) == 0, "ema_update: buffers must be 16-byte aligned");
  hipLaunchKernelGGL(ema_update_kernel, dim3(ew_grid(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, avg, p, n, keep, take);
  UWU_LAUNCH_CHECK("ema_update");
  return UWU_OK;
}

extern "C" int uwu_ema_swap(float* avg, float* p, void* p_bf16, int64_t n, int mode, void* stream) {
  UWU_CHECK_ARG(avg && p && n > 0 && (mode == 0 || mode == 1), "ema_swap: bad args");
  UWU_CHECK_ARG((((uintptr_t)avg | (uintptr_t)p) & 15) == 0, "ema_swap: buffers must be 16-byte aligned");
  UWU_CHECK_ARG(p_bf16 == nullptr || ((uintptr_t)p_bf16 & 7) == 0, "ema_swap: bf16 shadow must be 8-byte aligned");
  const uintptr_t lo = (uintptr_t)avg < (uintptr_t)p ? (uintptr_t)avg : (uintptr_t)p;
  const uintptr_t hi = (uintptr_t)avg < (uintptr_t)p ? (uintptr_t)p : (uintptr_t)avg;
  UWU_CHECK_ARG((hi - lo) / 4 >= (uint64_t)n, "ema_swap: avg and p must not overlap");
  hipLaunchKernelGGL(ema_swap_kernel, dim3(ew_grid(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, (uint32_t*)avg,
                     (uint32_t*)p, (bf16_t*)p_bf16, n, mode == 0);
  UWU_LAUNCH_CHECK("ema_swap");
  return UWU_OK;
}

extern "C" int uwu_sfadamw_step(float* y, float* g, float* z, float* v, void* p_bf16, int64_t n, double lr_t, double beta1,
                                double beta2, double eps, double weight_decay, double c, double bc2, float pre_scale,
                                const float* clip, int zero_grad, void* stream) {
  UWU_CHECK_ARG(y && g && z && v, "sfadamw_step: null pointer");
  UWU_CHECK_ARG(n > 0, "sfadamw_step: n must be positive");
  UWU_CHECK_ARG((((uintptr_t)y | (uintptr_t)g | (uintptr_t)z | (uintptr_t)v) & 15) == 0,
                "sfadamw_step: buffers must be 16-byte aligned");
  UWU_CHECK_ARG(p_bf16 == nullptr || ((uintptr_t)p_bf16 & 7) == 0, "sfadamw_step: bf16 shadow must be 8-byte aligned");
  UWU_CHECK_ARG(c >= 0.0 && c <= 1.0 && bc2 > 0.0 && bc2 <= 1.0, "sfadamw_step: c must be in [0, 1] and bc2 in (0, 1]");
  // the folded factors in double on the host, as the package forms them with python floats; each is rounded to fp32 once
  const double a = lr_t * (beta1 * (1.0 - c) - 1.0);
  hipLaunchKernelGGL(sfadamw_kernel, dim3(ew_grid(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, y, g, z, v,
                     (bf16_t*)p_bf16, n, (float)beta2, (float)(1.0 - beta2), (float)(1.0 / bc2), (float)eps,
                     (float)weight_decay, (float)c, (float)(1.0 - c), (float)a, (float)(-lr_t), pre_scale, clip, zero_grad);
  UWU_LAUNCH_CHECK("sfadamw_step");
  return UWU_OK;
}

extern "C" int uwu_sf_average(const float* y, const float* z, float* out, int64_t n, double weight, void* stream) {
  UWU_CHECK_ARG(y && z && out, "sf_average: null pointer");
  UWU_CHECK_ARG(n > 0, "sf_average: n must be positive");
  UWU_CHECK_ARG((((uintptr_t)y | (uintptr_t)z | (uintptr_t)out) & 15) == 0, "sf_average: buffers must be 16-byte aligned");
  hipLaunchKernelGGL(sf_average_kernel, dim3(ew_grid(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, y, z, out, n,
                     (float)weight, (float)(1.0 - weight));
  UWU_LAUNCH_CHECK("sf_average");
  return UWU_OK;
}

extern "C" int uwu_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream) {
  UWU_CHECK_ARG(src && dst && n > 0, "cast_f32_to_bf16: bad args");
  hipLaunchKernelGGL((cast_kernel<float, bf16_t>), dim3(ew_grid(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, src,
                     (bf16_t*)dst, n);
  UWU_LAUNCH_CHECK("cast_f32_to_bf16");
  return UWU_OK;
}

extern "C" int uwu_cast_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream) {
  UWU_CHECK_ARG(src && dst && n > 0, "cast_bf16_to_f32: bad args");
  hipLaunchKernelGGL((cast_kernel<bf16_t, float>), dim3(ew_grid(n / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)src, dst, n);
  UWU_LAUNCH_CHECK("cast_bf16_to_f32");
  return UWU_OK;
}
