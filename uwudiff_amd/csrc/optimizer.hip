// Flat-buffer optimizer kernels: global grad norm (+clip coefficient), fused AdamW / Lion / AdamWFP16 with bf16 shadow
// refresh, the weight average (update, exchange with the weights), dtype casts.  HBM-bound: AdamW moves 28 B/param, Lion and
// AdamWFP16 20 B/param (+2 B/param for the bf16 shadow, +4 B/param for the zeroed gradient), the average's update 12 B/param.
// Prodigy (further down) is three kernels round two global sums: 40 + 18 B/param with the shadow and the zeroed gradient.
// The 8-bit block-wise AdamW / Lion (last section) keep 1 B per moment and parameter and one fp32 scale per 256: 16 / 14 B/param.
// Schedule-free AdamW (next to the weight average, whose exchange kernel it uses) moves AdamW's 28 B/param; its average 12 B/param.
// Reference: src/duwu/trainer/trainer.py:52-74 (torch.optim.AdamW + Lightning gradient_clip_val),
// src/duwu/trainer/optimizers.py (AdamWFP16), lion_pytorch.Lion (configs/demo_training*.yaml, commented alternative).
#include "common.h"

// stage 1: per-block partial sums (deterministic order), stage 2: one block folds the partials
__global__ void __launch_bounds__(256) sqnorm_partial_kernel(const float* __restrict__ g, int64_t n,
                                                             float* __restrict__ partial) {
  __shared__ float red[4];
  const int64_t n4 = n >> 2;
  float a = 0.f;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 v = load4(g + 4 * i);
    a += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (blockIdx.x == 0) {  // tail
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) a += g[i] * g[i];
  }
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

// torch.optim.AdamW (single tensor, no amsgrad):
//   p *= 1 - lr*wd ; m = lerp(m, g, 1-b1) ; v = b2*v + (1-b2) g^2 ;
//   p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// zero_grad: the consumed gradient is overwritten with zeros in the same pass (the next backward accumulates into the flat
// buffer: 4 more bytes written per parameter instead of a separate fill kernel that writes 4 and a launch)
__global__ void __launch_bounds__(256) adamw_kernel(float* __restrict__ p, float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    bf16_t* __restrict__ pbf, int64_t n, float lr, float b1,
                                                    float b2, float eps, float wd, float step_size,
                                                    float inv_bc2_sqrt, float pre_scale,
                                                    const float* __restrict__ clip, int zero_grad) {
  const float gscale = pre_scale * (clip ? clip[1] : 1.f);
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const float decay = 1.f - lr * wd;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 pv = load4(p + 4 * i), gv = load4(g + 4 * i), mv = load4(m + 4 * i), vv = load4(v + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gg = gv[j] * gscale;
      float pp = pv[j] * decay;
      float mm = mv[j] + (gg - mv[j]) * (1.f - b1);
      float vn = vv[j] * b2 + (1.f - b2) * gg * gg;
      float denom = sqrtf(vn) * inv_bc2_sqrt + eps;
      pp = pp - step_size * (mm / denom);
      pv[j] = pp;
      mv[j] = mm;
      vv[j] = vn;
    }
    store4(p + 4 * i, pv);
    store4(m + 4 * i, mv);
    store4(v + 4 * i, vv);
    if (pbf) store4(pbf + 4 * i, pv);
    if (zero_grad) store4(g + 4 * i, f32x4{0.f, 0.f, 0.f, 0.f});
  }
  if (blockIdx.x == 0) {
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
      float gg = g[i] * gscale;
      float pp = p[i] * decay;
      float mm = m[i] + (gg - m[i]) * (1.f - b1);
      float vn = v[i] * b2 + (1.f - b2) * gg * gg;
      pp = pp - step_size * (mm / (sqrtf(vn) * inv_bc2_sqrt + eps));
      p[i] = pp;
      m[i] = mm;
      v[i] = vn;
      if (pbf) pbf[i] = (bf16_t)pp;
      if (zero_grad) g[i] = 0.f;
    }
  }
}

// lion_pytorch.Lion (Chen et al. 2023, Algorithm 2), in the package's order:
//   p *= 1 - lr*wd ; c = b1*m + (1-b1) g ; p -= lr*sign(c) (sign(0) = 0) ; m = b2*m + (1-b2) g
__device__ __forceinline__ void lion_elem(float& p, float g, float& m, float decay, float lr, float b1, float omb1,
                                          float b2, float omb2) {
  const float c = m * b1 + g * omb1;
  const float s = c > 0.f ? 1.f : (c < 0.f ? -1.f : 0.f);
  p = p * decay - lr * s;
  m = m * b2 + g * omb2;
}

__global__ void __launch_bounds__(256) lion_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                   bf16_t* __restrict__ pbf, int64_t n, float lr, float b1, float omb1,
                                                   float b2, float omb2, float decay, float pre_scale,
                                                   const float* __restrict__ clip, int zero_grad) {
  const float gscale = pre_scale * (clip ? clip[1] : 1.f);
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 pv = load4(p + 4 * i), gv = load4(g + 4 * i), mv = load4(m + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pp = pv[j], mm = mv[j];
      lion_elem(pp, gv[j] * gscale, mm, decay, lr, b1, omb1, b2, omb2);
      pv[j] = pp;
      mv[j] = mm;
    }
    store4(p + 4 * i, pv);
    store4(m + 4 * i, mv);
    if (pbf) store4(pbf + 4 * i, pv);
    if (zero_grad) store4(g + 4 * i, f32x4{0.f, 0.f, 0.f, 0.f});
  }
  if (blockIdx.x == 0) {
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
      float pp = p[i], mm = m[i];
      lion_elem(pp, g[i] * gscale, mm, decay, lr, b1, omb1, b2, omb2);
      p[i] = pp;
      m[i] = mm;
      if (pbf) pbf[i] = (bf16_t)pp;
      if (zero_grad) g[i] = 0.f;
    }
  }
}

// AdamWFP16 (optimizers.py:96-120 as called from :78-92): both moments live in fp16, the update is computed in fp32 from
// the widened moments and uses the UNROUNDED new moments; no first-moment bias correction, no weight decay here.
//   m = float(m16)*b1 + (1-b1) g ; v = float(v16)*b2 + (1-b2) g^2 ; p -= lr*sqrt(1-b2^step) * m / (sqrt(v) + eps)
//   m16 = half(m) ; v16 = half(v)   -- v_cvt_f16_f32: round to nearest even, subnormals kept, overflow -> inf (what
//   torch.Tensor.half() does).  Nothing is clamped: a v that underflowed to 0 or sits at inf is the reference's behaviour.
typedef _Float16 f16_t;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void adamw16_elem(float& p, float g, f16_t& m16, f16_t& v16, float b1, float omb1, float b2,
                                             float omb2, float eps, float step_size) {
  const float m = (float)m16 * b1 + g * omb1;
  const float v = (float)v16 * b2 + omb2 * g * g;
  p = p - step_size * (m / (sqrtf(v) + eps));
  m16 = (f16_t)m;
  v16 = (f16_t)v;
}

// 8 elements per lane: the fp16 state goes through 16-byte accesses like the fp32 buffers (two of them per 8 elements).
// m16 / v16 are only 8-byte aligned (chunk offsets are multiples of 4 elements): `head` (0 or up to 4) leading elements
// are peeled off as scalars so that the body's fp16 accesses start on a 16-byte boundary; p and g stay 16-byte aligned.
__global__ void __launch_bounds__(256) adamw16_kernel(float* __restrict__ p, float* __restrict__ g,
                                                      f16_t* __restrict__ m16, f16_t* __restrict__ v16,
                                                      bf16_t* __restrict__ pbf, int64_t n, int head, float b1, float omb1,
                                                      float b2, float omb2, float eps, float step_size,
                                                      float pre_scale, const float* __restrict__ clip, int zero_grad) {
  const float gscale = pre_scale * (clip ? clip[1] : 1.f);
  const int64_t n8 = (n - head) >> 3;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool pbf16B = (((uintptr_t)(pbf + head)) & 15) == 0;  // wave-uniform
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    const int64_t e = head + 8 * i;
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
  }
  if (blockIdx.x == 0) {  // the peeled head [0, head) and the tail [head + 8*n8, n): fewer than 12 elements
    const int64_t tail0 = head + (n8 << 3);
    const int64_t extra = head + (n - tail0);
    for (int64_t k = threadIdx.x; k < extra; k += 256) {
      const int64_t i = k < head ? k : tail0 + (k - head);
      float pp = p[i];
      f16_t mm = m16[i], vn = v16[i];
      adamw16_elem(pp, g[i] * gscale, mm, vn, b1, omb1, b2, omb2, eps, step_size);
      p[i] = pp;
      m16[i] = mm;
      v16[i] = vn;
      if (pbf) pbf[i] = (bf16_t)pp;
      if (zero_grad) g[i] = 0.f;
    }
  }
}

// p *= factor over one tensor's range (AdamWFP16's accumulated weight decay, optimizers.py:117-118), shadow refreshed
__global__ void __launch_bounds__(256) param_decay_kernel(float* __restrict__ p, bf16_t* __restrict__ pbf, int64_t n,
                                                          int head, float factor) {
  const int64_t n4 = (n - head) >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool pbf8B = (((uintptr_t)(pbf + head)) & 7) == 0;  // wave-uniform
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const int64_t e = head + 4 * i;
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
  }
  if (blockIdx.x == 0) {
    const int64_t tail0 = head + (n4 << 2);
    const int64_t extra = head + (n - tail0);
    for (int64_t k = threadIdx.x; k < extra; k += 256) {
      const int64_t i = k < head ? k : tail0 + (k - head);
      const float pp = p[i] * factor;
      p[i] = pp;
      if (pbf) pbf[i] = (bf16_t)pp;
    }
  }
}

// Weight averaging (uwudiff_amd/averaging.py; torch.optim.swa_utils.AveragedModel as Lightning's WeightAveraging drives it):
//   avg = keep * avg + take * p      one multiply and one fused multiply-add per element, 8 B read + 4 B written per parameter
__global__ void __launch_bounds__(256) ema_update_kernel(float* __restrict__ avg, const float* __restrict__ p, int64_t n,
                                                         float keep, float take) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 av = load4(avg + 4 * i), pv = load4(p + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) av[j] = __builtin_fmaf(keep, av[j], take * pv[j]);
    store4(avg + 4 * i, av);
  }
  if (blockIdx.x == 0) {
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) avg[i] = __builtin_fmaf(keep, avg[i], take * p[i]);
  }
}

// The average put in place of the weights without moving a pointer: p <- avg (and the bf16 shadow of the new p, rounded as
// cast_kernel rounds), avg <- the old p when `exchange`.  The fp32 words travel as integers: every bit pattern survives.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }

__global__ void __launch_bounds__(256) ema_swap_kernel(uint32_t* __restrict__ avg, uint32_t* __restrict__ p,
                                                       bf16_t* __restrict__ pbf, int64_t n, int exchange) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const u32x4 av = *reinterpret_cast<const u32x4*>(avg + 4 * i);
    if (exchange) {
      const u32x4 pv = *reinterpret_cast<const u32x4*>(p + 4 * i);
      *reinterpret_cast<u32x4*>(avg + 4 * i) = pv;
    }
    *reinterpret_cast<u32x4*>(p + 4 * i) = av;
    if (pbf) store4(pbf + 4 * i, f32x4{bits_f32(av[0]), bits_f32(av[1]), bits_f32(av[2]), bits_f32(av[3])});
  }
  if (blockIdx.x == 0) {
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
      const uint32_t a = avg[i];
      if (exchange) avg[i] = p[i];
      p[i] = a;
      if (pbf) pbf[i] = from_f32<bf16_t>(bits_f32(a));
    }
  }
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
__device__ __forceinline__ void sfadamw_elem(float& y, float g, float& z, float& v, float b2, float omb2, float inv_bc2,
                                             float eps, float wd, float c, float omc, float a, float neg_lr) {
  // every multiply-add is written out: the vector body and the scalar tail round alike, whatever the compiler would contract
  const float vn = __builtin_fmaf(v, b2, (omb2 * g) * g);
  const float gn = __builtin_fmaf(wd, y, g / (sqrtf(vn * inv_bc2) + eps));
  y =__builtin_fmaf(a, gn, lerp2(y, z, c, omc));
  z = __builtin_fmaf(neg_lr, gn, z);
  v = vn;
}

__global__ void __launch_bounds__(256) sfadamw_kernel(float* __restrict__ y, float* __restrict__ g, float* __restrict__ z,
                                                      float* __restrict__ v, bf16_t* __restrict__ pbf, int64_t n, float b2,
                                                      float omb2, float inv_bc2, float eps, float wd, float c, float omc,
                                                      float a, float neg_lr, float pre_scale,
                                                      const float* __restrict__ clip, int zero_grad) {
  const float gscale = pre_scale * (clip ? clip[1] : 1.f);
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 yv = load4(y + 4 * i), gv = load4(g + 4 * i), zv = load4(z + 4 * i), vv = load4(v + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float yy = yv[j], zz = zv[j], vn = vv[j];
      sfadamw_elem(yy, gv[j] * gscale, zz, vn, b2, omb2, inv_bc2, eps, wd, c, omc, a, neg_lr);
      yv[j] = yy;
      zv[j] = zz;
      vv[j] = vn;
    }
    store4(y + 4 * i, yv);
    store4(z + 4 * i, zv);
    store4(v + 4 * i, vv);
    if (pbf) store4(pbf + 4 * i, yv);
    if (zero_grad) store4(g + 4 * i, f32x4{0.f, 0.f, 0.f, 0.f});
  }
  if (blockIdx.x == 0) {
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
      float yy = y[i], zz = z[i], vn = v[i];
      sfadamw_elem(yy, g[i] * gscale, zz, vn, b2, omb2, inv_bc2, eps, wd, c, omc, a, neg_lr);
      y[i] = yy;
      z[i] = zz;
      v[i] = vn;
      if (pbf) pbf[i] = (bf16_t)yy;
      if (zero_grad) g[i] = 0.f;
    }
  }
}

// out = lerp(y, z, w), out of place: the averaged weights x of the schedule-free rule at w = 1 - 1/beta1.  8 B read + 4 B written.
__global__ void __launch_bounds__(256) sf_average_kernel(const float* __restrict__ y, const float* __restrict__ z,
                                                         float* __restrict__ out, int64_t n, float w, float omw) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 yv = load4(y + 4 * i), zv = load4(z + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) yv[j] = lerp2(yv[j], zv[j], w, omw);
    store4(out + 4 * i, yv);
  }
  if (blockIdx.x == 0) {
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) out[i] = lerp2(y[i], z[i], w, omw);
  }
}

template <typename TS, typename TD>
__global__ void __launch_bounds__(256) cast_kernel(const TS* __restrict__ s, TD* __restrict__ d, int64_t n) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) store4(d + 4 * i, load4(s + 4 * i));
  if (blockIdx.x == 0)
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) d[i] = from_f32<TD>(to_f32(s[i]));
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

// ---------------------------------------------------------------------------------------------------------------- Prodigy
// prodigyopt.Prodigy (Mishchenko & Defazio, "Prodigy: An Expeditiously Adaptive Parameter-Free Learner") on a flat buffer.
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

// d * lr * bc from the block's d and k: the statistics pass and the finalize pass both call this, so they use the same dlr
__device__ __forceinline__ double prodigy_dlr(double d, double k, double lr, double beta1, double beta2, int use_bc) {
  double bc = 1.0;
  if (use_bc) bc = sqrt(1.0 - pow(beta2, k + 1.0)) / (1.0 - pow(beta1, k + 1.0));
  return d * lr * bc;
}

// fixed-order sum of one double per thread over a 256-thread workgroup (LDS tree: the same order on every run)
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

struct ProdigyCoef {
  double gscale, wd_coupled, b1, c1, b2, c2, b3, cs;
};

// one element in double: the products, p0 - p and the sums carry no fp32 rounding; each stored moment is rounded once
__device__ __forceinline__ void prodigy_elem(float p, float g, float p0, float& m, float& v, float& s, const ProdigyCoef& c,
                                             double& num, double& den) {
  const double pd = (double)p;
  const double gd = (double)g * c.gscale + c.wd_coupled * pd;
  num += gd * ((double)p0 - pd);
  m = (float)(c.b1 * (double)m + c.c1 * gd);
  v = (float)(c.b2 * (double)v + c.c2 * gd * gd);
  s = (float)(c.b3 * (double)s + c.cs * gd);
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
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  double num = 0.0, den = 0.0;
  if (lr > 0.0) {
    const double d = scal[UWU_PRODIGY_D];
    const double dlr = prodigy_dlr(d, scal[UWU_PRODIGY_K], lr, beta1, beta2, use_bc);
    ProdigyCoef c;
    c.gscale = (double)(pre_scale * (clip ? clip[1] : 1.f));  // the fp32 factor uwu_adamw_step multiplies by
    c.wd_coupled = wd_coupled;
    c.b1 = beta1;
    c.c1 = d * omb1;
    c.b2 = beta2;
    c.c2 = d * d * omb2;
    c.b3 = beta3;
    c.cs = (d / d0) * (safeguard ? d : dlr);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
      const f32x4 pv = load4(p + 4 * i), gv = load4(g + 4 * i), qv = load4(p0 + 4 * i);
      f32x4 mv = load4(m + 4 * i), vv = load4(v + 4 * i), sv = load4(s + 4 * i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float mm = mv[j], vn = vv[j], ss = sv[j];
        prodigy_elem(pv[j], gv[j], qv[j], mm, vn, ss, c, num, den);
        mv[j] = mm;
        vv[j] = vn;
        sv[j] = ss;
      }
      store4(m + 4 * i, mv);
      store4(v + 4 * i, vv);
      store4(s + 4 * i, sv);
      if (zero_grad) store4(g + 4 * i, f32x4{0.f, 0.f, 0.f, 0.f});
    }
    if (blockIdx.x == 0) {  // tail
      for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
        prodigy_elem(p[i], g[i], p0[i], m[i], v[i], s[i], c, num, den);
        if (zero_grad) g[i] = 0.f;
      }
    }
  } else if (zero_grad) {  // lr == 0: no statistics; the gradient is consumed all the same
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride)
      store4(g + 4 * i, f32x4{0.f, 0.f, 0.f, 0.f});
    if (blockIdx.x == 0)
      for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) g[i] = 0.f;
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
  const double d_numerator = beta3 * scal[UWU_PRODIGY_D_NUMERATOR] + (d / d0) * dlr * num;
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
// and the new d, fp32 as adamw_kernel; nothing at all when the step returned early.
__global__ void __launch_bounds__(256) prodigy_apply_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                            const float* __restrict__ v, bf16_t* __restrict__ pbf, int64_t n,
                                                            const double* __restrict__ scal, double eps, double wd_decoupled) {
  if (scal[UWU_PRODIGY_SKIPPED] != 0.0) return;
  const double dlr_d = scal[UWU_PRODIGY_DLR];
  const float dlr = (float)dlr_d, deps = (float)(scal[UWU_PRODIGY_D] * eps), decay = (float)(1.0 - wd_decoupled * dlr_d);
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 pv = load4(p + 4 * i);
    const f32x4 mv = load4(m + 4 * i), vv = load4(v + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) pv[j] = pv[j] * decay - dlr * (mv[j] / (sqrtf(vv[j]) + deps));
    store4(p + 4 * i, pv);
    if (pbf) store4(pbf + 4 * i, pv);
  }
  if (blockIdx.x == 0) {
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
      const float pp = p[i] * decay - dlr * (m[i] / (sqrtf(v[i]) + deps));
      p[i] = pp;
      if (pbf) pbf[i] = (bf16_t)pp;
    }
  }
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

// ------------------------------------------------------------------------------------------------ 8-bit blockwise state
// AdamW and Lion whose moments live as 8-bit codes with one fp32 scale (absmax) per block of 256 elements: the state layout of
// bitsandbytes' AdamW8bit / Lion8bit (block-wise dynamic quantisation, Dettmers et al. 2022).  The rule is written out at
// uwu_adamw8_step (include/uwu_hip.h): dequantise, the arithmetic of adamw_kernel / lion_elem on the fp32 values, the block's new
// absmax, the nearest table entry of value / absmax.  Two things the package does are NOT reproduced: it applies the weight decay
// after the update (here first, as adamw_kernel does: O(lr^2 wd) per step apart), and after quantising the first moment it moves a
// code whose sign differs from the value's to the neighbouring entry (its sign-preservation fix-up); here the code is the
// nearest entry and nothing else.
//
// One 256-element block is one wave at 4 elements per lane: p and g move as 16-byte accesses, the codes as one dword per lane,
// the block maximum is a DPP wave reduction, so the loop has no barrier.  Blocks are counted from the buffer's start; a launch
// covers whole blocks (the last may be partial: those lanes take the element-wise path).  Both tables are staged in LDS once per
// workgroup; the search is a binary search over the staged table (8 dependent reads, a 9th for the upper neighbour) and assumes
// nothing about the table but that it increases (see Q8Table for the order it is staged in).  Per parameter: 10 B read + 6 B written for AdamW (+ 2 B shadow, + 4 B zeroed g).
// A staged table: T in index order (dequantisation, the upper neighbour) and E, the same entries in the level order of the binary
// search over T[1..255] (E[1] = T[128], E[2] = T[64], E[3] = T[192], ...; E[0] = T[0]).  Searched in index order, level k reads
// only entries whose index is an odd multiple of 2^(8-k): 8 distinct entries in ONE of the 32 LDS banks at level 4, 16 in two banks
// at level 5 -- most of a wave's lanes queue behind each other.  In level order a level's entries are consecutive dwords.
struct Q8Table {
  float T[256], E[256];
};

__device__ __forceinline__ void q8_stage(Q8Table& Q, const float* __restrict__ q) {  // 256 threads; the caller synchronises
  const int i = threadIdx.x;
  Q.T[i] = q[i];
  const int k = 32 - __builtin_clz(i | 1);  // the level of E[i], 1..8
  const int r = i - (1 << (k - 1));         // its place within the level
  Q.E[i] = q[i ? (2 * r + 1) << (8 - k) : 0];
}

__device__ __forceinline__ uint32_t q8_nearest(const Q8Table& Q, float x) {
  int i = 1;  // after 8 levels i - 256 = the number of entries T[1..255] that are <= x = the index of the last entry <= x
  float tlo = Q.E[0];
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const float t = Q.E[i];
    const bool c = t <= x;
    tlo = c ? t : tlo;
    i = 2 * i + (c ? 1 : 0);
  }
  const int lo = i - 256, hi = lo < 255 ? lo + 1 : 255;
  return (Q.T[hi] - x) < (x - tlo) ? hi : lo;  // a tie stays at the lower index
}

// the 4 elements of one lane: vector accesses when all 4 lie inside the buffer, element by element in the ragged last block
struct Q8Lane {
  int64_t e;
  int valid;
};

__device__ __forceinline__ void q8_load(const Q8Lane& L, const float* p, const float* g, f32x4& pv, f32x4& gv) {
  if (L.valid == 4) {
    pv = load4(p + L.e);
    gv = load4(g + L.e);
  } else {
    pv = f32x4{0.f, 0.f, 0.f, 0.f};
    gv = pv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < L.valid) {
        pv[j] = p[L.e + j];
        gv[j] = g[L.e + j];
      }
    }
  }
}

__device__ __forceinline__ uint32_t q8_load_codes(const Q8Lane& L, const uint8_t* c8) {
  if (L.valid == 4) return *reinterpret_cast<const uint32_t*>(c8 + L.e);
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < L.valid) c |= (uint32_t)c8[L.e + j] << (8 * j);
  return c;
}

__device__ __forceinline__ void q8_store_codes(const Q8Lane& L, uint8_t* c8, uint32_t c) {
  if (L.valid == 4) {
    *reinterpret_cast<uint32_t*>(c8 + L.e) = c;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < L.valid) c8[L.e + j] = (uint8_t)(c >> (8 * j));
  }
}

__device__ __forceinline__ void q8_store(const Q8Lane& L, float* p, float* g, bf16_t* pbf, f32x4 pv, int zero_grad) {
  if (L.valid == 4) {
    store4(p + L.e, pv);
    if (pbf) store4(pbf + L.e, pv);
    if (zero_grad) store4(g + L.e, f32x4{0.f, 0.f, 0.f, 0.f});
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < L.valid) {
        p[L.e + j] = pv[j];
        if (pbf) pbf[L.e + j] = (bf16_t)pv[j];
        if (zero_grad) g[L.e + j] = 0.f;
      }
    }
  }
}

__device__ __forceinline__ Q8Lane q8_lane(int64_t blk, int lane, int64_t n) {
  Q8Lane L;
  L.e = blk * 256 + 4 * lane;
  const int64_t left = n - L.e;
  L.valid = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
  return L;
}

// value / absmax quantised against the staged table, 4 codes packed in lane order; absmax == 0: the code nearest to 0
__device__ __forceinline__ uint32_t q8_quantise4(const Q8Table& Q, f32x4 x, float amax) {
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) c |= q8_nearest(Q, amax > 0.f ? x[j] / amax : 0.f) << (8 * j);
  return c;
}

__global__ void __launch_bounds__(256) adamw8_kernel(float* __restrict__ p, float* __restrict__ g, uint8_t* __restrict__ m8,
                                                     uint8_t* __restrict__ v8, float* __restrict__ am, float* __restrict__ av,
                                                     const float* __restrict__ qm, const float* __restrict__ qv,
                                                     bf16_t* __restrict__ pbf, int64_t n, int64_t blk0, int64_t blk1, float omb1,
                                                     float b2, float omb2, float eps, float decay, float step_size,
                                                     float inv_bc2_sqrt, float pre_scale, const float* __restrict__ clip,
                                                     int zero_grad) {
  __shared__ Q8Table Qm, Qv;
  q8_stage(Qm, qm);
  q8_stage(Qv, qv);
  __syncthreads();
  const float gscale = pre_scale * (clip ? clip[1] : 1.f);
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t blk = blk0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); blk < blk1; blk += stride) {  // wave-uniform
    const Q8Lane L = q8_lane(blk, lane, n);
    f32x4 pv, gv, mv, vv;
    q8_load(L, p, g, pv, gv);
    const uint32_t mc = q8_load_codes(L, m8), vc = q8_load_codes(L, v8);
    const float am_old = am[blk], av_old = av[blk];
    float mmax = 0.f, vmax = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float m_old = j < L.valid ? Qm.T[(mc >> (8 * j)) & 255] * am_old : 0.f;
      const float v_old = j < L.valid ? Qv.T[(vc >> (8 * j)) & 255] * av_old : 0.f;
      const float gg = gv[j] * gscale;
      float pp = pv[j] * decay;
      const float mm = m_old + (gg - m_old) * omb1;
      const float vn = v_old * b2 + omb2 * gg * gg;
      const float denom = sqrtf(vn) * inv_bc2_sqrt + eps;
      pp = pp - step_size * (mm / denom);  // the unrounded new moments
      pv[j] = pp;
      mv[j] = mm;
      vv[j] = vn;
      mmax = fmaxf(mmax, fabsf(mm));
      vmax = fmaxf(vmax, vn);
    }
    mmax = wave_max(mmax);
    vmax = wave_max(vmax);
    q8_store_codes(L, m8, q8_quantise4(Qm, mv, mmax));
    q8_store_codes(L, v8, q8_quantise4(Qv, vv, vmax));
    if (lane == 0) {
      am[blk] = mmax;
      av[blk] = vmax;
    }
    q8_store(L, p, g, pbf, pv, zero_grad);
  }
}

__global__ void __launch_bounds__(256) lion8_kernel(float* __restrict__ p, float* __restrict__ g, uint8_t* __restrict__ m8,
                                                    float* __restrict__ am, const float* __restrict__ qm,
                                                    bf16_t* __restrict__ pbf, int64_t n, int64_t blk0, int64_t blk1, float lr,
                                                    float b1, float omb1, float b2, float omb2, float decay, float pre_scale,
                                                    const float* __restrict__ clip, int zero_grad) {
  __shared__ Q8Table Qm;
  q8_stage(Qm, qm);
  __syncthreads();
  const float gscale = pre_scale * (clip ? clip[1] : 1.f);
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t blk = blk0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); blk < blk1; blk += stride) {  // wave-uniform
    const Q8Lane L = q8_lane(blk, lane, n);
    f32x4 pv, gv, mv;
    q8_load(L, p, g, pv, gv);
    const uint32_t mc = q8_load_codes(L, m8);
    const float am_old = am[blk];
    float mmax = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pp = pv[j], mm = j < L.valid ? Qm.T[(mc >> (8 * j)) & 255] * am_old : 0.f;
      lion_elem(pp, gv[j] * gscale, mm, decay, lr, b1, omb1, b2, omb2);
      pv[j] = pp;
      mv[j] = mm;
      mmax = fmaxf(mmax, fabsf(mm));
    }
    mmax = wave_max(mmax);
    q8_store_codes(L, m8, q8_quantise4(Qm, mv, mmax));
    if (lane == 0) am[blk] = mmax;
    q8_store(L, p, g, pbf, pv, zero_grad);
  }
}

// the element range [e0, e1) of a buffer of n elements as whole 256-element blocks
static inline bool q8_range_ok(int64_t n, int64_t e0, int64_t e1) {
  return n > 0 && e0 >= 0 && e0 < e1 && e1 <= n && (e0 & 255) == 0 && ((e1 & 255) == 0 || e1 == n);
}

extern "C" int uwu_adamw8_step(float* p, float* g, void* state1, void* state2, float* absmax1, float* absmax2,
                               const float* qmap1, const float* qmap2, void* p_bf16, int64_t n, int64_t e0, int64_t e1,
                               double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                               float pre_scale, const float* clip, int zero_grad, void* stream) {
  UWU_CHECK_ARG(p && g && state1 && state2 && absmax1 && absmax2 && qmap1 && qmap2, "uwu_adamw8_step: null pointer");
  UWU_CHECK_ARG((((uintptr_t)p | (uintptr_t)g) & 15) == 0, "uwu_adamw8_step: p and g must be 16-byte aligned");
  UWU_CHECK_ARG((((uintptr_t)state1 | (uintptr_t)state2 | (uintptr_t)absmax1 | (uintptr_t)absmax2 | (uintptr_t)qmap1 |
                  (uintptr_t)qmap2) & 3) == 0,
                "uwu_adamw8_step: codes, absmax and tables must be 4-byte aligned");
  UWU_CHECK_ARG(p_bf16 == nullptr || ((uintptr_t)p_bf16 & 7) == 0, "uwu_adamw8_step: bf16 shadow must be 8-byte aligned");
  UWU_CHECK_ARG(q8_range_ok(n, e0, e1),
                "uwu_adamw8_step: bad range [%lld, %lld) of %lld: e0 must be a multiple of 256, e1 a multiple of 256 or n",
                (long long)e0, (long long)e1, (long long)n);
  UWU_CHECK_ARG(step >= 1, "uwu_adamw8_step: step counts from 1");
  // bias corrections, 1 - beta and 1 - lr*wd in double on the host, as python does
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  const int64_t blk0 = e0 >> 8, blk1 = (e1 + 255) >> 8;
  hipLaunchKernelGGL(adamw8_kernel, dim3(ew_grid(blk1 - blk0, 4)), dim3(256), 0, (hipStream_t)stream, p, g, (uint8_t*)state1,
                     (uint8_t*)state2, absmax1, absmax2, qmap1, qmap2, (bf16_t*)p_bf16, n, blk0, blk1, (float)(1.0 - beta1),
                     (float)beta2, (float)(1.0 - beta2), (float)eps, (float)(1.0 - lr * weight_decay), (float)(lr / bc1),
                     (float)(1.0 / sqrt(bc2)), pre_scale, clip, zero_grad);
  UWU_LAUNCH_CHECK("uwu_adamw8_step");
  return UWU_OK;
}

extern "C" int uwu_lion8_step(float* p, float* g, void* state1, float* absmax1, const float* qmap1, void* p_bf16, int64_t n,
                              int64_t e0, int64_t e1, double lr, double beta1, double beta2, double weight_decay,
                              float pre_scale, const float* clip, int zero_grad, void* stream) {
  UWU_CHECK_ARG(p && g && state1 && absmax1 && qmap1, "uwu_lion8_step: null pointer");
  UWU_CHECK_ARG((((uintptr_t)p | (uintptr_t)g) & 15) == 0, "uwu_lion8_step: p and g must be 16-byte aligned");
  UWU_CHECK_ARG((((uintptr_t)state1 | (uintptr_t)absmax1 | (uintptr_t)qmap1) & 3) == 0,
                "uwu_lion8_step: codes, absmax and table must be 4-byte aligned");
  UWU_CHECK_ARG(p_bf16 == nullptr || ((uintptr_t)p_bf16 & 7) == 0, "uwu_lion8_step: bf16 shadow must be 8-byte aligned");
  UWU_CHECK_ARG(q8_range_ok(n, e0, e1),
                "uwu_lion8_step: bad range [%lld, %lld) of %lld: e0 must be a multiple of 256, e1 a multiple of 256 or n",
                (long long)e0, (long long)e1, (long long)n);
  const int64_t blk0 = e0 >> 8, blk1 = (e1 + 255) >> 8;
  hipLaunchKernelGGL(lion8_kernel, dim3(ew_grid(blk1 - blk0, 4)), dim3(256), 0, (hipStream_t)stream, p, g, (uint8_t*)state1,
                     absmax1, qmap1, (bf16_t*)p_bf16, n, blk0, blk1, (float)lr, (float)beta1, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), (float)(1.0 - lr * weight_decay), pre_scale, clip, zero_grad);
  UWU_LAUNCH_CHECK("uwu_lion8_step");
  return UWU_OK;
}
