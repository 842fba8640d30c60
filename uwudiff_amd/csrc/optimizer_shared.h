// What the flat-buffer optimizer kernels (optimizer.hip, optimizer_prodigy.hip, optimizer_8bit.hip, optimizer_adafactor.hip) share:
// the one traversal, the step shape on top of it, and the update rules and sums that more than one file uses.
#pragma once
#include "common.h"

// The rounding contract.  hipcc contracts a*b + c into one fused multiply-add wherever it likes, per copy of an
// expression.  From here to the end of the including file it may not: a fused multiply-add is a __builtin_fmaf / __builtin_fma, a
// product that is rounded first is a named intermediate, and nothing else fuses.  Every rule is written once and serves the vector
// body, the scalar head and tail and the 8-bit kernels alike, so where an element sits in a launch never changes its bits.
#pragma clang fp contract(off)

// Grid-stride over the whole groups of W (4 or 8) elements of [head, n): vec(e) takes the group that starts at element e.  Workgroup
// 0 then takes the peeled head [0, head) and the tail one element at a time: elem(i).  256 threads per workgroup.
template <int W, typename Vec, typename Elem>
__device__ __forceinline__ void for_each_group(int64_t n, int head, Vec vec, Elem elem) {
  static_assert(W == 4 || W == 8, "groups of 4 or 8 elements");
  const int64_t ng = (n - head) >> (W == 8 ? 3 : 2);
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ng; i += stride) vec(head + W * i);
  if (blockIdx.x == 0) {
    const int64_t tail0 = head + ng * W;
    const int64_t extra = head + (n - tail0);
    for (int64_t k = threadIdx.x; k < extra; k += 256) elem(k < head ? k : tail0 + (k - head));
  }
}

// the fp32 factor every step multiplies the gradient by: the loss scale's inverse times the clip coefficient of the norm kernel
__device__ __forceinline__ float grad_scale(float pre_scale, const float* __restrict__ clip) {
  return pre_scale * (clip ? clip[1] : 1.f);
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

// One element's write-back where the traversal is not flat_step's (the per-tensor tiles of optimizer_adafactor.hip): the parameter,
// its bf16 shadow as flat_step's tail rounds it, and the consumed gradient.
__device__ __forceinline__ void flat_write_back(float* __restrict__ p, bf16_t* __restrict__ pbf, float* __restrict__ g, int64_t i,
                                                float pp, int zero_grad) {
  p[i] = pp;
  if (pbf) pbf[i] = (bf16_t)pp;
  if (zero_grad) g[i] = 0.f;
}

// The common step: rule(p, g, s) updates one parameter and its NS fp32 state values from the raw gradient g (the rule scales it).
// Then p and the state are stored, the bf16 shadow refreshed and the consumed gradient overwritten with zeros in the same pass (the
// next backward accumulates into the flat buffer: 4 more bytes written per parameter instead of a fill kernel and a launch).
template <int NS, typename Rule>
__device__ __forceinline__ void flat_step(float* __restrict__ p, float* __restrict__ g, float* const (&s)[NS],
                                          bf16_t* __restrict__ pbf, int64_t n, int zero_grad, Rule rule) {
  for_each_group<4>(n, 0, [&](int64_t e) {
    f32x4 pv = load4(p + e), gv = load4(g + e), sv[NS];
    for (int k = 0; k < NS; ++k) sv[k] = load4(s[k] + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pp = pv[j], ss[NS];
      for (int k = 0; k < NS; ++k) ss[k] = sv[k][j];
      rule(pp, gv[j], ss);
      pv[j] = pp;
      for (int k = 0; k < NS; ++k) sv[k][j] = ss[k];
    }
    store4(p + e, pv);
    for (int k = 0; k < NS; ++k) store4(s[k] + e, sv[k]);
    if (pbf) store4(pbf + e, pv);
    if (zero_grad) store4(g + e, f32x4{0.f, 0.f, 0.f, 0.f});
  }, [&](int64_t i) {
    float pp = p[i], ss[NS];
    for (int k = 0; k < NS; ++k) ss[k] = s[k][i];
    rule(pp, g[i], ss);
    p[i] = pp;
    for (int k = 0; k < NS; ++k) s[k][i] = ss[k];
    if (pbf) pbf[i] = (bf16_t)pp;
    if (zero_grad) g[i] = 0.f;
  });
}

// torch.optim.AdamW (single tensor, no amsgrad), with gs = g * gscale:
//   p *= 1 - lr*wd ; m = lerp(m, gs, 1-b1) ; v = b2*v + (1-b2) gs^2 ;
//   p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)            (the unrounded new moments)
// Fused: gscale*g - m (the product is not rounded on this path), m + omb1*(.), b2*v + (.), inv_bc2_sqrt*sqrt(v) + eps, decay*p - (.).
// Rounded first: gs = gscale*g for the square, omb2*gs, (omb2*gs)*gs, the quotient, step_size*quotient.
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float gscale, float decay, float omb1, float b2,
                                           float omb2, float eps, float step_size, float inv_bc2_sqrt) {
  const float gs = gscale * g;
  const float mn = __builtin_fmaf(omb1, __builtin_fmaf(gscale, g, -m), m);
  const float vn = __builtin_fmaf(b2, v, gs * (omb2 * gs));
  const float denom = __builtin_fmaf(inv_bc2_sqrt, sqrtf(vn), eps);
  const float upd = -step_size * (mn / denom);  // the sign rides on the uniform factor: no negation per element
  p = __builtin_fmaf(decay, p, upd);
  m = mn;
  v = vn;
}

// lion_pytorch.Lion (Chen et al. 2023, Algorithm 2), in the package's order, g already scaled:
//   p *= 1 - lr*wd ; c = b1*m + (1-b1) g ; p -= lr*sign(c) (sign(0) = 0) ; m = b2*m + (1-b2) g
// Fused: b1*m + (.), decay*p - (.), b2*m + (.).  Rounded first: omb1*g, omb2*g, lr*sign.
__device__ __forceinline__ void lion_elem(float& p, float g, float& m, float decay, float lr, float b1, float omb1, float b2,
                                          float omb2) {
  const float c = __builtin_fmaf(b1, m, omb1 * g);
  const float s = c > 0.f ? 1.f : (c < 0.f ? -1.f : 0.f);
  const float upd = lr * s;
  p = __builtin_fmaf(decay, p, -upd);
  m = __builtin_fmaf(b2, m, omb2 * g);
}
