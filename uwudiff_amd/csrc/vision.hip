// The CLIP image tower's own kernels and the CLIP score (uwudiff_amd/vision_model.py, uwudiff_amd/metrics.py; DESIGN.md section
// 4.29).  Forward only: the tower is frozen.  Its attention is uwu_attention_bidir_fwd in attention_text.hip; the patch
// embedding, the projections and the feed-forward run on uwu_gemm, the LayerNorms on uwu_add_ln_modulate_fwd.
//
//   uwu_clip_patches      images [B, 3, S, S] -> the A operand of the patch-embedding GEMM [B * (S / p)^2, ld], columns in the
//                         order (channel, row in patch, column in patch) of patch_embedding.weight.view(D, 3 p p); CLIP's
//                         preprocessing of a [0, 255] image fused in
//   uwu_vit_embed         class token + patch rows + position table -> [B * T, D]
//   uwu_clip_score_accum  100 cos(image_b, text_b) per pair, and their sum and count added to a double accumulator in a fixed order
#include <math.h>

#include "common.h"

namespace {

struct Norm3 {
  float mean[3], std[3];
};

// one thread per output element: the reads of consecutive threads walk a patch row (p contiguous pixels), the writes are contiguous
template <typename TI, typename TO, bool NORM>
__global__ void __launch_bounds__(256) clip_patches_kernel(const TI* __restrict__ img, TO* __restrict__ out, int64_t rows, int S, int p, int ld,
                                                           Norm3 nm) {
  const int G = S / p, K = 3 * p * p;
  const int64_t total = rows * ld;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / ld;
    const int col = (int)(i - row * ld);
    float v = 0.f;  // the columns that pad 3 p p to ld
    if (col < K) {
      const int64_t b = row / (G * G);
      const int pi = (int)(row - b * G * G), py = pi / G, px = pi - py * G;
      const int c = col / (p * p), r = col - c * p * p, iy = r / p, ix = r - iy * p;
      v = (float)img[((b * 3 + c) * S + py * p + iy) * (int64_t)S + px * p + ix];
      if constexpr (NORM) {
        v = fminf(fmaxf(v, 0.f), 255.f);  // NaN -> 0
        v = (v / 255.f - nm.mean[c]) / nm.std[c];
      }
    }
    out[i] = from_f32<TO>(v);
  }
}

// out[b, 0, :] = cls + pos[0];  out[b, 1 + i, :] = patch[b Np + i, :] + pos[1 + i]
template <typename T>
__global__ void __launch_bounds__(256) vit_embed_kernel(const T* __restrict__ patch, const T* __restrict__ cls, const T* __restrict__ pos,
                                                        T* __restrict__ out, int64_t rows, int Tn, int D) {
  const int per = D / 8;
  const int64_t total = rows * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / per;
    const int c = (int)(i - row * per) * 8;
    const int64_t b = row / Tn;
    const int t = (int)(row - b * Tn);
    const f32x8 a = t == 0 ? load8(cls + c) : load8(patch + (b * (Tn - 1) + t - 1) * D + c);
    store8(out + row * D + c, a + load8(pos + (int64_t)t * D + c));
  }
}

// one wave per pair: fp32 dot product and the two squared norms, lanes striding over P
template <typename T>
__global__ void __launch_bounds__(256) clip_score_kernel(const T* __restrict__ img, const T* __restrict__ txt, float* __restrict__ scores, int B,
                                                         int P) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;  // wave-uniform
  float ab = 0.f, aa = 0.f, bb = 0.f;
  for (int c = lane; c < P; c += 64) {
    const float x = to_f32(img[(int64_t)b * P + c]), y = to_f32(txt[(int64_t)b * P + c]);
    ab = fmaf(x, y, ab);
    aa = fmaf(x, x, aa);
    bb = fmaf(y, y, bb);
  }
  ab = wave_sum(ab);
  aa = wave_sum(aa);
  bb = wave_sum(bb);
  if (lane == 0) scores[b] = 100.f * (ab / (sqrtf(aa) * sqrtf(bb)));
}

// ONE workgroup: thread t adds scores[t], scores[t + 256], ... in double, then a tree over the 256 partial sums; thread 0 alone
// touches acc.  The order of every addition is fixed by B, so the same batches give the same bits; launches on one stream are
// ordered, so successive batches need no atomics either.
__global__ void __launch_bounds__(256) clip_score_sum_kernel(const float* __restrict__ scores, double* acc, int B) {
  __shared__ double part[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < B; i += 256) s += (double)scores[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    acc[0] += part[0];
    acc[1] += (double)B;
  }
}

}  // namespace

extern "C" int uwu_clip_patches(const void* images, int in_u8, void* out, int B, int S, int p, int ld, int normalize, const float* mean,
                                const float* std, int dtype, void* stream) {
  UWU_CHECK_ARG(images && out && (!normalize || (mean && std)), "clip_patches: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "clip_patches: bad dtype %d", dtype);
  UWU_CHECK_ARG(B > 0 && S > 0 && p > 0 && S % p == 0, "clip_patches: bad shape B = %d, S = %d, p = %d (S must be a multiple of p)", B, S, p);
  UWU_CHECK_ARG((int64_t)3 * p * p <= ld && ld <= 0x7FFFFFFF / 2, "clip_patches: ld = %d < 3 p p = %d", ld, 3 * p * p);
  UWU_CHECK_ARG(!in_u8 || normalize, "clip_patches: a uint8 image is a [0, 255] image: normalize must be set");
  Norm3 nm{{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};
  if (normalize)
    for (int c = 0; c < 3; ++c) {
      UWU_CHECK_ARG(isfinite(mean[c]) && isfinite(std[c]) && std[c] > 0.f, "clip_patches: bad mean / std of channel %d", c);
      nm.mean[c] = mean[c];
      nm.std[c] = std[c];
    }
  const int64_t rows = (int64_t)B * (S / p) * (S / p);
  const int grid = ew_grid(rows * ld, 256);
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
#define UWU_CP_LAUNCH(TI, TO, NORM) \
  hipLaunchKernelGGL((clip_patches_kernel<TI, TO, NORM>), dim3(grid), dim3(256), 0, st, (const TI*)images, (TO*)out, rows, S, p, ld, nm)
  if (in_u8) {
    if (dtype == UWU_BF16) UWU_CP_LAUNCH(uint8_t, bf16_t, true);
    else UWU_CP_LAUNCH(uint8_t, float, true);
  } else if (normalize) {
    if (dtype == UWU_BF16) UWU_CP_LAUNCH(float, bf16_t, true);
    else UWU_CP_LAUNCH(float, float, true);
  } else {
    if (dtype == UWU_BF16) UWU_CP_LAUNCH(float, bf16_t, false);
    else UWU_CP_LAUNCH(float, float, false);
  }
#undef UWU_CP_LAUNCH
  prof.done(UWU_PROF_OTHER, dtype == UWU_BF16 ? 0 : 1, 0.0, 3.0 * B * S * S * (in_u8 ? 1 : 4) + (double)rows * ld * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("clip_patches");
  return UWU_OK;
}

extern "C" int uwu_vit_embed(const void* patch_out, const void* class_embedding, const void* pos_table, void* out, int B, int T, int D,
                             int dtype, void* stream) {
  UWU_CHECK_ARG(patch_out && class_embedding && pos_table && out, "vit_embed: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "vit_embed: bad dtype %d", dtype);
  UWU_CHECK_ARG(B > 0 && T >= 2 && D > 0 && D % 8 == 0, "vit_embed: bad shape B = %d, T = %d, D = %d (T = patches + 1, D a multiple of 8)", B, T, D);
  UWU_CHECK_ARG((((uintptr_t)patch_out | (uintptr_t)class_embedding | (uintptr_t)pos_table | (uintptr_t)out) & 15) == 0,
                "vit_embed: misaligned pointer");
  const int64_t rows = (int64_t)B * T;
  const int grid = ew_grid(rows * (D / 8), 256);
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  if (dtype == UWU_BF16)
    hipLaunchKernelGGL(vit_embed_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)patch_out, (const bf16_t*)class_embedding,
                       (const bf16_t*)pos_table, (bf16_t*)out, rows, T, D);
  else
    hipLaunchKernelGGL(vit_embed_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)patch_out, (const float*)class_embedding,
                       (const float*)pos_table, (float*)out, rows, T, D);
  prof.done(UWU_PROF_OTHER, dtype == UWU_BF16 ? 0 : 1, 0.0, 2.0 * B * T * D * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("vit_embed");
  return UWU_OK;
}

extern "C" int uwu_clip_score_accum(const void* image_embeds, const void* text_embeds, float* scores, double* acc, int B, int P, int dtype,
                                    void* stream) {
  UWU_CHECK_ARG(image_embeds && text_embeds && scores && acc, "clip_score_accum: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "clip_score_accum: bad dtype %d", dtype);
  UWU_CHECK_ARG(B > 0 && P > 0, "clip_score_accum: bad shape B = %d, P = %d", B, P);
  UWU_CHECK_ARG(((uintptr_t)scores & 3) == 0 && ((uintptr_t)acc & 7) == 0 &&
                    (((uintptr_t)image_embeds | (uintptr_t)text_embeds) & (dtype == UWU_BF16 ? 1 : 3)) == 0,
                "clip_score_accum: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  if (dtype == UWU_BF16)
    hipLaunchKernelGGL(clip_score_kernel<bf16_t>, dim3(cdiv(B, 4)), dim3(256), 0, st, (const bf16_t*)image_embeds, (const bf16_t*)text_embeds,
                       scores, B, P);
  else
    hipLaunchKernelGGL(clip_score_kernel<float>, dim3(cdiv(B, 4)), dim3(256), 0, st, (const float*)image_embeds, (const float*)text_embeds,
                       scores, B, P);
  hipLaunchKernelGGL(clip_score_sum_kernel, dim3(1), dim3(256), 0, st, (const float*)scores, acc, B);
  prof.done(UWU_PROF_OTHER, dtype == UWU_BF16 ? 0 : 1, 6.0 * B * P, 2.0 * B * P * (dtype == UWU_BF16 ? 2 : 4));
  UWU_LAUNCH_CHECK("clip_score_accum");
  return UWU_OK;
}
