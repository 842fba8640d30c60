// Sampling glue around the denoiser, the VAE decoder and the PNG encoder (reference src/duwu/sampling/sampling.py:109-126,
// cfg.py:113-125, data/utils.py:10-19).  All HBM-bound streaming kernels: 16-byte accesses, grid-stride loops over a capped grid.
// The noise-drawing sampler update (uwu_sampler_combine_draw) lives in objective.hip beside the device functions it shares.
#include "common.h"

// ---------------------------------------------------------------------------------------
// cfg.py:116-118 + k_diffusion_wrapper.py:103-106: the guidance batch cat([x, x]) * c_in.  One read, two writes (12 B / element).
__global__ void __launch_bounds__(256) cfg_input_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t total4, float s) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const f32x4 v = load4(x + 4 * i) * s;
    store4(y + 4 * i, v);
    store4(y + 4 * (total4 + i), v);
  }
}

extern "C" int uwu_cfg_input(const float* x, float* y, int B, int64_t n, float c_in, void* stream) {
  UWU_CHECK_ARG(x && y, "cfg_input: null pointer");
  UWU_CHECK_ARG(B > 0 && n > 0 && ((int64_t)B * n) % 4 == 0, "cfg_input: B * n = %lld must be a positive multiple of 4",
                (long long)B * (long long)n);
  UWU_CHECK_ARG((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "cfg_input: pointers must be 16-byte aligned");
  const int64_t total4 = (int64_t)B * n / 4;
  hipLaunchKernelGGL(cfg_input_kernel, dim3(ew_grid(total4, 256)), dim3(256), 0, (hipStream_t)stream, x, y, total4, c_in);
  UWU_LAUNCH_CHECK("cfg_input");
  return UWU_OK;
}

// ---------------------------------------------------------------------------------------
// sampling.py:114-116: y = (rescale ? x / std_b : x) * vae_std + vae_mean, std_b = torch.std over the n elements of sample b (n - 1).
// Two deterministic stages.  Stage 1: workgroup (k, b) owns elements [k * LF_CHUNK, (k + 1) * LF_CHUNK) of sample b, held in registers:
// its sum gives the chunk mean, then the squared deviations from THAT mean are summed (no E[x^2] - E[x]^2 cancellation); it stores
// (mean_k, M2_k).  Stage 2: every workgroup adds the partials of its sample in ascending k (Chan et al.'s pairwise update of mean / M2)
// and writes its chunk.  The partition depends on n alone and nothing is accumulated atomically, so a sample's output bits do not
// depend on the batch it is in.
constexpr int LF_CHUNK = 4096;  // 256 lanes x 4 trips x 4 elements

__global__ void __launch_bounds__(256) latent_stats_kernel(const float* __restrict__ x, int64_t n, int nchunk, float* __restrict__ part) {
  __shared__ float red[4];
  const int k = blockIdx.x, b = blockIdx.y;
  const float* xb = x + (int64_t)b * n;
  const int64_t base = (int64_t)k * LF_CHUNK;
  const int64_t left = n - base;
  const int cnt = (int)(left < LF_CHUNK ? left : LF_CHUNK);
  f32x4 v[4];
  bool ok[4];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = j * 1024 + 4 * (int)threadIdx.x;
    ok[j] = e < cnt;  // n % 4 == 0: a vector is inside or outside as a whole
    v[j] = ok[j] ? load4(xb + base + e) : f32x4{0.f, 0.f, 0.f, 0.f};
    s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
  }
  const float mean = block_sum<4>(s, red) / (float)cnt;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (ok[j]) {
      const f32x4 d = v[j] - mean;
      q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
  const float m2 = block_sum<4>(q, red);
  if (threadIdx.x == 0) {
    float* p = part + 2 * ((int64_t)b * nchunk + k);
    p[0] = mean;
    p[1] = m2;
  }
}

__global__ void __launch_bounds__(256) latent_finish_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, int nchunk,
                                                            const float* __restrict__ part, float vae_std, float vae_mean) {
  __shared__ float sd_s;
  const int k = blockIdx.x, b = blockIdx.y;
  if (part) {
    if (threadIdx.x == 0) {
      const float* p = part + 2 * (int64_t)b * nchunk;
      float cnt = 0.f, mean = 0.f, m2 = 0.f;
      for (int j = 0; j < nchunk; ++j) {  // ascending chunk order
        const int64_t left = n - (int64_t)j * LF_CHUNK;
        const float cj = (float)(left < LF_CHUNK ? left : LF_CHUNK);
        const float tot = cnt + cj, delta = p[2 * j] - mean;
        mean += delta * (cj / tot);
        m2 += p[2 * j + 1] + delta * delta * (cnt * cj / tot);
        cnt = tot;
      }
      sd_s = sqrtf(m2 / (float)(n - 1));
    }
    __syncthreads();
  }
  const float sd = part ? sd_s : 1.f;
  const int64_t base = (int64_t)b * n + (int64_t)k * LF_CHUNK;
  const int64_t left = n - (int64_t)k * LF_CHUNK;
  const int cnt = (int)(left < LF_CHUNK ? left : LF_CHUNK);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = j * 1024 + 4 * (int)threadIdx.x;
    if (e < cnt) {
      f32x4 v = load4(x + base + e);
      if (part) v = v / sd;
      store4(y + base + e, v * vae_std + vae_mean);
    }
  }
}

static inline int lf_chunks(int64_t n) { return (int)((n + LF_CHUNK - 1) / LF_CHUNK); }

extern "C" size_t uwu_latent_finish_ws_bytes(int B, int64_t n) {
  if (B <= 0 || n <= 0) return 0;
  return (size_t)B * (size_t)lf_chunks(n) * 2 * sizeof(float);
}

extern "C" int uwu_latent_finish(const float* x, float* y, int B, int64_t n, int rescale, float vae_std, float vae_mean, void* ws,
                                 size_t ws_bytes, void* stream) {
  UWU_CHECK_ARG(x && y, "latent_finish: null pointer");
  UWU_CHECK_ARG(B > 0 && B <= 65535 && n > 0 && n % 4 == 0, "latent_finish: B=%d n=%lld (n must be a positive multiple of 4)", B,
                (long long)n);
  UWU_CHECK_ARG(!rescale || n > 1, "latent_finish: the unbiased deviation needs n > 1");
  UWU_CHECK_ARG((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "latent_finish: pointers must be 16-byte aligned");
  const int nchunk = lf_chunks(n);
  if (rescale) {
    UWU_CHECK_ARG(ws && ws_bytes >= uwu_latent_finish_ws_bytes(B, n), "latent_finish: workspace of %zu bytes needed",
                  uwu_latent_finish_ws_bytes(B, n));
    hipLaunchKernelGGL(latent_stats_kernel, dim3(nchunk, B), dim3(256), 0, (hipStream_t)stream, x, n, nchunk, (float*)ws);
    UWU_LAUNCH_CHECK("latent_finish (stats)");
  }
  hipLaunchKernelGGL(latent_finish_kernel, dim3(nchunk, B), dim3(256), 0, (hipStream_t)stream, x, y, n, nchunk,
                     rescale ? (const float*)ws : (const float*)nullptr, vae_std, vae_mean);
  UWU_LAUNCH_CHECK("latent_finish");
  return UWU_OK;
}

// ---------------------------------------------------------------------------------------
// data/utils.py:10-19 (vae_image_postprocess) for a batch: [B, 3, H, W] fp32 / bf16 planes -> uint8 [B, H, W, 3],
//   u8 = trunc(clamp((x * 0.5 + 0.5) * 255, 0, 255))     in fp32, in that order (the reference truncates; it does not round).
// The output is one stream of 3 * B * H * W bytes; a lane takes four consecutive pixels of it (12 bytes = three dwords at a 12-byte
// offset, so dword-aligned whatever H and W are).  With H * W a multiple of 4 the four pixels lie in one image and each plane is read
// with one vector load; otherwise a group may straddle two images and is read pixel by pixel.
#pragma clang fp contract(off)
__device__ __forceinline__ unsigned image_level(float x) {
  float v = (x * 0.5f + 0.5f) * 255.f;
  v = fminf(fmaxf(v, 0.f), 255.f);
  return (unsigned)v;
}
struct __attribute__((packed, aligned(4))) U32x3 { unsigned a, b, c; };

template <typename T>
__global__ void __launch_bounds__(256) image_u8_kernel(const T* __restrict__ x, unsigned char* __restrict__ y, int64_t HW, int64_t npix) {
  const int64_t groups = (npix + 3) / 4;
  const bool vec = (HW % 4) == 0;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t p0 = 4 * g;
    unsigned q[4][3];
    if (vec) {  // npix = B * HW is a multiple of 4 too: the group is whole
      const int64_t b = p0 / HW, p = p0 - b * HW;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f32x4 v = load4(x + (b * 3 + c) * HW + p);
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j][c] = image_level(v[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t pj = p0 + j;
        const bool in = pj < npix;
        const int64_t b = in ? pj / HW : 0, p = in ? pj - b * HW : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) q[j][c] = in ? image_level(to_f32(x[(b * 3 + c) * HW + p])) : 0u;
      }
    }
    if (p0 + 4 <= npix) {
      U32x3 o;
      o.a = q[0][0] | (q[0][1] << 8) | (q[0][2] << 16) | (q[1][0] << 24);
      o.b = q[1][1] | (q[1][2] << 8) | (q[2][0] << 16) | (q[2][1] << 24);
      o.c = q[2][2] | (q[3][0] << 8) | (q[3][1] << 16) | (q[3][2] << 24);
      *reinterpret_cast<U32x3*>(y + 3 * p0) = o;
    } else {  // the last, partial group of the stream
      for (int j = 0; j < 4; ++j)
        if (p0 + j < npix)
          for (int c = 0; c < 3; ++c) y[3 * (p0 + j) + c] = (unsigned char)q[j][c];
    }
  }
}

extern "C" int uwu_image_u8(const void* x, int dtype, void* y, int B, int H, int W, void* stream) {
  UWU_CHECK_ARG(x && y, "image_u8: null pointer");
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "image_u8: bad dtype %d", dtype);
  UWU_CHECK_ARG(B > 0 && H > 0 && W > 0, "image_u8: bad shape B=%d H=%d W=%d", B, H, W);
  UWU_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 3) == 0, "image_u8: misaligned pointer");
  const int64_t HW = (int64_t)H * W, npix = (int64_t)B * HW;
  const int grid = ew_grid((npix + 3) / 4, 256);
  if (dtype == UWU_F32)
    hipLaunchKernelGGL((image_u8_kernel<float>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)x, (unsigned char*)y, HW, npix);
  else
    hipLaunchKernelGGL((image_u8_kernel<bf16_t>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (unsigned char*)y, HW,
                       npix);
  UWU_LAUNCH_CHECK("image_u8");
  return UWU_OK;
}
