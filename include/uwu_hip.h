/*
 * uwu_hip.h -- C ABI of libuwu_hip.so: the MI355X (gfx950) kernels behind the `duwu`
 * training inner loop.
 *
 * The reference (KohakuBlueleaf/UwUDiff) has NO FFI on this path: its boundary is a Python
 * plugin slot (`instantiate_any`, reference src/duwu/utils/__init__.py:41-50; `load_any`,
 * src/duwu/loader.py:58-67).  Each entry below therefore cites the reference *Python* lines
 * whose torch/diffusers op sequence it replaces; INTEGRATION.md shows the ctypes binding a
 * maintainer adds on the reference side.
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch tensors' data_ptr());
 *   - no entry allocates, frees or synchronises; work is enqueued on `stream` (a hipStream_t
 *     passed as void*);
 *   - return 0 on success, a negative UWU_E* code otherwise; uwu_last_error() gives the text;
 *   - `dtype` arguments: UWU_F32 = 0, UWU_BF16 = 1 (storage type of the activation operands;
 *     accumulation, statistics, loss and optimizer state are always fp32).
 */
#ifndef UWU_HIP_H
#define UWU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UWU_F32 0
#define UWU_BF16 1
#define UWU_I64 2 /* int64 indices: only where an entry says it takes them (uwu_timestep_stats_accum) */

#define UWU_OK 0
#define UWU_EINVAL (-1)   /* bad argument / unsupported shape */
#define UWU_ELAUNCH (-2)  /* hipLaunch error */
#define UWU_ENOTIMPL (-3)

/* prediction / target parameterisations (reference src/duwu/loss/diffusion.py:84-125) */
#define UWU_PT_EPSILON 0
#define UWU_PT_V 1
#define UWU_PT_SAMPLE 2
#define UWU_PT_RF 3

/* element losses of the fused objective (the reference's `loss` argument, src/duwu/loss/diffusion.py:27): uwu_loss_elem_fwd_bwd */
#define UWU_LOSS_MSE 0
#define UWU_LOSS_L1 1
#define UWU_LOSS_HUBER 2     /* loss_param = delta > 0 */
#define UWU_LOSS_SMOOTH_L1 3 /* loss_param = beta > 0 (beta = 0 is UWU_LOSS_L1) */

/* GEMM epilogues */
#define UWU_EPI_NONE 0
#define UWU_EPI_BIAS 1       /* C = A.B + bias[n]                                        */
#define UWU_EPI_BIAS_GELU 2  /* C = A.B + bias ; C2 = gelu_tanh(C)   (fc1 forward)       */
#define UWU_EPI_DGELU 3      /* C = (A.B) * gelu_tanh'(aux[m,n])     (fc2 dgrad -> dU); if C2 != NULL it is a
                                float[N] receiving += column sums of C (fc1 bias gradient)              */
#define UWU_EPI_BIAS_SILU 4  /* C = silu(A.B + bias)                 (timestep MLP)      */
#define UWU_EPI_ACCUM 5      /* C += A.B  (fp32 C only; wgrad accumulation, split-K)     */

const char* uwu_last_error(void);
int uwu_version(void);
/* The library's environment switches (UWU_GEMM_*, ...: kernel A/B comparisons and sweeps, tools/README.md) are read once
 * and cached; call this after changing one inside a running process.  Returns the new generation number. */
int uwu_env_refresh(void);
/* Zero `bytes` bytes of device memory on `stream` (hipMemsetAsync): the flat gradient buffer and the optimizer moments at their
 * creation (reference: torch.zeros_like in torch.optim.AdamW's state initialisation / autograd's first accumulation). */
int uwu_memset_zero(void* p, uint64_t bytes, void* stream);

/* ------------------------------------------------------------------ objective (a1-a10) */

/* Per-sample schedule gather: replaces the Python loops at diffusion.py:58 (B x nonzero().item()),
 * :146 and :159-161.  coef[b] = {sigma_b, weight_b, sqrt(abar_t), sqrt(1-abar_t)}.
 *   sigma_b  = sigmas_desc[N-1-t_b]                         (diffusion.py:53-62)
 *   weight_b = [min(snr,gamma)/snr | /(snr+1) for v]  x  [1/sqrt(min(snr,1000))]   (:141-167)
 * snr_mode: 0 none, 1 epsilon form, 2 v form; debias: 0/1. */
int uwu_schedule_gather(const int64_t* timesteps, const float* sigmas_desc, const float* all_snr,
                        const float* alphas_cumprod, int n_train, int B, int snr_mode, float gamma,
                        int debias, float* coef, void* stream);

/* Rectified-flow time sampling: rectified_flow.py:29-42 and sigma_to_timestep :98-129.
 *   time = u01*smax/(1+smax); sigma = time/(1-time); timesteps = log-sigma piecewise-linear inverse
 * over log_sigmas_asc[n_train] (ascending log of sigmas[:-1] flipped).  coef[b] = {sigma,1,0,0}. */
int uwu_rf_time_to_sigma(const float* u01, float sigma_max, const float* log_sigmas_asc, int n_train,
                         int B, float* coef, float* timesteps, void* stream);

/* Forward process, diffusion.py:77-82 / rectified_flow.py:67-71:
 *   noisy = (x + noise*sigma_b) * (sigma_b^2+1)^-1/2 ; fp32 out and (optional, may be NULL) bf16 copy.
 * n = elements per sample. */
int uwu_qsample(const float* x, const float* noise, const float* coef, int B, int64_t n, float* noisy,
                void* noisy_bf16, void* stream);

/* The same with the VAE latent normalisation of trainer.py:241-244 folded in: x_norm = (x - vae_mean) / vae_std
 * (written once: it is the clean latent the loss compares against), noisy = (x_norm + noise*sigma_b)*(sigma_b^2+1)^-1/2. */
int uwu_qsample_norm(const float* x, const float* noise, const float* coef, int B, int64_t n, float vae_mean,
                     float vae_std, float* x_norm, float* noisy, void* stream);

/* In-kernel draws of the training objective (diffusion.py:68-70 `torch.randint(0, N, (B,))`, :75 `torch.randn_like(x)`;
 * rectified_flow.py:37 `torch.rand(B)`): Philox4x32-10, counter = offset + element group, key = seed (no device state).  The
 * host mirror reserves the offset ranges in the reference's order of draws (noise, then timesteps / u01) from torch's CUDA
 * generator.  uwu_philox_raw: n_counters x 4 raw words (parity with oracle/philox.py); uwu_philox_normal: n N(0,1) floats, 4 per
 * counter (Box-Muller); uwu_draw_timesteps: t[b] = (word (b % 4) of counter b / 4) * n_train >> 32; uwu_draw_u01: the same word
 * as ((r >> 8) + 1/2) / 2^24.  uwu_qsample_draw = uwu_qsample / uwu_qsample_norm with the noise drawn inside (element group i of
 * the [B, n] tensor = counter offset + i): writes noise, noisy and (use_norm) x_norm in one pass. */
int uwu_philox_raw(uint32_t* out, int64_t n_counters, uint64_t seed, uint64_t offset, void* stream);
int uwu_philox_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
int uwu_draw_timesteps(int64_t* timesteps, int n_train, int B, uint64_t seed, uint64_t offset, void* stream);
int uwu_draw_u01(float* u01, int B, uint64_t seed, uint64_t offset, void* stream);
int uwu_qsample_draw(const float* x, const float* coef, int B, int64_t n, int use_norm, float vae_mean, float vae_std,
                     float* x_norm, float* noise, float* noisy, uint64_t seed, uint64_t offset, void* stream);
/* AutoencoderKL posterior: moments fp32 channels-last [B*HW][ldm] (mean in channels 0 .. latent-1, logvar in latent .. 2 latent-1)
 * -> fp32 NCHW [B, latent, HW]:  z = mean + exp(0.5 clamp(logvar, -30, 20)) * eps, element i of z taking element i of
 * uwu_philox_normal(B*latent*HW, seed, offset);  mean_out / logvar_out (clamped) are the same moments as NCHW.  Each of the three
 * outputs may be null (at least one is not); nothing is drawn when z is null.  B*latent*HW must be a multiple of 4. */
int uwu_posterior_draw(const float* moments, int ldm, int B, int latent, int64_t HW, float* z, float* mean_out, float* logvar_out,
                       uint64_t seed, uint64_t offset, void* stream);

/* Conditioning front-end, text_encoders.py:196-262: place one text encoder's hidden states src [B,S,F] (fp32 / bf16),
 * times its attention mask [B,S] (int64, may be NULL: zero_for_padding off or no mask), into the zero-filled context
 * out [B,S_total,F_total] (fp32) at sequence offset s_off (its concat bucket) and feature offset f_off (its place
 * inside the bucket; narrower buckets stay zero-padded on the feature axis). */
int uwu_ctx_place(const void* src, int dtype, const int64_t* mask, float* out, int B, int S, int F, int S_total,
                  int F_total, int s_off, int f_off, void* stream);

/* Fused prediction conversion + target + per-sample weighted MSE + d loss/d model_output,
 * diffusion.py:177-193 (+ :100-139) and rectified_flow.py:79-96.
 *   xt: the tensor the reference passes as `xt` (clean x for DiffusionLoss :177, noisy for RF :80).
 *   out_dtype: dtype of model_output and of grad_out.
 *   pred/target may be NULL (aux outputs).  losses[b] = w_b * mean((pred-target)^2);
 *   grad_out = d mean_b(losses) / d model_output.  force_convert=1 is the RF path (always converts). */
int uwu_loss_fwd_bwd(const float* x, const float* noise, const float* xt, const void* model_output,
                     int out_dtype, const float* coef, int pred_type, int target_type, int force_convert,
                     int B, int64_t n, float* losses, float* loss_mean, void* grad_out, float* pred,
                     float* target, void* stream);
/* The same with the element loss chosen: losses[b] = w_b * mean_i rho(d_bi), grad_out = w_b c_b rho'(d) / (n B), d = pred - target,
 * c_b = d pred / d model_output.  loss_kind is a UWU_LOSS_*; loss_param is Huber's delta / SmoothL1's beta (FLT_MIN <= loss_param <= FLT_MAX:
 * positive, normal and finite; ignored by MSE and L1):
 *   MSE       rho = d^2                                              rho' = 2 d
 *   L1        rho = |d|                                              rho' = sign(d), 0 at d == 0
 *   HUBER     rho = |d| < delta ? d^2 / 2 : delta (|d| - delta / 2)  rho' = |d| < delta ? d : delta sign(d)
 *   SMOOTH_L1 rho = |d| < beta ? d^2 / (2 beta) : |d| - beta / 2     rho' = |d| < beta ? d / beta : sign(d)
 * A NaN in d is a NaN in that element of grad_out and in losses[b] for every kind (torch's L1Loss gives gradient 0 there);
 * d = +-inf gives rho = inf and rho' = +-delta / +-1.  uwu_loss_fwd_bwd is this entry with UWU_LOSS_MSE. */
int uwu_loss_elem_fwd_bwd(const float* x, const float* noise, const float* xt, const void* model_output,
                          int out_dtype, const float* coef, int pred_type, int target_type, int force_convert,
                          int loss_kind, float loss_param, int B, int64_t n, float* losses, float* loss_mean,
                          void* grad_out, float* pred, float* target, void* stream);

/* y[i] *= *scale (device scalar); used when autograd hands a non-unit upstream gradient. */
int uwu_scale_inplace(void* y, int dtype, int64_t n, const float* scale, void* stream);
/* y[i] = x[i] * *scale: the same for a SAVED gradient that must stay as it is (the loss's d/d(model output), produced in its
 * forward pass, reference diffusion.py:170-193 via autograd) -- one pass instead of a clone + the in-place form. */
int uwu_scale_into(const void* x, void* y, int dtype, int64_t n, const float* scale, void* stream);
/* y[i] = (float)x[i] for the int64 timesteps the loss hands the denoiser (reference diffusion.py:68-70 draws them as int64,
 * rope_unet.py / the DiT's timestep embedding reads them as floats): the conversion in front of the forward, on the library's stream. */
int uwu_cast_i64_to_f32(const int64_t* x, float* y, int64_t n, void* stream);

/* Conditioning front-end (section 8f rank 4): ragged -> padded aggregation of per-caption embeddings.
 * Reference src/duwu/utils/aggregation.py:6-171.  `starts` = device int32 [B+1] prefix sums of n_elements; one "unit"
 * is one caption's [seq, ...] block of unit_bytes contiguous bytes (any dtype: pure byte movement).
 *   concat: out[b, 0 : n_b * unit] = emb[starts[b] : starts[b+1]], the rest of the max_n * unit row = pad pattern
 *           (pad_bits = the pad value's bit pattern in the low elem_size bytes)       aggregation.py:15-39,64-108
 *   split:  inverse of concat (gathers the valid prefix of every padded row)           aggregation.py:111-171
 *   first:  out[b] = emb[starts[b]]                                                    aggregation.py:174-185 */
int uwu_aggregate_concat(const void* emb, const int* starts, void* out, int B, int max_n, int64_t unit_bytes,
                         int elem_size, uint64_t pad_bits, void* stream);
int uwu_aggregate_split(const void* cat, const int* starts, void* out, int B, int max_n, int64_t unit_bytes,
                        void* stream);
int uwu_aggregate_first(const void* emb, const int* starts, void* out, int B, int64_t unit_bytes, void* stream);

/* Sampler (section 8f rank 1).  One Euler-ancestral step with classifier-free guidance, fused:
 *   eps = uncond + (cond-uncond)*cfg  (reference sampling/cfg.py:113-125; eps_uncond NULL -> no guidance)
 *   denoised = x - sigma*eps          (sampling/k_diffusion_wrapper.py:98-108)
 *   x' = x + eps*(sigma_down - sigma) + noise*s_noise*sigma_up   (sampling/k_diffusion_euler.py:42-47)
 * denoised may be NULL.  uwu_scale_copy: y = x*scale (the c_in = 1/sqrt(sigma^2+1) input scaling). */
int uwu_sampler_step(const float* x, const float* eps_cond, const float* eps_uncond, const float* noise, float* out,
                     float* denoised, int64_t n, float cfg, float sigma, float sigma_down, float sigma_up,
                     float s_noise, void* stream);
/* General sampler update for the DPM-Solver-2 and CFG++ variants (sampling/k_diffusion_dpm2.py:8-111,
 * k_diffusion_euler.py:51-106): every step of those samplers is
 *   out = base + a * eps_cfg + b * eps_uncond + c * noise,   eps_cfg = eps_uncond + (eps_cond - eps_uncond) * cfg
 * for scalars (a, b, c) derived from the sigmas on the host (denoised = x - sigma eps; to_d(x, sigma, denoised) = eps).
 * eps_uncond NULL: unguided (eps_uncond := eps_cond).  noise NULL: no noise term. */
int uwu_sampler_combine(const float* base, const float* eps_cond, const float* eps_uncond, const float* noise,
                        float* out, int64_t n, float cfg, float a, float b, float c, void* stream);
int uwu_scale_copy(const float* x, float* y, int64_t n, float scale, void* stream);

/* Prompt-to-image sampling glue.
 * uwu_cfg_input: the guidance batch of the denoiser.  x fp32 [B, n] -> y fp32 [2B, n], both halves x * c_in: one read and two writes
 *   instead of uwu_scale_copy + torch.cat (reference sampling/cfg.py:116-118, k_diffusion_wrapper.py:103-106).  B * n % 4 == 0.
 * uwu_sampler_combine_draw: uwu_sampler_combine with the noise term drawn in the kernel -- element i takes element i of
 *   uwu_philox_normal(n, seed, offset), the counter convention of uwu_qsample_draw -- so no noise tensor exists in memory
 *   (k_diffusion_euler.py:46-47, :104-105; k_diffusion_dpm2.py:32-35, :86-89).  Same device functions as the two entries it fuses:
 *   bit-identical to uwu_philox_normal followed by uwu_sampler_combine.  n % 4 == 0.
 * uwu_latent_finish: y = (rescale ? x / std_b : x) * vae_std + vae_mean on fp32 [B, n] latents, std_b = torch.std over the n elements
 *   of sample b (divisor n - 1) (sampling/sampling.py:114-116).  Two deterministic stages over a partition that depends on n alone
 *   (per-workgroup partials added in ascending order): a sample's bits do not depend on its batch.  ws: uwu_latent_finish_ws_bytes(B, n)
 *   bytes, needed with rescale only.  n % 4 == 0.
 * uwu_image_u8: vae_image_postprocess for a batch (data/utils.py:10-19).  x [B, 3, H, W] (UWU_F32 / UWU_BF16) -> y uint8 [B, H, W, 3],
 *   trunc(clamp((x * 0.5 + 0.5) * 255, 0, 255)) in fp32 in that order.  Any H, W. */
int uwu_cfg_input(const float* x, float* y, int B, int64_t n, float c_in, void* stream);
int uwu_sampler_combine_draw(const float* base, const float* eps_cond, const float* eps_uncond, float* out, int64_t n, float cfg,
                             float a, float b, float c, uint64_t seed, uint64_t offset, void* stream);
size_t uwu_latent_finish_ws_bytes(int B, int64_t n);
int uwu_latent_finish(const float* x, float* y, int B, int64_t n, int rescale, float vae_std, float vae_mean, void* ws,
                      size_t ws_bytes, void* stream);
int uwu_image_u8(const void* x, int dtype, void* y, int B, int H, int W, void* stream);

/* ------------------------------------------------------------------ training images
 * resize_and_crop_image (data/utils.py:25-58) for a batch of decoded pictures: Pillow's 8-bit resampler, byte for byte, then the crop,
 * ToTensor and Normalize(0.5, 0.5).
 *
 * The rule for one axis with `in` source pixels, `out` output pixels and a filter of support S (doubles, libm's sin):
 *   scale = in / out; fs = max(scale, 1); support = S * fs; ksize = ceil(support) * 2 + 1
 *   output xx: center = (xx + 0.5) * scale; xmin = max((int)(center - support + 0.5), 0); n = min((int)(center + support + 0.5), in) - xmin
 *              w[x] = filter((x + xmin - center + 0.5) / fs), x < n; k[x] = w[x] / (sum of w, ascending x)
 *              K[x] = (int)(k < 0 ? k * 2^22 - 0.5 : k * 2^22 + 0.5)
 *   pixel   = clamp((2^21 + sum_x src[xmin + x] * K[x]) >> 22, 0, 255)   (int32 accumulator, arithmetic shift, per channel)
 * The horizontal pass runs first and writes uint8; the vertical pass reads that; a pass whose axis keeps its size is skipped.
 *
 * uwu_resample_ksize / uwu_resample_coeffs: HOST-ONLY (no device call, usable without a GPU; the pointers are HOST pointers).
 *   coeffs int32 [count, ksize] (entries past n are 0) and bounds int32 [count, 2] = (xmin, n) for the output indices
 *   first .. first + count - 1 of one axis.  ksize: the row length, or UWU_EINVAL for a bad size / filter.
 * uwu_image_resize_crop: src is ONE device buffer of src_bytes bytes holding B uint8 [h, w, 3] pictures.  HOST arrays describe them:
 *   src_off int64 [B]    byte offset of picture b
 *   meta    int32 [B, 6] (src_h, src_w, new_h, new_w, top, left): its size, the size it is resized to, its window in the resized picture
 *   tab_off int64 [B, 4] offsets (int32 elements) into the DEVICE buffer `tables` (tables_len elements) of: the horizontal coeffs
 *                        [Wt, ksize] and bounds [Wt, 2] of output columns left .. left + Wt - 1, the vertical coeffs [Ht, ksize] and
 *                        bounds [Ht, 2] of output rows top .. top + Ht - 1 (uwu_resample_coeffs's layout; ignored for a skipped pass)
 *   out [B, 3, Ht, Wt] (UWU_F32 / UWU_BF16): normalize = 1 writes (u / 255 - 0.5) / 0.5, normalize = 0 writes u / 255, each the fp32
 *   value of that chain of IEEE operations (bf16: its round-to-nearest-even).  Two launches per group of 16 pictures: the horizontal
 *   pass writes only the source rows the window's output rows touch into ws (uwu_image_resize_crop_ws_bytes), the vertical pass
 *   reads them.  Every argument is checked on the host before anything is launched (window inside the resized picture, resized
 *   size >= target, B / Ht / Wt >= 1, pointers non-null and 16-byte aligned, offsets inside src and tables, dtype, filter); a bound
 *   read from `tables` is clamped to the rows / columns the picture has, so a wrong table gives wrong pixels, never a stray read. */
#define UWU_FILTER_BILINEAR 0 /* support 1 */
#define UWU_FILTER_BICUBIC 1  /* support 2, a = -0.5 */
#define UWU_FILTER_LANCZOS 2  /* support 3 */
int uwu_resample_ksize(int in_size, int out_size, int filter);
int uwu_resample_coeffs(int in_size, int out_size, int filter, int first, int count, int32_t* coeffs, int32_t* bounds);
size_t uwu_image_resize_crop_ws_bytes(int B, const int32_t* meta, int Ht, int Wt, int filter);
int uwu_image_resize_crop(const void* src, int64_t src_bytes, const int64_t* src_off, const int32_t* meta, const int32_t* tables,
                          int64_t tables_len, const int64_t* tab_off, void* out, int dtype, int B, int Ht, int Wt, int filter,
                          int normalize, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ optimizer (a15) */

/* Roundings.  Every update rule below is one function of one element (csrc/optimizer_shared.h and the optimizer*.hip files), with
 * each fused multiply-add and each separately rounded product written out and compiler contraction off.  An element's result
 * therefore does not depend on where it sits in a launch (16-byte vector body, scalar head or tail, ragged 8-bit block), nor on
 * n, the chunking or the grid.  fma(a, b, c) below is one rounding of a*b + c; every other operation rounds by itself:
 *   AdamW       gs = gscale*g ; m = fma(1-beta1, fma(gscale, g, -m), m) ; v = fma(beta2, v, gs*((1-beta2)*gs))
 *               p = fma(1 - lr*wd, p, -(lr/bc1) * (m / fma(1/sqrt(bc2), sqrt(v), eps)))         (8-bit AdamW: the same function)
 *   Lion        c = fma(beta1, m, (1-beta1)*g) ; p = fma(1 - lr*wd, p, -(lr*sign(c))) ; m = fma(beta2, m, (1-beta2)*g)
 *   AdamWFP16   m = fma(1-beta1, g, beta1*float(m16)) ; v = fma(beta2, float(v16), g*((1-beta2)*g))
 *               p = fma(-step_size, m / (sqrt(v) + eps), p) ; m16 = half(m), v16 = half(v) of the fp32-rounded values
 *   Prodigy     in double: g = fma(gscale, g, wd*p) ; sum += fma(p0 - p, g, .) ; exp_avg = fma(beta1, exp_avg, (d(1-beta1))*g) ;
 *               exp_avg_sq = fma(beta2, exp_avg_sq, g*((d d (1-beta2))*g)) ; s = fma(beta3, s, cs*g) ; each stored as fp32 ;
 *               in fp32: p = fma(p, 1 - wd*dlr, -(dlr * (exp_avg / (sqrt(exp_avg_sq) + d*eps))))
 *   average     avg = fma(keep, avg, take*p) ; schedule-free AdamW: at uwu_sfadamw_step
 * g in Lion, AdamWFP16 and schedule-free AdamW is the rounded product of the gradient and gscale = pre_scale * clip[1].
 * 1 - lr*wd is fma(-lr, wd, 1) in fp32 on the device for uwu_adamw_step and a double difference on the host elsewhere. */

/* Global L2 norm of a flat fp32 buffer (Lightning gradient_clip_val, demo_training.yaml:12):
 * out[0] = sum(g^2) * pre_scale^2 ; out[1] = clip coefficient min(1, max_norm/(sqrt(out[0])+1e-6))
 * (max_norm <= 0 -> 1).  partial: workspace of >= 1024 floats. */
int uwu_grad_sqnorm_clip(const float* g, int64_t n, float pre_scale, float max_norm, float* partial,
                         float* out, void* stream);

/* torch.optim.AdamW single-tensor semantics (trainer.py:52-74, demo_training_latent.yaml:30-39) on flat
 * buffers; g_eff = g * pre_scale * clip[1] (clip may be NULL).  Also refreshes the bf16 shadow
 * (may be NULL).  step is the 1-based step count. */
int uwu_adamw_step(float* p, float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, float pre_scale,
                   const float* clip, int zero_grad, void* stream);

/* lion_pytorch.Lion (the commented alternative of demo_training.yaml:48, demo_training_latent.yaml:31 and
 * demo_training_lycoris.yaml:49; Chen et al. 2023, Algorithm 2) on flat buffers, in the package's order:
 *   p *= 1 - lr*wd ; c = beta1*m + (1-beta1)*g ; p -= lr*sign(c), sign(0) = 0 ; m = beta2*m + (1-beta2)*g
 * m is fp32.  g = g * pre_scale * clip[1] (clip may be NULL); p_bf16 (may be NULL) is refreshed; zero_grad leaves g
 * zeroed.  p, g, m 16-byte aligned, p_bf16 8-byte aligned.  The hyper-parameters are doubles: 1 - beta and 1 - lr*wd are
 * formed in double on the host as python does (1 - 0.999f is off by 1.3e-5 relative). */
int uwu_lion_step(float* p, float* g, float* m, void* p_bf16, int64_t n, double lr, double beta1, double beta2,
                  double weight_decay, float pre_scale, const float* clip, int zero_grad, void* stream);

/* duwu.trainer.optimizers.AdamWFP16 (optimizers.py:96-120 as called from :78-92): AdamW with both moments in fp16
 * (m16, v16: IEEE half), no first-moment bias correction, no weight decay (see uwu_param_decay):
 *   m = float(m16)*beta1 + (1-beta1)*g ; v = float(v16)*beta2 + (1-beta2)*g*g
 *   p -= lr*sqrt(1-beta2^step) * m / (sqrt(v) + eps)       (the unrounded fp32 m and v)
 *   m16 = half(m) ; v16 = half(v)    round to nearest even, subnormals kept, overflow -> inf; nothing is clamped
 * g, p_bf16, zero_grad, step as in uwu_adamw_step.  p, g 16-byte aligned; m16, v16, p_bf16 8-byte aligned, m16 and v16
 * at the same offset within 16 bytes (chunk offsets are multiples of 4 elements). */
int uwu_adamw_fp16_step(float* p, float* g, void* m16, void* v16, void* p_bf16, int64_t n, double lr, double beta1,
                        double beta2, double eps, int step, float pre_scale, const float* clip, int zero_grad,
                        void* stream);

/* p *= factor over n elements, p_bf16 (may be NULL) refreshed: AdamWFP16's accumulated weight decay of one tensor,
 * `p.add_(p, alpha=-decay_this_iteration)` (optimizers.py:117-118) with factor = 1 - decay_this_iteration.  Any
 * element alignment. */
int uwu_param_decay(float* p, void* p_bf16, int64_t n, double factor, void* stream);

/* AdamW with 8-bit block-wise moments: the state layout of bitsandbytes.optim.AdamW8bit (Dettmers et al. 2022, "8-bit Optimizers
 * via Block-wise Quantization") on flat buffers.  The package is not a dependency: the rule is restated here.
 *
 * State: state1 / state2 hold one uint8 code per element, absmax1 / absmax2 one fp32 scale per block, qmap1 / qmap2 the code
 * tables: 256 fp32 values each, strictly increasing, within [-1, 1] (the package's signed / unsigned dynamic maps; the kernel
 * assumes nothing else about them).  Block b covers elements [256 b, 256 b + 256) counted from the buffer's start; the last
 * block may be partial.  All pointers are the buffers' BASE pointers; the launch updates the element range [e0, e1) of the n
 * elements, e0 a multiple of 256, e1 a multiple of 256 or equal to n.  Per block, in one pass:
 *   m = qmap1[state1] * absmax1[b] ; v = qmap2[state2] * absmax2[b]
 *   g = g * pre_scale * clip[1]                            (clip may be NULL; the fp32 factor of uwu_adamw_step)
 *   p *= 1 - lr*wd ; m = m + (g - m) * (1-beta1) ; v = beta2*v + (1-beta2)*g*g
 *   p -= lr/(1-beta1^step) * m / (sqrt(v)/sqrt(1-beta2^step) + eps)        (the unrounded fp32 m and v)
 *   absmax1[b] = max |m| ; absmax2[b] = max v               over the block's elements inside the buffer
 *   state1 = the index of the entry of qmap1 nearest to m / absmax1[b], a tie to the lower index; state2 likewise
 *   a block whose new absmax is 0 gets the code of the entry nearest to 0 (127 / 0 in the package's maps) and absmax 0
 * p_bf16 (may be NULL) is refreshed, zero_grad leaves g zeroed, step is the 1-based step count.  The hyper-parameters are
 * doubles: 1 - beta, 1 - lr*wd and the bias corrections are formed in double on the host (see uwu_lion_step).
 * Not reproduced from the package: it applies the weight decay after the update (O(lr^2 wd) per step apart) and moves a first-
 * moment code whose sign differs from the value's to its neighbour after quantising.
 * No atomics, and a block's result does not depend on the grid or on the range it was launched in: the same inputs give the
 * same bits.  p, g 16-byte aligned; codes, absmax and tables 4-byte aligned; p_bf16 8-byte aligned.
 * 10 B read + 6 B written per parameter (+ 2 B for the shadow, + 4 B for the zeroed gradient). */
int uwu_adamw8_step(float* p, float* g, void* state1, void* state2, float* absmax1, float* absmax2, const float* qmap1,
                    const float* qmap2, void* p_bf16, int64_t n, int64_t e0, int64_t e1, double lr, double beta1, double beta2,
                    double eps, double weight_decay, int step, float pre_scale, const float* clip, int zero_grad, void* stream);

/* Lion with an 8-bit block-wise moment (bitsandbytes.optim.Lion8bit's state layout): the step of uwu_lion_step with
 * m = qmap1[state1] * absmax1[b] before it and absmax1[b] = max |m|, state1 = nearest entry of m / absmax1[b] after it.  Blocks,
 * base pointers, the range [e0, e1), alignment and determinism as in uwu_adamw8_step. */
int uwu_lion8_step(float* p, float* g, void* state1, float* absmax1, const float* qmap1, void* p_bf16, int64_t n, int64_t e0,
                   int64_t e1, double lr, double beta1, double beta2, double weight_decay, float pre_scale, const float* clip,
                   int zero_grad, void* stream);

/* prodigyopt.Prodigy (Mishchenko & Defazio, "Prodigy: An Expeditiously Adaptive Parameter-Free Learner") on flat buffers: a
 * step is uwu_prodigy_stats per chunk, then uwu_prodigy_finalize, then uwu_prodigy_apply, all on one stream, nothing read back.
 * With g = g * pre_scale * clip[1] (clip may be NULL; the fp32 factor of uwu_adamw_step), the package's step is
 *   beta3 = beta3 or sqrt(beta2) ; bc = sqrt(1 - beta2^(k+1)) / (1 - beta1^(k+1)) if use_bias_correction else 1
 *   dlr   = d * lr * bc                                                        (the OLD d)
 *   if weight_decay != 0 and not decouple:  g += weight_decay * p
 *   d_numerator = beta3 * d_numerator + (d/d0) * dlr * sum_i g_i (p0_i - p_i)
 *   exp_avg     = beta1 * exp_avg    + d * (1-beta1) * g
 *   exp_avg_sq  = beta2 * exp_avg_sq + d*d * (1-beta2) * g*g
 *   s           = beta3 * s + (d/d0) * (d if safeguard_warmup else dlr) * g
 *   d_denom     = sum_i |s_i|
 *   if d_denom == 0:  return              (p, the shadow and k keep their values)
 *   d_hat = d_coef * d_numerator / d_denom ; if d == d0: d = max(d, d_hat)
 *   d_max = max(d_max, d_hat) ; d = min(d_max, d * growth_rate)
 *   if weight_decay != 0 and decouple:  p *= 1 - weight_decay * dlr
 *   p -= dlr * exp_avg / (sqrt(exp_avg_sq) + d * eps)                          (the OLD dlr, the NEW d)
 *   k += 1
 * lr == 0 skips the moments, s and both sums as the package does (d_numerator still decays; d_denom is 0: the early return).
 *
 * scalars: UWU_PRODIGY_SCALARS doubles on the device, 8-byte aligned, in the order of the UWU_PRODIGY_* indices; a fresh block
 * is {d0, d0, 0, 0, 0, 0, 0, 0}.  beta3 is passed resolved (never 0 for "None").  The hyper-parameters are doubles: 1 - beta is
 * formed in double on the host (see uwu_lion_step), and everything derived from d on the device in double. */
#define UWU_PRODIGY_SCALARS 8
#define UWU_PRODIGY_D 0           /* the step size estimate */
#define UWU_PRODIGY_D_MAX 1
#define UWU_PRODIGY_D_NUMERATOR 2
#define UWU_PRODIGY_D_DENOM 3     /* of the last step */
#define UWU_PRODIGY_D_HAT 4       /* of the last step that did not return early */
#define UWU_PRODIGY_K 5           /* steps taken (early returns not counted) */
#define UWU_PRODIGY_SKIPPED 6     /* 1 when the last step returned early (d_denom == 0), else 0 */
#define UWU_PRODIGY_DLR 7         /* the last step's dlr (its OLD d): what uwu_prodigy_apply moves p by */

/* Workgroups (= workspace slots) uwu_prodigy_stats uses for n elements: a function of n alone.  0 for n <= 0. */
int uwu_prodigy_stats_blocks(int64_t n);

/* The statistics pass over one chunk of n elements: updates exp_avg, exp_avg_sq and s in place from the block's d and k, leaves
 * g zeroed when zero_grad, and writes one partial of sum g (p0 - p) and one of sum |s| per workgroup to
 * ws[2 * (slot0 + b)], ws[2 * (slot0 + b) + 1], b < uwu_prodigy_stats_blocks(n): slots of their own, no atomics.  Products,
 * p0 - p and the sums are formed in double; each stored moment is rounded to fp32 once.  p and p0 are only read.  ws holds
 * 2 * ws_slots doubles; slot0 + blocks > ws_slots is refused.  The six buffers 16-byte aligned, scalars and ws 8-byte aligned,
 * n > 0.  24 B read + 12 B written per parameter (+ 4 B for the zeroed gradient). */
int uwu_prodigy_stats(const float* p, float* g, const float* p0, float* exp_avg, float* exp_avg_sq, float* s, int64_t n,
                      const double* scalars, double* ws, int64_t ws_slots, int64_t slot0, double lr, double beta1, double beta2,
                      double beta3, double weight_decay, int decouple, double d0, int use_bias_correction, int safeguard_warmup,
                      float pre_scale, const float* clip, int zero_grad, void* stream);

/* One workgroup: adds the partials of slots [0, nslots) in slot order in double (bit-identical run to run at a fixed chunking)
 * and applies the scalar recurrence above to the block: d_numerator, d_denom, dlr always; d, d_max, d_hat, k and skipped = 0
 * unless d_denom == 0 (then skipped = 1 and nothing else).  One thread writes.  lr, betas and use_bias_correction as given to
 * uwu_prodigy_stats in this step. */
int uwu_prodigy_finalize(double* scalars, const double* ws, int64_t nslots, double lr, double beta1, double beta2, double beta3,
                         double d0, double d_coef, double growth_rate, int use_bias_correction, void* stream);

/* The update over the whole buffer, from the block uwu_prodigy_finalize left: the decoupled decay and
 * p -= dlr * exp_avg / (sqrt(exp_avg_sq) + d * eps) in fp32 (dlr, d * eps and 1 - weight_decay * dlr rounded once from double),
 * p_bf16 (may be NULL) refreshed as uwu_cast_f32_to_bf16 rounds.  Does nothing at all when skipped is set.  p, exp_avg,
 * exp_avg_sq 16-byte aligned, p_bf16 8-byte aligned, n > 0.  12 B read + 4 B written per parameter (+ 2 B for the shadow). */
int uwu_prodigy_apply(float* p, const float* exp_avg, const float* exp_avg_sq, void* p_bf16, int64_t n, const double* scalars,
                      double eps, double weight_decay, int decouple, void* stream);

/* transformers.optimization.Adafactor (Shazeer & Stern, "Adafactor: Adaptive Learning Rates with Sublinear Memory Cost") on flat
 * buffers.  The rule is per tensor: the flat buffer's tensors are described by a table, and a step is, per set of tensors whose
 * gradient is complete, uwu_adafactor_stats, then uwu_adafactor_norm, then uwu_adafactor_apply on one stream: four kernel launches
 * whatever the number of tensors, nothing read back, no atomics.  With g = g * pre_scale * clip[1] (clip may be NULL; the fp32
 * factor of uwu_adamw_step), step t (1-based) and the host's doubles
 *   beta2t = 1 - t^decay_rate ; lr_t = lr, or with relative_step min(warmup_init ? 1e-6 t : 1e-2, 1/sqrt(t))
 * the package's step of one tensor W, seen as [R, C] = [shape[0], prod(shape[1:])] when it has two or more dimensions, is
 *   U = g^2 + eps0
 *   factored:    row[i] = beta2t row[i] + (1 - beta2t) mean_j U[i,j] ; col[j] = beta2t col[j] + (1 - beta2t) mean_i U[i,j]
 *                u[i,j] = (rsqrt(row[i] / mean_i row[i]) * rsqrt(col[j])) * g[i,j]
 *   unfactored:  v = beta2t v + (1 - beta2t) U ; u = rsqrt(v) * g
 *   u /= max(1, RMS(u) / clip_threshold) ; u *= alpha      RMS(x) = ||x||_2 / sqrt(numel)
 *                                                          alpha = lr_t * (scale_parameter ? max(eps1, RMS(W)) : 1)
 *   beta1 given: m = beta1 m + (1 - beta1) u ; u = m
 *   W -= weight_decay * alpha * W ; W -= u
 * row * col is never formed (a tensor without gradient has both near eps0 = 1e-30: the product underflows fp32).
 *
 * Table: UWU_ADAFACTOR_FIELDS int64 per tensor, the same on the host (table_host) and on the device (table):
 *   0 offset in the flat buffer (a multiple of 4 elements)    1 R (0: a 1-D tensor)    2 C (1-D: the length)
 *   3 offset of row[R] in `row`    4 offset of col[C] in `col`    5 offset of v[C] in `v` (1-D only)
 *   6 offset of uwu_adafactor_ws_floats(R, C) floats in `fws`     7 offset of uwu_adafactor_ws_doubles(R, C) doubles in `dws`
 * Rows ascend: every range of row i + 1 (flat buffer, state, workspaces) starts at or behind the end of row i's.  R * C < 2^31.
 * Launch list (launch_host, and the same words on the device: launch): 3 * nready + 2 int64 --
 *   [0, nready)                 the tensors to update, as ascending table indices
 *   [nready, 2 nready + 1)      prefix sums of uwu_adafactor_tiles(R, C) over them (workgroup starts; the total last)
 *   [2 nready + 1, 3 nready + 2)  prefix sums of uwu_adafactor_moment_blocks(R, C) likewise
 * Every entry point checks the listed rows on the host copies before it launches anything: ranges inside the buffers whose lengths
 * the descriptor gives, offsets that are multiples of 4, R * C < 2^31, no overlap, consistent starts.  Nothing outside the listed
 * tensors is read or written: the gaps between tensors (padding) are never touched.
 * Determinism: workgroup b serves tile b - start[s] of the s-th listed tensor, the tiling and the order of every sum are functions
 * of (R, C) alone, and per-tensor sums are double partials (one per workgroup) that each consumer adds in a fixed order: a
 * tensor's result is bit-identical whichever launch it was part of. */
#define UWU_ADAFACTOR_FIELDS 8
typedef struct {
  float* p;              /* the flat parameters, n elements, 16-byte aligned */
  float* g;              /* their gradient, n elements, 16-byte aligned */
  void* p_bf16;          /* the bf16 shadow of p (n elements, 8-byte aligned) or NULL */
  float* row;            /* exp_avg_sq_row of all factored tensors, n_row floats */
  float* col;            /* exp_avg_sq_col likewise, n_col floats */
  float* v;              /* exp_avg_sq of all 1-D tensors, n_v floats */
  float* m;              /* exp_avg (beta1), n elements laid out as p, 16-byte aligned; NULL without beta1 */
  float* rms;            /* RMS(W) per tensor as of its last step with scale_parameter, ntensors floats */
  float* fws;            /* workspace: tile partials of the row and column sums, n_fws floats */
  double* dws;           /* workspace: per-workgroup partials of sum W^2, sum u^2 and sum row, n_dws doubles */
  const int64_t* table_host;
  const int64_t* table;  /* the device copy */
  int32_t ntensors;
  int64_t n, n_row, n_col, n_v, n_fws, n_dws;
} UwuAdafactorDesc;

/* Functions of the shape alone (R = 0: 1-D of length C): workgroups of the tile passes, workgroups of the moments pass (0 for a
 * 1-D tensor), workspace floats and doubles.  0 for R < 0 or C < 1. */
int64_t uwu_adafactor_tiles(int64_t R, int64_t C);
int64_t uwu_adafactor_moment_blocks(int64_t R, int64_t C);
int64_t uwu_adafactor_ws_floats(int64_t R, int64_t C);
int64_t uwu_adafactor_ws_doubles(int64_t R, int64_t C);

/* Pass 1, two launches.  Per tile: partial row and column sums of U = g^2 + eps0 into fws (1-D: v = fma(beta2t, v, (1-beta2t) U)
 * directly) and, when scale_parameter, a partial of sum W^2 in double.  Then one thread per row and per column: the tile partials
 * added in tile order, mean = sum / count, moment = fma(beta2t, moment, (1-beta2t) mean), and one double partial of sum_i row[i]
 * per workgroup.  p and g are only read.  beta2t in [0, 1), eps0 >= 0.  8 B read per parameter with scale_parameter, else 4. */
int uwu_adafactor_stats(const UwuAdafactorDesc* d, const int64_t* launch_host, const int64_t* launch, int nready, double beta2t,
                        double eps0, int scale_parameter, float pre_scale, const float* clip, void* stream);

/* Pass 2: per tile a double partial of sum u^2, u before the clip from the finished moments of the whole tensor and mean(row)
 * (the partials of pass 1 in order).  g is only read.  4 B read per parameter. */
int uwu_adafactor_norm(const UwuAdafactorDesc* d, const int64_t* launch_host, const int64_t* launch, int nready, float pre_scale,
                       const float* clip, void* stream);

/* Pass 3: u again (the same expression: the same bits), u = (u / max(1, RMS(u) / clip_threshold)) * alpha, with use_beta1
 * m = fma(beta1, m, (1-beta1) u) and u = m, W = fma(-(weight_decay alpha), W, W) when that factor is not 0, W -= u; p_bf16
 * refreshed as uwu_cast_f32_to_bf16 rounds, g zeroed when zero_grad, rms[tensor] = RMS(W) (before the update) when
 * scale_parameter.  A NaN sum keeps its NaN through both max().  clip_threshold > 0, beta1 in [0, 1) (ignored without
 * use_beta1), d->m given with use_beta1.  8 B read + 4 B written per parameter (+ 8 for m, + 2 for the shadow, + 4 for the zeroed
 * gradient). */
int uwu_adafactor_apply(const UwuAdafactorDesc* d, const int64_t* launch_host, const int64_t* launch, int nready, double lr_t,
                        double eps1, double clip_threshold, int scale_parameter, int use_beta1, double beta1, double weight_decay,
                        float pre_scale, const float* clip, int zero_grad, void* stream);

/* Weight averaging on flat buffers (torch.optim.swa_utils.AveragedModel as lightning.pytorch.callbacks.WeightAveraging /
 * EMAWeightAveraging drive it; uwudiff_amd/averaging.py):
 *   avg[i] = fma(keep, avg[i], take * p[i])      fp32: two roundings per element, 8 B read and 4 B written per parameter
 * keep and take are formed in double on the host and rounded once (an EMA: keep = decay, take = 1 - decay; 1 - 0.999f is off
 * by 1.3e-5 relative; the running mean after n updates: keep = n / (n + 1), take = 1 / (n + 1)).  avg and p 16-byte aligned,
 * n > 0.  p is only read. */
int uwu_ema_update(float* avg, const float* p, int64_t n, float keep, float take, void* stream);

/* The average put in place of the weights, no pointer moved, one pass, no third buffer:
 *   mode 0:  avg[i] <-> p[i]      bit for bit (NaN payloads, -0.0 and subnormals survive: the words travel as integers)
 *   mode 1:  p[i] = avg[i]        avg is only read
 * and p_bf16[i] (may be NULL) = the bf16 rounding of the new p[i], as uwu_cast_f32_to_bf16 rounds.  Mode 0 is its own inverse.
 * avg and p 16-byte aligned, p_bf16 8-byte aligned, n > 0; avg == p and overlapping [avg, avg + n) / [p, p + n) are refused. */
int uwu_ema_swap(float* avg, float* p, void* p_bf16, int64_t n, int mode, void* stream);

/* schedulefree.AdamWScheduleFree (Defazio et al., "The Road Less Scheduled"; AdamWScheduleFree.step, single-tensor path, package
 * 1.4) on flat buffers.  The package is not a dependency: the rule is restated here.  y is the parameter as training holds it (the
 * gradient is taken there), z the base iterate, v the second moment.  Per step the host advances, as python floats (doubles):
 *   sched = (k+1)/warmup_steps if k < warmup_steps else 1 ; bc2 = 1 - beta2^(k+1) ; lr_t = lr * sched
 *   lr_max = max(lr_t, lr_max) ; weight = (k+1)^r * lr_max^weight_lr_power ; weight_sum += weight
 *   c = weight / weight_sum   (0 when weight_sum == 0)
 * and the launch does, per element, with g = g * pre_scale * clip[1] (clip may be NULL; the fp32 factor of uwu_adamw_step):
 *   v  = beta2*v + (1-beta2)*g*g
 *   gn = g / (sqrt(v / bc2) + eps) + weight_decay*y                       (y BEFORE the interpolation below)
 *   y  = lerp(y, z, c)      torch.lerp: y + c*(z - y) for c < 0.5, else z - (z - y)*(1 - c): at c = 1 (the first step) exactly z
 *   y  = y + lr_t*(beta1*(1-c) - 1) * gn
 *   z  = z - lr_t*gn
 * lr_t*(beta1*(1-c) - 1), 1/bc2, 1 - beta2 and 1 - c are formed in double on the host and rounded to fp32 once; the arithmetic
 * per element is fp32 with every multiply-add fused by hand, so a result does not depend on the grid or on the chunk it was
 * launched in.  p_bf16 (may be NULL) receives the new y as uwu_cast_f32_to_bf16 rounds, zero_grad leaves g zeroed.  c in [0, 1],
 * bc2 in (0, 1], n > 0; y, g, z, v 16-byte aligned, p_bf16 8-byte aligned.  16 B read + 12 B written per parameter (+ 2 B for
 * the shadow, + 4 B for the zeroed gradient): the traffic of uwu_adamw_step. */
int uwu_sfadamw_step(float* y, float* g, float* z, float* v, void* p_bf16, int64_t n, double lr_t, double beta1, double beta2,
                     double eps, double weight_decay, double c, double bc2, float pre_scale, const float* clip, int zero_grad,
                     void* stream);

/* out[i] = lerp(y[i], z[i], weight), torch.lerp's two branches as above, out of place: the weights to evaluate under the
 * schedule-free rule are x = lerp(y, z, 1 - 1/beta1).  weight and 1 - weight are rounded to fp32 once from double.  y and z are
 * only read; out must not partly overlap them.  All three 16-byte aligned, n > 0.  8 B read + 4 B written per parameter. */
int uwu_sf_average(const float* y, const float* z, float* out, int64_t n, double weight, void* stream);

int uwu_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int uwu_cast_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream);

/* ------------------------------------------------------------------ LyCORIS adapters
 * Segment table of uwu_adapter_merge: one row of 13 int64 per adapted tensor [rows, cols] (a norm vector: rows = 1):
 *   kind, rows, cols, base_off, eff_off, shadow_off, pa, pb, pc, r, out_k, in_n, scale (fp32 bits in the low word)
 * offsets in elements (base / eff / shadow: multiples of 64; eff_off / shadow_off < 0: no such output);
 * pa / pb / pc index the adapter parameter buffer p:
 *   UWU_ADAPTER_NORM           delta[e]   = p[pa + e]
 *   UWU_ADAPTER_LORA           delta[i,j] = scale * sum_t up[i,t] down[t,j]            up = p+pa [rows, r], down = p+pb [r, cols]
 *   UWU_ADAPTER_LOKR           delta      = scale * kron(w1, w2)                       w1 = p+pa [rows/out_k, cols/in_n], w2 = p+pb [out_k, in_n]
 *   UWU_ADAPTER_LOKR_LOWRANK   as LOKR with w2 = w2_a w2_b                             w2_a = p+pb [out_k, r], w2_b = p+pc [r, in_n]
 * uwu_adapter_merge writes W_eff = base + delta to eff (fp32) and / or shadow (bf16, rounded as uwu_cast_f32_to_bf16) in
 * one launch of nblocks workgroups; blk_start [nseg + 1] = exclusive prefix sum of ceil(rows * cols / 4096) per row.
 * r <= 128.  eff may alias base (merging into the base weights in place). */
#define UWU_ADAPTER_NORM 0
#define UWU_ADAPTER_LORA 1
#define UWU_ADAPTER_LOKR 2
#define UWU_ADAPTER_LOKR_LOWRANK 3
int uwu_adapter_merge(const float* base, const float* p, const int64_t* table, const int64_t* blk_start, int nseg,
                      int64_t nblocks, float* eff, void* shadow, void* stream);
/* Adapter gradient of one adapted [N, K] weight from its fp32 weight gradient dw (row-major, overwritten form), ACCUMULATED
 * into g (same offsets pa / pb / pc as in p); kinds LORA, LOKR, LOKR_LOWRANK as above.  Deterministic: dw is read once,
 * workgroup partials go to ws and are summed in a fixed order (no float atomics).  ws_elems: floats of ws --
 *   LORA:  ceil(K/256) N r + ceil(N/32) r K
 *   LOKR*: out_l ceil(out_k in_n / 2048) in_m + out_l out_k in_n + 2 out_k in_n   (out_l = N/out_k, in_m = K/in_n) */
int uwu_adapter_grad(const float* dw, int64_t N, int64_t K, int kind, const float* p, float* g, int64_t pa, int64_t pb,
                     int64_t pc, int r, int out_k, int in_n, float scale, float* ws, int64_t ws_elems, void* stream);
/* Weight decomposition (DoRA): W' = m V / n with V = base + delta (delta as above), one magnitude m
 * and one norm n = ||V||_2 + 2^-23 per row (orient 1, wd_on_out) or per column (orient 0) of an adapted [rows, cols] Linear.
 * Segment table: one row of 16 int64 per decomposed tensor -- the 13 fields of uwu_adapter_merge, then
 *   dora_off (m in p: rows or cols floats), norm_off (n in norms: as many floats), orient
 * `table` is the device copy the kernels read, `table_host` the same rows in host memory: every row is checked (kind LORA /
 * LOKR / LOKR_LOWRANK, r in [1, 128], base / eff / shadow offsets multiples of 64, nblocks) before anything is launched.
 * uwu_adapter_dora_norms writes n of every segment in one launch; the sum of squares is added in double in an order fixed
 * by the shape (no float atomics).  blk_start [nseg + 1] = exclusive prefix sum of ceil(rows / 4) (orient 1) or
 * ceil(cols / 64) (orient 0) per row.
 * uwu_adapter_dora_merge writes W' to eff and / or shadow with the conventions of uwu_adapter_merge (blk_start as there:
 * ceil(rows * cols / 4096)); it reads the norms the previous launch wrote.  eff may alias base. */
int uwu_adapter_dora_norms(const float* base, const float* p, const int64_t* table, const int64_t* table_host,
                           const int64_t* blk_start, int nseg, int64_t nblocks, float* norms, void* stream);
int uwu_adapter_dora_merge(const float* base, const float* p, const int64_t* table, const int64_t* table_host,
                           const int64_t* blk_start, int nseg, int64_t nblocks, const float* norms, float* eff, void* shadow,
                           void* stream);
/* The stage in front of uwu_adapter_grad for a decomposed [N, K] weight.  dw holds dL/dW' on entry and dL/dV on return (in
 * place); dL/dm is ACCUMULATED into g at dora_off.  With t = <dw, V> over a row (wd_on_out != 0) or a column, u = ||V||:
 *   dm = t / n,  dV = m / n (dw - V t / (n u))   (the second term 0 where u = 0)
 * base: this weight's frozen fp32 values, norms: its n (both already offset); V is recomputed from base and p, and u^2 is
 * summed next to t (the bracket is evaluated in double as (dw - V t / u^2) + V t / u^2 eps / n: it cancels where one element
 * carries the row or column).  dw and base are 16-byte aligned where K is a multiple of 4.  Deterministic: fixed-order sums;
 * per column they go through ws (8-byte aligned).  ws_elems: floats of ws -- 0 (wd_on_out) or 4 ceil(N / 256) K. */
int uwu_adapter_dora_grad(float* dw, const float* base, int64_t N, int64_t K, int kind, const float* p, float* g, int64_t pa,
                          int64_t pb, int64_t pc, int r, int out_k, int in_n, float scale, int64_t dora_off,
                          const float* norms, int wd_on_out, float* ws, int64_t ws_elems, void* stream);
/* Convolution adapters on a 3x3 convolution weight stored [cout_store, 9, cin_store] (tap-major,
 * channel-contiguous; rows >= cout and channels >= cin are padding: they hold zeros, get delta 0 and no gradient).  The
 * adapter tensors are stored tap-major too, in the TRUE sizes (no padding), scale as above:
 *   UWU_ADAPTER_CONV_LORA           delta[o,t,c] = scale sum_i up[o,i] down[i,t,c]     up = p+pa [cout, r], down = p+pb [r, 9, cin]
 *   UWU_ADAPTER_CONV_TUCKER         as CONV_LORA with down := T,  T[i,t,c] = sum_j mid[i,t,j] dn[j,c]
 *                                                                 up = p+pa [cout, r], dn = p+pb [r, cin], mid = p+pc [r, 9, r]
 *   UWU_ADAPTER_CONV_LOKR           delta[a out_k + k, t, b in_n + l] = scale w1[a,b] w2[k,t,l]
 *                                                                 w1 = p+pa [cout/out_k, cin/in_n], w2 = p+pb [out_k, 9, in_n]
 *   UWU_ADAPTER_CONV_LOKR_LOWRANK   as CONV_LOKR with w2 = w2_a w2_b                   w2_a = p+pb [out_k, r], w2_b = p+pc [r, 9, in_n]
 * Segment table of uwu_adapter_conv_merge: one row of 17 int64 per convolution -- the 13 fields of uwu_adapter_merge
 * (rows = cout_store, cols = 9 cin_store), then cout, cin, cin_store, t_off (CONV_TUCKER: where T [r, 9, cin] of this
 * segment lives in tws).  `table_host` is the same table in host memory: every row is checked before anything is launched.
 * Two launches for all segments: T of every CONV_TUCKER segment into tws (nform workgroups; form_start [nseg + 1] = exclusive
 * prefix sum of ceil(9 r cin / 256) for CONV_TUCKER rows, 0 for the others; nform = 0: no such launch), then W_eff = base +
 * delta into eff / shadow as uwu_adapter_merge does (blk_start: ceil(rows * cols / 4096)).  eff may alias base. */
#define UWU_ADAPTER_CONV_LORA 4
#define UWU_ADAPTER_CONV_TUCKER 5
#define UWU_ADAPTER_CONV_LOKR 6
#define UWU_ADAPTER_CONV_LOKR_LOWRANK 7
int uwu_adapter_conv_merge(const float* base, const float* p, const int64_t* table, const int64_t* table_host,
                           const int64_t* blk_start, const int64_t* form_start, int nseg, int64_t nblocks, int64_t nform,
                           float* tws, int64_t tws_elems, float* eff, void* shadow, void* stream);
/* Adapter gradient of one adapted convolution from its fp32 weight gradient dw [cout_store, 9 cin_store], ACCUMULATED into
 * g (offsets pa / pb / pc as in p).  dw is read once; partials go to ws and are added in a fixed order (no float atomics).
 * CONV_TUCKER: T is formed in ws, d_up and dT come from the LoRA-shaped pass, one chain launch adds d_mid and d_dn.
 * ws_elems, with K = 9 cin, W2 = 9 out_k in_n, out_l = cout / out_k, in_m = cin / in_n:
 *   CONV_LORA:    ceil(K/256) cout r + ceil(cout/32) r K          CONV_TUCKER: that + 2 r K
 *   CONV_LOKR*:   out_l ceil(W2 / 2048) in_m + out_l W2 + 2 W2 */
int uwu_adapter_conv_grad(const float* dw, int64_t cout_store, int64_t cin_store, int64_t cout, int64_t cin, int kind,
                          const float* p, float* g, int64_t pa, int64_t pb, int64_t pc, int r, int out_k, int in_n,
                          float scale, float* ws, int64_t ws_elems, void* stream);

/* ------------------------------------------------------------------ gradient exchange (section 8e)
 * One RCCL communicator per rank (librccl resolved at run time), created once; uwu_allreduce_flat sums a slice of the
 * flat fp32 gradient buffer over the ranks in place on the caller's stream (reference: the bucketed all-reduce of
 * Lightning DDP, configs/demo_training.yaml:5-7).  uwu_comm_unique_id: 128 bytes made by rank 0, to be handed to every
 * rank through any side channel; uwu_comm_init is collective.  The 1/world average stays folded into the optimizer
 * kernels (pre_scale).  uwudiff_amd/gradsync.py uses it when UWU_RCCL_DIRECT=1 (default: torch.distributed's RCCL
 * process group, which needs no second communicator). */
int uwu_comm_unique_id(void* id128);
int uwu_comm_init(const void* id128, int rank, int world, void** comm);
int uwu_allreduce_flat(void* comm, float* buf, int64_t n, void* stream);
int uwu_comm_destroy(void* comm);

/* ------------------------------------------------------------------ dense contractions (a11-a13) */

/* C[M,N] = opA(A) . opB(B)  (+ epilogue), fp32 accumulate on MFMA.
 *   transA=0: A is [M,K] row-major (lda);  transA=1: A is [K,M] row-major (lda).
 *   transB=0: B is [N,K] row-major (ldb) -- torch Linear weight layout; transB=1: B is [K,N] (ldb).
 *   dtype: operand storage (UWU_F32 -> v_mfma_f32_16x16x4_f32, UWU_BF16 -> v_mfma_f32_16x16x32_bf16).
 *   c_dtype: storage of C / C2 (bf16 or fp32).  bias fp32[N].  aux: [M,N] operand-dtype tensor (ldaux).
 *   split_k > 1 requires UWU_EPI_ACCUM with fp32 C (atomic accumulation).
 * Replaces nn.Linear forward / dgrad / wgrad inside the denoiser (rope_unet.py:122-166). */
int uwu_gemm(const void* A, const void* B, void* C, void* C2, const float* bias, const void* aux,
             int M, int N, int K, int lda, int ldb, int ldc, int ldaux, int transA, int transB, int dtype,
             int c_dtype, int epilogue, int split_k, void* stream);
/* Name of the kernel family that the most recent GEMM launch of this process went to ("" before the first): "gemm" (128x128),
 * "gemm_r3_256" / "gemm_r3_128" (ring, 256x128 / 128x128 tiles), "gemm_big" (256x256), "gemm_wide" (192x384), "gemm_m64"
 * (64x128), "gemm_as" (A-stationary), "gemm_p8" / "gemm_p8n" (8-phase 256x256 / 128x384), the fp8 kernels "gemm_f8" /
 * "gemm_f8(emit)" / "gemm_f8(split-K)" (two-stage) and "gemm_p8f" / "gemm_p8f(split-K)" (8-phase), and the weight-gradient
 * families' own names.  A static string; for tests that must know which kernel a dispatch rule chose. */
const char* uwu_gemm_last_kernel(void);

/* fp8 operands (OCP e4m3 / e5m2, BASELINE.json config 5 "fp8 MFMA GEMMs"; the reference has no fp8 path -- its
 * Linear is nn.Linear under bf16 autocast, rope_unet.py:122-166, demo_training_latent.yaml:6):
 *   C[M,N] = (A[M,K] . B[N,K]^T) / (scale_a * scale_b)  (+ epilogue), both operands contraction-contiguous fp8 bytes,
 * v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales (2x the bf16 MFMA rate), fp32 accumulate.
 * A has element format fmt_a (UWU_FP8_E4M3 or UWU_FP8_E5M2: output gradients), B is e4m3.  scale_a / scale_b: device
 * floats, the per-tensor quantisation scales (x_fp8 = x * scale).  Epilogues NONE / BIAS / BIAS_GELU / DGELU write
 * bf16 C (C2, aux bf16 as in uwu_gemm); UWU_EPI_ACCUM adds into fp32 C through split-K partial sums in `scratch`
 * (uwu_gemm_fp8_scratch_bytes).  K % 128 == 0, leading dimensions multiples of 16 bytes. */
#define UWU_FP8_E4M3 0
#define UWU_FP8_E5M2 1
size_t uwu_gemm_fp8_scratch_bytes(int M, int N, int K);
int uwu_gemm_fp8(const void* A, const void* B, void* C, void* C2, const float* bias, const void* aux, int M, int N,
                 int K, int lda, int ldb, int ldc, int ldaux, int fmt_a, int epilogue, const float* scale_a,
                 const float* scale_b, void* scratch, size_t scratch_bytes, void* stream);

/* The same GEMM whose epilogue also EMITS the fp8 operand of the next GEMMs (delayed scaling: the scale of a tensor is
 * known before the tensor exists), so that no quantising pass reads the bf16 result again:
 *   UWU_EPI_BIAS_GELU: C = bf16 pre-activation A.B^T + bias (required: the backward pass reads it), q8 [M,N] / q8t [N,M] =
 *                      e4m3(gelu(pre-activation) * q_scale[0])
 *   UWU_EPI_DGELU:     v = (A.B^T) * gelu'(aux); C must be NULL (no bf16 copy); colsum[N] += column sums of v if non-NULL;
 *                      q8 / q8t = e5m2(v * q_scale[0])
 * q_amax (optional) receives max |value| by atomic max (the next step's scale).  Either of q8 / q8t may be NULL.
 * Values saturate to the format's +-max and a NaN stays a NaN byte (see uwu_fp8_quantize for the non-finite contract).
 * M, N multiples of 16; ldq >= N, ldqt >= M, multiples of 16.  Reference: the MLP of the transformer block,
 * rope_unet.py:399-411 (nn.Linear -> GELU(tanh) -> nn.Linear under autocast); the fp8 path is this build's (config 5). */
int uwu_gemm_fp8_emit(const void* A, const void* B, void* C, float* colsum, const float* bias, const void* aux, int M, int N,
                      int K, int lda, int ldb, int ldc, int ldaux, int fmt_a, int epilogue, const float* scale_a,
                      const float* scale_b, void* q8, int ldq, void* q8t, int ldqt, const float* q_scale, float* q_amax,
                      void* stream);

/* 3x3 convolution, padding 1, stride 1 or 2, channels-last bf16, as an implicit GEMM: the MFMA ring kernels gather
 * their activation operand pixel by pixel (per-lane LDS-DMA source addresses, a zero page for the padding) so no
 * im2col matrix exists in HBM (reference: the resblock / down / up-sample Conv2d of diffusers' UNet2DConditionModel,
 * src/duwu/modules/unet_patch.py:13-57).  x [B,H,W,C], w [Cout][3][3][C] (the layout of this build's flat parameter
 * blob), y / dy [B,Ho,Wo,Cout].  uwu_conv3x3_implicit_ok tells whether a shape is covered (bf16, C and Cout multiples
 * of 32, B, H, W > 0, B*Ho*Wo a multiple of 32); other shapes use uwu_im2col3x3 + uwu_gemm.  wgrad accumulates into fp32 dw / db. */
int uwu_conv3x3_implicit_ok(int B, int H, int W, int C, int Cout, int stride, int dtype);
int uwu_conv3x3_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int Cout,
                    int stride, int dtype, void* stream);
/* 3x3 / stride 2 convolution padded RIGHT AND BOTTOM only, forward (the AutoencoderKL encoder's downsampler: F.pad(x, (0,1,0,1)),
 * then stride 2 / padding 0):  y[b,oy,ox,:] = bias + sum_{ky,kx} w[:,ky,kx,:] . x[b, 2 oy + ky, 2 ox + kx, :], zero where the index
 * reaches H or W;  Ho = (H - 2) / 2 + 1, Wo likewise (H, W >= 2).  Same layouts as uwu_conv3x3_fwd.  bf16 shapes with C and Cout
 * multiples of 32 and B*Ho*Wo a multiple of 32 run as an implicit GEMM and need no workspace; every other shape (bf16 with
 * C % 8 == 0, fp32 with C % 4 == 0) gathers a [B*Ho*Wo, 9*C] column matrix into ws and runs uwu_gemm on it.
 * uwu_conv3x3_s2br_ws_bytes: the workspace that shape needs (0: none, or a shape the entry point refuses). */
size_t uwu_conv3x3_s2br_ws_bytes(int B, int H, int W, int C, int Cout, int dtype);
int uwu_conv3x3_s2br_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int Cout, int dtype,
                         void* ws, size_t ws_bytes, void* stream);
int uwu_conv3x3_dgrad(const void* dy, const void* w, void* dx, int B, int H, int W, int C, int Cout, int stride, int dtype,
                      void* stream);
size_t uwu_conv3x3_wgrad_scratch_bytes(int C, int Cout, int64_t Mo);
int uwu_conv3x3_wgrad(const void* dy, const void* x, float* dw, float* db, int B, int H, int W, int C, int Cout, int stride,
                      int dtype, void* scratch, size_t scratch_bytes, void* stream);

/* Per-tensor fp8 quantisation (quant.hip).  amax: device float, max |x| is folded in with an atomic max (caller zeroes
 * it, or uwu_fp8_update_scales does).  update_scales: scale[i] = FMT_MAX(fmt[i]) / (amax[i] * margin) where amax[i] > 0
 * (otherwise the previous scale, or 1), then amax[i] = 0 -- the "delayed scaling" step between two training steps, or
 * the second half of just-in-time scaling.  quantize: one pass over x [M,K] (bf16 / fp32, row-major, ldx) writing any
 * of out [M,K] (ldo), out_t [K,M] (ldt; the operand layout of a contraction over M), colsum[K] += column sums of x
 * (fp32 atomics; a bias gradient), amax.  Values are saturated to the format's largest finite number.
 * Non-finite input (the contract of the whole fp8 chain; tests/test_fp8_chain_gpu.py):
 *   quantize       x * scale is rounded to nearest even; +-inf and everything past +-max give the code of +-max; a NaN gives
 *                  a byte that decodes to NaN (which of the NaN codes is not specified), in out and out_t alike.  The column
 *                  sum of a column that holds a NaN is NaN.
 *   amax           (uwu_fp8_amax and the amax of quantize / the emitting kernels) an Inf element makes it +inf; a NaN
 *                  element is NOT recorded -- the bytes keep a NaN visible, amax does not.
 *   update_scales  stores q = FMT_MAX / (amax * margin), formed in fp32, only where amax > 0 and q is finite and positive
 *                  (q overflows for amax below ~1.3e-36 e4m3 / 1.7e-34 e5m2 and is 0 where amax * margin overflows; a NaN or
 *                  Inf amax never qualifies); otherwise the previous scale stays if it is finite and positive, else 1.
 *                  amax is reset in every case, and a stored scale is always finite and positive.
 *   emitters       uwu_gemm_fp8_emit and uwu_add_ln_modulate_fwd_q8 saturate and keep NaN exactly as quantize does: a NaN
 *                  code in an operand row makes that row of q8 (that column of q8t) and of C decode to NaN; a NaN in a
 *                  LayerNorm input row makes its mean, rstd and every byte of the row NaN; other rows are unaffected. */
int uwu_fp8_amax(const void* x, int dtype, int64_t n, float* amax, void* stream);
int uwu_fp8_update_scales(float* amax, float* scale, const int* fmt, int n, float margin, void* stream);
int uwu_fp8_quantize(const void* x, int dtype, int M, int K, int ldx, const float* scale, int fmt, void* out, int ldo,
                     void* out_t, int ldt, float* amax, float* colsum, void* stream);

/* Weight gradient of a Linear with caller-provided split-K scratch:  C[M,N] (fp32) += A[K,M]^T . B[K,N], both
 * operands K-major (A = dY [tokens, out], B = X [tokens, in]; reference: autograd of nn.Linear inside the blocks,
 * rope_unet.py:122-166).  bf16 operands with K % 32 == 0 run the streaming kernel (LDS-DMA + transposing LDS
 * reads, K split into a multiple of 8 slices, one group of slices per XCD); with `scratch` of at least
 * uwu_gemm_wgrad_scratch_bytes(M, N, K) bytes the slices are written there and summed by a second kernel, with
 * scratch == NULL they are accumulated with fp32 atomics.  Other shapes / fp32 operands are
 * uwu_gemm(transA=1, transB=1, UWU_EPI_ACCUM) with `blocks` workgroups as the split-K target.
 * bias_grad (optional, fp32[M]) += column sums of A = the Linear's bias gradient; the streaming kernel computes it
 * with extra MFMAs against an all-ones fragment instead of a separate pass over dY.
 * Results differ only in summation order.
 * The 192 x 384 / 384 x 192 kernel (M or N a multiple of 384, K >= 32768) runs its K loop as two wave groups one barrier
 * apart; UWU_TRW_GROUPS=0 keeps its eight waves in phase instead -- the same result bit for bit (tools/README.md). */
size_t uwu_gemm_wgrad_scratch_bytes(int M, int N, int K);
int uwu_gemm_wgrad(const void* A, const void* B, float* C, float* bias_grad, int M, int N, int K, int lda, int ldb,
                   int ldc, int dtype, int blocks, void* scratch, size_t scratch_bytes, void* stream);

/* Two weight gradients that share K (the token count) and the dtype: C_a[M_a,N_a] += A_a[K,M_a]^T . B_a[K,N_a] and the same for
 * member b, each with its own shape, leading dimensions and optional bias gradient.  The wide streaming kernel flushes one
 * fp32 tile per CU to the split-K scratch at the end of every launch, whatever the size of the weight; when both members take
 * that kernel with the same tile orientation and have at most 32 tiles together, they run as ONE launch (member b's tiles
 * follow member a's inside every K slice, scratch [slice][a's M x N, then b's M x N]) and one reduce.
 * uwu_gemm_wgrad_pair_scratch_bytes returns the scratch that needs, or 0 when the shapes are not grouped.  With a smaller
 * scratch, misaligned operands or shapes that are not grouped the call is two uwu_gemm_wgrad calls on the same scratch, and
 * its results are theirs bit for bit.  Grouped results differ from them only in summation order. */
size_t uwu_gemm_wgrad_pair_scratch_bytes(int M_a, int N_a, int M_b, int N_b, int K);
int uwu_gemm_wgrad_pair(const void* A_a, const void* B_a, float* C_a, float* bias_grad_a, int M_a, int N_a, int lda_a,
                        int ldb_a, int ldc_a, const void* A_b, const void* B_b, float* C_b, float* bias_grad_b, int M_b,
                        int N_b, int lda_b, int ldb_b, int ldc_b, int K, int dtype, int blocks, void* scratch,
                        size_t scratch_bytes, void* stream);

/* Live measurement for bench.py's `roofline` object: when enabled, every uwu_gemm launch is bracketed by a HIP
 * event pair recorded on that launch's stream; collect() returns the summed launch duration, the summed
 * algorithmic FLOPs (2*M*N*K) and the launch count for operand kind 0 (bf16) or 1 (fp32). */
int uwu_gemm_prof_enable(int on);
int uwu_gemm_prof_collect(int kind, double* ms, double* flops, int* launches);

/* The same, per kernel family (measurement harness): tag = one of UWU_PROF_* (or < 0: all GEMM
 * tags), kind 0 = bf16 / fp8 operands, 1 = fp32, < 0 = any.  flops / bytes are the ALGORITHMIC work of the recorded
 * launches (GEMM 2*M*N*K and operands + outputs once; attention 4*T*Tk*d per head forward, x2.5 backward, and
 * q/k/v/o (+ gradients) once; LayerNorm: every tensor it reads or writes once). */
enum {
  UWU_PROF_GEMM_FWD = 0, UWU_PROF_GEMM_DGRAD = 1, UWU_PROF_GEMM_WGRAD = 2, UWU_PROF_GEMM_FC1_GELU = 3,
  UWU_PROF_GEMM_FC2_DGELU = 4, UWU_PROF_ATTN_FWD = 5, UWU_PROF_ATTN_BWD = 6, UWU_PROF_LN_FWD = 7, UWU_PROF_LN_BWD = 8,
  UWU_PROF_CONV = 9, UWU_PROF_OTHER = 10
};
int uwu_prof_enable(int on);
int uwu_prof_collect(int tag, int kind, double* ms, double* flops, double* bytes, int* launches);

/* out[n] (+)= sum_m X[m,n]   (bias gradients). accumulate: 0 overwrite, 1 add. */
int uwu_colsum(const void* X, int dtype, int M, int N, int ldx, float* out, int accumulate, void* stream);

/* fp32 Linears with at most 64 rows (the conditioning path: timestep MLP, pooled-text projection, the adaLN modulation
 * Linear of all blocks -- reference src/duwu/modules/rope_unet.py:306-309,393-411 run these as nn.Linear on [B, *]).
 * Matrix-vector layouts that read / update the weight matrix once (csrc/skinny.hip).  uwu_skinny_linear_ok() says whether
 * a shape is covered (M <= 64, X [M, K] fits LDS); dgrad additionally needs K <= 512.
 *   fwd:   Y[M,N] = X[M,K] . W[N,K]^T (+ bias) ; epilogue UWU_EPI_NONE / _BIAS / _BIAS_SILU (Y2 = silu(Y))
 *   dgrad: dX[M,K] = dY[M,N] . W[N,K]           (dX overwritten)
 *   wgrad: dW[N,K] += dY^T . X ; db[N] += column sums of dY (db may be NULL) */
int uwu_skinny_linear_ok(int M, int N, int K);
int uwu_skinny_linear_fwd(const float* X, const float* W, const float* bias, float* Y, float* Y2, int M, int N, int K,
                          int epilogue, void* stream);
int uwu_skinny_linear_dgrad(const float* dY, const float* W, float* dX, int M, int N, int K, void* stream);
int uwu_skinny_linear_wgrad(const float* dY, const float* X, float* dW, float* db, int M, int N, int K, void* stream);
/* batched: out[b, n] (+)= sum_m X[b, m, n] for `batch` contiguous [M, ldx] slabs. */
int uwu_colsum_batched(const void* X, int dtype, int batch, int M, int N, int ldx, float* out, int accumulate,
                       void* stream);

/* ------------------------------------------------------------------ norms / modulation (a13) */

/* adaLN-Zero pre-norm with fused residual update (rope_unet.py:306-309, 344-349, 393-411):
 *   x_out = x_in + gate_b * y            (y/gate may be NULL: x_out = x_in, not written if x_out==x_in)
 *   h     = LayerNorm(x_out; eps, no affine) * (1 + scale_b) + shift_b          (affine = 0, adaLN-Zero)
 *   h     = LayerNorm(x_out; eps) * scale + shift   with mod_ld = 0: one shared (gamma, beta) row  (affine = 1,
 *           the plain pre-LN of the SDXL transformer blocks; dscale/dshift then are dgamma/dbeta)
 * x_*, y, h: [B*T, D] in `dtype`; shift/scale/gate: fp32 rows of a [B, mod_ld] buffer; mean/rstd fp32[B*T]. */
int uwu_add_ln_modulate_fwd(const void* x_in, const void* y, const float* gate, const float* shift,
                            const float* scale, int mod_ld, void* x_out, void* h, float* mean, float* rstd,
                            int B, int T, int D, float eps, int affine, int dtype, void* stream);
/* fp8 mode, delayed scaling: the same LayerNorm whose output leaves ONLY as the e4m3 operand of the next GEMMs -- q8 [B*T, D]
 * (contraction over D) and q8t [D, B*T] (the weight gradient's contraction over the tokens) = sat(h * q_scale[0]); q_amax
 * (optional) receives max |h|.  sat keeps NaN (uwu_fp8_quantize's contract): a NaN in a row makes all its bytes NaN.
 * bf16 tensors, per-sample shift / scale required, B*T a multiple of 64, D <= 1536. */
int uwu_add_ln_modulate_fwd_q8(const void* x_in, const void* y, const float* gate, const float* shift, const float* scale,
                               int mod_ld, void* x_out, void* q8, int ldq, void* q8t, int ldqt, const float* q_scale,
                               float* q_amax, float* mean, float* rstd, int B, int T, int D, float eps, void* stream);


/* Backward of the above, fused with the residual/gate backward of the branch that feeds x:
 *   dx_out = dx_in + LN_bwd(dh * (1+scale_b))        (dx_in may be NULL for the last norm)
 *   dy     = gate_b * dx_out                          (if y given)
 *   dshift_b += sum_t dh ; dscale_b += sum_t dh*xhat ; dgate_b += sum_t dx_out*y   (fp32 atomics)
 * mean / rstd are used exactly as given (normally the forward's).  dmod rows live in a [B, mod_ld] fp32 buffer; the sums are
 * ADDED to its contents (zero it for plain gradients) in arbitrary order, so two runs agree to fp32 rounding, not bit for
 * bit; nothing outside the three D-wide slices is written, and a NULL dshift / dscale / dgate skips that sum.
 * D: a multiple of 8 up to 3072 -- narrower than the forward, which takes D <= 4096; a wider D is refused with
 * UWU_EINVAL before anything is launched.  affine = 1 with mod_ld = 0, no y, dshift and dscale given and D <= 2048 runs the
 * one-vector kernel (8 waves, 16 / 32 / 64 rows per workgroup by M); every other call runs the per-sample kernel, whose rows
 * per workgroup (32 down to 1) follow the powers of two that divide T. */
int uwu_add_ln_modulate_bwd(const void* dh, const void* x, const float* mean, const float* rstd,
                            const float* scale, const void* dx_in, const void* y, const float* gate,
                            int mod_ld, void* dx_out, void* dy, float* dshift, float* dscale, float* dgate,
                            int B, int T, int D, int affine, int dtype, void* stream);

/* ------------------------------------------------------------------ attention (a12) */

/* o = softmax(scale * Q K^T) V, non-causal, no mask (rope_unet.py:151-153 F.scaled_dot_product_attention;
 * diffusers AttnProcessor2_0 for the stock UNet).  Row (b,t) of q lives at q + (b*Tq+t)*ldq + h*d, likewise
 * k/v with Tk, ldk/ldv and o with ldo -- so a packed [B*T, 3*H*d] projection is addressed in place with
 * q=base, k=base+H*d, v=base+2*H*d, ld=3*H*d, and cross-attention (Tk=77) uses separate tensors.
 * lse: fp32 [B,H,Tq] log-sum-exp of the scaled scores (saved for backward). */
int uwu_attention_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int Tq, int Tk,
                      int H, int d, int ldq, int ldk, int ldv, int ldo, float scale, int dtype, void* stream);
/* One head of width 512, Tq = Tk = T >= 1, forward only, no lse (the AutoencoderKL mid-block attention): q/k/v/o [B*T, >= 512]
 * with row strides ld* (multiples of 8 for bf16, 4 for fp32; 16-byte aligned bases).  bf16: MFMA flash kernel with online
 * softmax, no T x T tensor in memory; fp32: exact-fp32 VALU kernel. */
int uwu_attention_d512_fwd(const void* q, const void* k, const void* v, void* o, int B, int T, int ldq, int ldk, int ldv, int ldo,
                           float scale, int dtype, void* stream);
/* Causal self-attention of a CLIP text transformer, forward only, no lse (transformers CLIPAttention under the causal mask of
 * CLIPTextTransformer plus the padding mask built from `attention_mask`):  o = softmax(scale * Q K^T + M) V, where key j is visible
 * to query i iff j <= i and (key_mask == NULL or key_mask[b, j] != 0).  key_mask: int64 [B, T], the tokenizer's attention_mask as
 * ConcatTextEncoders holds it.  Addressing as uwu_attention_fwd (Tq = Tk = T), so a packed [B*T, 3*H*d] projection is read in
 * place.  d = 64 and 1 <= T <= 128, anything else is refused; row strides multiples of 8 (bf16) / 4 (fp32) elements, 16-byte
 * aligned bases.  Precondition, not checked on the device: key_mask[b, 0] != 0 (tokenizers always emit bos, so no row is fully
 * masked; a row that is comes out as zeros).  bf16: MFMA kernel, one workgroup per (batch, head), K / V staged once in LDS,
 * T padded to the MFMA tile inside the kernel, key tiles above the diagonal skipped, plain softmax in registers; fp32: exact-fp32
 * VALU kernel. */
int uwu_attention_causal_fwd(const void* q, const void* k, const void* v, const int64_t* key_mask, void* o, int B, int T, int H,
                             int d, int ldq, int ldk, int ldv, int ldo, float scale, int dtype, void* stream);
/* CLIPTextEmbeddings: out[b,t,:] = tok_table[ids[b,t],:] + pos_table[t,:].  ids int64 [B, T]; tok_table [vocab, D], pos_table
 * [>= T, D] and out [B*T, D] in `dtype`; D a multiple of 8, 16-byte aligned tables.  An id outside [0, vocab) is CLAMPED to the
 * nearest valid row (torch's embedding raises instead): nothing outside the table is ever read. */
int uwu_text_embed(const int64_t* ids, const void* tok_table, const void* pos_table, void* out, int B, int T, int D, int vocab,
                   int dtype, void* stream);
/* y = act(x + bias) on [M, N] rows of stride ld (elements), the activations of CLIPMLP that the GEMM epilogue does not have:
 * UWU_ACT_QUICK_GELU  v * sigmoid(1.702 v)  (transformers QuickGELUActivation, CLIP-L),  UWU_ACT_GELU_ERF  0.5 v (1 + erf(v /
 * sqrt 2))  (nn.GELU, OpenCLIP-bigG).  bias fp32 [N] or NULL; y == x allowed; N and ld multiples of 8, 16-byte aligned.  fp32
 * tensors are evaluated in double, bf16 tensors in fp32. */
#define UWU_ACT_QUICK_GELU 0
#define UWU_ACT_GELU_ERF 1
int uwu_bias_act_fwd(const void* x, const float* bias, void* y, int M, int N, int ld, int kind, int dtype, void* stream);
/* CLIP pooled output: pooled[b,:] = h[b, p_b, :] with p_b found on the device.  eos_id == 2: p_b = first position of the largest
 * id (`input_ids.argmax(-1)`, the legacy rule of transformers' CLIPTextTransformer that every SDXL checkpoint takes); otherwise
 * p_b = first position whose id equals eos_id, position 0 if there is none (`(input_ids == eos).int().argmax(-1)`).
 * h [B*T, D], pooled [B, D] in `dtype`; D a multiple of 8. */
int uwu_text_pool(const int64_t* ids, const void* h, void* pooled, int B, int T, int D, int eos_id, int dtype, void* stream);
/* Self-attention of a T5 encoder, forward only, no lse (transformers T5Attention: bidirectional, a learned bias per head that
 * depends on key - query only, plus the padding mask built from `attention_mask`):
 *   o = softmax(scale * Q K^T + rel_bias[h, j - i + T - 1] + M) V      i: query, j: key
 * rel_bias: fp32 [H, 2 T - 1] (uwu_t5_rel_bias gathers it; no [H, T, T] tensor exists anywhere).  key_mask: int64 [B, T] or NULL;
 * key j is visible iff key_mask == NULL or key_mask[b, j] != 0.  A hidden key never contributes, whatever its K / V rows hold (NaN
 * included).  Precondition: every sequence has at least one visible key; a sequence without one gives rows of zeros, not NaN.
 * Addressing as uwu_attention_causal_fwd (packed [B*T, 3*H*64] projections are read in place: strides in elements, multiples of 8
 * (bf16) / 4 (fp32), 16-byte aligned bases).  d == 64, 1 <= T <= 512, B * H <= 65535; anything else is refused.  T5 passes scale
 * = 1.  bf16: MFMA kernel tiled over blocks of 64 queries, keys walked 64 at a time with an online softmax (T padded to the tile
 * inside the kernel); fp32: exact-fp32 VALU kernel. */
int uwu_attention_relbias_fwd(const void* q, const void* k, const void* v, const float* rel_bias, const int64_t* key_mask, void* o,
                              int B, int T, int H, int d, int ldq, int ldk, int ldv, int ldo, float scale, int dtype, void* stream);
/* Bidirectional self-attention without a bias, forward only, no lse (the CLIP image tower, transformers CLIPAttention with no
 * mask):  o = softmax(scale * Q K^T + M) V.  key_mask: int64 [B, T] or NULL (the ViT passes NULL); key j is visible iff key_mask ==
 * NULL or key_mask[b, j] != 0.  A hidden key never contributes, whatever its K / V rows hold (NaN included).  Precondition: every
 * sequence has at least one visible key; a sequence without one gives rows of zeros, not NaN.  Addressing, alignment and refusals
 * as uwu_attention_relbias_fwd (packed [B*T, 3*H*64] projections are read in place: strides in elements, multiples of 8 (bf16) /
 * 4 (fp32), 16-byte aligned bases).  d == 64, 1 <= T <= 1024, B * H <= 65535; anything else is refused -- d == 80 (ViT-H/14,
 * apple/DFN5B-CLIP-ViT-H-14-378) is not built.  bf16: the MFMA kernel of uwu_attention_relbias_fwd compiled a second time without its
 * bias row (one template, two instantiations: 64-query blocks, 64-key chunks, online softmax, T padded to the tile inside the
 * kernel; without the bias row nothing in it depends on T, hence the higher cap); fp32: the same exact-fp32 VALU kernel with the bias read switched off. */
int uwu_attention_bidir_fwd(const void* q, const void* k, const void* v, const int64_t* key_mask, void* o, int B, int T, int H, int d,
                            int ldq, int ldk, int ldv, int ldo, float scale, int dtype, void* stream);
/* The A operand of a ViT's patch-embedding GEMM.  images: [B, 3, S, S] contiguous, fp32 (in_u8 == 0) or uint8 (in_u8 != 0); out:
 * [B * (S/p)^2, ld] in `dtype`, row b (S/p)^2 + py (S/p) + px holding patch (py, px) of image b in the column order (c, i, j) =
 * c p p + i p + j, so that patch_embedding.weight viewed as [D, 3 p p] is the B operand unchanged; columns 3 p p .. ld - 1 are
 * written as zeros (ld pads the row to what uwu_gemm takes: 3 * 14 * 14 = 588 is no multiple of 8).  normalize != 0 fuses CLIP's
 * preprocessing of a [0, 255] image:  v = clamp(x, 0, 255) (NaN -> 0),  out = (v / 255 - mean[c]) / std[c]  in fp32, each step
 * rounded once; mean and std are HOST pointers to three floats each (std > 0), read before the call returns.  normalize == 0
 * copies x as it is (pixel_values that were normalised elsewhere; mean / std may be NULL; fp32 input only).  S % p == 0. */
int uwu_clip_patches(const void* images, int in_u8, void* out, int B, int S, int p, int ld, int normalize, const float* mean,
                     const float* std, int dtype, void* stream);
/* CLIPVisionEmbeddings after the patch GEMM:  out[b, 0, :] = class_embedding + pos_table[0],  out[b, 1 + i, :] = patch_out[b Np +
 * i, :] + pos_table[1 + i]  with Np = T - 1 (the patch convolution has no bias in CLIP).  patch_out [B * Np, D], class_embedding
 * [D], pos_table [T, D], out [B * T, D], all contiguous in `dtype`; the sum is taken in fp32 and rounded once; D a multiple of 8,
 * 16-byte aligned. */
int uwu_vit_embed(const void* patch_out, const void* class_embedding, const void* pos_table, void* out, int B, int T, int D, int dtype,
                  void* stream);
/* CLIP score of B (image, text) pairs, accumulated on the device:  scores[b] = 100 cos(image_embeds[b], text_embeds[b])  (fp32
 * dot product and norms; a zero embedding gives NaN, as the division it stands for does),  acc[0] += sum_b scores[b],  acc[1] += B.
 * image_embeds, text_embeds [B, P] contiguous in `dtype`; scores fp32 [B]; acc: two doubles on the device, zeroed by the caller
 * before the first batch.  The sum runs in ONE workgroup in an order fixed by B, in double, and only one thread touches acc: no
 * floating-point atomics, the same batches in the same order give the same bits.  No host synchronisation: the caller reads acc
 * when it wants the mean. */
int uwu_clip_score_accum(const void* image_embeds, const void* text_embeds, float* scores, double* acc, int B, int P, int dtype,
                         void* stream);
/* Per-timestep statistics of a validation batch, accumulated on the device (reference src/duwu/trainer/callbacks.py:76-91: a Python
 * loop over all n_steps timesteps with three masked reductions each).  For every sample b whose bucket k = trunc(timesteps[b]) (toward
 * zero, as `.long()`: 3.9 -> 3, -0.5 -> 0) lies in [0, n_steps):  stats[0][k] += 1,  stats[1][k] += losses[b],  stats[2][k] += losses[b]^2.
 * A sample with a bucket outside that range or a NaN timestep is ignored; a NaN or inf loss reaches its own bucket only.  losses fp32
 * [B]; timesteps [B], int64 (t_dtype = UWU_I64) or fp32 (UWU_F32); stats: 3 * n_steps doubles, zeroed by the caller before the first
 * batch.  With loss_mean (ONE fp32 on the device, the batch's scalar loss):  totals[0] += B * *loss_mean,  totals[1] += B  (two
 * doubles; the sample-weighted mean of an epoch is totals[0] / totals[1]); loss_mean == NULL skips that, and totals may then be NULL.
 * Everything is accumulated in double, the square is formed in double.  Each bucket is owned by one thread, which adds its samples in
 * ascending b, and one thread writes totals: no atomics, bits independent of the launch geometry, and two calls give what one call on
 * the concatenation gives.  B > 0, 1 <= n_steps <= 65536.  No host synchronisation. */
int uwu_timestep_stats_accum(const float* losses, const void* timesteps, int t_dtype, const float* loss_mean, int B, int n_steps,
                             double* stats, double* totals, void* stream);

/* ------------------------------------------------------------------ InceptionV3 feature extractor and FID statistics (4.37) */
/* Forward convolution on channels-last activations, y = [relu](conv(x, w) + bias), as an implicit GEMM on the MFMA units (no column
 * matrix in memory) in both dtypes (bf16: v_mfma_f32_16x16x32_bf16; fp32: v_mfma_f32_16x16x4_f32, the parity mode).  Kernel (KH, KW)
 * one of 1x1, 3x3, 5x5, 1x7, 7x1, 1x3, 3x1; stride 1 or 2; zero padding (ph, pw) below the kernel size.  x: rows of ldx elements, one
 * per input pixel (b, iy, ix), the convolution reading channels xoff .. xoff + C - 1 of each; y: rows of ldy elements, one per output
 * pixel, channels yoff .. yoff + Cout - 1 written and every other element of the row left alone (a branch writes its slice of a
 * concatenation); Ho = (H + 2 ph - KH) / stride + 1, Wo likewise.  w [Cout][KH][KW][C] in `dtype`, bias fp32 [Cout] or NULL.  C,
 * Cout, ldx, ldy, xoff, yoff multiples of 8 (48 and 80 channels need no padding), B Ho Wo arbitrary (a true M tail), 16-byte aligned
 * pointers.  uwu_conv2d_ok: 1 where the shape is built, 0 where uwu_conv2d_fwd refuses it (before any launch, y untouched);
 * uwu_conv2d_ws_bytes: the workspace the shape needs -- 0 for every shape today, the argument is there for an explicit route.
 * Reference: the BasicConv2d of torch-fidelity's FeatureExtractorInceptionV3, which torchmetrics' FrechetInceptionDistance wraps
 * (reference src/duwu/metrics/fid.py:5). */
int uwu_conv2d_ok(int B, int H, int W, int C, int Cout, int KH, int KW, int stride, int ph, int pw, int ldx, int xoff, int ldy, int yoff,
                  int dtype);
size_t uwu_conv2d_ws_bytes(int B, int H, int W, int C, int Cout, int KH, int KW, int stride, int ph, int pw, int ldx, int xoff, int ldy,
                           int yoff, int dtype);
int uwu_conv2d_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int Cout, int KH, int KW,
                   int stride, int ph, int pw, int ldx, int xoff, int ldy, int yoff, int relu, int dtype, void* ws, size_t ws_bytes,
                   void* stream);
/* The A operand of Conv2d_1a_3x3 (3 -> 32, 3x3, stride 2, no padding).  images [B, 3, H, W] contiguous: uint8 (in_u8 != 0) taken as
 * they are, or fp32 in [0, 1] turned into  v = trunc(clamp(x, 0, 1) * 255)  (the product rounded to fp32, then truncated; NaN -> 0);
 * then  (v - 128) / 128,  exact in bf16.  out [B Ho Wo, 32] in `dtype`, Ho = (H - 3) / 2 + 1: column 9 c + 3 ky + kx of row
 * (b, oy, ox) is pixel (c, 2 oy + ky, 2 ox + kx), the order of conv.weight.view(32, 27); columns 27 .. 31 are zeros. */
int uwu_inception_stem(const void* images, int in_u8, void* out, int B, int H, int W, int dtype, void* stream);
/* 3x3 pooling, channels-last, strided in and out like uwu_conv2d_fwd.  MAX_S2: stride 2, no padding, Ho = (H - 3) / 2 + 1 (H, W >= 3);
 * MAX_S1P1: stride 1, padding 1 that never wins (the maximum over the pixels inside the image); AVG_S1P1: stride 1, padding 1, the
 * sum over the pixels inside the image divided by their number, 4 / 6 / 9 (count_include_pad = False), in fp32.  C a multiple of 8. */
#define UWU_POOL_MAX_S2 0
#define UWU_POOL_MAX_S1P1 1
#define UWU_POOL_AVG_S1P1 2
int uwu_pool2d_fwd(const void* x, void* y, int B, int H, int W, int C, int mode, int ldx, int xoff, int ldy, int yoff, int dtype,
                   void* stream);
/* y[m, yoff .. yoff + N) = max(., 0) in place on M rows of ldy elements: the ReLU behind a uwu_gemm with UWU_EPI_BIAS, which is how the
 * extractor runs the 1x1 convolutions that uwu_gemm was measured faster on.  N, ldy, yoff multiples of 8. */
int uwu_relu_rows(void* y, int64_t M, int N, int ldy, int yoff, int dtype, void* stream);
/* out[b, c] = mean over the HW pixels of x[b, :, c], added in ascending order in fp32; x rows of ldx elements in `dtype`, out fp32 [B, C] */
int uwu_global_avgpool(const void* x, float* out, int B, int HW, int C, int ldx, int dtype, void* stream);
/* FID statistics of a batch of features, accumulated on the device.  features fp32 [B, D] contiguous; acc: 1 + D + D D doubles,
 * zeroed by the caller before the first batch:  acc[0] += B,  acc[1 + d] += sum_b f[b, d],  acc[1 + D + i D + j] += sum_b f[b, i]
 * f[b, j].  Products and sums in double, b ascending; every element is owned by one thread: no floating-point atomics, the same
 * batches in the same order give the same bits.  D a multiple of 64, at most 8192.  No host synchronisation. */
int uwu_fid_stats_accum(const float* features, double* acc, int B, int D, void* stream);

/* T5LayerNorm with the previous sublayer's residual add fused in:  x_out = x_in + y (y may be NULL: x_out is then not written and
 * may be NULL),  n_out = x_out * rsqrt(mean(x_out^2) + eps) * weight -- no mean subtraction, no bias.  x_in, y, x_out, n_out [M, D]
 * contiguous in `dtype`, weight fp32 [D]; D a multiple of 8, 16-byte aligned; statistics in fp32, taken of x_out as stored.
 * x_out may be x_in; n_out aliases nothing. */
int uwu_add_rmsnorm_fwd(const void* x_in, const void* y, const float* weight, void* x_out, void* n_out, int M, int D, float eps,
                        int dtype, void* stream);
/* The gate of T5 v1.1's feed-forward:  out[M, F] = act(u[:, :F]) * u[:, F:2F]  on the [M, 2F] output of one GEMM over wi_0 | wi_1
 * stored back to back (rows of stride ldu / ldo elements, multiples of 8; F a multiple of 8; 16-byte aligned; out must not overlap
 * u).  UWU_GATE_GELU_TANH: transformers NewGELUActivation, 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))).  fp32 tensors are
 * evaluated in double, bf16 tensors in fp32. */
#define UWU_GATE_GELU_TANH 0
int uwu_gated_act_fwd(const void* u, void* out, int M, int F, int ldu, int ldo, int kind, int dtype, void* stream);
/* T5's relative-position bias per offset:  out[h, o] = weight[bucket[o], h]  for o = key - query + T - 1 in [0, n), n = 2 T - 1.
 * weight fp32 [num_buckets, H] (relative_attention_bias.weight), bucket int32 [n] (computed by the host; entries are clamped to
 * the table), out fp32 [H, n]. */
int uwu_t5_rel_bias(const float* weight, const int32_t* bucket, float* out, int num_buckets, int H, int n, void* stream);
/* out[b,t,:] = tok_table[ids[b,t],:]: uwu_text_embed without a position table (T5 has none); the same clamping of ids. */
int uwu_token_embed(const int64_t* ids, const void* tok_table, void* out, int B, int T, int D, int vocab, int dtype, void* stream);
/* dq/dk/dv use the strides of q/k/v; dO uses ldo.  delta: fp32 workspace [B,H,Tq] (rowsum(dO*O)). */
int uwu_attention_bwd(const void* q, const void* k, const void* v, const void* o, const void* dO,
                      const float* lse, float* delta, void* dq, void* dk, void* dv, int B, int Tq, int Tk, int H,
                      int d, int ldq, int ldk, int ldv, int ldo, float scale, int dtype, void* stream);
/* The same with an additive score bias per key: o = softmax(scale * Q K^T + key_bias[b, :]) V.  key_bias: fp32
 * [B, Tk], shared by every head and query row and not differentiated -- this is how the reference applies
 * `encoder_attention_mask` to cross-attention: `(1 - mask) * -10000.0`, unsqueezed over the query axis
 * (rope_unet.py:440-453) and broadcast over heads by `prepare_attention_mask` (rope_unet.py:106-114) before
 * F.scaled_dot_product_attention(attn_mask=...) (rope_unet.py:151-153).  Finite values only. */
int uwu_attention_bias_fwd(const void* q, const void* k, const void* v, const float* key_bias, void* o, float* lse,
                           int B, int Tq, int Tk, int H, int d, int ldq, int ldk, int ldv, int ldo, float scale,
                           int dtype, void* stream);
int uwu_attention_bias_bwd(const void* q, const void* k, const void* v, const float* key_bias, const void* o,
                           const void* dO, const float* lse, float* delta, void* dq, void* dk, void* dv, int B,
                           int Tq, int Tk, int H, int d, int ldq, int ldk, int ldv, int ldo, float scale, int dtype,
                           void* stream);
/* Which kernels uwu_attention_fwd (pass = 0) / uwu_attention_bwd (pass = 1) and their key-bias forms run on this shape: 1 = the MFMA
 * kernels (bf16; head dim 40 / 64 / 72 / 80 / 128; row strides multiples of 8; Tq a multiple of 64, or -- at head dim 40 / 64 / 80 -- any Tq
 * above 256, whose last query tile is guarded), 0 = the generic ones.  HOST-ONLY (no device call, usable without a GPU).  It is the predicate the dispatch
 * itself evaluates; the dispatch also wants every tensor 16-byte aligned, which this query assumes. */
int uwu_attention_route(int pass, int Tq, int Tk, int d, int ldq, int ldk, int ldv, int ldo, int dtype);

/* Axial RoPE with learnable per-head log-frequencies, exactly as the reference writes it (src/duwu/modules/rope.py:
 * 56-71, 83-108; applied to q and k at rope_unet.py:143-147).  x/y: [rows, ldx] token-major with H heads of width d;
 * pos: fp32 [rows, 2] (h, w); fh/fw: fp32 [H, d/4].  bwd: dx, and (optional) dfh/dfw += gradient wrt log-freqs. */
int uwu_axial_rope_fwd(const void* x, const float* pos, const float* fh, const float* fw, void* y, int64_t rows,
                       int H, int d, int ldx, int dtype, void* stream);
int uwu_axial_rope_bwd(const void* x, const void* dy, const float* pos, const float* fh, const float* fw, void* dx,
                       float* dfh, float* dfw, int64_t rows, int H, int d, int ldx, int dtype, void* stream);

/* Axial RoPE folded into self-attention (rope_unet.py:143-153: RoPE on q and k, then SDPA): the attention kernels multiply
 * q and k by the factor table tab [T, ldt] (fp32; head h's d columns at h*d; shared positions pos [T,2]) while staging
 * them, so no rotated copy of q / k exists.  bf16, head dim 64, T == Tk a multiple of 64 up to 256 (the DiT shapes).
 * uwu_attention_rope_bwd returns dq / dk wrt the ROTATED q' / k'; uwu_axial_rope_bwd (x = the raw q / k, dy = those, dx in
 * place) turns them into the gradients of q / k and of the log-frequencies. */
int uwu_axial_rope_bwd_shared(const void* x, const void* dy, const float* pos, int pos_rows, const float* fh, const float* fw,
                              void* dx, float* dfh, float* dfw, int64_t rows, int H, int d, int ldx, int dtype, void* stream);
int uwu_axial_rope_table(const float* pos, const float* fh, const float* fw, float* tab, int T, int H, int d, int ldt,
                         void* stream);
int uwu_attention_rope_fwd(const void* q, const void* k, const void* v, const float* rope_tab, void* o, float* lse, int B,
                           int T, int H, int d, int ldq, int ldk, int ldv, int ldo, int ldt, float scale, int dtype,
                           void* stream);
int uwu_attention_rope_bwd(const void* q, const void* k, const void* v, const float* rope_tab, const void* o, const void* dO,
                           const float* lse, void* dq, void* dk, void* dv, int B, int T, int H, int d, int ldq, int ldk,
                           int ldv, int ldo, int ldt, float scale, int dtype, void* stream);

/* ------------------------------------------------------------------ embeddings / layout (a11, a13) */

/* Sinusoidal timestep features [B, dim]: [cos(t*f_i) | sin(t*f_i)], f_i = exp(-ln(max_period)*i/half). */
int uwu_timestep_embedding(const float* t, int B, int dim, float max_period, void* out, int dtype,
                           void* stream);
/* y = silu(x) elementwise (dtype in/out); dx = dy * silu'(x). */
int uwu_silu_fwd(const void* x, void* y, int64_t n, int dtype, void* stream);
int uwu_silu_bwd(const void* x, const void* dy, void* dx, int64_t n, int dtype, void* stream);

/* out = a + b elementwise (same dtype). */
int uwu_add(const void* a, const void* b, void* out, int64_t n, int dtype, void* stream);
/* dst[c][r] = src[r][c], bf16 (a weight matrix laid out contraction-contiguous for the input-gradient GEMM) */
int uwu_transpose_bf16(const void* src, void* dst, int rows, int cols, int ld_src, int ld_dst, void* stream);

/* patchify: latent [B,C,H,W] (fp32) -> tokens [B*(H/p)*(W/p), C*p*p] (dtype), feature order (c,ph,pw).
 * unpatchify is the inverse (tokens -> fp32 image).  Conv2d(k=p,s=p) patch embedding == patchify + GEMM. */
int uwu_patchify(const float* img, void* tok, int B, int C, int H, int W, int p, int dtype, void* stream);
int uwu_unpatchify(const void* tok, int dtype, float* img, int B, int C, int H, int W, int p, void* stream);
/* x[b,t,:] += pos[t,:]  (fixed 2-D sin-cos table, fp32 [T,D]) */
int uwu_add_pos(void* x, const float* pos, int B, int T, int D, int dtype, void* stream);

/* ------------------------------------------------------------------ UNet2DConditionModel-shape denoiser (a11) */
/* Channels-last activations x[b, p, c] (p = y*W + x).  Replace the torch/diffusers op sequences of
 * ResnetBlock2D / Transformer2DModel / Down-/Upsample2D (reference src/duwu/modules/unet_patch.py:13-57). */

/* y = GroupNorm(x; G groups, eps, gamma, beta) [then SiLU if silu]; mean/rstd: fp32 [B*G]. */
int uwu_groupnorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                      int B, int HW, int C, int G, float eps, int silu, int dtype, void* stream);
/* dgamma/dbeta are accumulated (fp32 atomics); either may be NULL (a frozen norm).  ws: fp32 scratch of 2*B*G floats.
 * Both directions: C % 8 == 0, C <= 4096, 16-byte aligned tensors (whole-row vector accesses). */
/* uwu_groupnorm_fwd with a fixed summation order: per-workgroup partial sums in ws (uwu_groupnorm_fwd_det_ws_bytes), added in
 * ascending order, the row partition a function of the image alone.  The statistics of a sample, and so y, are the same bits
 * between launches and between batch sizes (the atomics of uwu_groupnorm_fwd give agreement to fp32 rounding only).  Same
 * shapes and refusals as uwu_groupnorm_fwd. */
size_t uwu_groupnorm_fwd_det_ws_bytes(int B, int HW, int C, int G);
int uwu_groupnorm_fwd_det(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, void* ws,
                          size_t ws_bytes, int B, int HW, int C, int G, float eps, int silu, int dtype, void* stream);
int uwu_groupnorm_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                      const float* beta, void* dx, float* dgamma, float* dbeta, float* ws, int B, int HW, int C, int G,
                      int silu, int dtype, void* stream);
/* 3x3 / padding 1 / stride 1|2 convolution = im2col + uwu_gemm: col[(b,oy,ox), (ky,kx,c)]; col2im is the adjoint
 * in gather form (no atomics). */
int uwu_im2col3x3(const void* x, void* col, int B, int H, int W, int C, int stride, int dtype, void* stream);
int uwu_col2im3x3(const void* dcol, void* dx, int B, int H, int W, int C, int stride, int dtype, void* stream);
/* GEGLU feed-forward gate: hg [M, 2F] = (h | gate) -> out [M, F] = h * gelu_erf(gate), and its backward. */
int uwu_geglu_fwd(const void* hg, void* out, int64_t M, int F, int dtype, void* stream);
int uwu_geglu_bwd(const void* hg, const void* dout, void* dhg, int64_t M, int F, int dtype, void* stream);
/* nearest-neighbour 2x upsample [B,H,W,C] -> [B,2H,2W,C]; backward=1: src is d(out) [B,2H,2W,C], dst d(in). */
int uwu_upsample2x(const void* src, void* dst, int B, int H, int W, int C, int backward, int dtype, void* stream);
/* x[b, p, :] += v[b, :] (time-embedding injection). */
int uwu_add_rowvec(void* x, const void* v, int B, int HW, int C, int dtype, void* stream);
/* NCHW fp32 <-> channels-last (dtype). */
int uwu_nchw_to_cl(const float* nchw, void* cl, int B, int C, int HW, int dtype, void* stream);
int uwu_cl_to_nchw(const void* cl, float* nchw, int B, int C, int HW, int dtype, void* stream);

/* ------------------------------------------------------------------ whole-network drivers */

/* DiT forward/backward: all kernel launches of one network pass issued from C++ (no per-op
 * host round trip).  The argument block is a plain C struct of device pointers and sizes. */
typedef struct uwu_dit_desc {
  int32_t B, T, D, H, L, mlp_ratio, in_ch, out_ch, patch, img, dtype, cond_dim, freq_dim;
  float ln_eps;
  int32_t mod_total;   /* = L*6*D + 2*D : all adaLN linears batched in one GEMM */
  /* parameter blob (operand dtype copy for GEMM operands, fp32 master for biases) */
  const void* w;        /* operand-dtype flat parameters  */
  const float* w32;     /* fp32 master flat parameters    */
  float* g32;           /* fp32 flat gradient buffer (accumulated into) */
  /* offsets (in elements) into the flat blobs */
  int64_t off_patch_w, off_patch_b, off_t_w1, off_t_b1, off_t_w2, off_t_b2, off_y_w, off_y_b,
      off_mod_w, off_mod_b, off_final_w, off_final_b;
  int64_t off_layer0, layer_stride; /* per layer: qkv_w, qkv_b, o_w, o_b, fc1_w, fc1_b, fc2_w, fc2_b */
  const float* pos;     /* [T, D] fp32 */
  void* ws;             /* activation workspace (saved for backward) */
  size_t ws_bytes;
  void* const* layer_done; /* optional: L hipEvent_t handles (or NULL).  uwu_dit_backward records layer_done[l] on its
                              stream once every parameter-gradient launch of block l has been issued, so a data-parallel
                              host can start reducing that block's slice of g32 while the backward continues
                              (blocks finish in the order L-1 .. 0; the non-block parameters finish last). */
  /* fp8 Linears (BASELINE config 5): 0 = off; 1 = just-in-time per-tensor scaling (amax pass, then quantise); 2 = delayed
   * scaling (quantise with the scale derived from the previous step's amax; call with 1 for the first step).  Needs
   * dtype == UWU_BF16, D % 128 == 0.  Roles (12 per block, index 12*l + r): r 0-3 = inputs of qkv / proj / fc1 / fc2
   * (e4m3), 4-7 = their output gradients (e5m2), 8-11 = their weights (e4m3). */
  /* optional second stream (hipStream_t) for the weight gradients of small batches (B*T <= 16384 token rows, bf16): they
   * run beside the chain of input gradients, ordered by events; NULL = everything on the call's stream. */
  void* side_stream;
  /* axial-RoPE self-attention (rope_unet.py:143-147): rope != 0 rotates q and k inside the
   * attention kernels with learnable per-layer, per-head log-frequencies at w32 + off_rope_h / off_rope_w ([L, H, d/4]
   * each; gradients into g32 at the same offsets) and the shared token positions pos_xy [T, 2] (fp32). */
  int32_t rope;
  int64_t off_rope_h, off_rope_w;
  const float* pos_xy;
  int32_t fp8;
  float* f8_scale;      /* [12 L] per-tensor quantisation scales */
  float* f8_amax;       /* [12 L] running max |x| of the current step */
  const int32_t* f8_fmt; /* [12 L] UWU_FP8_E4M3 / UWU_FP8_E5M2 per role */
  /* block recomputation (the reference's enable_gradient_checkpointing, test_scripts/test_train.py:38-39; diffusers
   * rope_unet.py:484-507 checkpoints per transformer block): != 0 keeps per block only its input x0 and the row statistics
   * of its first LayerNorm; every other saved activation lives in ONE slab shared by all blocks, and uwu_dit_backward reruns
   * block l - 1 from its kept input before it needs that block's tensors.  Workspace: L * (M*D + 8 M) + one full block slab
   * instead of L full slabs.  Same kernels on the same inputs: the recomputed tensors are bit-identical. */
  int32_t checkpoint;
} uwu_dit_desc;

size_t uwu_dit_workspace_bytes(const uwu_dit_desc* d);
/* noisy: fp32 [B,C,H,W]; t: fp32 [B]; cond: fp32 [B, cond_dim] or NULL; out: fp32 [B,out_ch,H,W] */
int uwu_dit_forward(const uwu_dit_desc* d, const float* noisy, const float* t, const float* cond,
                    float* out, void* stream);
/* dout: fp32 [B,out_ch,H,W] gradient of the loss wrt the network output; parameter gradients are ACCUMULATED
 * into d->g32 (zero it at the start of a step).  uwu_dit_backward_cond adds the gradient of the pooled-
 * conditioning projection (it needs the caller's `cond` tensor again). */
int uwu_dit_backward(const uwu_dit_desc* d, const float* dout, void* stream);
int uwu_dit_backward_cond(const uwu_dit_desc* d, const float* cond, void* stream);
/* elements per transformer block in the flat parameter blob (every tensor padded to 64 elements):
 * qkv_w[3D,D] qkv_b[3D] o_w[D,D] o_b[D] fc1_w[rD,D] fc1_b[rD] fc2_w[D,rD] fc2_b[D] */
int64_t uwu_dit_layer_param_stride(int D, int mlp_ratio);

#ifdef __cplusplus
}
#endif
#endif /* UWU_HIP_H */
