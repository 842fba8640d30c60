// Validation statistics.
//   uwu_timestep_stats_accum  per-timestep count / sum / sum of squares of the per-sample losses of one validation batch, added to
//                             a double accumulator that lives on the device for the whole validation pass
// Reference: src/duwu/trainer/callbacks.py:76-91 walks `for timestep in range(n_diffusion_time_steps)` with a boolean mask and
// three masked reductions per timestep -- a few thousand launches and a host sync per masked index, every validation batch.
//
// Here every bucket has ONE owner: thread t of the grid owns bucket t, keeps its three doubles in registers and scans the batch's
// (bucket, loss) pairs, which the workgroup stages in LDS a chunk at a time (every lane reads the same LDS word: a broadcast, no
// bank conflict).  The owner adds its samples in ascending b, so the bits of a bucket depend on the samples alone, not on the launch
// geometry, and two calls give what one call on the concatenation gives.  No atomics.  n_steps * B compares: 3 M at B = 3072,
// n_steps = 1000.
#include "common.h"

namespace {

constexpr int TS_THREADS = 256;  // buckets per workgroup
constexpr int TS_CHUNK = 1024;   // samples staged per round: 8 KB of LDS

// bucket of a timestep: truncation toward zero (`aux_output.timesteps.long()`), -1 for what the reference's loop never matches
__device__ __forceinline__ int ts_bucket(int64_t t, int n_steps) { return (t >= 0 && t < (int64_t)n_steps) ? (int)t : -1; }
__device__ __forceinline__ int ts_bucket(float t, int n_steps) {
  // (-1, 0) truncates to 0; NaN fails both compares; the range test comes before the conversion, which is undefined outside int
  return (t > -1.f && t < (float)n_steps) ? (int)t : -1;
}

template <typename TT>
__global__ void __launch_bounds__(TS_THREADS) timestep_stats_kernel(const float* __restrict__ losses, const TT* __restrict__ timesteps,
                                                                    const float* __restrict__ loss_mean, int B, int n_steps,
                                                                    double* __restrict__ stats, double* __restrict__ totals) {
  __shared__ __attribute__((aligned(16))) int s_bucket[TS_CHUNK];
  __shared__ float s_loss[TS_CHUNK];
  const int own = blockIdx.x * TS_THREADS + threadIdx.x;
  const bool live = own < n_steps;
  double cnt = 0.0, sum = 0.0, sq = 0.0;
  if (live) {
    cnt = stats[own];
    sum = stats[(int64_t)n_steps + own];
    sq = stats[2 * (int64_t)n_steps + own];
  }
  for (int base = 0; base < B; base += TS_CHUNK) {
    const int n = min(TS_CHUNK, B - base);
    __syncthreads();  // the previous chunk has been scanned
    for (int i = threadIdx.x; i < ((n + 3) & ~3); i += TS_THREADS) {  // (the tail of the last group of four matches no owner)
      s_bucket[i] = i < n ? ts_bucket(timesteps[base + i], n_steps) : -1;
      s_loss[i] = i < n ? losses[base + i] : 0.f;
    }
    __syncthreads();
    if (live) {
      // four buckets per LDS read (ds_read_b128), the reads of the unrolled groups issued ahead of the compares: the scan is bound
      // by LDS latency, not by the compares.  Within a group the samples are still taken in ascending b.
#pragma unroll 4
      for (int i = 0; i < n; i += 4) {
        const int4 k = *reinterpret_cast<const int4*>(&s_bucket[i]);
        if (k.x == own | k.y == own | k.z == own | k.w == own) {
          const int kk[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (kk[j] == own) {
              const double l = (double)s_loss[i + j];
              cnt += 1.0;
              sum += l;
              sq += l * l;  // the product of two floats is exact in double, so a contraction into an fma rounds the same
            }
          }
        }
      }
    }
  }
  if (live) {
    stats[own] = cnt;
    stats[(int64_t)n_steps + own] = sum;
    stats[2 * (int64_t)n_steps + own] = sq;
  }
  if (loss_mean != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {  // the one writer of totals
    totals[0] = __dadd_rn(totals[0], __dmul_rn((double)B, (double)loss_mean[0]));  // product rounded, then added: not contracted
    totals[1] += (double)B;
  }
}

}  // namespace

extern "C" int uwu_timestep_stats_accum(const float* losses, const void* timesteps, int t_dtype, const float* loss_mean, int B, int n_steps,
                                        double* stats, double* totals, void* stream) {
  UWU_CHECK_ARG(losses && timesteps && stats, "timestep_stats_accum: null pointer");
  UWU_CHECK_ARG(totals || !loss_mean, "timestep_stats_accum: loss_mean needs totals");
  UWU_CHECK_ARG(t_dtype == UWU_I64 || t_dtype == UWU_F32, "timestep_stats_accum: timesteps must be int64 or fp32, got dtype %d", t_dtype);
  UWU_CHECK_ARG(B > 0, "timestep_stats_accum: bad batch B = %d", B);
  UWU_CHECK_ARG(n_steps >= 1 && n_steps <= 65536, "timestep_stats_accum: n_steps = %d outside 1..65536", n_steps);
  UWU_CHECK_ARG((((uintptr_t)losses | (uintptr_t)loss_mean) & 3) == 0 && ((uintptr_t)timesteps & (t_dtype == UWU_I64 ? 7 : 3)) == 0 &&
                    (((uintptr_t)stats | (uintptr_t)totals) & 7) == 0,
                "timestep_stats_accum: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  UwuProfScope prof(stream);
  const dim3 grid(cdiv(n_steps, TS_THREADS)), block(TS_THREADS);
  if (t_dtype == UWU_I64)
    hipLaunchKernelGGL(timestep_stats_kernel<int64_t>, grid, block, 0, st, losses, (const int64_t*)timesteps, loss_mean, B, n_steps, stats,
                       totals);
  else
    hipLaunchKernelGGL(timestep_stats_kernel<float>, grid, block, 0, st, losses, (const float*)timesteps, loss_mean, B, n_steps, stats,
                       totals);
  prof.done(UWU_PROF_OTHER, 0, 3.0 * B, 12.0 * B + 48.0 * n_steps);
  UWU_LAUNCH_CHECK("timestep_stats_accum");
  return UWU_OK;
}
