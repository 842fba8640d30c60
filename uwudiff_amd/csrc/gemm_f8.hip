// fp8 (OCP e4m3 / e5m2) GEMM for gfx950 on the block-scaled MFMA: BASELINE config 5 ("fp8 MFMA GEMMs"), uwu_gemm_fp8 and
// uwu_gemm_fp8_emit.  Shapes served: K % 128 == 0 with 16-byte addressable operands -- every shape that the 8-phase kernel of
// gemm_p8f.hip does not take.  The reference has no fp8 path: its Linear is nn.Linear under bf16 autocast (reference
// src/duwu/modules/rope_unet.py:122-166; the MLP that the emitting forms serve: rope_unet.py:399-411).
//
// v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales (E8M0 = 127) runs at twice the bf16 rate (MI355X_MICROARCH.md,
// Matrix cores) -- the non-scaled fp8 MFMAs only reach the bf16 rate.  ONE kernel shape serves forward, input gradient and
// weight gradient because every operand is handed over contraction-contiguous ("NT"): the quantising kernels of
// quant.hip write the transposed fp8 copies (W^T for dgrad, dY^T / X^T for wgrad) while they convert.
//   C[M,N] = alpha * A[M,K] . B[N,K]^T,  alpha = 1 / (scale_a * scale_b)  (per-tensor quantisation scales, read from
//   device memory so that delayed scaling needs no host round trip), fp32 accumulate, bf16 (or fp32 partial) out.
// Structure = gemm_big_kernel (gemm.hip): 256x256 tile, 8 waves (2 x 4 of 128 x 64), K-step = 128-byte rows = 128 fp8 = ONE MFMA
// per 16x16 output fragment and step (the bf16 kernel: two MFMAs of K = 32), two LDS-DMA stages of 64 KB, same swizzled
// image.  A lane's 32 operand bytes are 16-byte chunks fq and 4 + fq of the row -- a permutation of k applied to both
// operands alike, chosen because those are exactly the two conflict-free reads of the bf16 kernel.
// FA: element format of the A operand (0 = e4m3, 1 = e5m2: output gradients); B (weights / activations) is e4m3.
// PART: split-K partial sums (fp32) into a dense scratch [split][M][N]; splitk_reduce_kernel (gemm_wgrad.hip) adds them to C.
#include "gemm_shared.h"

namespace {

struct f8_t { unsigned char v; };
template <> struct GT<f8_t> { static constexpr int EPC = 16; static constexpr int BK = 128; };
typedef int i32x8 __attribute__((ext_vector_type(8)));

// EMIT (UWU_EPI_BIAS_GELU / UWU_EPI_DGELU): the operand the NEXT fp8 GEMMs contract over is produced here instead of by a
// quantising pass over the bf16 result (quant.hip: 4 bytes of HBM traffic per element, 0.25 ms per [49152, 4608] tensor):
//   BIAS_GELU: C = bf16 pre-activation (kept for the backward pass), q8 / q8t = e4m3(gelu(.) * q_scale)
//   DGELU:     C2 = float[N] column sums if non-null, q8 / q8t = e5m2(result * q_scale); no bf16 copy (nothing reads it)
// The 256 x 256 result tile is staged in LDS twice -- as it is and transposed (a 4 x 4 byte block sits in the dwords of four
// neighbouring lanes: four quad broadcasts + two v_perm_b32 give each lane four consecutive ROWS of one column) -- and leaves
// as whole 256-byte rows of both images.
constexpr int F8Q_PITCH = 272;  // bytes per staged row (68 dwords: the dword writes of a wave spread over all 32 banks)
constexpr int F8_EMIT_LDS = 2 * 256 * F8Q_PITCH + 2 * 256 * 4 + 64;

template <int FMT>
__device__ __forceinline__ unsigned f8_pack4(const f32x4& v, float s) {
  const float mx = FMT == 0 ? 448.f : 57344.f;
  float a = f8_sat(v[0] * s, mx), b = f8_sat(v[1] * s, mx);
  float c = f8_sat(v[2] * s, mx), d = f8_sat(v[3] * s, mx);
  int r;
  if constexpr (FMT == 0) {
    r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
  } else {
    r = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false);
    r = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, r, true);
  }
  return (unsigned)r;
}

// FULL: the tile has no row / column past M / N (a wave-uniform fact) -- the per-element masks of the ragged form (a v_cndmask per
// element and output, ~8 % of this epilogue's VALU) are compiled out.
template <int EPI, bool FULL = false>
__device__ __forceinline__ void f8_emit_epilogue(f32x4 (&acc)[8][4], const GemmArgs& g, char* smem, int m0, int n0, int tid) {
  constexpr int FMT = EPI == UWU_EPI_DGELU ? 1 : 0;
  constexpr int QP = F8Q_PITCH;
  const int lane = tid & 63, wave = tid >> 6, wm = wave >> 2, wn = wave & 3, fr = lane & 15, fq = lane >> 4;
  unsigned char* t_rm = reinterpret_cast<unsigned char*>(smem);
  unsigned char* t_tr = t_rm + 256 * QP;
  float* cs = reinterpret_cast<float*>(smem + 2 * 256 * QP);  // [2][256] column sums of the two wave rows
  float* red = cs + 512;                                      // [8] per-wave |max|
  bf16_t* C = static_cast<bf16_t*>(g.C);
  const bf16_t* aux = static_cast<const bf16_t*>(g.aux);
  float* colsum = EPI == UWU_EPI_DGELU ? reinterpret_cast<float*>(g.C2) : nullptr;
  const float qs = g.q_scale[0];
  const int m_w = m0 + wm * 128, n_w = n0 + wn * 64;
  f32x4 bias[4], csum[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n_w + 16 * j + 4 * fq;
    bias[j] = (EPI == UWU_EPI_BIAS_GELU && n < g.N) ? load4(g.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    csum[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  auto aux_row = [&](int i, uint2 (&dst)[4]) {
    const int m = m_w + 16 * i + fr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n_w + 16 * j + 4 * fq;
      // (predicated in the FULL form too: unconditional, hipcc hoisted the aux loads of all eight rows and spilled 42 registers)
      dst[j] = (m < g.M && n < g.N) ? *reinterpret_cast<const uint2*>(aux + (int64_t)m * g.ldaux + n) : uint2{0u, 0u};
    }
  };
  uint2 ar[2][4];
  if constexpr (EPI == UWU_EPI_DGELU) aux_row(0, ar[0]);
  __syncthreads();  // every wave has left the K loop: the stages are free
  const bool odd = fq & 1;
  const int kq = lane & 3;
  const unsigned sel = 0x0c0c0400u + (unsigned)kq * 0x0101u;
  float mx = 0.f;
  auto pack = [](const f32x4& v) {
    bf16x4 b = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
    return *reinterpret_cast<uint2*>(&b);
  };
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int ml = wm * 128 + 16 * i + fr, m = m0 + ml;
    const bool mok = m < g.M;
    __builtin_amdgcn_sched_barrier(0);  // (keeps the unrolled rows apart: hoisted aux loads of later rows spilled registers)
    if constexpr (EPI == UWU_EPI_DGELU)
      if (i + 1 < 8) aux_row(i + 1, ar[(i + 1) & 1]);
    f32x4 v[4], o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n_w + 16 * j + 4 * fq;
      v[j] = acc[i][j];
      if constexpr (EPI == UWU_EPI_BIAS_GELU) {
        v[j] = v[j] + bias[j];
        o[j] = gelu_tanh_f4(v[j]);
      } else {
        const bf16x4 u = *reinterpret_cast<const bf16x4*>(&ar[i & 1][j]);
        v[j] = v[j] * dgelu_tanh_f4(f32x4{(float)u[0], (float)u[1], (float)u[2], (float)u[3]});
        o[j] = v[j];
        if (FULL || (mok && n < g.N)) csum[j] = csum[j] + v[j];
      }
      if constexpr (!FULL)
        if (!(mok && n < g.N)) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) mx = fmaxf(mx, fabsf(o[j][e]));
      asm volatile("" : "+v"(mx));  // (taken now: left to the optimiser the max chain sank to the end of the tile and o[] was spilled)
      const unsigned pk = f8_pack4<FMT>(o[j], qs);
      const int nl = wn * 64 + 16 * j + 4 * fq;
      *reinterpret_cast<unsigned*>(t_rm + ml * QP + nl) = pk;
      // 4 x 4 byte transpose inside the quad of lanes that holds rows 4 (fr / 4) .. + 3 of these four columns
      // (quad broadcasts: every lane is written, so there is no "old" value to set up -- update_dpp(0, ..) cost a v_mov per DPP)
      const int pi = (int)pk;
      const unsigned d0 = (unsigned)__builtin_amdgcn_mov_dpp(pi, 0x00, 0xF, 0xF, true);
      const unsigned d1 = (unsigned)__builtin_amdgcn_mov_dpp(pi, 0x55, 0xF, 0xF, true);
      const unsigned d2 = (unsigned)__builtin_amdgcn_mov_dpp(pi, 0xAA, 0xF, 0xF, true);
      const unsigned d3 = (unsigned)__builtin_amdgcn_mov_dpp(pi, 0xFF, 0xF, 0xF, true);
      const unsigned lo = __builtin_amdgcn_perm(d1, d0, sel), hi = __builtin_amdgcn_perm(d3, d2, sel);
      *reinterpret_cast<unsigned*>(t_tr + (nl + kq) * QP + (ml & ~3)) = lo | (hi << 16);
      __builtin_amdgcn_sched_barrier(0);  // (fragment by fragment: the scheduler otherwise kept every o[] alive for the max chain and spilled)
    }
    if constexpr (EPI == UWU_EPI_BIAS_GELU) {  // bf16 pre-activation: paired 16-byte stores as epilogue_tile (8 consecutive columns per lane)
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        typedef unsigned su32x2 __attribute__((ext_vector_type(2)));
        typedef unsigned su32x4 __attribute__((ext_vector_type(4)));
        const uint2 p0 = pack(v[2 * jp]), p1 = pack(v[2 * jp + 1]);
        const su32x2 sx = __builtin_amdgcn_permlane16_swap(p0.x, p1.x, false, false);
        const su32x2 sy = __builtin_amdgcn_permlane16_swap(p0.y, p1.y, false, false);
        const int nb = n_w + 32 * jp;
        const int n = odd ? nb + 16 + 4 * (fq - 1) : nb + 4 * fq;
        if (FULL || (mok && n < g.N)) {
          const su32x4 ov = su32x4{sx[0], sy[0], sx[1], sy[1]};
          su32x4* ptr = reinterpret_cast<su32x4*>(C + (int64_t)m * g.ldc + n);
          __builtin_nontemporal_store(ov, ptr);  // read again in the backward pass only
        }
      }
    }
  }
  if (colsum) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 t = csum[j];
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = row16_sum(t[e]);
      if (fr == 0) store4(cs + wm * 256 + wn * 64 + 16 * j + 4 * fq, t);
    }
  }
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  if (colsum && tid < 256 && n0 + tid < g.N) atomicAdd(colsum + n0 + tid, cs[tid] + cs[256 + tid]);
  if (g.q_amax && tid == 0) {
    float a = red[0];
#pragma unroll
    for (int w = 1; w < 8; ++w) a = fmaxf(a, red[w]);
    // (look first: atomics on one address serialise; almost every workgroup can skip it -- quant.hip)
    const unsigned cur = __hip_atomic_load(reinterpret_cast<unsigned*>(g.q_amax), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__float_as_uint(a) > cur) atomicMax(reinterpret_cast<unsigned*>(g.q_amax), __float_as_uint(a));
  }
  // both images leave as whole rows: 16 lanes x 16 bytes = one 256-byte row per 16 threads, 32 rows per pass
  unsigned char* q8 = static_cast<unsigned char*>(g.q8);
  unsigned char* q8t = static_cast<unsigned char*>(g.q8t);
  const int r0 = tid >> 4, c16 = 16 * (tid & 15);
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int r = 32 * p + r0;
    if (q8 && m0 + r < g.M && n0 + c16 < g.N)
      *reinterpret_cast<uint4*>(q8 + (int64_t)(m0 + r) * g.ldq + n0 + c16) = *reinterpret_cast<const uint4*>(t_rm + r * QP + c16);
    if (q8t && n0 + r < g.N && m0 + c16 < g.M)
      *reinterpret_cast<uint4*>(q8t + (int64_t)(n0 + r) * g.ldqt + m0 + c16) = *reinterpret_cast<const uint4*>(t_tr + r * QP + c16);
  }
}

template <typename TC, int EPI, int FA, bool PART, bool EMIT = false>
__global__ void __launch_bounds__(512, 2) gemm_f8_kernel(const GemmArgs g, const float* __restrict__ scale_a,
                                                         const float* __restrict__ scale_b) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int STAGE = 4 * TILE_BYTES;  // A0 | A1 | W0 | W1
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int fr = lane & 15, fq = lane >> 4;
  const int nblk = g.tiles_m * g.tiles_n;
  int bid = blockIdx.x, zsl = 0;
  if constexpr (PART) {  // K slices: XCD x takes slices x, x + 8, ... (all tiles of a slice share one L2, as gemm_tr_kernel)
    const int xcd = bid & 7, loc = bid >> 3;
    zsl = xcd + 8 * (loc / nblk);
    bid = loc % nblk;
    if (zsl >= g.wide) return;  // uniform per block
  }
  int tile = bid;
  if constexpr (!PART) {  // XCD-aware tile order as in gemm_kernel
    const int xcd = bid & 7, loc = bid >> 3;
    const int q = nblk >> 3, rm = nblk & 7;
    tile = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + loc;
  }
  const int tm = tile / g.tiles_n, tn = tile - tm * g.tiles_n;
  const int m0 = tm * 256, n0 = tn * 256;
  int s_begin = 0, s_end = g.K >> 7;
  if constexpr (PART) {
    s_begin = zsl * g.k_tiles_per_split;
    if (s_begin + g.k_tiles_per_split < s_end) s_end = s_begin + g.k_tiles_per_split;
    if (s_end <= s_begin) return;  // uniform per block
  }
  const f8_t* A = static_cast<const f8_t*>(g.A);
  const f8_t* B = static_cast<const f8_t*>(g.B);
  const int half = tid >> 8, t256 = tid & 255;
  auto issue = [&](int s) {
    char* st = smem + (s & 1) * STAGE;
    glds_tile<f8_t>(A, g.lda, m0 + 128 * half, s * 128, g.M, st + half * TILE_BYTES, t256);
    glds_tile<f8_t>(B, g.ldb, n0 + 128 * half, s * 128, g.N, st + (2 + half) * TILE_BYTES, t256);
  };
  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto frag = [&](const char* base, int row) {
    const uint4 lo = lds_read128_asm(base + swz(row, fq)), hi = lds_read128_asm(base + swz(row, 4 + fq));
    return i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
  };

  issue(s_begin);
  for (int s = s_begin; s < s_end; ++s) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // stage s landed (this wave's pieces)
    __builtin_amdgcn_s_barrier();                     // ... everybody's; everybody is done reading stage s - 1
    if (s + 1 < s_end) issue(s + 1);
    const char* la = smem + (s & 1) * STAGE + wm * TILE_BYTES;
    const char* lb = smem + (s & 1) * STAGE + (2 + (wn >> 1)) * TILE_BYTES;
    i32x8 bf[4], af[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bf[j] = frag(lb, (wn & 1) * 64 + 16 * j + fr);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = frag(la, 64 * h + 16 * i + fr);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)  // swapped operands (a lane ends up with 4 consecutive columns): MFMA-A = weight fragment
          acc[4 * h + i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bf[j], af[i], acc[4 * h + i][j], 0, FA, 0,
                                                                               0x7F7F7F7F, 0, 0x7F7F7F7F);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  const float alpha = 1.f / (scale_a[0] * scale_b[0]);
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = acc[i][j] * alpha;
  if constexpr (PART) {
    float* P = static_cast<float*>(g.C2) + (int64_t)zsl * g.M * g.N;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = m0 + wm * 128 + 16 * i + fr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + 16 * j + 4 * fq;
        if (m < g.M && n < g.N) store4(P + (int64_t)m * g.N + n, acc[i][j]);
      }
    }
  } else if constexpr (EMIT) {
    // (the dGELU form keeps the masked epilogue only: a second copy of it cost that kernel 32 spilled registers)
    if (EPI == UWU_EPI_BIAS_GELU && m0 + 256 <= g.M && n0 + 256 <= g.N) f8_emit_epilogue<EPI, EPI == UWU_EPI_BIAS_GELU>(acc, g, smem, m0, n0, tid);
    else f8_emit_epilogue<EPI, false>(acc, g, smem, m0, n0, tid);
  } else {
    EpiPre<bf16_t, 8, 4> pre;
    epi_prefetch<bf16_t, 8, 4, EPI>(pre, g, m0 + wm * 128, n0 + wn * 64, fr, fq);
    epilogue_tile<bf16_t, TC, 8, 4, EPI>(acc, pre, g, m0 + wm * 128, n0 + wn * 64, fr, fq,
                                         reinterpret_cast<float*>(smem) + (wn >> 1) * 256, wm, wn & 1,
                                         wm == 0 ? (tid & 127) : 128);
  }
}

template <int EPI, int FA>
int launch_f8(GemmArgs g, const float* sa, const float* sb, hipStream_t st) {
  g.tiles_m = (g.M + 255) / 256;
  g.tiles_n = (g.N + 255) / 256;
  const GemmProf prof = {gemm_tag(g, false, false), 0, 2.0 * g.M * g.N * g.K, gemm_bytes(g, 1, 2)};
  return gemm_launch<gemm_f8_kernel<bf16_t, EPI, FA, false>>("gemm_f8", 2 * 4 * TILE_BYTES, dim3(g.tiles_m * g.tiles_n), 512, st, prof,
                                                            g, sa, sb);
}
template <int EPI, int FA>
int launch_f8_emit(GemmArgs g, const float* sa, const float* sb, hipStream_t st) {
  constexpr int LDS = F8_EMIT_LDS > 2 * 4 * TILE_BYTES ? F8_EMIT_LDS : 2 * 4 * TILE_BYTES;  // (141 KB of LDS: not every part has it)
  g.tiles_m = (g.M + 255) / 256;
  g.tiles_n = (g.N + 255) / 256;
  // bytes: operands once, the bf16 output (if any), the dGELU aux, both fp8 images
  double by = (double)g.M * g.K + (double)g.N * g.K + (double)g.M * g.N * ((g.C ? 2 : 0) + (g.aux ? 2 : 0) + (g.q8 ? 1 : 0) + (g.q8t ? 1 : 0));
  const GemmProf prof = {gemm_tag(g, false, false), 0, 2.0 * g.M * g.N * g.K, by};
  return gemm_launch<gemm_f8_kernel<bf16_t, EPI, FA, false, true>>("gemm_f8(emit)", LDS, dim3(g.tiles_m * g.tiles_n), 512, st, prof, g,
                                                                  sa, sb);
}
// number of K slices for an fp8 weight gradient: enough workgroups for ~2 rounds of the chip, >= 4 K-steps per slice
int f8_split(int tiles, int steps) {
  int split = (512 + tiles - 1) / tiles;
  split = (split + 7) / 8 * 8;
  while (split > 8 && split * 4 > steps) split -= 8;
  if (split > steps) split = steps;
  return split < 1 ? 1 : split;
}
template <int FA>
int launch_f8_part(GemmArgs g, const float* sa, const float* sb, void* scratch, hipStream_t st) {
  constexpr auto kern = gemm_f8_kernel<float, UWU_EPI_NONE, FA, true>;
  constexpr int LDS = 2 * 4 * TILE_BYTES;
  RETURN_IF(gemm_lds_optin<kern>("gemm_f8(split-K)", LDS));
  g_uwu_gemm_last_kernel.store("gemm_f8(split-K)", std::memory_order_relaxed);
  g.tiles_m = (g.M + 255) / 256;
  g.tiles_n = (g.N + 255) / 256;
  const int tiles = g.tiles_m * g.tiles_n, steps = g.K / 128;
  int split = f8_split(tiles, steps);
  g.k_tiles_per_split = (steps + split - 1) / split;
  split = (steps + g.k_tiles_per_split - 1) / g.k_tiles_per_split;
  g.wide = split;
  g.C2 = scratch;
  const int grid = 8 * tiles * ((split + 7) / 8);
  UwuProfScope prof(st);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), LDS, st, g, sa, sb);
  uwu_launch_splitk_reduce(static_cast<const float*>(scratch), static_cast<float*>(g.C), g.M, g.N, g.ldc, split, st);
  prof.done(UWU_PROF_GEMM_WGRAD, 0, 2.0 * g.M * g.N * g.K, ((double)g.M * g.K + (double)g.N * g.K) + (double)g.M * g.N * 4);
  UWU_LAUNCH_CHECK("gemm_f8(split-K)");
  return UWU_OK;
}

}  // namespace

extern "C" size_t uwu_gemm_fp8_scratch_bytes(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K < 128) return 0;
  const int tiles = ((M + 255) / 256) * ((N + 255) / 256);
  const int a = f8_split(tiles, K / 128), b = K % 128 ? 0 : uwu_gemm_p8f_split(tiles, K / 128);  // (either kernel may take it)
  return (size_t)(a > b ? a : b) * M * N * sizeof(float);
}

extern "C" int uwu_gemm_fp8(const void* A, const void* B, void* C, void* C2, const float* bias, const void* aux, int M,
                            int N, int K, int lda, int ldb, int ldc, int ldaux, int fmt_a, int epilogue,
                            const float* scale_a, const float* scale_b, void* scratch, size_t scratch_bytes,
                            void* stream) {
  UWU_CHECK_ARG(A && B && C && scale_a && scale_b, "gemm_fp8: null operand");
  UWU_CHECK_ARG(M > 0 && N > 0 && K > 0 && K % 128 == 0, "gemm_fp8: K=%d must be a positive multiple of 128", K);
  UWU_CHECK_ARG(fmt_a == UWU_FP8_E4M3 || fmt_a == UWU_FP8_E5M2, "gemm_fp8: bad operand format %d", fmt_a);
  UWU_CHECK_ARG((((uintptr_t)A | (uintptr_t)B) & 15) == 0 && lda % 16 == 0 && ldb % 16 == 0 && lda >= K && ldb >= K,
                "gemm_fp8: operands must be 16-byte aligned with leading dimensions that are multiples of 16");
  GemmArgs g{};
  g.A = A; g.B = B; g.C = C; g.C2 = C2; g.bias = bias; g.aux = aux;
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldaux = ldaux; g.epi = epilogue;
  hipStream_t st = (hipStream_t)stream;
  if (epilogue == UWU_EPI_ACCUM) {  // C fp32 += (weight gradient): split-K partial sums in `scratch`
    UWU_CHECK_ARG(N % 4 == 0 && ldc % 4 == 0 && ldc >= N && ((uintptr_t)C & 15) == 0, "gemm_fp8: ACCUM needs 16-byte rows in C");
    UWU_CHECK_ARG(scratch && ((uintptr_t)scratch & 15) == 0 && scratch_bytes >= uwu_gemm_fp8_scratch_bytes(M, N, K),
                  "gemm_fp8: ACCUM needs uwu_gemm_fp8_scratch_bytes(M, N, K) of scratch");
    if (uwu_gemm_p8f_part_ok(g)) {  // the 8-phase kernel over (K slice, tile) units, then the same reduce
      UwuProfScope prof(stream);
      RETURN_IF(uwu_launch_gemm_p8f_part(g, fmt_a == UWU_FP8_E5M2, scale_a, scale_b, scratch, st));
      uwu_launch_splitk_reduce(static_cast<const float*>(scratch), static_cast<float*>(C), M, N, ldc, g.wide, st);
      prof.done(UWU_PROF_GEMM_WGRAD, 0, 2.0 * M * N * K, ((double)M * K + (double)N * K) + (double)M * N * 4);
      UWU_LAUNCH_CHECK("gemm_p8f(split-K)");
      return UWU_OK;
    }
    return fmt_a == UWU_FP8_E5M2 ? launch_f8_part<1>(g, scale_a, scale_b, scratch, st)
                                 : launch_f8_part<0>(g, scale_a, scale_b, scratch, st);
  }
  UWU_CHECK_ARG(N % 8 == 0 && ldc % 8 == 0 && ldc >= N && ((uintptr_t)C & 15) == 0, "gemm_fp8: N and ldc must be multiples of 8");
  g.wide = 1;
  if (epilogue == UWU_EPI_BIAS || epilogue == UWU_EPI_BIAS_GELU)
    UWU_CHECK_ARG(bias && ((uintptr_t)bias & 15) == 0, "gemm_fp8: bias missing/misaligned");
  if (epilogue == UWU_EPI_BIAS_GELU) UWU_CHECK_ARG(C2 && ((uintptr_t)C2 & 15) == 0, "gemm_fp8: C2 missing/misaligned");
  if (epilogue == UWU_EPI_DGELU)
    UWU_CHECK_ARG(aux && ldaux % 4 == 0 && ldaux >= N && ((uintptr_t)aux & 7) == 0, "gemm_fp8: aux missing/misaligned");
  if (uwu_gemm_p8f_ok(g)) {
    UwuProfScope prof(stream);
    RETURN_IF(uwu_launch_gemm_p8f(g, fmt_a == UWU_FP8_E5M2, scale_a, scale_b, st));
    prof.done(gemm_tag(g, false, false), 0, 2.0 * M * N * K, gemm_bytes(g, 1, 2));
    return UWU_OK;
  }
#define F8_CASE(E)                                                                   \
  case E:                                                                            \
    return fmt_a == UWU_FP8_E5M2 ? launch_f8<E, 1>(g, scale_a, scale_b, st) : launch_f8<E, 0>(g, scale_a, scale_b, st);
  switch (epilogue) {
    F8_CASE(UWU_EPI_NONE) F8_CASE(UWU_EPI_BIAS) F8_CASE(UWU_EPI_BIAS_GELU) F8_CASE(UWU_EPI_DGELU)
  }
#undef F8_CASE
  uwu_set_error("gemm_fp8: epilogue %d not available", epilogue);
  return UWU_EINVAL;
}

extern "C" int uwu_gemm_fp8_emit(const void* A, const void* B, void* C, float* colsum, const float* bias, const void* aux,
                                 int M, int N, int K, int lda, int ldb, int ldc, int ldaux, int fmt_a, int epilogue,
                                 const float* scale_a, const float* scale_b, void* q8, int ldq, void* q8t, int ldqt,
                                 const float* q_scale, float* q_amax, void* stream) {
  UWU_CHECK_ARG(A && B && scale_a && scale_b && q_scale && (q8 || q8t), "gemm_fp8_emit: null operand");
  UWU_CHECK_ARG(epilogue == UWU_EPI_BIAS_GELU || epilogue == UWU_EPI_DGELU, "gemm_fp8_emit: epilogue %d not available", epilogue);
  UWU_CHECK_ARG(M > 0 && N > 0 && K > 0 && K % 128 == 0, "gemm_fp8_emit: K=%d must be a positive multiple of 128", K);
  UWU_CHECK_ARG(M % 16 == 0 && N % 16 == 0, "gemm_fp8_emit: M=%d and N=%d must be multiples of 16", M, N);
  UWU_CHECK_ARG(fmt_a == UWU_FP8_E4M3 || fmt_a == UWU_FP8_E5M2, "gemm_fp8_emit: bad operand format %d", fmt_a);
  UWU_CHECK_ARG((((uintptr_t)A | (uintptr_t)B) & 15) == 0 && lda % 16 == 0 && ldb % 16 == 0 && lda >= K && ldb >= K,
                "gemm_fp8_emit: operands must be 16-byte aligned with leading dimensions that are multiples of 16");
  UWU_CHECK_ARG(!C || (ldc % 8 == 0 && ldc >= N && ((uintptr_t)C & 15) == 0), "gemm_fp8_emit: C / ldc misaligned");
  UWU_CHECK_ARG(!q8 || (ldq % 16 == 0 && ldq >= N && ((uintptr_t)q8 & 15) == 0), "gemm_fp8_emit: q8 / ldq misaligned");
  UWU_CHECK_ARG(!q8t || (ldqt % 16 == 0 && ldqt >= M && ((uintptr_t)q8t & 15) == 0), "gemm_fp8_emit: q8t / ldqt misaligned");
  GemmArgs g{};
  g.A = A; g.B = B; g.C = C; g.C2 = colsum; g.bias = bias; g.aux = aux;
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldaux = ldaux; g.epi = epilogue;
  g.q8 = q8; g.q8t = q8t; g.q_scale = q_scale; g.q_amax = q_amax; g.ldq = ldq; g.ldqt = ldqt;
  g.wide = 1;
  hipStream_t st = (hipStream_t)stream;
  if (epilogue == UWU_EPI_BIAS_GELU) {
    UWU_CHECK_ARG(C && bias && ((uintptr_t)bias & 15) == 0 && !colsum, "gemm_fp8_emit: BIAS_GELU needs C (the pre-activation) and bias");
    return fmt_a == UWU_FP8_E5M2 ? launch_f8_emit<UWU_EPI_BIAS_GELU, 1>(g, scale_a, scale_b, st)
                                 : launch_f8_emit<UWU_EPI_BIAS_GELU, 0>(g, scale_a, scale_b, st);
  }
  UWU_CHECK_ARG(aux && ldaux % 4 == 0 && ldaux >= N && ((uintptr_t)aux & 7) == 0, "gemm_fp8_emit: aux missing/misaligned");
  UWU_CHECK_ARG(!C, "gemm_fp8_emit: DGELU emits fp8 only (C must be NULL)");
  return fmt_a == UWU_FP8_E5M2 ? launch_f8_emit<UWU_EPI_DGELU, 1>(g, scale_a, scale_b, st)
                               : launch_f8_emit<UWU_EPI_DGELU, 0>(g, scale_a, scale_b, st);
}
