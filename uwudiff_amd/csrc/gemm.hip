// MFMA GEMM for gfx950: C[M,N] = opA(A) . opB(B) (+ epilogue), fp32 accumulate.
//
// One kernel template serves the three contractions of every Linear in the denoiser:
//   forward  Y  = X  . W^T          (transA=0, transB=0)   K-contiguous operands
//   dgrad    dX = dY . W            (transA=0, transB=1)   W is [red][out]   -> transposed staging of B
//   wgrad    dW = dY^T . X          (transA=1, transB=1)   both [red][out]   -> transposed staging of A and B
// and both operand types: bf16 (v_mfma_f32_16x16x32_bf16) and exact fp32 (v_mfma_f32_16x16x4_f32, the
// parity mode).  Reference op sequence replaced: nn.Linear fwd/bwd inside diffusers blocks
// (reference src/duwu/modules/rope_unet.py:122-166, 404).
//
// Tiling: 128x128 output tile per 256-thread workgroup (4 waves, 2x2, 64x64 per wave = 4x4 MFMA 16x16 tiles),
// K step = 128 bytes per row (64 bf16 / 32 fp32), LDS double-buffered (2 x 32 KB -> 2 workgroups per CU).
// LDS image: [row][128 B], 16-B chunk c of row r stored at chunk (c ^ (r>>1) ^ (r>>4)) & 7:
//   * fragment reads (ds_read_b128, lane -> row, fixed chunk) are bank-conflict free,
//   * row-major staging writes (8 lanes x 16 B per row) are conflict free,
//   * transposed staging writes (ds_write_b64 bf16 / ds_write_b128 fp32) are <= 2-way.
// The fp32 path reuses the same image: lane group g=lane>>4 reads chunk 4*kk+g and feeds element e of it to
// the e-th 16x16x4 MFMA, i.e. a k-permutation applied identically to A and B.
// Global->LDS goes through registers (prefetch of tile t+1 issued before the MFMAs of tile t); K-strided
// operands are transposed in registers (4x8 bf16 / 4x4 fp32 blocks) so HBM reads stay 16 B/lane coalesced.
//
// This file holds that kernel (every shape, type and transpose: what no faster kernel takes ends here), the LDS-DMA kernels
// for bf16 operands with A K-contiguous that grew out of it (gemm_r3_kernel 256x128 / 128x128 ring and its implicit-GEMM 3x3
// convolution forms, gemm_big_kernel 256x256, gemm_wide_kernel 192x384, gemm_m64_kernel 64x128), uwu_gemm and dispatch_trans,
// which hands a shape to the first kernel whose rule accepts it.  These kernels share one translation unit because they
// share the force-inlined pieces of gemm_shared.h instantiation by instantiation (glds_tile, the transposing-read helpers,
// epilogue_tile): hipcc's interprocedural passes run over those helpers before they are inlined, so the machine code of a
// kernel depends on which other callers its translation unit holds.  Other kernel families live in files of their own and are
// reached through the host functions declared in gemm_shared.h:
//   gemm_as.hip     A-stationary kernel for K = 384
//   gemm_wgrad.hip  streaming weight-gradient kernels (both operands K-major), the split-K reduce, uwu_gemm_wgrad
//   gemm_f8.hip     fp8 operands (uwu_gemm_fp8, uwu_gemm_fp8_emit)
//   gemm_p8.hip, gemm_p8n.hip, gemm_p8f.hip   the 8-phase kernels
#include "gemm_shared.h"

namespace {

// ACC = atomic-accumulate epilogue (standard accumulator orientation: registers walk rows, lanes walk
// 16 consecutive columns -> 64-B atomic segments).  Otherwise the MFMA operands are swapped so that each lane
// owns 4 consecutive columns of one row and can apply the epilogue on / store 8-16 B vectors directly.
// GL = LDS-DMA staging (only with TA = TB = false and full K tiles).
template <typename T, typename TC, bool TA, bool TB, bool ACC, bool GL = false, int EPI = -1>
__global__ void __launch_bounds__(256, 2) gemm_kernel(const GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BK = GT<T>::BK;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // XCD-aware tile order: blocks b and b+8 share an XCD (round-robin dispatch), so give every XCD a
  // contiguous run of tile ids (n fastest) -> the n-tiles of one A row-panel hit the same L2.
  const int nblk = g.tiles_m * g.tiles_n;
  int tile;
  {
    const int bid = blockIdx.x, xcd = bid & 7, loc = bid >> 3;
    const int q = nblk >> 3, rm = nblk & 7;
    tile = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + loc;
  }
  const int tm = tile / g.tiles_n, tn = tile - tm * g.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  const int ktiles = (g.K + BK - 1) / BK;
  const int kt_begin = blockIdx.z * g.k_tiles_per_split;
  int kt_end = kt_begin + g.k_tiles_per_split;
  if (kt_end > ktiles) kt_end = ktiles;
  if (kt_begin >= kt_end) return;  // uniform per block

  const T* A = static_cast<const T*>(g.A);
  const T* B = static_cast<const T*>(g.B);

  Stager<T, TA> sa;
  Stager<T, TB> sb;
  EpiPre<T, 4, 4> pre;
  // (compile-time epilogues only: the run-time variants would hold bias AND aux registers through the K loop)
  if constexpr (!ACC && EPI >= 0) epi_prefetch<T, 4, 4, EPI>(pre, g, m0 + wm * 64, n0 + wn * 64, lane & 15, lane >> 4);
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if constexpr (GL) {
    glds_tile<T>(A, g.lda, m0, kt_begin * BK, g.M, smem, tid);
    glds_tile<T>(B, g.ldb, n0, kt_begin * BK, g.N, smem + TILE_BYTES, tid);
  } else {
    sa.load(A, g.lda, m0, kt_begin * BK, g.M, g.K, tid);
    sb.load(B, g.ldb, n0, kt_begin * BK, g.N, g.K, tid);
    sa.store(smem, tid);
    sb.store(smem + TILE_BYTES, tid);
  }
  __syncthreads();

  const int fr = lane & 15, fq = lane >> 4;
  for (int kt = kt_begin; kt < kt_end; ++kt) {
    const int cur = (kt - kt_begin) & 1;
    const char* la = smem + cur * 2 * TILE_BYTES;
    const char* lb = la + TILE_BYTES;
    const bool more = (kt + 1 < kt_end);
    if (more) {
      if constexpr (GL) {  // DMA the next tile straight into the other stage (free since the last barrier)
        char* na = smem + (cur ^ 1) * 2 * TILE_BYTES;
        glds_tile<T>(A, g.lda, m0, (kt + 1) * BK, g.M, na, tid);
        glds_tile<T>(B, g.ldb, n0, (kt + 1) * BK, g.N, na + TILE_BYTES, tid);
      } else {  // prefetch next tile into registers; latency hides under the MFMAs below
        sa.load(A, g.lda, m0, (kt + 1) * BK, g.M, g.K, tid);
        sb.load(B, g.ldb, n0, (kt + 1) * BK, g.N, g.K, tid);
      }
    }
    if constexpr (GL) {
      // both k-halves' fragments up front (two register sets); the MFMAs of half 0 run under the reads of half 1
      uint4 af[2][4], bf[2][4];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int i = 0; i < 4; ++i) af[kk][i] = lds_read128_asm(la + swz(wm * 64 + 16 * i + fr, 4 * kk + fq));
#pragma unroll
        for (int j = 0; j < 4; ++j) bf[kk][j] = lds_read128_asm(lb + swz(wn * 64 + 16 * j + fr, 4 * kk + fq));
        if (kk == 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) mma_frag<T>(bf[0][j], af[0][i], acc[i][j]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) mma_frag<T>(bf[1][j], af[1][i], acc[i][j]);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next stage has landed (this wave's pieces)
      __builtin_amdgcn_s_barrier();                     // ... everybody's; and everybody is done reading `cur`
      continue;
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      uint4 af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        af[i] = *reinterpret_cast<const uint4*>(la + swz(wm * 64 + 16 * i + fr, 4 * kk + fq));
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bf[j] = *reinterpret_cast<const uint4*>(lb + swz(wn * 64 + 16 * j + fr, 4 * kk + fq));
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if constexpr (ACC)
            mma_frag<T>(af[i], bf[j], acc[i][j]);
          else
            mma_frag<T>(bf[j], af[i], acc[i][j]);
        }
    }
    if constexpr (!GL) {
      if (more) {
        char* na = smem + (cur ^ 1) * 2 * TILE_BYTES;
        sa.store(na, tid);
        sb.store(na + TILE_BYTES, tid);
      }
    }
    __syncthreads();  // with LDS-DMA outstanding hipcc drains vmcnt(0) here: the next stage is complete
  }

  // ---------------------------------------------------------------- epilogue
  if constexpr (ACC) {
    float* C = static_cast<float*>(g.C);
    const bool alone = gridDim.z == 1;  // one K slice: this workgroup is the tile's only writer -> plain read-add-write
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + 16 * j + fr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + wm * 64 + 16 * i + 4 * fq + r;
          if (m < g.M && n < g.N) {
            float* c = C + (int64_t)m * g.ldc + n;
            if (alone) *c += acc[i][j][r];
            else atomicAdd(c, acc[i][j][r]);
          }
        }
      }
  } else {
    if constexpr (EPI < 0) epi_prefetch<T, 4, 4, EPI>(pre, g, m0 + wm * 64, n0 + wn * 64, fr, fq);
    epilogue_tile<T, TC, 4, 4, EPI>(acc, pre, g, m0 + wm * 64, n0 + wn * 64, fr, fq, reinterpret_cast<float*>(smem), wm, wn);
  }
}

// ---- ring kernel for the token-parallel Linears: forward (B = W [N,K]) and input gradient (B = W [K,N]) ---------
// PMC on the 128x128 kernel (65536x1152x384): the L2 -> LDS intake (903 MB per launch at ~12 TB/s chip-wide) is the
// longest phase and the waves are parked 46 % of their cycles on the 2-stage pipeline; its input-gradient path stages
// the K-major weight through registers (v_perm + ds_write_b64: 20 % LDS conflicts, 5x more VALU than MFMA
// instructions).  Same two-workgroups-per-CU structure (independent barriers: one workgroup's MFMAs run under the
// other's waits, and tile ends / store bursts stagger by themselves), but:
//   * K-step 32, everything staged by LDS-DMA into a ring (counted vmcnt waits, one barrier per K-step, fragment
//     reads as inline asm, see lds_read128_asm): FI = 8 -> 256x128 tile (85 flop per L2 byte instead of 64), 3 stages
//     of 24 KB; FI = 4 -> 128x128 tile, 4 stages of 16 KB;
//   * A (activations / output gradients, K-contiguous): image [rows][64 B], 16-byte chunk c of row r at position
//     c ^ G[(r>>2)&3], G = {0,3,2,1} (conflict-free in the four ds_read_b128 lane groups); the DMA writes lane-linear,
//     so the swizzle is applied to the per-lane source address;
//   * B: TB = 0 the same image (weight rows are K-contiguous); TB = 1 the K-major weight goes to LDS untouched as a
//     [32 k][128 n] sub-image and the fragments are gathered by ds_read_b64_tr_b16 (layout: gemm_tr_kernel, gemm_wgrad.hip).

// CONV (implicit-GEMM 3x3 convolution, channels-last, padding 1; no im2col matrix in HBM): the A rows are gathered --
// LDS-DMA takes a per-lane source address, so a K-step of a tap reads the tile's pixels shifted by that tap and the
// zero page where the tap falls outside the image.  K runs channel-chunk-major, tap-minor: the nine taps of a 32-channel
// chunk re-read the same few KB of activations (L1 / L2 hits) before the next chunk is touched.
//   CONV = 1 forward:  Y[(b,oy,ox), co] = sum_{tap,c} X[b, oy s + ky - 1, ox s + kx - 1, c] W[co][tap][c]   (TB = 0)
//   CONV = 2 dgrad:    dX[(b,iy,ix), c] = sum_{tap,co} dY[b, (iy + 1 - ky) / s, (ix + 1 - kx) / s, co] W[co][tap][c]
//                      (TB = 1: for a fixed tap the weight is a [co][c] matrix with row stride 9 C)
//   CONV = 3 forward, stride 2, padded right and bottom only (the AutoencoderKL encoder's downsampler):
//                      Y[(b,oy,ox), co] = sum_{tap,c} X[b, 2 oy + ky, 2 ox + kx, c] W[co][tap][c], zero where the index reaches H or W
template <typename TC, int EPI, bool TB, int FI, int CONV = 0>
__global__ void __launch_bounds__(256, 2) gemm_r3_kernel(const GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef bf16_t T;
  static_assert(FI == 8 || FI == 4, "256x128 or 128x128");
  constexpr int RBM = 32 * FI, RBN = 128;
  constexpr int A_BYTES = RBM * R_ROWB, STAGE = A_BYTES + R_BSUB;
  constexpr int NST = FI == 8 ? 3 : 4;
  constexpr int QA = FI / 2, PS = QA + 2;  // DMA instructions per wave per K-step: A pieces + 2 B pieces
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int nblk = g.tiles_m * g.tiles_n;
  int tile;
  {  // XCD-aware tile order as in gemm_kernel
    const int bid = blockIdx.x, xcd = bid & 7, loc = bid >> 3;
    const int q = nblk >> 3, rm = nblk & 7;
    tile = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + loc;
  }
  const int tm = tile / g.tiles_n, tn = tile - tm * g.tiles_n;
  const int m0 = tm * RBM, n0 = tn * RBN;
  const int nk = g.K >> 5;

  // per-lane DMA sources (rows / columns past the operand are clamped: their products are never stored)
  const int prow = lane >> 2;
  const int csrc = ((lane & 3) ^ r_gsw(prow)) & 3;  // logical chunk that must land at position lane & 3
  const T* pa[QA];
  const T* pb[2];
  int cy[QA], cx[QA];  // CONV: row -> (image base folded into pa, y, x) of the output (1) / input (2) pixel
  const T* const zsrc = static_cast<const T*>(g.zero) + 8 * 0;
#pragma unroll
  for (int q = 0; q < QA; ++q) {
    int row = m0 + 16 * (wave + 4 * q) + prow;
    if constexpr (CONV == 0) {
      if (row >= g.M) row = g.M - 1;
      pa[q] = static_cast<const T*>(g.A) + (int64_t)row * g.lda + 8 * csrc;
    } else {
      // rows of this GEMM = pixels of the (CONV 1: output, CONV 2: input) image; the gathered tensor is the other one
      const int RH = CONV != 2 ? g.cHo : g.cH, RW = CONV != 2 ? g.cWo : g.cW;  // row image
      const int GH = CONV != 2 ? g.cH : g.cHo, GW = CONV != 2 ? g.cW : g.cWo;  // gathered image
      int b, rem, y, x;
      divmod24(row < g.M ? row : 0, RH * RW, 1.f / (float)(RH * RW), b, rem);
      divmod24(rem, RW, 1.f / (float)RW, y, x);
      if (row >= g.M) y = -100000;  // every tap out of range -> zero rows
      cy[q] = y;
      cx[q] = x;
      pa[q] = static_cast<const T*>(g.A) + (int64_t)b * GH * GW * g.lda + 8 * csrc;
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    if constexpr (!TB) {
      int row = n0 + 16 * (wave + 4 * q) + prow;
      if (row >= g.N) row = g.N - 1;
      pb[q] = static_cast<const T*>(g.B) + (int64_t)row * g.ldb + 8 * csrc;
    } else {  // piece P = wave + 4 q: k-rows 4 P .. 4 P + 3 of the sub-image, 256 B each
      const int drow = lane >> 4;
      const int dchunk = (lane & 15) ^ (((drow & 3) << 2) | (wave & 3));  // (P & 3) == (wave & 3)
      int x = n0 + 8 * dchunk;
      if (x > g.N - 8) x = g.N - 8;
      pb[q] = static_cast<const T*>(g.B) + (int64_t)(4 * (wave + 4 * q) + drow) * g.ldb + x;
    }
  }
  const int64_t bstep = TB ? (int64_t)32 * g.ldb : 32;
  auto issue = [&](int s) {
    char* st = smem + (s % NST) * STAGE + wave * 1024;
    int64_t boff = s * bstep;
    if constexpr (CONV != 0) {
      const int ch = s / 9, tap = s - 9 * ch, ky = tap / 3, kx = tap - 3 * ky;  // wave-uniform
      // weight: [co][tap][c].  forward (TB = 0): row co, columns tap C + 32 ch;  dgrad (TB = 1): rows 32 ch .. of the
      // [co][c] matrix of this tap (row stride ldb = 9 C)
      boff = TB ? (int64_t)32 * ch * g.ldb + tap * g.cC : (int64_t)tap * g.cC + 32 * ch;
#pragma unroll
      for (int q = 0; q < QA; ++q) {
        int gy, gx;
        bool ok;
        if constexpr (CONV == 1) {
          gy = cy[q] * g.cS + ky - 1;
          gx = cx[q] * g.cS + kx - 1;
          ok = gy >= 0 && gy < g.cH && gx >= 0 && gx < g.cW;
        } else if constexpr (CONV == 3) {
          gy = cy[q] * 2 + ky;
          gx = cx[q] * 2 + kx;
          ok = gy >= 0 && gy < g.cH && gx < g.cW;  // (gy < 0: a row past M)
        } else {
          const int ty = cy[q] + 1 - ky, tx = cx[q] + 1 - kx;
          ok = ty >= 0 && tx >= 0;
          if (g.cS == 2) {
            ok = ok && !((ty | tx) & 1);
            gy = ty >> 1;
            gx = tx >> 1;
          } else {
            gy = ty;
            gx = tx;
          }
          ok = ok && gy < g.cHo && gx < g.cWo;
        }
        const int GW = CONV != 2 ? g.cW : g.cWo;
        const T* src = ok ? pa[q] + (int64_t)(gy * GW + gx) * g.lda + 32 * ch : zsrc;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(st + q * 4096), 16, 0, 0);
      }
    } else {
#pragma unroll
      for (int q = 0; q < QA; ++q)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pa[q] + s * 32),
                                         (__attribute__((address_space(3))) void*)(st + q * 4096), 16, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pb[q] + boff),
                                       (__attribute__((address_space(3))) void*)(st + A_BYTES + q * 4096), 16, 0, 0);
  };

  f32x4 acc[FI][4];
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  EpiPre<T, FI, 4> pre;
  if constexpr (EPI >= 0) epi_prefetch<T, FI, 4, EPI>(pre, g, m0 + wm * 16 * FI, n0 + wn * 64, fr, fq);

  const unsigned smem_base = (unsigned)(size_t)((const __attribute__((address_space(3))) char*)smem);
  const unsigned a_off = (unsigned)r_swz(wm * 16 * FI + fr, fq);
  const unsigned b_off = (unsigned)(A_BYTES + r_swz(wn * 64 + fr, fq));                     // TB = 0
  const unsigned b_t0 = A_BYTES + tr_lane_base(lane, 0, 8 * wn), b_t1 = A_BYTES + tr_lane_base(lane, 1, 8 * wn);  // TB = 1

  issue(0);
  if (nk > 1) issue(1);
  if (NST > 3 && nk > 2) issue(2);
  for (int s = 0; s < nk; ++s) {
    // K-step s has landed (this wave's pieces); the younger operations are the pieces of the steps issued after it
    const int ahead = nk - 1 - s < NST - 2 ? nk - 1 - s : NST - 2;
    if (ahead >= 2) r_wait_vm<2 * PS>();
    else if (ahead == 1) r_wait_vm<PS>();
    else r_wait_vm<0>();
    __builtin_amdgcn_s_barrier();              // ... everybody's; and everybody is done reading stage (s-1) % NST
    if (s + NST - 1 < nk) issue(s + NST - 1);  // -> stage (s-1) % NST
    const unsigned sb0 = smem_base + (unsigned)((s % NST) * STAGE);
    uint4 bf[4], af[FI];
    if constexpr (!TB) {
      bf[0] = r_read128<0>(sb0 + b_off);
      bf[1] = r_read128<1024>(sb0 + b_off);
      bf[2] = r_read128<2048>(sb0 + b_off);
      bf[3] = r_read128<3072>(sb0 + b_off);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint2 lo = t_read_tr<0>(sb0 + (b_t0 ^ (unsigned)(j << 5)));
        const uint2 hi = t_read_tr<0>(sb0 + (b_t1 ^ (unsigned)(j << 5)));
        bf[j] = uint4{lo.x, lo.y, hi.x, hi.y};
      }
    }
    const unsigned sa = sb0 + a_off;
    af[0] = r_read128<0>(sa);
    af[1] = r_read128<1024>(sa);
    af[2] = r_read128<2048>(sa);
    af[3] = r_read128<3072>(sa);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if constexpr (FI == 8) {
      af[4] = r_read128<4096>(sa);
      af[5] = r_read128<5120>(sa);
      af[6] = r_read128<6144>(sa);
      af[7] = r_read128<7168>(sa);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) mma_frag<T>(bf[j], af[i], acc[i][j]);
    if constexpr (FI == 8) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 4; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) mma_frag<T>(bf[j], af[i], acc[i][j]);
    }
  }
  if constexpr (EPI < 0) epi_prefetch<T, FI, 4, EPI>(pre, g, m0 + wm * 16 * FI, n0 + wn * 64, fr, fq);
  epilogue_tile<T, TC, FI, 4, EPI>(acc, pre, g, m0 + wm * 16 * FI, n0 + wn * 64, fr, fq, reinterpret_cast<float*>(smem),
                                   wm, wn);
}

// ---- 256x256 tile, one 8-wave workgroup per CU: 128 flop per L2 -> LDS byte (the 256x128 ring: 85) -----------------
// Not persistent on purpose: a persistent variant with the next tile's first stage in flight under the epilogue was
// 20 % SLOWER (vmcnt also counts the epilogue's stores, and the CUs' store bursts line up); as separate workgroups
// the tiles drift apart by themselves.
// A [M,K] K-contiguous, K-step 64 (128-byte rows: whole cache lines per DMA row), two stages of 64 KB.
// Waves 2 (M) x 4 (N): each 128 x 64 (FI = 8, FJ = 4).  A and (TB = 0) W [N,K]: the 128-row sub-tiles of gemm_kernel's
// LDS-DMA path (glds_tile / swz), A sub-tile = wm, W sub-tile = wn >> 1.  TB = 1 (input gradients, W [K,N]): four
// [32 k][128 n] sub-images per stage (k-half, n-half) read by ds_read_b64_tr_b16 exactly as in gemm_r3_kernel.
template <typename TC, int EPI, bool TB>
__global__ void __launch_bounds__(512, 2) gemm_big_kernel(const GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef bf16_t T;
  constexpr int STAGE = 4 * TILE_BYTES;  // A0 | A1 | W0 | W1
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int fr = lane & 15, fq = lane >> 4;
  const int nblk = g.tiles_m * g.tiles_n;
  int tile;
  {  // XCD-aware tile order as in gemm_kernel
    const int bid = blockIdx.x, xcd = bid & 7, loc = bid >> 3;
    const int q = nblk >> 3, rm = nblk & 7;
    tile = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + loc;
  }
  const int tm = tile / g.tiles_n, tn = tile - tm * g.tiles_n;
  const int m0 = tm * 256, n0 = tn * 256;
  const int nk = g.K >> 6;
  const T* A = static_cast<const T*>(g.A);
  const T* B = static_cast<const T*>(g.B);
  const int half = tid >> 8, t256 = tid & 255;
  // TB = 1: this wave moves piece P = wave (k-rows 4P .. 4P+3, 256 B each) of each of the four sub-images
  const T* pbt[2] = {nullptr, nullptr};
  if constexpr (TB) {
    const int drow = lane >> 4;
    const int dchunk = (lane & 15) ^ (((drow & 3) << 2) | (wave & 3));
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
      int x = n0 + 128 * nh + 8 * dchunk;
      if (x > g.N - 8) x = g.N - 8;
      pbt[nh] = B + (int64_t)(4 * wave + drow) * g.ldb + x;
    }
  }
  auto issue = [&](int s) {
    char* st = smem + (s & 1) * STAGE;
    glds_tile<T>(A, g.lda, m0 + 128 * half, s * 64, g.M, st + half * TILE_BYTES, t256);
    if constexpr (!TB) {
      glds_tile<T>(B, g.ldb, n0 + 128 * half, s * 64, g.N, st + (2 + half) * TILE_BYTES, t256);
    } else {
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int nh = 0; nh < 2; ++nh)
          __builtin_amdgcn_global_load_lds(
              (const __attribute__((address_space(1))) void*)(pbt[nh] + (int64_t)(64 * s + 32 * kh) * g.ldb),
              (__attribute__((address_space(3))) void*)(st + 2 * TILE_BYTES + (2 * kh + nh) * R_BSUB + wave * 1024), 16,
              0, 0);
    }
  };
  const unsigned smem_base = (unsigned)(size_t)((const __attribute__((address_space(3))) char*)smem);
  const unsigned b_t0 = tr_lane_base(lane, 0, 8 * (wn & 1)), b_t1 = tr_lane_base(lane, 1, 8 * (wn & 1));
  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  issue(0);
  for (int s = 0; s < nk; ++s) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // stage s landed (this wave's pieces)
    __builtin_amdgcn_s_barrier();                     // ... everybody's; everybody is done reading stage s - 1
    if (s + 1 < nk) issue(s + 1);
    const char* la = smem + (s & 1) * STAGE + wm * TILE_BYTES;
    const char* lb = smem + (s & 1) * STAGE + (2 + (wn >> 1)) * TILE_BYTES;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      uint4 bf[4], af[8];
      if constexpr (!TB) {
#pragma unroll
        for (int j = 0; j < 4; ++j) bf[j] = lds_read128_asm(lb + swz((wn & 1) * 64 + 16 * j + fr, 4 * kk + fq));
      } else {
        const unsigned sub = smem_base + (unsigned)((s & 1) * STAGE + 2 * TILE_BYTES + (2 * kk + (wn >> 1)) * R_BSUB);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint2 lo = t_read_tr<0>(sub + (b_t0 ^ (unsigned)(j << 5)));
          const uint2 hi = t_read_tr<0>(sub + (b_t1 ^ (unsigned)(j << 5)));
          bf[j] = uint4{lo.x, lo.y, hi.x, hi.y};
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = lds_read128_asm(la + swz(16 * i + fr, 4 * kk + fq));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int i = 4; i < 8; ++i) af[i] = lds_read128_asm(la + swz(16 * i + fr, 4 * kk + fq));
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) mma_frag<T>(bf[j], af[i], acc[i][j]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 4; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) mma_frag<T>(bf[j], af[i], acc[i][j]);
    }
  }
  // (epilogue inputs are fetched here, not before the K loop: the accumulators leave no registers to hold them)
  EpiPre<T, 8, 4> pre;
  epi_prefetch<T, 8, 4, EPI>(pre, g, m0 + wm * 128, n0 + wn * 64, fr, fq);
  // dGELU column sums: two column groups of 128 (wn >> 1), each folded by its 2 x 2 waves; waves 0-3 flush
  epilogue_tile<T, TC, 8, 4, EPI>(acc, pre, g, m0 + wm * 128, n0 + wn * 64, fr, fq,
                                  reinterpret_cast<float*>(smem) + (wn >> 1) * 256, wm, wn & 1, wm == 0 ? (tid & 127) : 128);
}

// ---- 192x384 tile, 8 waves (2 x 4 of 96 x 96: FI = FJ = 6): the N = 384 / 1152 Linears ---------------------------
// With N = 384 the 256x128 ring reads every A row-panel three times (once per column tile); this tile covers the whole
// width, so A crosses L2 -> LDS once (128 flop per byte, as the 256x256 kernel, without its column padding).
// Same structure as gemm_big_kernel: K-step 64 (128-byte rows), two stages of 72 KB, one workgroup per CU.
// Images: A 192 rows | W 384 rows (TB = 0, swz) or 2 x 3 sub-images [32 k][128 n] (TB = 1, transposing reads).
template <typename TC, int EPI, bool TB>
__global__ void __launch_bounds__(512, 2) gemm_wide_kernel(const GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef bf16_t T;
  constexpr int FI = 6, FJ = 6, BMR = 192, BNC = 384;
  constexpr int A_BYTES = BMR * ROW_BYTES, STAGE = (BMR + BNC) * ROW_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int fr = lane & 15, fq = lane >> 4;
  const int nblk = g.tiles_m * g.tiles_n;
  int tile;
  {  // XCD-aware tile order as in gemm_kernel
    const int bid = blockIdx.x, xcd = bid & 7, loc = bid >> 3;
    const int q = nblk >> 3, rm = nblk & 7;
    tile = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + loc;
  }
  const int tm = tile / g.tiles_n, tn = tile - tm * g.tiles_n;
  const int m0 = tm * BMR, n0 = tn * BNC;
  const int nk = g.K >> 6;
  const T* A = static_cast<const T*>(g.A);
  const T* B = static_cast<const T*>(g.B);

  // per-lane DMA sources; piece p = wave + 8 q is rows 8p .. 8p+7 of an image (lane: row lane>>3, 16-byte slot lane&7
  // receives the logical chunk the swizzle assigns to that slot).  Rows past the operand are clamped.
  const T* pa[3];
  const T* pb[6];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int row = 8 * (wave + 8 * q) + (lane >> 3);
    const int c = ((lane & 7) ^ (row >> 1) ^ (row >> 4)) & 7;
    int grow = m0 + row;
    if (grow >= g.M) grow = g.M - 1;
    pa[q] = A + (int64_t)grow * g.lda + 8 * c;
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    if constexpr (!TB) {
      const int row = 8 * (wave + 8 * q) + (lane >> 3);
      const int c = ((lane & 7) ^ (row >> 1) ^ (row >> 4)) & 7;
      int grow = n0 + row;
      if (grow >= g.N) grow = g.N - 1;
      pb[q] = B + (int64_t)grow * g.ldb + 8 * c;
    } else {  // q = 3 kh + nh: piece P = wave (k-rows 4P .. 4P+3) of sub-image (kh, nh)
      const int kh = q / 3, nh = q - 3 * kh;
      const int drow = lane >> 4;
      const int dchunk = (lane & 15) ^ (((drow & 3) << 2) | (wave & 3));
      int x = n0 + 128 * nh + 8 * dchunk;
      if (x > g.N - 8) x = g.N - 8;
      pb[q] = B + (int64_t)(32 * kh + 4 * wave + drow) * g.ldb + x;
    }
  }
  // N = 384: this workgroup is the only reader of its A rows -> streaming (nt) DMA, so that the once-read activation does
  // not displace what the neighbouring launches re-read (per-kernel time unchanged, whole step +1.4 % on the same box)
  const bool a_once = g.tiles_n == 1;
  auto issue = [&](int s) {
    char* st = smem + (s & 1) * STAGE;
    if (a_once) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pa[q] + 64 * s),
                                         (__attribute__((address_space(3))) void*)(st + (wave + 8 * q) * 1024), 16, 0, 2);
    } else {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pa[q] + 64 * s),
                                         (__attribute__((address_space(3))) void*)(st + (wave + 8 * q) * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      if constexpr (!TB)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pb[q] + 64 * s),
                                         (__attribute__((address_space(3))) void*)(st + A_BYTES + (wave + 8 * q) * 1024),
                                         16, 0, 0);
      else
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pb[q] + (int64_t)(64 * s) * g.ldb),
                                         (__attribute__((address_space(3))) void*)(st + A_BYTES + q * R_BSUB + wave * 1024),
                                         16, 0, 0);
    }
  };
  const unsigned smem_base = (unsigned)(size_t)((const __attribute__((address_space(3))) char*)smem);
  // TB = 1: fragment j starts at column 96 wn + 16 j: sub-image (col >> 7), first 8-column chunk (col & 127) >> 3
  unsigned tb0[FJ], tb1[FJ];
  if constexpr (TB) {
#pragma unroll
    for (int j = 0; j < FJ; ++j) {
      const int col = 96 * wn + 16 * j;
      tb0[j] = A_BYTES + (col >> 7) * R_BSUB + tr_lane_base(lane, 0, (col & 127) >> 3);
      tb1[j] = A_BYTES + (col >> 7) * R_BSUB + tr_lane_base(lane, 1, (col & 127) >> 3);
    }
  }
  f32x4 acc[FI][FJ];
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int j = 0; j < FJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  issue(0);
  for (int s = 0; s < nk; ++s) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // stage s landed (this wave's pieces)
    __builtin_amdgcn_s_barrier();                     // ... everybody's; everybody is done reading stage s - 1
    if (s + 1 < nk) issue(s + 1);
    const char* la = smem + (s & 1) * STAGE;
    const char* lb = la + A_BYTES;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      uint4 bf[FJ], af[FI];
      if constexpr (!TB) {
#pragma unroll
        for (int j = 0; j < FJ; ++j) bf[j] = lds_read128_asm(lb + swz(96 * wn + 16 * j + fr, 4 * kk + fq));
      } else {
        const unsigned sb = smem_base + (unsigned)((s & 1) * STAGE + kk * 3 * R_BSUB);
#pragma unroll
        for (int j = 0; j < FJ; ++j) {
          const uint2 lo = t_read_tr<0>(sb + tb0[j]);
          const uint2 hi = t_read_tr<0>(sb + tb1[j]);
          bf[j] = uint4{lo.x, lo.y, hi.x, hi.y};
        }
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) af[i] = lds_read128_asm(la + swz(96 * wm + 16 * i + fr, 4 * kk + fq));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int i = 3; i < FI; ++i) af[i] = lds_read128_asm(la + swz(96 * wm + 16 * i + fr, 4 * kk + fq));
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) mma_frag<T>(bf[j], af[i], acc[i][j]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 3; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) mma_frag<T>(bf[j], af[i], acc[i][j]);
    }
  }
  EpiPre<T, FI, FJ> pre;
  epi_prefetch<T, FI, FJ, EPI>(pre, g, m0 + wm * 96, n0 + wn * 96, fr, fq);
  epilogue_tile<T, TC, FI, FJ, EPI>(acc, pre, g, m0 + wm * 96, n0 + wn * 96, fr, fq, nullptr, wm, wn & 1);
}

// ---- 64x128 tile for small token counts (a 128x128 grid that would leave most CUs idle) ---------------------------
// Per-GPU batch 16 (the reference yaml) is M = 4096 rows: 32 x 3 = 96 tiles of 128x128 for an N = 384 Linear on 256
// CUs.  Half-height tiles double the workgroups; 4 waves of 32 x 64 (FI = 2, FJ = 4), K-step 64, three LDS-DMA stages of
// 24 KB.  Operand images as in gemm_kernel's LDS-DMA path (TB = 0) / gemm_r3_kernel's transposing reads (TB = 1).
constexpr int M64_NST = 3;
template <typename TC, int EPI, bool TB>
__global__ void __launch_bounds__(256, 2) gemm_m64_kernel(const GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef bf16_t T;
  constexpr int A_BYTES = 64 * ROW_BYTES, STAGE = A_BYTES + TILE_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int nblk = g.tiles_m * g.tiles_n;
  int tile;
  {  // XCD-aware tile order as in gemm_kernel
    const int bid = blockIdx.x, xcd = bid & 7, loc = bid >> 3;
    const int q = nblk >> 3, rm = nblk & 7;
    tile = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + loc;
  }
  const int tm = tile / g.tiles_n, tn = tile - tm * g.tiles_n;
  const int m0 = tm * 64, n0 = tn * 128;
  const int nk = g.K >> 6;
  const T* A = static_cast<const T*>(g.A);
  const T* B = static_cast<const T*>(g.B);
  // A: pieces p = wave + 4 q (rows 8p .. 8p+7); TB = 1: piece P = wave + 4 q of the k-half sub-images
  const T* pa[2];
  const T* pbt[2] = {nullptr, nullptr};
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int row = 8 * (wave + 4 * q) + (lane >> 3);
    const int c = ((lane & 7) ^ (row >> 1) ^ (row >> 4)) & 7;
    int grow = m0 + row;
    if (grow >= g.M) grow = g.M - 1;
    pa[q] = A + (int64_t)grow * g.lda + 8 * c;
    if constexpr (TB) {
      const int drow = lane >> 4;
      const int dchunk = (lane & 15) ^ (((drow & 3) << 2) | (wave & 3));
      int x = n0 + 8 * dchunk;
      if (x > g.N - 8) x = g.N - 8;
      pbt[q] = B + (int64_t)(4 * (wave + 4 * q) + drow) * g.ldb + x;
    }
  }
  auto issue = [&](int s) {
    char* st = smem + (s % M64_NST) * STAGE;
#pragma unroll
    for (int q = 0; q < 2; ++q)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pa[q] + 64 * s),
                                       (__attribute__((address_space(3))) void*)(st + (wave + 4 * q) * 1024), 16, 0, 0);
    if constexpr (!TB) {
      glds_tile<T>(B, g.ldb, n0, s * 64, g.N, st + A_BYTES, tid);
    } else {
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int q = 0; q < 2; ++q)
          __builtin_amdgcn_global_load_lds(
              (const __attribute__((address_space(1))) void*)(pbt[q] + (int64_t)(64 * s + 32 * kh) * g.ldb),
              (__attribute__((address_space(3))) void*)(st + A_BYTES + kh * R_BSUB + (wave + 4 * q) * 1024), 16, 0, 0);
    }
  };
  const unsigned smem_base = (unsigned)(size_t)((const __attribute__((address_space(3))) char*)smem);
  const unsigned b_t0 = A_BYTES + tr_lane_base(lane, 0, 8 * wn), b_t1 = A_BYTES + tr_lane_base(lane, 1, 8 * wn);
  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  EpiPre<T, 2, 4> pre;
  epi_prefetch<T, 2, 4, EPI>(pre, g, m0 + wm * 32, n0 + wn * 64, fr, fq);

  // 3-stage ring, two K-steps in flight (6 DMA instructions per wave and stage, counted waits).  With one step in flight
  // a K-step cost a whole load latency (~0.9 us: the fc1 input gradient at batch 16, K = 1536, took 22 us).
  issue(0);
  if (nk > 1) issue(1);
  for (int s = 0; s < nk; ++s) {
    if (s + 1 < nk) r_wait_vm<6>(); else r_wait_vm<0>();  // stage s landed (this wave's pieces)
    __builtin_amdgcn_s_barrier();                         // ... everybody's; everybody is done reading stage s - 1
    if (s + 2 < nk) issue(s + 2);
    const char* la = smem + (s % M64_NST) * STAGE;
    const char* lb = la + A_BYTES;
    uint4 af[2][2], bf[2][4];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int i = 0; i < 2; ++i) af[kk][i] = lds_read128_asm(la + swz(wm * 32 + 16 * i + fr, 4 * kk + fq));
      if constexpr (!TB) {
#pragma unroll
        for (int j = 0; j < 4; ++j) bf[kk][j] = lds_read128_asm(lb + swz(wn * 64 + 16 * j + fr, 4 * kk + fq));
      } else {
        const unsigned sb = smem_base + (unsigned)((s % M64_NST) * STAGE + kk * R_BSUB);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint2 lo = t_read_tr<0>(sb + (b_t0 ^ (unsigned)(j << 5)));
          const uint2 hi = t_read_tr<0>(sb + (b_t1 ^ (unsigned)(j << 5)));
          bf[kk][j] = uint4{lo.x, lo.y, hi.x, hi.y};
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) mma_frag<T>(bf[kk][j], af[kk][i], acc[i][j]);
  }
  epilogue_tile<T, TC, 2, 4, EPI>(acc, pre, g, m0 + wm * 32, n0 + wn * 64, fr, fq, reinterpret_cast<float*>(smem), wm, wn);
}

template <typename T, typename TC, bool TA, bool TB, bool ACC, bool GL = false, int EPI = -1>
int launch(const GemmArgs& g, int split, hipStream_t st) {
  const GemmProf prof = {gemm_tag(g, TB, ACC), sizeof(T) == 2 ? 0 : 1, 2.0 * g.M * g.N * g.K, gemm_bytes(g, sizeof(T), sizeof(TC))};
  return gemm_launch<gemm_kernel<T, TC, TA, TB, ACC, GL, EPI>>("gemm", 4 * TILE_BYTES, dim3(g.tiles_m * g.tiles_n, 1, split), 256, st,
                                                              prof, g);
}

template <typename TC, int EPI, bool TB, int FI, int CONV = 0>
int launch_r3(GemmArgs g, hipStream_t st) {
  constexpr int LDS = (FI == 8 ? 3 : 4) * (32 * FI * R_ROWB + R_BSUB);
  g.tiles_m = (g.M + 32 * FI - 1) / (32 * FI);
  g.tiles_n = (g.N + 127) / 128;
  GemmProf prof = gemm_prof(g, TB, sizeof(TC));
  if (CONV) prof = {UWU_PROF_CONV, 0, 2.0 * g.M * g.N * g.K, ((double)g.M * g.K / 9 + (double)g.N * g.K + (double)g.M * g.N) * 2};
  return gemm_launch<gemm_r3_kernel<TC, EPI, TB, FI, CONV>>(FI == 8 ? "gemm_r3_256" : "gemm_r3_128", LDS,  // 256x128 / 128x128 tiles
                                                           dim3(g.tiles_m * g.tiles_n), 256, st, prof, g);
}
template <typename TC, int EPI, bool TB>
int launch_big(GemmArgs g, hipStream_t st) {
  g.tiles_m = (g.M + 255) / 256;
  g.tiles_n = (g.N + 255) / 256;
  return gemm_launch<gemm_big_kernel<TC, EPI, TB>>("gemm_big", 2 * 4 * TILE_BYTES, dim3(g.tiles_m * g.tiles_n), 512, st,
                                                  gemm_prof(g, TB, sizeof(TC)), g);
}
template <typename TC, int EPI, bool TB>
int launch_wide(GemmArgs g, hipStream_t st) {
  g.tiles_m = (g.M + 191) / 192;
  g.tiles_n = g.N / 384;
  return gemm_launch<gemm_wide_kernel<TC, EPI, TB>>("gemm_wide", 2 * (192 + 384) * ROW_BYTES, dim3(g.tiles_m * g.tiles_n), 512, st,
                                                   gemm_prof(g, TB, sizeof(TC)), g);
}
template <typename TC, int EPI, bool TB>
int launch_m64(GemmArgs g, hipStream_t st) {
  g.tiles_m = (g.M + 63) / 64;
  g.tiles_n = (g.N + 127) / 128;
  return gemm_launch<gemm_m64_kernel<TC, EPI, TB>>("gemm_m64", M64_NST * (64 * ROW_BYTES + TILE_BYTES), dim3(g.tiles_m * g.tiles_n),
                                                  256, st, gemm_prof(g, TB, sizeof(TC)), g);
}

// Ring kernel choice for bf16 operands with A K-contiguous: 0 = gemm_kernel, 8 = 256x128, 4 = 128x128.
// 256x128 pays off on the wide-N Linears (65536x1152x384: 84 us against 97; x1536: 108 against 132); with 768 tiles
// (N = 384) the second round of 512 workgroup slots would be half empty.  The 128x128 ring (4 stages) replaces
// gemm_kernel's register-staged input-gradient path (K-major weight: qkv dgrad 96 -> 70 us, fc1 dgrad 111 -> 90).
static int pick_r3(const GemmArgs& g, bool tb) {
  static UwuEnv on("UWU_GEMM_R3");  // "0": off (test_gemm_r3_exact_integers_and_dgelu)
  if (on.get().is('0')) return 0;
  if (g.K % 32 || g.K < 96) return 0;
  if ((((uintptr_t)g.A | (uintptr_t)g.B) & 15) || g.lda % 8 || g.ldb % 8) return 0;
  if (tb && (g.N % 8 || g.N < 8)) return 0;
  // tile thresholds 512 / 128: the sweep at per-GPU batches 16..256 found them never losing
  const int64_t t8 = (int64_t)((g.M + 255) / 256) * ((g.N + 127) / 128);
  // long contractions (the UNet's K = 640 .. 5120): the larger tile's operand reuse pays from one workgroup per CU on
  // (SDXL shape, 12 x 4x128x128: 480 tiles of 256x128 per 1280-wide Linear; 30.6 -> 31.8 images/s)
  if (t8 >= (g.K >= 640 ? 256 : 512)) return 8;
  const int64_t t4 = (int64_t)((g.M + 127) / 128) * ((g.N + 127) / 128);
  return (tb && t4 >= 128) ? 4 : 0;  // K-contiguous B at N = 384: gemm_kernel's 128-byte rows measured faster (proj 35 vs 43 us)
}

// 256x256 kernel: taken where the 256x128 ring would be and N is a multiple of 256 (no padded column tiles).
// Same-box A/B of the whole step: DiT-S/2 +1.8 % (only its two GELU Linears qualify: fc1 + GELU 187 -> 167 us at B = 256;
// the dGELU input gradient is a wash there),
// DiT-B/2 +5.5 %, DiT-L/2 +1.9 %, SDXL UNet +-0.  UWU_GEMM_BIG=0 turns it off
// (test_gemm_big_tile_matches_128_kernel).
// (A masked ragged last column tile was tried on DiT-XL/2's N = 3456 / 1152 Linears: +0.4 % at 4 % padding, -1.8 % at
// 11 % -- not taken.)
static bool use_big(const GemmArgs& g) {
  static UwuEnv on("UWU_GEMM_BIG");
  return !on.get().is('0') && g.K % 64 == 0 && g.N % 256 == 0;
}

// 192x384 kernel: N a multiple of 384 (and not of 256), and enough tiles that the last round of one-workgroup-per-CU
// tiles is not mostly empty.  Same box, M = 131072: qkv fwd 193 -> 183 us, fc2 fwd 207 -> 185, qkv / fc1 input gradients
// 149 -> 138 / 191 -> 172; at M = 65536 (342 tiles of 192 rows = 1.3 rounds of 256 CUs) it loses 5-10 %, hence the
// fill rule.  UWU_GEMM_WIDE=0 turns it off, =1 forces it
// (test_gemm_wide_tile_matches_128_kernel).
static bool use_wide(const GemmArgs& g) {
  if (g.K % 64 || g.N % 384 || g.N % 256 == 0) return false;
  static UwuEnv on("UWU_GEMM_WIDE");
  if (on.get().is('0')) return false;
  if (on.is('1')) return true;
  const int64_t tiles = (int64_t)((g.M + 191) / 192) * (g.N / 384);
  const int64_t rounds = (tiles + 255) / 256;
  return tiles * 100 >= rounds * 256 * 85;
}
// 64x128 kernel: when the 128x128 grid has fewer tiles than the chip has CUs.  UWU_GEMM_M64=0 turns it off
// (test_gemm_m64_tile_matches_128_kernel).
static bool use_m64(const GemmArgs& g, bool tb) {
  static UwuEnv on("UWU_GEMM_M64");
  if (on.get().is('0')) return false;
  if (g.K % 64 || (((uintptr_t)g.A | (uintptr_t)g.B) & 15) || g.lda % 8 || g.ldb % 8) return false;
  if (tb && (g.N % 8 || g.N < 8)) return false;
  const int64_t tiles = (int64_t)((g.M + 127) / 128) * ((g.N + 127) / 128);
  return tiles < 256 && g.M > 64;
}

template <typename T, typename TC>
int dispatch_trans(const GemmArgs& g, int ta, int tb, bool acc, int split, hipStream_t st) {
  if (acc) {
    if constexpr (sizeof(TC) == 4) {
      if constexpr (sizeof(T) == 2) {
        if (ta == 1 && tb == 1) {
          const int tr = split > 1 ? uwu_gemm_pick_tr(g) : 0;  // the streaming kernel chooses its own number of K slices
          GemmArgs gt = g;
          gt.bias = nullptr;  // (the fused bias gradient is uwu_gemm_wgrad's)
          if (tr == 1) return uwu_launch_gemm_tr<8, 4>(gt, nullptr, 0, st);
          if (tr == 2) return uwu_launch_gemm_tr<4, 8>(gt, nullptr, 0, st);
        }
      }
      if (ta == 1 && tb == 1) return launch<T, float, true, true, true>(g, split, st);
      if (ta == 0 && tb == 0) return launch<T, float, false, false, true>(g, split, st);
      if (ta == 0 && tb == 1) return launch<T, float, false, true, true>(g, split, st);
    }
    uwu_set_error("gemm: ACCUM epilogue needs fp32 C and (transA,transB) in {(0,0),(0,1),(1,1)}");
    return UWU_EINVAL;
  }
  constexpr bool hot = sizeof(T) == 2 && sizeof(TC) == 2;  // bf16 in / bf16 out: compile-time epilogues
  if (ta == 0 && tb == 0) {
    if constexpr (hot) {
      if (uwu_gemm_p8_ok(g, false)) return uwu_launch_gemm_p8(g, false, st);
      if (g.N % 256 && uwu_gemm_p8n_ok(g, false)) return uwu_launch_gemm_p8n(g, false, st);
    }
    if constexpr (sizeof(T) == 2) {
      const int r3 = pick_r3(g, false);
      if (r3 == 8) {
        if constexpr (hot) {
          if (g.epi == UWU_EPI_BIAS && uwu_gemm_use_as_bias() && uwu_gemm_use_as(g, sizeof(TC))) return uwu_launch_gemm_as<TC, UWU_EPI_BIAS>(g, st);
          if (use_wide(g)) {
            if (g.epi == UWU_EPI_NONE) return launch_wide<TC, UWU_EPI_NONE, false>(g, st);
            if (g.epi == UWU_EPI_BIAS) return launch_wide<TC, UWU_EPI_BIAS, false>(g, st);
          }
          if (g.epi == UWU_EPI_BIAS_GELU && uwu_gemm_use_as(g, sizeof(TC))) return uwu_launch_gemm_as<TC, UWU_EPI_BIAS_GELU>(g, st);
          if (g.epi == UWU_EPI_DGELU && g.C2 == nullptr && g.aux && g.ldaux % 8 == 0 && ((uintptr_t)g.aux & 15) == 0 &&
              uwu_gemm_use_as(g, sizeof(TC)))
            return uwu_launch_gemm_as<TC, UWU_EPI_DGELU>(g, st);
          if (use_big(g)) {
            if (g.epi == UWU_EPI_BIAS_GELU) return launch_big<TC, UWU_EPI_BIAS_GELU, false>(g, st);
            if (g.epi == UWU_EPI_NONE) return launch_big<TC, UWU_EPI_NONE, false>(g, st);
            if (g.epi == UWU_EPI_BIAS) return launch_big<TC, UWU_EPI_BIAS, false>(g, st);
          }
          if (g.epi == UWU_EPI_NONE) return launch_r3<TC, UWU_EPI_NONE, false, 8>(g, st);
          if (g.epi == UWU_EPI_BIAS) return launch_r3<TC, UWU_EPI_BIAS, false, 8>(g, st);
          if (g.epi == UWU_EPI_BIAS_GELU) return launch_r3<TC, UWU_EPI_BIAS_GELU, false, 8>(g, st);
        }
        return launch_r3<TC, -1, false, 8>(g, st);
      }
    }
    if constexpr (hot) {
      if (use_m64(g, false)) {
        if (g.epi == UWU_EPI_NONE) return launch_m64<TC, UWU_EPI_NONE, false>(g, st);
        if (g.epi == UWU_EPI_BIAS) return launch_m64<TC, UWU_EPI_BIAS, false>(g, st);
        if (g.epi == UWU_EPI_BIAS_GELU) return launch_m64<TC, UWU_EPI_BIAS_GELU, false>(g, st);
      }
    }
    if (g.K % GT<T>::BK == 0) {
      if constexpr (hot) {
        if (g.epi == UWU_EPI_NONE) return launch<T, TC, false, false, false, true, UWU_EPI_NONE>(g, split, st);
        if (g.epi == UWU_EPI_BIAS) return launch<T, TC, false, false, false, true, UWU_EPI_BIAS>(g, split, st);
        if (g.epi == UWU_EPI_BIAS_GELU) return launch<T, TC, false, false, false, true, UWU_EPI_BIAS_GELU>(g, split, st);
      }
      return launch<T, TC, false, false, false, true>(g, split, st);
    }
    return launch<T, TC, false, false, false>(g, split, st);
  }
  if (ta == 0 && tb == 1) {
    if constexpr (hot) {
      if (uwu_gemm_p8_ok(g, true)) return uwu_launch_gemm_p8(g, true, st);
      if (g.N % 256 && uwu_gemm_p8n_ok(g, true)) return uwu_launch_gemm_p8n(g, true, st);
      const int r3 = pick_r3(g, true);
      if (r3 == 8 && use_wide(g) && g.epi == UWU_EPI_NONE) return launch_wide<TC, UWU_EPI_NONE, true>(g, st);
      if (r3 == 8 && use_big(g)) {
        if (g.epi == UWU_EPI_DGELU) return launch_big<TC, UWU_EPI_DGELU, true>(g, st);
        if (g.epi == UWU_EPI_NONE) return launch_big<TC, UWU_EPI_NONE, true>(g, st);
      }
      if (r3 == 8 && g.epi == UWU_EPI_NONE) return launch_r3<TC, UWU_EPI_NONE, true, 8>(g, st);
      if (r3 == 8 && g.epi == UWU_EPI_DGELU) return launch_r3<TC, UWU_EPI_DGELU, true, 8>(g, st);
      if (r3 != 8 && use_m64(g, true)) {
        if (g.epi == UWU_EPI_NONE) return launch_m64<TC, UWU_EPI_NONE, true>(g, st);
        if (g.epi == UWU_EPI_DGELU) return launch_m64<TC, UWU_EPI_DGELU, true>(g, st);
      }
      if (r3 == 4 && g.epi == UWU_EPI_NONE) return launch_r3<TC, UWU_EPI_NONE, true, 4>(g, st);
      if (r3 == 4 && g.epi == UWU_EPI_DGELU) return launch_r3<TC, UWU_EPI_DGELU, true, 4>(g, st);
      if (g.epi == UWU_EPI_NONE) return launch<T, TC, false, true, false, false, UWU_EPI_NONE>(g, split, st);
      if (g.epi == UWU_EPI_DGELU) return launch<T, TC, false, true, false, false, UWU_EPI_DGELU>(g, split, st);
    }
    return launch<T, TC, false, true, false>(g, split, st);
  }
  if (ta == 1 && tb == 1) return launch<T, TC, true, true, false>(g, split, st);
  uwu_set_error("gemm: (transA=1, transB=0) is not instantiated");
  return UWU_EINVAL;
}

}  // namespace

// ---- implicit-GEMM 3x3 convolution (padding 1, stride 1 / 2, channels-last bf16): no im2col matrix ------------------------
__device__ uint4 g_conv_zero[4];  // zero page for padded pixels (zero-initialised device memory)

static const void* conv_zero_page() {
  static void* p = nullptr;
  if (!p && hipGetSymbolAddress(&p, HIP_SYMBOL(g_conv_zero)) != hipSuccess) p = nullptr;
  return p;
}

extern "C" int uwu_conv3x3_implicit_ok(int B, int H, int W, int C, int Cout, int stride, int dtype) {
  if (dtype != UWU_BF16 || C % 32 || Cout % 32 || C < 32 || Cout < 32 || (stride != 1 && stride != 2)) return 0;
  if (B <= 0 || H <= 0 || W <= 0) return 0;  // an empty image has Mo = 0, a multiple of 32: not a shape to launch
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const int64_t Mi = (int64_t)B * H * W, Mo = (int64_t)B * Ho * Wo;
  if (Mi >= (1 << 24) || Mo >= (1 << 24) || Mo % 32 || 9 * (int64_t)C >= (1 << 24)) return 0;
  return 1;
}

int uwu_conv3x3_args(GemmArgs& g, int B, int H, int W, int C, int stride) {
  g.cH = H; g.cW = W; g.cC = C; g.cS = stride;
  g.cHo = (H - 1) / stride + 1;
  g.cWo = (W - 1) / stride + 1;
  g.zero = conv_zero_page();
  if (!g.zero) { uwu_set_error("conv3x3: zero page unavailable"); return UWU_ELAUNCH; }
  return UWU_OK;
}

// y[(b,oy,ox), co] = sum x[b, oy s + ky - 1, ox s + kx - 1, c] w[co][ky][kx][c] + bias[co]
extern "C" int uwu_conv3x3_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int Cout,
                               int stride, int dtype, void* stream) {
  UWU_CHECK_ARG(x && w && y && B > 0 && H > 0 && W > 0, "conv3x3_fwd: bad argument");
  UWU_CHECK_ARG(uwu_conv3x3_implicit_ok(B, H, W, C, Cout, stride, dtype), "conv3x3_fwd: shape not covered by the implicit-GEMM kernel (C=%d Cout=%d)", C, Cout);
  UWU_CHECK_ARG((((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) & 15) == 0 && (!bias || ((uintptr_t)bias & 15) == 0), "conv3x3_fwd: misaligned tensor");
  GemmArgs g{};
  RETURN_IF(uwu_conv3x3_args(g, B, H, W, C, stride));
  g.A = x; g.B = w; g.C = y; g.bias = bias;
  g.M = B * g.cHo * g.cWo; g.N = Cout; g.K = 9 * C; g.lda = C; g.ldb = 9 * C; g.ldc = Cout;
  g.epi = bias ? UWU_EPI_BIAS : UWU_EPI_NONE;
  g.wide = (Cout % 8 == 0) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (bias) return launch_r3<bf16_t, UWU_EPI_BIAS, false, 8, 1>(g, st);
  return launch_r3<bf16_t, UWU_EPI_NONE, false, 8, 1>(g, st);
}

// dx[(b,iy,ix), c] = sum dy[b, (iy + 1 - ky) / s, (ix + 1 - kx) / s, co] w[co][ky][kx][c]   (positions that divide evenly)
extern "C" int uwu_conv3x3_dgrad(const void* dy, const void* w, void* dx, int B, int H, int W, int C, int Cout, int stride,
                                 int dtype, void* stream) {
  UWU_CHECK_ARG(dy && w && dx && B > 0 && H > 0 && W > 0, "conv3x3_dgrad: bad argument");
  UWU_CHECK_ARG(uwu_conv3x3_implicit_ok(B, H, W, C, Cout, stride, dtype), "conv3x3_dgrad: shape not covered by the implicit-GEMM kernel");
  UWU_CHECK_ARG((((uintptr_t)dy | (uintptr_t)w | (uintptr_t)dx) & 15) == 0, "conv3x3_dgrad: misaligned tensor");
  GemmArgs g{};
  RETURN_IF(uwu_conv3x3_args(g, B, H, W, C, stride));
  g.A = dy; g.B = w; g.C = dx;
  g.M = B * H * W; g.N = C; g.K = 9 * Cout; g.lda = Cout; g.ldb = 9 * C; g.ldc = C;
  g.epi = UWU_EPI_NONE;
  g.wide = (C % 8 == 0) ? 1 : 0;
  return launch_r3<bf16_t, UWU_EPI_NONE, true, 8, 2>(g, (hipStream_t)stream);
}

// ---- 3x3 / stride 2 convolution padded right and bottom only: F.pad(x, (0, 1, 0, 1)) + conv2d(stride 2, padding 0) -------------
// (forward only; the AutoencoderKL encoder's downsamplers.)  Ho = (H - 2) / 2 + 1.  bf16 shapes that meet the ring kernel's
// conditions run as the implicit GEMM above with the CONV = 3 pixel map; every other shape gathers the column matrix into the
// caller's workspace (uwu_conv3x3_s2br_ws_bytes) and runs uwu_gemm on it (bf16 or fp32).
int uwu_im2col3x3_s2br(const void* x, void* col, int B, int H, int W, int C, int dtype, hipStream_t st);  // unet_ops.hip

static bool conv_s2br_implicit(int B, int H, int W, int C, int Cout, int dtype) {
  if (dtype != UWU_BF16 || C % 32 || Cout % 32 || C < 32 || Cout < 32) return false;
  const int Ho = (H - 2) / 2 + 1, Wo = (W - 2) / 2 + 1;
  const int64_t Mi = (int64_t)B * H * W, Mo = (int64_t)B * Ho * Wo;
  return Mi < (1 << 24) && Mo % 32 == 0 && 9 * (int64_t)C < (1 << 24);
}

static bool conv_s2br_shape_ok(int B, int H, int W, int C, int Cout, int dtype) {
  if (dtype != UWU_BF16 && dtype != UWU_F32) return false;
  const int epc = dtype == UWU_BF16 ? 8 : 4;
  if (B <= 0 || H < 2 || W < 2 || C <= 0 || Cout <= 0 || C % epc) return false;
  return (int64_t)B * H * W < ((int64_t)1 << 31) / 9 && (int64_t)B * H * W * C < ((int64_t)1 << 40);
}

extern "C" size_t uwu_conv3x3_s2br_ws_bytes(int B, int H, int W, int C, int Cout, int dtype) {
  if (!conv_s2br_shape_ok(B, H, W, C, Cout, dtype) || conv_s2br_implicit(B, H, W, C, Cout, dtype)) return 0;
  const int Ho = (H - 2) / 2 + 1, Wo = (W - 2) / 2 + 1;
  return (size_t)B * Ho * Wo * 9 * C * (dtype == UWU_BF16 ? 2 : 4);
}

extern "C" int uwu_conv3x3_s2br_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int Cout,
                                    int dtype, void* ws, size_t ws_bytes, void* stream) {
  UWU_CHECK_ARG(x && w && y, "conv3x3_s2br_fwd: null pointer");
  UWU_CHECK_ARG(conv_s2br_shape_ok(B, H, W, C, Cout, dtype),
                "conv3x3_s2br_fwd: bad shape B=%d H=%d W=%d C=%d Cout=%d dtype=%d (H, W >= 2; C a multiple of 8 (bf16) / 4 (fp32))", B, H, W, C,
                Cout, dtype);
  UWU_CHECK_ARG((((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) & 15) == 0 && (!bias || ((uintptr_t)bias & 15) == 0),
                "conv3x3_s2br_fwd: misaligned tensor");
  const int Ho = (H - 2) / 2 + 1, Wo = (W - 2) / 2 + 1;
  hipStream_t st = (hipStream_t)stream;
  if (conv_s2br_implicit(B, H, W, C, Cout, dtype)) {
    GemmArgs g{};
    RETURN_IF(uwu_conv3x3_args(g, B, H, W, C, 2));
    g.cHo = Ho; g.cWo = Wo;
    g.A = x; g.B = w; g.C = y; g.bias = bias;
    g.M = B * Ho * Wo; g.N = Cout; g.K = 9 * C; g.lda = C; g.ldb = 9 * C; g.ldc = Cout;
    g.epi = bias ? UWU_EPI_BIAS : UWU_EPI_NONE;
    g.wide = (Cout % 8 == 0) ? 1 : 0;
    if (bias) return launch_r3<bf16_t, UWU_EPI_BIAS, false, 8, 3>(g, st);
    return launch_r3<bf16_t, UWU_EPI_NONE, false, 8, 3>(g, st);
  }
  const size_t need = (size_t)B * Ho * Wo * 9 * C * (dtype == UWU_BF16 ? 2 : 4);
  UWU_CHECK_ARG(ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0,
                "conv3x3_s2br_fwd: this shape needs a 16-byte aligned workspace of %zu bytes (uwu_conv3x3_s2br_ws_bytes)", need);
  RETURN_IF(uwu_im2col3x3_s2br(x, ws, B, H, W, C, dtype, st));
  return uwu_gemm(ws, w, y, nullptr, bias, nullptr, B * Ho * Wo, Cout, 9 * C, 9 * C, 9 * C, Cout, 0, 0, 0, dtype, dtype,
                  bias ? UWU_EPI_BIAS : UWU_EPI_NONE, 1, stream);
}

extern "C" int uwu_gemm(const void* A, const void* B, void* C, void* C2, const float* bias, const void* aux, int M,
                        int N, int K, int lda, int ldb, int ldc, int ldaux, int transA, int transB, int dtype,
                        int c_dtype, int epilogue, int split_k, void* stream) {
  UWU_CHECK_ARG(A && B && C, "gemm: null operand");
  UWU_CHECK_ARG(M > 0 && N > 0 && K > 0, "gemm: bad shape M=%d N=%d K=%d", M, N, K);
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "gemm: bad dtype %d", dtype);
  UWU_CHECK_ARG(c_dtype == UWU_F32 || c_dtype == dtype, "gemm: c_dtype must be fp32 or the operand dtype");
  const int epc = dtype == UWU_BF16 ? 8 : 4;
  const int bk = dtype == UWU_BF16 ? 64 : 32;
  // 16-byte vector access rules (checked on the host so a bad shape can never fault on the device)
  UWU_CHECK_ARG((((uintptr_t)A | (uintptr_t)B) & 15) == 0, "gemm: A/B must be 16-byte aligned");
  UWU_CHECK_ARG(lda % epc == 0 && ldb % epc == 0, "gemm: lda/ldb must be multiples of %d", epc);
  UWU_CHECK_ARG(transA ? (M % epc == 0) : (K % epc == 0), "gemm: A contiguous extent must be a multiple of %d", epc);
  UWU_CHECK_ARG(transB ? (N % epc == 0) : (K % epc == 0), "gemm: B contiguous extent must be a multiple of %d", epc);
  UWU_CHECK_ARG(lda >= (transA ? M : K) && ldb >= (transB ? N : K), "gemm: leading dimension too small");
  UWU_CHECK_ARG(epilogue >= UWU_EPI_NONE && epilogue <= UWU_EPI_ACCUM, "gemm: bad epilogue %d", epilogue);
  const bool acc = epilogue == UWU_EPI_ACCUM;
  if (!acc) {
    UWU_CHECK_ARG(split_k <= 1, "gemm: split_k needs UWU_EPI_ACCUM");
    UWU_CHECK_ARG(N % 4 == 0 && ldc % 4 == 0 && ldc >= N, "gemm: N and ldc must be multiples of 4");
    const int cal = c_dtype == UWU_BF16 ? 7 : 15;
    UWU_CHECK_ARG(((uintptr_t)C & cal) == 0, "gemm: C misaligned");
    if (epilogue == UWU_EPI_BIAS || epilogue == UWU_EPI_BIAS_GELU || epilogue == UWU_EPI_BIAS_SILU)
      UWU_CHECK_ARG(bias && ((uintptr_t)bias & 15) == 0, "gemm: bias missing/misaligned");
    if (epilogue == UWU_EPI_BIAS_GELU || epilogue == UWU_EPI_BIAS_SILU)
      UWU_CHECK_ARG(C2 && ((uintptr_t)C2 & cal) == 0, "gemm: C2 missing/misaligned");
    if (epilogue == UWU_EPI_DGELU)
      UWU_CHECK_ARG(aux && ldaux % 4 == 0 && ldaux >= N && ((uintptr_t)aux & (dtype == UWU_BF16 ? 7 : 15)) == 0,
                    "gemm: aux missing/misaligned");
  } else {
    UWU_CHECK_ARG(c_dtype == UWU_F32 && ldc >= N, "gemm: ACCUM needs fp32 C");
  }
  GemmArgs g{};
  g.A = A; g.B = B; g.C = C; g.C2 = C2; g.bias = bias; g.aux = aux;
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldaux = ldaux; g.epi = epilogue;
  g.tiles_m = (M + BM - 1) / BM;
  g.tiles_n = (N + BN - 1) / BN;
  // 16-byte epilogue stores need 8-column granularity and 16-byte aligned rows
  g.wide = (!acc && c_dtype == UWU_BF16 && N % 8 == 0 && ldc % 8 == 0 && ((uintptr_t)C & 15) == 0 &&
            (C2 == nullptr || epilogue == UWU_EPI_DGELU || ((uintptr_t)C2 & 15) == 0)) ? 1 : 0;
  g.aux16 = (epilogue == UWU_EPI_DGELU && dtype == UWU_BF16 && N % 8 == 0 && ldaux % 8 == 0 && ((uintptr_t)aux & 15) == 0) ? 1 : 0;

  const int ktiles = (K + bk - 1) / bk;
  int split = split_k < 1 ? 1 : split_k;
  if (split > ktiles) split = ktiles;
  g.k_tiles_per_split = (ktiles + split - 1) / split;
  split = (ktiles + g.k_tiles_per_split - 1) / g.k_tiles_per_split;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == UWU_BF16) {
    if (c_dtype == UWU_BF16) return dispatch_trans<bf16_t, bf16_t>(g, transA, transB, acc, split, st);
    return dispatch_trans<bf16_t, float>(g, transA, transB, acc, split, st);
  }
  return dispatch_trans<float, float>(g, transA, transB, acc, split, st);
}

// (the profiler entry points live in prof.cpp: uwu_prof_enable / uwu_prof_collect; uwu_gemm_prof_* wrap them)
