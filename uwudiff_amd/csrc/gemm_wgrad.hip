// Streaming weight-gradient GEMMs for gfx950: dW[M,N] (fp32) += A[K,M]^T . B[K,N], both operands K-major bf16 (A = dY [tokens, out],
// B = X [tokens, in]), split along K.
//
// Shapes served: K % 32 == 0, M and N multiples of 8, 16-byte addressable operands --
//   gemm_tr_kernel   256x128 / 128x256 tiles, two workgroups per CU: reductions from K = 2048 on; its CONVW form is the weight
//                    gradient of the implicit-GEMM 3x3 convolution
//   gemm_trw_kernel  192x384 / 384x192 tiles, one workgroup per CU: M or N a multiple of 384 and K >= 32768
//                    (uwu_gemm_wgrad_pair: two such gradients over the same K as one launch + one reduce)
// and the two kernels that add the split-K slices of a scratch into C (also used by the fp8 weight gradients of gemm_f8.hip).
// Everything else goes to uwu_gemm(transA = 1, transB = 1, UWU_EPI_ACCUM) in gemm.hip.
// Reference op sequence replaced: the weight / bias gradient that autograd computes for nn.Linear inside the blocks (reference
// src/duwu/modules/rope_unet.py:122-166) and for the UNet's 3x3 Conv2d (src/duwu/modules/unet_patch.py:13-57).
#include "gemm_shared.h"

namespace {

// ---- weight-gradient kernel: both operands K-major (dW[M,N] += A[K,M]^T . B[K,N]), bf16, split-K + fp32 atomics ----
// PMC on the register-transposing path (1536x384x65536): MFMA busy 20 %, a third of the LDS cycles are the 2-way
// conflicts of the transposing ds_write_b64, and with 128x128 tiles the launch pulls 1.2 GB through L2.  Here the
// K-major tiles go to LDS untouched by LDS-DMA ([k][128 x] sub-images of 32 rows x 256 B) and the MFMA fragments
// are gathered by the CDNA4 transposing read ds_read_b64_tr_b16 (16 lanes read a 4 x 16 block and receive it
// column-major: lane i gets column i of 4 consecutive k) -- no VGPR round trip, no ds_write, no permutes.
// Tile 256x128 or 128x256 (FI x FJ = 8x4 / 4x8 accumulators per wave, 2x2 waves), K-step 32, 3-stage ring of 24 KB
// -> two workgroups per CU as gemm_r3_kernel (gemm.hip).  Sub-image layout (cdna_hip_programming.md T10, image (b)):
// 16-byte chunk ch of k-row r at  256 r + 16 (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))); the DMA writes lane-linear
// (4 rows per wave-instruction), so the XOR is applied to the per-lane source column.
constexpr int T_SUB = 32 * 256;        // one sub-image: 32 k-rows x 128 elements
constexpr int T_STAGE = 3 * T_SUB;     // A sub-images then B sub-images (2 + 1 or 1 + 2)
constexpr int T_NST = 3;
constexpr int T_PS = 6;                // DMA instructions per wave per K-step (24 pieces of 4 rows / 4 waves)


// PART: the split-K partial goes to a dense scratch [split][M][N] with plain 16-byte stores (swapped MFMA operands:
// a lane owns 4 consecutive columns) and splitk_reduce_kernel adds the slices to C -- global fp32 atomics move only
// ~1.3 TB/s chip-wide, and with ~500 workgroups x 128 KB of accumulators they cost as much as the whole K loop.
// CONVW (weight gradient of the implicit-GEMM 3x3 convolution): dW[co][(tap, c)] += sum_m dY[m][co] X[pixel(m) + tap][c].
// The B rows (K index m = output pixel) are gathered per lane: column x -> (tap, c) is fixed per lane, the pixel of
// row m is recomputed every K-step (two divmod24), padded positions read the zero page.
template <int FI, int FJ, bool PART, bool CONVW = false>
__global__ void __launch_bounds__(256, 2) gemm_tr_kernel(const GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef bf16_t T;
  static_assert((FI == 8 && FJ == 4) || (FI == 4 && FJ == 8), "256x128 or 128x256");
  constexpr int TBM = 32 * FI, TBN = 32 * FJ;
  constexpr int NA = TBM / 128;  // A sub-images per stage (B: 3 - NA)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  // Workgroup -> (output tile, K slice z).  All tiles of one K slice read the same A / B rows, so they must share an
  // L2: workgroups b and b+8 land on the same XCD (round-robin dispatch), hence XCD x = b & 7 takes the slices
  // z = x, x+8, ... and walks the tiles of one slice before the next.  (With the plain (tile, z) grid the tiles of
  // a slice were spread over all 8 XCDs: PMC showed 73 % L2 misses and ~700 MB of fabric reads per launch for
  // 250 MB of operands.)  g.wide carries the number of slices.
  // Weights with MANY tiles and a short reduction (the UNet's Linears: 400 tiles, 192 K-steps) need no 8-fold split for
  // parallelism, and 8 fp32 slices of such an output are far more traffic than the operands.  There the 8 XCDs form
  // xs slice lanes x 8 / xs tile lanes: XCD x takes the slices z = (x mod xs) + xs j of the tiles whose row (part_m) or
  // column index is congruent to x / xs -- an XCD still reads only its own share of one operand.  xs = 8 is the case above.
  const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
  const int sl = xcd & (g.xs - 1), tl = xcd / g.xs, TL = 8 / g.xs;
  const int jz = loc / g.nloc, rr = loc - jz * g.nloc;
  const int zsl = sl + g.xs * jz;
  if (zsl >= g.wide) return;  // uniform per block
  int tm, tn;
  if (g.part_m) {
    const int u = rr / g.tiles_n;
    tm = tl + TL * u;
    tn = rr - u * g.tiles_n;
  } else {
    const int u = rr / g.tiles_m;
    tn = tl + TL * u;
    tm = rr - u * g.tiles_m;
  }
  if (tm >= g.tiles_m || tn >= g.tiles_n) return;  // uniform per block
  const int m0 = tm * TBM, n0 = tn * TBN;
  const int s_begin = zsl * g.k_tiles_per_split;  // K-steps of 32 rows
  int s_end = s_begin + g.k_tiles_per_split;
  if (s_end > (g.K >> 5)) s_end = g.K >> 5;
  const int ns = s_end - s_begin;
  if (ns <= 0) return;  // uniform per block

  // ---- DMA: this wave's pieces P = wave + 4q (q < 6); sub-image P >> 3, rows 4 (P & 7) .. +3 of it
  const int drow = lane >> 4;
  const int dsw = ((drow & 3) << 2) | (wave & 3);  // f(row) of the destination row: (P & 7) & 3 == wave & 3
  const int dchunk = (lane & 15) ^ dsw;            // logical chunk that must land at position lane & 15
  const T* src[T_PS];
  int ctap[T_PS];  // CONVW: ky * 4 + kx of this lane's column in piece q
#pragma unroll
  for (int q = 0; q < T_PS; ++q) {
    const int P = wave + 4 * q, S = P >> 3, lp = P & 7;
    const bool isA = S < NA;
    int x = (isA ? m0 + 128 * S : n0 + 128 * (S - NA)) + 8 * dchunk;
    const int X = isA ? g.M : g.N;
    if (x > X - 8) x = X - 8;  // columns past the operand: clamped (their products are never accumulated)
    const T* base = static_cast<const T*>(isA ? g.A : g.B);
    ctap[q] = 0;
    if (CONVW && !isA) {
      int tap, c;
      divmod24(x, g.cC, 1.f / (float)g.cC, tap, c);
      const int ky = tap / 3;
      ctap[q] = ky * 4 + (tap - 3 * ky);
      src[q] = base + c;
    } else {
      src[q] = base + (int64_t)(s_begin * 32 + 4 * lp + drow) * (isA ? g.lda : g.ldb) + x;
    }
  }
  const int64_t stepA = (int64_t)32 * g.lda, stepB = (int64_t)32 * g.ldb;
  const float rcp_img = CONVW ? 1.f / (float)(g.cHo * g.cWo) : 0.f, rcp_w = CONVW ? 1.f / (float)g.cWo : 0.f;
  auto issue = [&](int s) {  // s = step index relative to s_begin
    char* st = smem + (s % T_NST) * T_STAGE;
#pragma unroll
    for (int q = 0; q < T_PS; ++q) {
      const int P = wave + 4 * q, S = P >> 3, lp = P & 7;
      const T* p;
      if (CONVW && S >= NA) {
        const int m = (s_begin + s) * 32 + 4 * lp + drow;  // output pixel (b, oy, ox); g.K = B Ho Wo is a multiple of 32
        int b, rem, oy, ox;
        divmod24(m, g.cHo * g.cWo, rcp_img, b, rem);
        divmod24(rem, g.cWo, rcp_w, oy, ox);
        const int gy = oy * g.cS + (ctap[q] >> 2) - 1, gx = ox * g.cS + (ctap[q] & 3) - 1;
        const bool ok = gy >= 0 && gy < g.cH && gx >= 0 && gx < g.cW;
        p = ok ? src[q] + ((int64_t)(b * g.cH + gy) * g.cW + gx) * g.cC : static_cast<const T*>(g.zero);
      } else {
        p = src[q] + s * (S < NA ? stepA : stepB);
      }
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)p,
                                       (__attribute__((address_space(3))) void*)(st + S * T_SUB + lp * 1024), 16, 0, 0);
    }
  };

  f32x4 acc[FI][FJ];
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int j = 0; j < FJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Fused bias gradient: g.bias != NULL asks for bias[m] += sum_k A[k][m] (the column sums of dY).  That is one more
  // output column with B = 1: extra MFMAs against a constant all-ones fragment (the MFMA pipe is 20 % busy in this
  // kernel), and the separate colsum pass over dY (28 us per Linear) disappears.
  // The tile's first column block does it (tn == 0); its two waves of equal wm split the FI row-fragments in halves
  // (two code copies, so the FI / 2 extra accumulators keep compile-time indices).
  const bool do_sum = g.bias != nullptr && tn == 0;  // wave-uniform
  constexpr int FH = FI / 2;
  f32x4 sacc[FH];
#pragma unroll
  for (int i = 0; i < FH; ++i) sacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint4 ones = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};  // 8 x bf16(1.0)

  // ---- transposed fragment reads: lane = 16 g + 4 q + p supplies row 8 g + 4 t + q, columns 4 p .. 4 p + 3 of the
  // fragment's 16-column block; fragment fi only flips chunk bits: address ^ (fi << 5)
  const int tg = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  auto tr_base = [&](int t, int xb8) {  // xb8 = (first column of the wave's share inside the sub-image) / 8
    const int krow = 8 * tg + 4 * t + tq;
    const int f = (tq << 2) | ((2 * tg + t) & 3);
    return (unsigned)(256 * krow + 16 * ((xb8 + (tp >> 1)) ^ f) + 8 * (tp & 1));
  };
  const unsigned smem_base = (unsigned)(size_t)((const __attribute__((address_space(3))) char*)smem);
  // A: FI == 8 -> the wave owns sub-image wm entirely; FI == 4 -> columns 64 wm .. of the single sub-image
  const unsigned a_sub = (FI == 8) ? wm * T_SUB : 0, a_xb8 = (FI == 8) ? 0 : 8 * wm;
  const unsigned b_sub = NA * T_SUB + ((FJ == 8) ? wn * T_SUB : 0), b_xb8 = (FJ == 8) ? 0 : 8 * wn;
  const unsigned a_t0 = a_sub + tr_base(0, a_xb8), a_t1 = a_sub + tr_base(1, a_xb8);
  const unsigned b_t0 = b_sub + tr_base(0, b_xb8), b_t1 = b_sub + tr_base(1, b_xb8);

  issue(0);
  if (ns > 1) issue(1);
  for (int s = 0; s < ns; ++s) {
    if (s + 1 < ns) r_wait_vm<T_PS>(); else r_wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    if (s + 2 < ns) issue(s + 2);
    const unsigned sb = smem_base + (unsigned)((s % T_NST) * T_STAGE);
    uint4 af[FI], bf[FJ];
#pragma unroll
    for (int j = 0; j < FJ; ++j) {
      const uint2 lo = t_read_tr<0>(sb + (b_t0 ^ (unsigned)(j << 5)));
      const uint2 hi = t_read_tr<0>(sb + (b_t1 ^ (unsigned)(j << 5)));
      bf[j] = uint4{lo.x, lo.y, hi.x, hi.y};
    }
#pragma unroll
    for (int i = 0; i < FI; ++i) {
      const uint2 lo = t_read_tr<0>(sb + (a_t0 ^ (unsigned)(i << 5)));
      const uint2 hi = t_read_tr<0>(sb + (a_t1 ^ (unsigned)(i << 5)));
      af[i] = uint4{lo.x, lo.y, hi.x, hi.y};
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
      for (int j = 0; j < FJ; ++j) {
        if constexpr (PART)
          mma_frag<T>(bf[j], af[i], acc[i][j]);
        else
          mma_frag<T>(af[i], bf[j], acc[i][j]);
      }
    if (do_sum) {
      if (wn == 0) {
#pragma unroll
        for (int i = 0; i < FH; ++i) {
          if constexpr (PART) mma_frag<T>(ones, af[i], sacc[i]);
          else mma_frag<T>(af[i], ones, sacc[i]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < FH; ++i) {
          if constexpr (PART) mma_frag<T>(ones, af[FH + i], sacc[i]);
          else mma_frag<T>(af[FH + i], ones, sacc[i]);
        }
      }
    }
  }
  if (do_sum) {
    float* bg = const_cast<float*>(g.bias);
#pragma unroll
    for (int i = 0; i < FH; ++i) {
      const int mb = m0 + wm * 16 * FI + 16 * (wn * FH + i);
      if constexpr (PART) {  // D[n][m]: column m = fr on the lane, every row equal
        const int m = mb + fr;
        if (fq == 0 && m < g.M) atomicAdd(bg + m, sacc[i][0]);
      } else {  // D[m][n]: rows 4 fq + r in the registers, every column equal
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = mb + 4 * fq + r;
          if (fr == 0 && m < g.M) atomicAdd(bg + m, sacc[i][r]);
        }
      }
    }
  }
  if constexpr (PART) {
    if (g.wide == 1) {  // one slice: the tile is this workgroup's alone -> plain read-modify-write of C
      float* C = static_cast<float*>(g.C);
#pragma unroll
      for (int i = 0; i < FI; ++i) {
        const int m = m0 + wm * 16 * FI + 16 * i + fr;
#pragma unroll
        for (int j = 0; j < FJ; ++j) {
          const int n = n0 + wn * 16 * FJ + 16 * j + 4 * fq;
          if (m < g.M && n < g.N) {
            float* c = C + (int64_t)m * g.ldc + n;
            store4(c, load4(c) + acc[i][j]);
          }
        }
      }
      return;
    }
    float* P = static_cast<float*>(g.C2) + (int64_t)zsl * g.M * g.N;
#pragma unroll
    for (int i = 0; i < FI; ++i) {
      const int m = m0 + wm * 16 * FI + 16 * i + fr;
#pragma unroll
      for (int j = 0; j < FJ; ++j) {
        const int n = n0 + wn * 16 * FJ + 16 * j + 4 * fq;
        if (m < g.M && n < g.N) store4(P + (int64_t)m * g.N + n, acc[i][j]);
      }
    }
    return;
  }
  // atomic accumulate (registers walk rows, lanes walk 16 consecutive columns -> 64-byte atomic segments)
  float* C = static_cast<float*>(g.C);
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int j = 0; j < FJ; ++j) {
      const int n = n0 + wn * 16 * FJ + 16 * j + fr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * 16 * FI + 16 * i + 4 * fq + r;
        if (m < g.M && n < g.N) atomicAdd(C + (int64_t)m * g.ldc + n, acc[i][j][r]);
      }
    }
}

// ---- wide streaming weight gradient: 192 x 384 or 384 x 192 tile, ONE 8-wave workgroup per CU ------------------------------
// Why: all tiles of a K slice read the same rows, so the UNIQUE bytes a launch has in flight are only
// (slices running at once) x (stages in flight) x (32 rows x (M + N) x 2 B).  With 256x128 tiles the 18 tiles of an fc1 slice
// leave room for ~3.5 slices per XCD: ~6 MB in flight chip-wide, which at ~2.6 us of loaded HBM latency is the 2.3-2.6 TB/s
// the 256x128 kernel measures (a third of the HBM rate, although it only READS).  A tile that spans the whole 384-wide
// operand needs 8 tiles per slice: 4 slices per XCD at one workgroup per CU, a 4-stage ring (3 in flight), every operand row
// crosses L2 -> LDS once per 192 (384) output rows instead of once per 128 -- ~2.5x the unique bytes in flight.
// Structure as gemm_tr_kernel (K-major operands untouched in LDS, ds_read_b64_tr_b16 fragments, split-K partials to a
// scratch + splitk_reduce_kernel, fused bias gradient); waves WM x WN, wave tile 96 x 96 (FI = FJ = 6: 144 accumulator
// registers; a 256-row tile needs 192 and spilled).  The 192-wide operand fills one and a half [32 k][128 x] sub-images: the
// DMA lanes of the unused half are masked off.
constexpr int W_NSUB = 5;                 // sub-images [32 k][128 x] per stage: NA for A, 5 - NA for B
constexpr int W_STAGE = W_NSUB * T_SUB;   // 40 KB
// Who waits for what in this kernel (at ~250 VGPRs the compiler copies registers around, and it believes an inline-asm
// ds_read has delivered at its #ASMEND -- a copy it placed between such a read and the hand-written lgkmcnt wait carried
// the PREVIOUS K-step's fragment into the bias MFMA; cdna_hip_programming.md section 5.7 item 1):
//   * fragment reads are the BUILTIN transposing read, so hipcc counts lgkmcnt itself and may interleave them with MFMAs;
//   * the LDS-DMA is inline asm (glds16_asm, gemm_shared.h: m0 set and restored inside the statement): invisible to hipcc, so it
//     neither waits vmcnt(0) before the visible reads nor drains the ring at the barrier; its completion is the hand-counted
//     vmcnt wait.
typedef short s16x4 __attribute__((ext_vector_type(4)));
// Grouped launch: a second weight gradient dW_b[M,N] += A_b[K,M]^T . B_b[K,N] that shares K, the slice count and the scratch
// with the one in GemmArgs (member a).  Every launch ends with the whole chip flushing its fp32 tiles to the scratch
// (256 x 192 x 384 x 4 B = 75 MB, whatever the size of the weight), so two small gradients in one launch halve that traffic and
// the number of reduces.  tiles == 0: a launch of member a alone.
struct TrwPair {
  const void* A;
  const void* B;
  const float* bias;
  int M, N, lda, ldb, tiles, tiles_n;  // tiles = member b's tile count, tiles_n = its tile columns
};
// GRP: the K loop as two wave groups one barrier apart (below); GRP = false keeps all eight waves in phase, one barrier per
// K-step (UWU_TRW_GROUPS=0).  Both run the same MFMAs on the same fragments in the same order per accumulator.
template <int WM, int WN, int FI, int FJ, int NST, bool GRP>
__global__ void __launch_bounds__(512, 2) gemm_trw_kernel(const GemmArgs g, const TrwPair p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef bf16_t T;
  static_assert(WM * WN == 8, "8 waves");
  constexpr int TBM = 16 * FI * WM, TBN = 16 * FJ * WN;
  constexpr int NA = (TBM + 127) / 128, NB = (TBN + 127) / 128;
  static_assert(NA + NB == W_NSUB, "five sub-images per stage");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave - wm * WN;
  const int fr = lane & 15, fq = lane >> 4;
  // Workgroup -> (K slice, tile) as in gemm_tr_kernel; the tiles of member b follow member a's inside every slice, so the
  // tiles of one (member, slice) still sit on one XCD, run in step and share their operand rows through its L2.
  const int tiles_a = g.tiles_m * g.tiles_n, nblk = tiles_a + p.tiles;
  const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
  const int zsl = xcd + 8 * (loc / nblk);
  int tile = loc % nblk;
  if (zsl >= g.wide) return;  // uniform per block
  const bool mb = tile >= tiles_a;  // uniform per block: the member costs scalar registers only
  if (mb) tile -= tiles_a;
  const T* const opA = static_cast<const T*>(mb ? p.A : g.A);
  const T* const opB = static_cast<const T*>(mb ? p.B : g.B);
  const float* const bias = mb ? p.bias : g.bias;
  const int M = mb ? p.M : g.M, N = mb ? p.N : g.N, lda = mb ? p.lda : g.lda, ldb = mb ? p.ldb : g.ldb;
  const int tiles_n = mb ? p.tiles_n : g.tiles_n;
  const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
  const int m0 = tm * TBM, n0 = tn * TBN;
  const int s_begin = zsl * g.k_tiles_per_split;
  int s_end = s_begin + g.k_tiles_per_split;
  if (s_end > (g.K >> 5)) s_end = g.K >> 5;
  const int ns = s_end - s_begin;
  if (ns <= 0) return;  // uniform per block

  // ---- DMA: wave w moves rows 4w .. 4w+3 of every sub-image (piece q = sub-image q)
  const int drow = lane >> 4;
  const int dchunk = (lane & 15) ^ (((drow & 3) << 2) | (wave & 3));
  const T* src[W_NSUB];
  bool live[W_NSUB];  // lanes whose 8 columns lie inside the tile (the last sub-image of a 192-wide operand is half used)
#pragma unroll
  for (int q = 0; q < W_NSUB; ++q) {
    const bool isA = q < NA;
    const int xl = 128 * (isA ? q : q - NA) + 8 * dchunk;  // column inside the tile
    live[q] = xl < (isA ? TBM : TBN);
    int x = (isA ? m0 : n0) + xl;
    const int X = isA ? M : N;
    if (x > X - 8) x = X - 8;  // columns past the operand: clamped (their products are never stored)
    src[q] = (isA ? opA : opB) + (int64_t)(s_begin * 32 + 4 * wave + drow) * (isA ? lda : ldb) + x;
  }
  const int64_t stepA = (int64_t)32 * lda, stepB = (int64_t)32 * ldb;
  const unsigned smem_base = (unsigned)(size_t)((const __attribute__((address_space(3))) char*)smem);
  auto issue = [&](int s) {
    const unsigned st = smem_base + (unsigned)((s % NST) * W_STAGE + wave * 1024);
#pragma unroll
    for (int q = 0; q < W_NSUB; ++q)
      if (live[q])  // (EXEC-masked DMA: the other lanes' LDS slots keep stale bytes no fragment reads; every wave has live lanes)
        glds16_asm(src[q] + s * (q < NA ? stepA : stepB), st + q * T_SUB);
  };

  f32x4 acc[FI][FJ];
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int j = 0; j < FJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // fused bias gradient (column sums of A = dY): row fragment fi is summed by wave column fi % WN, in its slot fi / WN
  const bool do_sum = bias != nullptr && tn == 0;  // wave-uniform, per member
  constexpr int FS = (FI + WN - 1) / WN;
  f32x4 sacc[FS];
#pragma unroll
  for (int i = 0; i < FS; ++i) sacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint4 ones = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};

  // fragment gidx of an operand (16 columns each, 8 per sub-image): sub-image gidx >> 3, chunk bits (gidx & 7) << 5
  const unsigned t0 = tr_lane_base(lane, 0, 0), t1 = tr_lane_base(lane, 1, 0);
  auto rd = [&](unsigned off) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)((__attribute__((address_space(3))) char*)smem + off));
  };
  auto frag = [&](unsigned stage_off, int gidx) {
    const unsigned sub = stage_off + (unsigned)((gidx >> 3) * T_SUB), fl = (unsigned)((gidx & 7) << 5);
    const s16x4 lo = rd(sub + (t0 ^ fl)), hi = rd(sub + (t1 ^ fl));
    uint4 r;
    r.x = ((unsigned)(unsigned short)lo[0]) | ((unsigned)(unsigned short)lo[1] << 16);
    r.y = ((unsigned)(unsigned short)lo[2]) | ((unsigned)(unsigned short)lo[3] << 16);
    r.z = ((unsigned)(unsigned short)hi[0]) | ((unsigned)(unsigned short)hi[1] << 16);
    r.w = ((unsigned)(unsigned short)hi[2]) | ((unsigned)(unsigned short)hi[3] << 16);
    return r;
  };
  const int ga0 = FI * wm, gb0 = 8 * NA + FJ * wn;  // (16-column fragment index counted over the operand's sub-images)

  constexpr int AHEAD = NST - 1;
  static_assert(NST == 4, "the vmcnt ladder below is written for three K-steps ahead");
#pragma unroll
  for (int s = 0; s < AHEAD; ++s)
    if (s < ns) issue(s);
  constexpr int GI = FI / 2;  // A fragments per half
  // this wave's pieces of K-step t have landed once at most the pieces of the younger ISSUED steps are outstanding.  Wherever it
  // is called below, the steps issued so far are 0 .. min(t + AHEAD - 1, ns - 1): up to AHEAD - 1 younger ones
  auto wait_step = [&](int t) __attribute__((always_inline)) {
    const int younger = ns - 1 - t < AHEAD - 1 ? ns - 1 - t : AHEAD - 1;
    if (younger >= 2) r_wait_vm<2 * W_NSUB>();
    else if (younger == 1) r_wait_vm<W_NSUB>();
    else r_wait_vm<0>();
  };
  if constexpr (!GRP) {
    for (int s = 0; s < ns; ++s) {
      wait_step(s);
      __syncthreads();  // everybody's pieces of step s; everybody is done reading stage (s - 1) % NST
      if (s + AHEAD < ns) issue(s + AHEAD);
      const unsigned so = (unsigned)((s % NST) * W_STAGE);
      uint4 bf[FJ], af[GI];
#pragma unroll
      for (int j = 0; j < FJ; ++j) bf[j] = frag(so, gb0 + j);
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
        for (int i = 0; i < GI; ++i) af[i] = frag(so, ga0 + GI * hh + i);
#pragma unroll
        for (int i = 0; i < GI; ++i)
#pragma unroll
          for (int j = 0; j < FJ; ++j) mma_frag<T>(bf[j], af[i], acc[GI * hh + i][j]);
        if (do_sum) {
#pragma unroll
          for (int i = 0; i < GI; ++i) {
            const int fi = GI * hh + i;
            if (fi % WN == wn) mma_frag<T>(ones, af[i], sacc[fi / WN]);
          }
        }
      }
    }
  } else {
    // Two wave groups ONE BARRIER APART, as gemm_p8_kernel (gemm_p8.hip): group 0 = waves 0-3 (one per SIMD), group 1 = their
    // SIMD partners 4-7 (WM x WN = 2 x 4: wave rows 0 / 1; 4 x 2: wave rows 0-1 / 2-3; partners share their B columns).  A K-step
    // is { DMA issue + 12 fragment reads | barrier | 36 (+ bias) MFMAs | barrier }, and group 1 passes one extra barrier before
    // its first step: while one wave of a SIMD issues MFMAs its partner reads the fragments of its own next MFMA interval, so the
    // matrix pipe does not wait for LDS and the two waves never read LDS or want the pipe at the same time.
    //
    // Ordering argument.  B(k) = the k-th workgroup barrier, B(0) the one in front of the loop; interval k lies between B(k) and
    // B(k+1).  Group 0 reads K-step s in interval 2s and multiplies it in 2s+1; group 1 reads it in 2s+1 and multiplies in 2s+2.
    // Every wave executes 2 ns + 2 barriers: B(0), [group 1: its idle interval 0], two per K-step, [group 0: one at the end].
    //   RAW  every wave retires its own pieces of step s by wait_step(s) in front of B(2s): both groups in interval 2s-1 --
    //        group 0 behind its MFMAs of step s-1, group 1 at the end of its reads of step s-1 (behind its issue of step s+2), step
    //        0 in front of B(0).  Group 0 reads step s behind B(2s), group 1 behind B(2s+1).  At either wait the issued steps
    //        are 0 .. min(s+2, ns-1), so the count is the one of the in-phase loop: the pieces of min(ns-1-s, 2) younger steps.
    //   WAR  step s+3 lands in stage (s-1) % 4.  Group 0 read that stage in interval 2s-2, group 1 in interval 2s-1, and each
    //        retired its reads (lgkmcnt(0)) in front of the barrier that closed the interval: B(2s) is the barrier that proves both
    //        groups done with it.  Group 0 issues step s+3 behind B(2s) (interval 2s), group 1 behind B(2s+1).
    // So a piece is 6 (group 0) or 5 (group 1) intervals = 3 or 2.5 K-steps ahead of its wait; the in-phase loop has 3.  Group 1
    // issuing in front of its MFMAs instead (interval 2s, the full 3 K-steps) gave the whole gain back: the five
    // DMA instructions then delay the MFMAs of a SIMD whose other wave is reading, and all eight waves request at once again.
    const int grp = wave >> 2;  // scalar
    auto bar = [&]() __attribute__((always_inline)) {
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    };
    wait_step(0);
    bar();                // B(0)
    if (grp == 1) bar();  // B(1): waves 4-7 run one barrier behind their SIMD partners
    for (int s = 0; s < ns; ++s) {
      // read interval
      if (s + AHEAD < ns) issue(s + AHEAD);
      const unsigned so = (unsigned)((s % NST) * W_STAGE);
      uint4 bf[FJ], af[FI];
#pragma unroll
      for (int j = 0; j < FJ; ++j) bf[j] = frag(so, gb0 + j);
#pragma unroll
      for (int i = 0; i < FI; ++i) af[i] = frag(so, ga0 + i);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the stage is free for the DMA issued behind the next barrier (WAR)
      if (grp == 1 && s + 1 < ns) wait_step(s + 1);
      bar();
      // MFMA interval (the order per accumulator is the in-phase loop's: one MFMA per K-step)
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
        for (int i = 0; i < GI; ++i)
#pragma unroll
          for (int j = 0; j < FJ; ++j) mma_frag<T>(bf[j], af[GI * hh + i], acc[GI * hh + i][j]);
        if (do_sum) {
#pragma unroll
          for (int i = 0; i < GI; ++i) {
            const int fi = GI * hh + i;
            if (fi % WN == wn) mma_frag<T>(ones, af[fi], sacc[fi / WN]);
          }
        }
      }
      __builtin_amdgcn_s_setprio(0);
      if (grp == 0 && s + 1 < ns) wait_step(s + 1);
      bar();
    }
    if (grp == 0) bar();  // every wave has passed the same number of barriers
  }
  if (do_sum) {
    float* bg = const_cast<float*>(bias);
#pragma unroll
    for (int i = 0; i < FS; ++i) {  // D[n][m]: column m = fr on the lane, every row equal
      const int fi = i * WN + wn;
      const int m = m0 + wm * 16 * FI + 16 * fi + fr;
      if (fi < FI && fq == 0 && m < M) atomicAdd(bg + m, sacc[i][0]);
    }
  }
  // scratch [slice][member a's M x N, then member b's M x N]  (p.M = p.N = 0 without a member b)
  const int64_t size_a = (int64_t)g.M * g.N;
  float* P = static_cast<float*>(g.C2) + (int64_t)zsl * (size_a + (int64_t)p.M * p.N) + (mb ? size_a : 0);
#pragma unroll
  for (int i = 0; i < FI; ++i) {
    const int m = m0 + wm * 16 * FI + 16 * i + fr;
#pragma unroll
    for (int j = 0; j < FJ; ++j) {
      const int n = n0 + wn * 16 * FJ + 16 * j + 4 * fq;
      if (m < M && n < N) store4(P + (int64_t)m * N + n, acc[i][j]);
    }
  }
}

// C[m][n] += sum over the split-K slices of the scratch [split][M][N]; one float4 per thread
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const float* __restrict__ part, float* __restrict__ C,
                                                            int M, int N, int ldc, int split) {
  const int64_t slice = (int64_t)M * N;
  for (int64_t idx = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; idx < slice; idx += (int64_t)gridDim.x * 1024) {
    f32x4 v = load4(part + idx);
    for (int z = 1; z < split; ++z) v = v + load4(part + z * slice + idx);
    const int m = (int)(idx / N), n = (int)(idx - (int64_t)m * N);
    float* c = C + (int64_t)m * ldc + n;
    store4(c, load4(c) + v);
  }
}

// The same sum with the slices divided among four lanes of threads: a workgroup takes 64 float4 of the output per pass, thread
// (zl, cl) adds slices zl, zl + 4, .. of column group cl on two accumulators (loads of 8 slices in flight), the four partial sums
// meet in LDS.  With one thread per output float4 a [384 x 384] gradient in 128 slices was 36 864 threads walking 128 dependent
// adds each on 144 of the 256 CUs.
// A slice may hold two outputs back to back (grouped weight gradients): elements from M * N on belong to Cb[Mb, Nb].  Either way
// every output element adds its slices in the same fixed order.
__device__ __forceinline__ void splitk_reduce4_body(const float* __restrict__ part, int split, float* __restrict__ C, int M,
                                                    int N, int ldc, float* __restrict__ Cb, int Mb, int Nb, int ldcb) {
  __shared__ f32x4 red[4][64];
  const int zl = threadIdx.x >> 6, cl = threadIdx.x & 63;
  const int64_t size_a = (int64_t)M * N, slice = size_a + (int64_t)Mb * Nb;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < slice; base += (int64_t)gridDim.x * 256) {
    const int64_t idx = base + 4 * cl;
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
    if (idx < slice) {
      int z = zl;
      for (; z + 4 < split; z += 8) {
        v0 = v0 + load4(part + (int64_t)z * slice + idx);
        v1 = v1 + load4(part + (int64_t)(z + 4) * slice + idx);
      }
      if (z < split) v0 = v0 + load4(part + (int64_t)z * slice + idx);
    }
    red[zl][cl] = v0 + v1;
    __syncthreads();
    if (zl == 0 && idx < slice) {
      const f32x4 v = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
      const bool second = idx >= size_a;
      const int64_t e = second ? idx - size_a : idx;
      const int n_out = second ? Nb : N;
      const int m = (int)(e / n_out), n = (int)(e - (int64_t)m * n_out);
      float* c = (second ? Cb + (int64_t)m * ldcb : C + (int64_t)m * ldc) + n;
      store4(c, load4(c) + v);
    }
    __syncthreads();
  }
}
__global__ void __launch_bounds__(256) splitk_reduce4_kernel(const float* __restrict__ part, float* __restrict__ C,
                                                             int M, int N, int ldc, int split) {
  splitk_reduce4_body(part, split, C, M, N, ldc, nullptr, 0, 0, 0);
}
__global__ void __launch_bounds__(256) splitk_reduce4_pair_kernel(const float* __restrict__ part, int split,
                                                                  float* __restrict__ C, int M, int N, int ldc,
                                                                  float* __restrict__ Cb, int Mb, int Nb, int ldcb) {
  splitk_reduce4_body(part, split, C, M, N, ldc, Cb, Mb, Nb, ldcb);
}
// the four-lane reduce over one output (Cb == NULL) or over the two outputs of a grouped launch: 64 float4 per workgroup and pass
void launch_splitk_reduce4(const float* part, int split, float* C, int M, int N, int ldc, float* Cb, int Mb, int Nb, int ldcb,
                           hipStream_t st) {
  const int64_t quads = ((int64_t)M * N + (int64_t)Mb * Nb) / 4;
  int rg = (int)((quads + 63) / 64);
  if (rg > 8192) rg = 8192;
  if (Cb) hipLaunchKernelGGL(splitk_reduce4_pair_kernel, dim3(rg), dim3(256), 0, st, part, split, C, M, N, ldc, Cb, Mb, Nb, ldcb);
  else hipLaunchKernelGGL(splitk_reduce4_kernel, dim3(rg), dim3(256), 0, st, part, C, M, N, ldc, split);
}
// Number of K slices for the streaming weight-gradient kernel: a multiple of 8 (one group of slices per XCD), as
// many groups as fit the XCD's 64 workgroup slots (32 CUs x 2) in one round.
// Outputs with >= 64 tiles of a reduction of a few thousand rows: fewer slices, the XCDs divided between slices and tiles
// (gemm_tr_kernel's xs): every halving of the slice count halves the fp32 slice traffic.
int tr_split(int tiles, int steps) {
  int split;
  if (tiles >= 320 && steps <= 1024) {  // (sweep at 6144 / 24576 tokens: 400 tiles 361 -> 193 us, 200 tiles 166 -> 115,
    split = 1;                                 //  150 tiles 122 -> 107, 100 tiles 223 -> 217; 50 tiles stay at 8 slices)
  } else if (tiles >= 140 && steps <= 1024) {
    split = 2;
  } else if (tiles >= 80 && steps <= 1024) {
    split = 4;
  } else {
    int per_xcd = 64 / tiles;
    if (per_xcd < 1) per_xcd = 1;
    split = 8 * per_xcd;
    while (split > 8 && split * 32 > steps) split -= 8;  // keep >= 32 K-steps per slice (batch 16: 3.82k -> 4.13k img/s, batch 64: 9.05k -> 9.79k with the four side streams)
  }
  if (split > steps) split = steps;
  return split < 1 ? 1 : split;
}
// slice lanes among the 8 XCDs: the largest power of two <= 8 that divides the slice count
int tr_xs(int split) { return split % 8 == 0 ? 8 : (split % 4 == 0 ? 4 : (split % 2 == 0 ? 2 : 1)); }

// wide weight-gradient kernel: K slices in groups of 8 (one group per XCD), one workgroup per CU
int trw_split(int tiles, int steps) {
  int per_xcd = 32 / tiles;
  if (per_xcd < 1) per_xcd = 1;
  int split = 8 * per_xcd;
  while (split > 8 && split * 8 > steps) split -= 8;  // keep >= 8 K-steps per slice
  if (split > steps) split = steps;
  return split < 1 ? 1 : split;
}
// 0 = not taken, 1 = 192 x 384 tiles, 2 = 384 x 192 tiles.  UWU_GEMM_TRW=0 turns it off
// (test_gemm_wgrad_many_tiles_xcd_partition).
int trw_kind(int M, int N, int K) {
  static UwuEnv on("UWU_GEMM_TRW");
  if (on.get().is('0')) return 0;
  // short reductions (per-GPU batch < 128 images): the 4-stage ring of a whole-LDS workgroup barely fills and nothing else fits
  // on its CU; the 256x128 kernel (two workgroups per CU) measured 1-2 % faster there.  UWU_GEMM_TRW=1 forces it
  // (test_gemm_wgrad_scratch_path).
  const bool force = on.is('1');
  if (K % 32 || K < (force ? 4096 : 32768) || M % 8 || N % 8) return 0;
  if (N % 384 == 0 && M >= 192) return 1;
  if (M % 384 == 0 && N >= 192) return 2;
  return 0;
}
int pick_trw(const GemmArgs& g) {
  if ((((uintptr_t)g.A | (uintptr_t)g.B) & 15) || g.lda % 8 || g.ldb % 8) return 0;
  return trw_kind(g.M, g.N, g.K);
}
int trw_tiles(int M, int N, int kind) { return kind == 1 ? ((M + 191) / 192) * (N / 384) : (M / 384) * ((N + 191) / 192); }
size_t trw_scratch_bytes(int M, int N, int K, int kind) {
  return (size_t)trw_split(trw_tiles(M, N, kind), K / 32) * M * N * sizeof(float);
}
// Two weight gradients in one launch: both take the same tile orientation, and together they have at most 32 tiles -- beyond
// that trw_split gives the pair the 8 slices each member has alone, and grouping saves no scratch traffic.  0 = not grouped.
size_t trw_pair_scratch_bytes(int Ma, int Na, int Mb, int Nb, int K) {
  const int kind = trw_kind(Ma, Na, K);
  if (!kind || trw_kind(Mb, Nb, K) != kind) return 0;
  const int tiles = trw_tiles(Ma, Na, kind) + trw_tiles(Mb, Nb, kind);
  if (tiles > 32) return 0;
  return (size_t)trw_split(tiles, K / 32) * ((size_t)Ma * Na + (size_t)Mb * Nb) * sizeof(float);
}
// b != NULL: the second member of a grouped launch (its A, B, C, bias, M, N and leading dimensions; K is g's)
template <int WM, int WN, int FI, int FJ, bool GRP>
int launch_trw(GemmArgs g, const GemmArgs* b, void* scratch, hipStream_t st) {
  constexpr int NST = 4;
  constexpr int TBM = 16 * FI * WM, TBN = 16 * FJ * WN;
  constexpr auto kern = gemm_trw_kernel<WM, WN, FI, FJ, NST, GRP>;
  RETURN_IF(gemm_lds_optin<kern>("gemm_trw", NST * W_STAGE));
  g.tiles_m = (g.M + TBM - 1) / TBM;
  g.tiles_n = (g.N + TBN - 1) / TBN;
  TrwPair p{};
  if (b) {
    p.A = b->A; p.B = b->B; p.bias = b->bias; p.M = b->M; p.N = b->N; p.lda = b->lda; p.ldb = b->ldb;
    p.tiles_n = (b->N + TBN - 1) / TBN;
    p.tiles = ((b->M + TBM - 1) / TBM) * p.tiles_n;
  }
  const int tiles = g.tiles_m * g.tiles_n + p.tiles, steps = g.K / 32;
  int split = trw_split(tiles, steps);
  g.k_tiles_per_split = (steps + split - 1) / split;
  split = (steps + g.k_tiles_per_split - 1) / g.k_tiles_per_split;
  g.wide = split;
  g.C2 = scratch;
  const int grid = 8 * tiles * ((split + 7) / 8);
  double flops = 2.0 * g.M * g.N * g.K, bytes = ((double)g.M * g.K + (double)g.N * g.K) * 2 + (double)g.M * g.N * 4;
  UwuProfScope prof(st);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), NST * W_STAGE, st, g, p);
  if (b) {
    launch_splitk_reduce4(static_cast<const float*>(scratch), split, static_cast<float*>(g.C), g.M, g.N, g.ldc,
                          static_cast<float*>(b->C), b->M, b->N, b->ldc, st);
    flops += 2.0 * b->M * b->N * g.K;
    bytes += ((double)b->M * g.K + (double)b->N * g.K) * 2 + (double)b->M * b->N * 4;
  } else {
    uwu_launch_splitk_reduce(static_cast<const float*>(scratch), static_cast<float*>(g.C), g.M, g.N, g.ldc, split, st);
  }
  prof.done(UWU_PROF_GEMM_WGRAD, 0, flops, bytes);  // (one record per launch: a grouped one carries both members' work)
  UWU_LAUNCH_CHECK("gemm_trw");
  return UWU_OK;
}

// The K loop's schedule: two wave groups one barrier apart; UWU_TRW_GROUPS=0 keeps the eight waves in phase (same results bit for
// bit: tests/test_wgrad_groups_gpu.py).  kind = trw_kind()'s tile orientation.
int launch_trw_kind(int kind, const GemmArgs& g, const GemmArgs* b, void* scratch, hipStream_t st) {
  static UwuEnv groups("UWU_TRW_GROUPS");
  if (groups.get().is('0'))
    return kind == 1 ? launch_trw<2, 4, 6, 6, false>(g, b, scratch, st) : launch_trw<4, 2, 6, 6, false>(g, b, scratch, st);
  return kind == 1 ? launch_trw<2, 4, 6, 6, true>(g, b, scratch, st) : launch_trw<4, 2, 6, 6, true>(g, b, scratch, st);
}

}  // namespace

// launches the reduce: the four-lane form from 8 slices on, one thread per float4 below
void uwu_launch_splitk_reduce(const float* part, float* C, int M, int N, int ldc, int split, hipStream_t st) {
  const int64_t quads = (int64_t)M * N / 4;
  if (split >= 8) {
    launch_splitk_reduce4(part, split, C, M, N, ldc, nullptr, 0, 0, 0, st);
    return;
  }
  int rg = (int)((quads + 255) / 256);
  if (rg > 4096) rg = 4096;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(rg), dim3(256), 0, st, part, C, M, N, ldc, split);
}

// K-major x K-major accumulate (the weight gradients): 0 = keep the 128x128 kernel, 1 = 256x128, 2 = 128x256
int uwu_gemm_pick_tr(const GemmArgs& g) {
  static UwuEnv on("UWU_GEMM_TR");  // "0": off (test_gemm_tr_exact_integers, test_gemm_tr_random)
  if (on.get().is('0')) return 0;
  if (g.K % 32 || g.K < 96 || g.M % 8 || g.N % 8 || g.M < 8 || g.N < 8) return 0;
  if ((((uintptr_t)g.A | (uintptr_t)g.B) & 15) || g.lda % 8 || g.ldb % 8) return 0;
  auto padded = [](int x, int b) { return (double)(((x + b - 1) / b) * b) / x; };
  const double w1 = padded(g.M, 256) * padded(g.N, 128), w2 = padded(g.M, 128) * padded(g.N, 256);
  const double w0 = padded(g.M, 128) * padded(g.N, 128);
  if ((w1 < w2 ? w1 : w2) > 1.35 * w0) return 0;  // too much padding: the small tile wastes less
  if (g.K < 2048) return 0;                       // short reductions: nothing to stream
  return w1 <= w2 ? 1 : 2;
}

template <int FI, int FJ, bool CONVW>
int uwu_launch_gemm_tr(GemmArgs g, void* scratch, size_t scratch_bytes, hipStream_t st) {
  RETURN_IF(gemm_lds_optin<gemm_tr_kernel<FI, FJ, false, CONVW>>("gemm_tr", T_NST * T_STAGE));
  RETURN_IF(gemm_lds_optin<gemm_tr_kernel<FI, FJ, true, CONVW>>("gemm_tr", T_NST * T_STAGE));
  g.tiles_m = (g.M + 32 * FI - 1) / (32 * FI);
  g.tiles_n = (g.N + 32 * FJ - 1) / (32 * FJ);
  const int tiles = g.tiles_m * g.tiles_n, steps = g.K / 32;
  int split = tr_split(tiles, steps);
  g.k_tiles_per_split = (steps + split - 1) / split;
  split = (steps + g.k_tiles_per_split - 1) / g.k_tiles_per_split;
  // 16-byte rows in the scratch and in C: slices go to the scratch (one slice: straight into C); otherwise 8 slice lanes + atomics
  const bool vec_ok = g.N % 4 == 0 && g.ldc % 4 == 0 && (((uintptr_t)g.C | (uintptr_t)scratch) & 15) == 0;
  const bool part = vec_ok && (split == 1 || (scratch && scratch_bytes >= (size_t)split * g.M * g.N * sizeof(float)));
  if (!part && split < 8 && steps >= 8) {  // the atomic path wants all XCDs through the slice lanes
    split = 8;
    g.k_tiles_per_split = (steps + split - 1) / split;
    split = (steps + g.k_tiles_per_split - 1) / g.k_tiles_per_split;
  }
  g.wide = split;
  g.xs = tr_xs(split);
  const int TL = 8 / g.xs;
  g.part_m = g.tiles_m >= g.tiles_n;
  g.nloc = g.part_m ? ((g.tiles_m + TL - 1) / TL) * g.tiles_n : ((g.tiles_n + TL - 1) / TL) * g.tiles_m;
  const int grid = 8 * g.nloc * ((split + g.xs - 1) / g.xs);
  UwuProfScope prof(st);
  if (part && split == 1) {
    hipLaunchKernelGGL((gemm_tr_kernel<FI, FJ, true, CONVW>), dim3(grid), dim3(256), T_NST * T_STAGE, st, g);
  } else if (part) {
    g.C2 = scratch;
    hipLaunchKernelGGL((gemm_tr_kernel<FI, FJ, true, CONVW>), dim3(grid), dim3(256), T_NST * T_STAGE, st, g);
    uwu_launch_splitk_reduce(static_cast<const float*>(scratch), static_cast<float*>(g.C), g.M, g.N, g.ldc, split, st);
  } else {
    hipLaunchKernelGGL((gemm_tr_kernel<FI, FJ, false, CONVW>), dim3(grid), dim3(256), T_NST * T_STAGE, st, g);
  }
  prof.done(CONVW ? UWU_PROF_CONV : UWU_PROF_GEMM_WGRAD, 0, 2.0 * g.M * g.N * g.K, ((double)g.M * g.K + (double)g.N * g.K) * 2 + (double)g.M * g.N * 4);
  UWU_LAUNCH_CHECK("gemm_tr");
  return UWU_OK;
}
template int uwu_launch_gemm_tr<8, 4>(GemmArgs, void*, size_t, hipStream_t);  // (named by dispatch_trans, gemm.hip)
template int uwu_launch_gemm_tr<4, 8>(GemmArgs, void*, size_t, hipStream_t);

extern "C" size_t uwu_conv3x3_wgrad_scratch_bytes(int C, int Cout, int64_t Mo) {
  return uwu_gemm_wgrad_scratch_bytes(Cout, 9 * C, (int)Mo);
}
// dw[co][ky][kx][c] += sum dy[(b,oy,ox), co] x[b, oy s + ky - 1, ox s + kx - 1, c];  db[co] += sum dy
extern "C" int uwu_conv3x3_wgrad(const void* dy, const void* x, float* dw, float* db, int B, int H, int W, int C, int Cout,
                                 int stride, int dtype, void* scratch, size_t scratch_bytes, void* stream) {
  UWU_CHECK_ARG(dy && x && dw && B > 0 && H > 0 && W > 0, "conv3x3_wgrad: bad argument");
  UWU_CHECK_ARG(uwu_conv3x3_implicit_ok(B, H, W, C, Cout, stride, dtype), "conv3x3_wgrad: shape not covered by the implicit-GEMM kernel");
  UWU_CHECK_ARG((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dw) & 15) == 0, "conv3x3_wgrad: misaligned tensor");
  GemmArgs g{};
  RETURN_IF(uwu_conv3x3_args(g, B, H, W, C, stride));
  g.A = dy; g.B = x; g.C = dw; g.bias = db;
  g.M = Cout; g.N = 9 * C; g.K = B * g.cHo * g.cWo; g.lda = Cout; g.ldb = C; g.ldc = 9 * C;
  g.epi = UWU_EPI_ACCUM;
  auto padded = [](int v, int b) { return (double)(((v + b - 1) / b) * b) / v; };
  const bool tall = padded(g.M, 256) * padded(g.N, 128) <= padded(g.M, 128) * padded(g.N, 256);
  hipStream_t st = (hipStream_t)stream;
  if (tall) return uwu_launch_gemm_tr<8, 4, true>(g, scratch, scratch_bytes, st);
  return uwu_launch_gemm_tr<4, 8, true>(g, scratch, scratch_bytes, st);
}

// Weight gradient with caller-provided split-K scratch: C[M,N] (fp32) += A[K,M]^T . B[K,N], operands K-major.
// When `scratch` holds uwu_gemm_wgrad_scratch_bytes(M, N, K) the split-K slices of the streaming kernel are written
// there and reduced by a second kernel; otherwise its slices are accumulated with atomics.  Shapes the streaming
// kernel does not take go to uwu_gemm(..., UWU_EPI_ACCUM) with `blocks` workgroups as the split-K target.
extern "C" size_t uwu_gemm_wgrad_scratch_bytes(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K < 32) return 0;
  // the larger of the two tile orientations' slice counts (uwu_gemm_pick_tr chooses by padding)
  const int t1 = ((M + 255) / 256) * ((N + 127) / 128), t2 = ((M + 127) / 128) * ((N + 255) / 256);
  const int s1 = tr_split(t1, K / 32), s2 = tr_split(t2, K / 32);
  size_t b = (size_t)(s1 > s2 ? s1 : s2) * M * N * sizeof(float);
  if (N % 384 == 0 && trw_scratch_bytes(M, N, K, 1) > b) b = trw_scratch_bytes(M, N, K, 1);
  if (M % 384 == 0 && trw_scratch_bytes(M, N, K, 2) > b) b = trw_scratch_bytes(M, N, K, 2);
  return b;
}

extern "C" int uwu_gemm_wgrad(const void* A, const void* B, float* C, float* bias_grad, int M, int N, int K, int lda,
                              int ldb, int ldc, int dtype, int blocks, void* scratch, size_t scratch_bytes,
                              void* stream) {
  UWU_CHECK_ARG(A && B && C, "gemm_wgrad: null operand");
  UWU_CHECK_ARG(M > 0 && N > 0 && K > 0 && blocks > 0, "gemm_wgrad: bad shape M=%d N=%d K=%d blocks=%d", M, N, K, blocks);
  UWU_CHECK_ARG(dtype == UWU_F32 || dtype == UWU_BF16, "gemm_wgrad: bad dtype %d", dtype);
  UWU_CHECK_ARG(lda >= M && ldb >= N && ldc >= N, "gemm_wgrad: leading dimension too small");
  if (dtype == UWU_BF16) {
    GemmArgs g{};
    g.A = A; g.B = B; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.epi = UWU_EPI_ACCUM;
    g.bias = bias_grad;
    const int trw = pick_trw(g);
    if (trw && scratch && (((uintptr_t)C | (uintptr_t)scratch) & 15) == 0 && ldc % 4 == 0 &&
        scratch_bytes >= trw_scratch_bytes(M, N, K, trw)) {
      return launch_trw_kind(trw, g, nullptr, scratch, (hipStream_t)stream);
    }
    const int tr = uwu_gemm_pick_tr(g);
    if (tr == 1) return uwu_launch_gemm_tr<8, 4>(g, scratch, scratch_bytes, (hipStream_t)stream);
    if (tr == 2) return uwu_launch_gemm_tr<4, 8>(g, scratch, scratch_bytes, (hipStream_t)stream);
  }
  if (bias_grad) {
    const int rc = uwu_colsum(A, dtype, K, M, lda, bias_grad, 1, stream);
    if (rc != UWU_OK) return rc;
  }
  const int tiles = ((M + 127) / 128) * ((N + 127) / 128);
  const int bk = dtype == UWU_BF16 ? 64 : 32;
  int split = (blocks + tiles - 1) / tiles;
  // a slice that adds a whole fp32 tile with atomics has to amortise them over >= 8 K steps (the cross-attention
  // key / value weights see K = B x 77 tokens: 5 slices of 1-2 steps each took 119 us, one slice of 8 takes 15)
  const int ksteps = (K + bk - 1) / bk;
  if (split > ksteps / 8) split = ksteps / 8;
  if (split < 1) split = 1;
  return uwu_gemm(A, B, C, nullptr, nullptr, nullptr, M, N, K, lda, ldb, ldc, 0, 1, 1, dtype, UWU_F32, UWU_EPI_ACCUM,
                  split, stream);
}

// Two weight gradients that share K (the token count) and the dtype, C_a += A_a^T . B_a and C_b += A_b^T . B_b, as ONE launch of
// the wide kernel + one reduce when uwu_gemm_wgrad_pair_scratch_bytes() is non-zero and `scratch` holds that much; otherwise two
// uwu_gemm_wgrad calls, one after the other on `stream`, with the same scratch.
extern "C" size_t uwu_gemm_wgrad_pair_scratch_bytes(int M_a, int N_a, int M_b, int N_b, int K) {
  if (M_a <= 0 || N_a <= 0 || M_b <= 0 || N_b <= 0 || K < 32) return 0;
  return trw_pair_scratch_bytes(M_a, N_a, M_b, N_b, K);
}

extern "C" int uwu_gemm_wgrad_pair(const void* A_a, const void* B_a, float* C_a, float* bias_grad_a, int M_a, int N_a, int lda_a,
                                   int ldb_a, int ldc_a, const void* A_b, const void* B_b, float* C_b, float* bias_grad_b,
                                   int M_b, int N_b, int lda_b, int ldb_b, int ldc_b, int K, int dtype, int blocks,
                                   void* scratch, size_t scratch_bytes, void* stream) {
  UWU_CHECK_ARG(A_a && B_a && C_a && A_b && B_b && C_b, "gemm_wgrad_pair: null operand");
  UWU_CHECK_ARG(M_a > 0 && N_a > 0 && M_b > 0 && N_b > 0 && K > 0, "gemm_wgrad_pair: bad shape");
  UWU_CHECK_ARG(lda_a >= M_a && ldb_a >= N_a && ldc_a >= N_a && lda_b >= M_b && ldb_b >= N_b && ldc_b >= N_b,
                "gemm_wgrad_pair: leading dimension too small");
  if (dtype == UWU_BF16 && scratch) {
    GemmArgs a{}, b{};
    a.A = A_a; a.B = B_a; a.C = C_a; a.bias = bias_grad_a; a.M = M_a; a.N = N_a; a.K = K; a.lda = lda_a; a.ldb = ldb_a; a.ldc = ldc_a;
    b.A = A_b; b.B = B_b; b.C = C_b; b.bias = bias_grad_b; b.M = M_b; b.N = N_b; b.K = K; b.lda = lda_b; b.ldb = ldb_b; b.ldc = ldc_b;
    a.epi = b.epi = UWU_EPI_ACCUM;
    const size_t need = trw_pair_scratch_bytes(M_a, N_a, M_b, N_b, K);
    const int kind = pick_trw(a);
    if (need && need <= scratch_bytes && kind && pick_trw(b) == kind && ldc_a % 4 == 0 && ldc_b % 4 == 0 &&
        (((uintptr_t)C_a | (uintptr_t)C_b | (uintptr_t)scratch) & 15) == 0) {
      return launch_trw_kind(kind, a, &b, scratch, (hipStream_t)stream);
    }
  }
  RETURN_IF(uwu_gemm_wgrad(A_a, B_a, C_a, bias_grad_a, M_a, N_a, K, lda_a, ldb_a, ldc_a, dtype, blocks, scratch, scratch_bytes, stream));
  return uwu_gemm_wgrad(A_b, B_b, C_b, bias_grad_b, M_b, N_b, K, lda_b, ldb_b, ldc_b, dtype, blocks, scratch, scratch_bytes, stream);
}
