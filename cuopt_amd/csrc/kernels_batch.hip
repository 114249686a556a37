// Shared-matrix batched PDHG (round 5; BASELINE config 5's pattern: the MIP heuristics re-solve the SAME A and c under different bounds,
// cpp/src/mip/relaxed_lp/relaxed_lp.cu:53-127; the reference builds a solver per call, its batch entry point -- cython_solve.cu:264-296 --
// is a thread pool of independent solves).  K = 2, 4, 8 or 16 LPs that share the matrix advance together:
//   * every LP keeps a full context of its own (pdlpdev_clone_shared: the matrices, their layouts, D_r, D_c and c are the parent's,
//     read-only; iterates, bounds, sums, control block, partials are the clone's): the major iterations -- KKT evaluation, restarts,
//     the primal weight -- run through the single-LP code, untouched, LP by LP;
//   * an attempt is FOUR launches for all K LPs: kb_primal (the K primal steps, xbar written interleaved), kb_a_dual and kb_at_step
//     (the two products, fused with the K dual steps / step-size sums), k_step_decision_batch (K workgroups, each k_step_decision);
//   * the two products serve all K LPs from ONE pass over the matrix.  The K gathered vectors are INTERLEAVED (v[j * K + l]): a
//     nonzero's gather is one 64-byte request (K = 8) for all LPs instead of K requests of 8 bytes -- the request rate is what bounds
//     the unstructured single-LP product (profiles/r05_gather_calibration.txt);
//   * the trajectories are BIT-IDENTICAL to the single solves': rows are summed left to right (the single kernels' order for rows
//     of <= 128 entries), the fused epilogues are the single kernels' expressions, and the per-workgroup partial sums reproduce the
//     panel kernels' grouping exactly -- workgroup <-> row panel (the single layout's own boundaries), lane t of an LP's wave
//     accumulates rows t, t + 512, ... in ascending order, the same wave tree (ds_swizzle butterflies) and wave-by-wave sum as
//     block_reduce (CSR stream layout: workgroup <-> row block, 256 "threads", four waves).  Hence the restriction: each matrix in
//     the row-sum variant of the panels or in the CSR stream layout, no row beyond 128 entries, no dense segments, columns ascending
//     within rows (else: not eligible, the caller keeps its independent solves).  Round 7 adds the jagged layout (kbj_*, below) for
//     parents created with cuoptamd_settings::batch_lanes >= K.
// What it buys (C3, 1e6 x 1e6, 1e7 nonzeros; profiles/r05_bench_lines.jsonl, c3_batch16 / c3_batch8): 14.7 k iterations/s aggregate
// over 16 LPs, 10.7 k over 8, against 6.0 k for one -- 2.43x / 1.77x; K = 4: 1.24x; K = 2: 0.80x (two single solves are faster).
// Why not more: only the MATRIX is shared.  A lockstep iteration of 8 LPs moves 1.85 GB at the fused floor (0.24 GB of matrix once,
// 8 x 0.18 GB of vectors, the interleaved copies) against 0.42 GB for one LP: at EQUAL fractions of the HBM roofline the ceiling is
// 8 x 0.42 / 1.85 = 1.80x (16 LPs: 1.92x); the single solve and the batch of 8 run at 0.31 of their floors, the batch of 16 at 0.40.
// The K = 8 products sit at ~300 us whatever their internal structure (row walk / LDS-staged chunks / autonomous waves, 1 to 32
// gathers in flight, 2 or 4 workgroups per CU: tools/batch_spmv_probe.hip, profiles/r05_batch_spmv_probe.txt): 1e7 gathered
// 128-byte lines from beyond L2 (the interleaved vector is 64 MB; an XCD's L2 holds 4) + 0.5 GB of streams ~ 1.8 GB at ~6 TB/s --
// K = 16 uses the whole line a miss fetches.  The single-LP panels avoid those line fills by sweeping 1.33 MB column slabs in step
// across the chip; eight interleaved vectors would need 46 slabs and a sweep synchronised to +-3 %: with the epilogue phases in
// between it does not hold (window-major orders in the probe: no gain once the epilogue is in).
#include <cstring>
#include <hip/hip_runtime.h>

#include "batch_common.hpp"
#include "pdlp_ctx.hpp"

#define LAUNCH_CHECK() HIP_TRY(hipGetLastError())

// single-LP kernels of the core (pdlp_device.hip), launched per LP
__global__ void k_step_decision_batch(const pdlpdev_decision_args* __restrict__ args);
__global__ void k_set_target(pdlpdev_ctl* ctl, int target);
__global__ void k_set_error(pdlpdev_ctl* ctl);

namespace {

// (kBT, kBatchMax, BatchLp, WaveLps: batch_common.hpp)
// ---- (1) the primal step of K LPs (k_primal's expressions, LP by LP) with xbar written INTERLEAVED ------------------------------
// wave <-> LP, lane <-> column: every per-LP stream is read and written in 512-byte pieces; the tile of xbar goes through LDS (one
// padded row per column) and leaves as whole entries of the interleaved vector.
template <int K>
__global__ void __launch_bounds__(kBT) kb_primal(const BatchLp* __restrict__ lp, int n, double* __restrict__ xK)
{
  __shared__ double tile[kBT][K + 1];
  using WL = WaveLps<K>;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, sub = WL::sub(wave);
  for (int t0 = blockIdx.x * kBT; t0 < n; t0 += gridDim.x * kBT) {
#pragma unroll
    for (int pass = 0; pass < WL::PASSES; ++pass) {
      const int l       = WL::lp(wave, pass);
      const BatchLp L   = lp[l];
      const bool active = loop_active(L.ctl);
      const int cur       = L.ctl->cur;
      const double tau    = L.ctl->tau;
      const double weight = L.ctl->step_size;
      const bool pend     = L.ctl->pending_avg != 0;
      const double* __restrict__ x   = cur ? L.x1 : L.x0;
      double* __restrict__ xn        = cur ? L.x0 : L.x1;
      const double* __restrict__ aty = cur ? L.aty1 : L.aty0;
#pragma unroll
      for (int q = sub; q < 8; q += WL::NSUB) {
        const int jl = lane + 64 * q, j = t0 + jl;
        double xb    = 0.0;
        if (active && j < n) {
          const double xj       = x[j];
          const double gradient = L.c[j] - aty[j];
          double next           = xj - (tau * gradient);
          next                  = dmax(dmin(next, L.ubd.ub_same ? L.ubd.ub : L.ub[j]), L.ubd.lb_same ? L.ubd.lb : L.lb[j]);
          xn[j]                 = next;
          xb                    = next - xj + next;
          if (pend) L.sumx[j] = L.sumx[j] + weight * xj;
        }
        tile[jl][l] = xb;
      }
    }
    __syncthreads();
    for (int f = threadIdx.x; f < kBT * K; f += kBT) {
      const int jl = f / K;
      if (t0 + jl < n) xK[(size_t)t0 * K + f] = tile[jl][f % K];
    }
    __syncthreads();
  }
}

// ---- (2), (3) the two products for K LPs ----------------------------------------------------------------------------------------
// The panel kernels' structure, K wide.  A workgroup owns the rows of ONE panel of the single-LP layout (same boundaries: the
// partial sums below are then the panel kernels' own) and walks them in blocks of 512 rows.  Per block the matrix entries -- one
// contiguous CSR range -- are read coalesced, a chunk at a time, and handed round through LDS; a GROUP of K / 2 lanes fetches one
// entry's K vector values (lane h: the LPs 2h and 2h + 1, one 16-byte load; K = 8: one 64-byte request per entry, K = 16: the whole
// 128-byte line a miss fetches anyway) and leaves the K products in LDS; lane (g, h) then adds the products of ITS rows (g, g + G,
// ...) left to right in registers -- the CSR order, the order every single-LP kernel uses for rows of up to 128 entries.  One
// barrier per chunk, two chunks of gathers in flight.  The fused epilogue runs wave <-> LP, lane <-> row (the row sums cross over
// through LDS): every per-LP stream is read and written in 512-byte pieces, and lane t of an LP's wave holds exactly the panel
// kernels' "thread t" accumulators (rows t, t + 512, ... of the panel in ascending order), so the wave tree and the wave-by-wave
// sum of block_reduce apply unchanged.
// (BatchGeometry, BatchShared, batch_block_sums, batch_cross_over, batch_block_partials: batch_common.hpp)

// rows of A for K LPs: y' = proj(y - sigma A xbar), ||dy||^2 partials, the deferred dual averaging (DualEpilogue, pdlp_epilogues.hpp);
// y' also goes, interleaved, to the vector the column side gathers from
template <int K, int VW>
__global__ void __launch_bounds__(kBT) kb_a_dual(int W, const int32_t* __restrict__ row0, const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                                 const double* __restrict__ val, const BatchLp* __restrict__ lp, const double* __restrict__ xK,
                                                 double* __restrict__ yK)
{
  __shared__ BatchShared<K> S;
  using WL = WaveLps<K>;
  const int w = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, sub = WL::sub(wave);
  const int r0 = row0[w], nr = row0[w + 1] - r0;
  double acc[WL::PASSES][1][8];
#pragma unroll
  for (int pass = 0; pass < WL::PASSES; ++pass)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[pass][0][j] = 0.0;
  for (int b0 = 0; b0 < nr; b0 += kBT) {
    double s[BatchGeometry<K>::RU][2];
    batch_block_sums<K>(S, r0, nr, b0, off, idx, val, xK, s);
    batch_cross_over<K>(S, s);
#pragma unroll
    for (int pass = 0; pass < WL::PASSES; ++pass) {
      const int l      = WL::lp(wave, pass);
      const BatchLp L  = lp[l];
      if (!loop_active(L.ctl)) continue;
      const int cur      = L.ctl->cur;
      const double sigma = L.ctl->sigma, weight = L.ctl->step_size;
      const bool pend    = L.ctl->pending_avg != 0;
      const double* __restrict__ y = cur ? L.y1 : L.y0;
      double* __restrict__ yn      = cur ? L.y0 : L.y1;
      double yv[8], lov[8], hiv[8], sy[8];
#pragma unroll
      for (int j = sub; j < 8; j += WL::NSUB) {
        const int r = b0 + lane + 64 * j, i = r0 + (r < nr ? r : 0);
        yv[j] = y[i], lov[j] = L.lo[i], hiv[j] = L.hi[i], sy[j] = pend ? L.sumy[i] : 0.0;
      }
#pragma unroll
      for (int j = sub; j < 8; j += WL::NSUB) {
        const int r = b0 + lane + 64 * j;
        if (r < nr) {
          const int i      = r0 + r;
          const double yi  = yv[j];
          double next      = yi - (sigma * S.u.sums[lane + 64 * j][l]);
          const double low = next + sigma * lov[j];
          const double up  = next + sigma * hiv[j];
          next             = dmax(low, dmin(up, 0.0));
          yn[i]            = next;
          S.u.sums[lane + 64 * j][l] = next;
          const double dy = next - yi;
          acc[pass][0][j % VW] += dy * dy;
          if (pend) L.sumy[i] = sy[j] + weight * yi;
        }
      }
    }
    __syncthreads();
    const int rows = nr - b0 < kBT ? nr - b0 : kBT;
    for (int f = threadIdx.x; f < rows * K; f += kBT) yK[(size_t)(r0 + b0) * K + f] = S.u.sums[f / K][f % K];
    __syncthreads();
  }
  batch_block_partials<K, 1, VW>(S, acc, lp, true, W, w);
}

// rows of A^T for K LPs: AtY' = A^T y', interaction and ||dx||^2 partials (StepEpilogue)
template <int K, int VW>
__global__ void __launch_bounds__(kBT) kb_at_step(int W, const int32_t* __restrict__ row0, const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                                  const double* __restrict__ val, const BatchLp* __restrict__ lp, const double* __restrict__ yK)
{
  __shared__ BatchShared<K> S;
  using WL = WaveLps<K>;
  const int w = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, sub = WL::sub(wave);
  const int r0 = row0[w], nr = row0[w + 1] - r0;
  double acc[WL::PASSES][2][8];
#pragma unroll
  for (int pass = 0; pass < WL::PASSES; ++pass)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[pass][0][j] = 0.0, acc[pass][1][j] = 0.0;
  for (int b0 = 0; b0 < nr; b0 += kBT) {
    double s[BatchGeometry<K>::RU][2];
    batch_block_sums<K>(S, r0, nr, b0, off, idx, val, yK, s);
    batch_cross_over<K>(S, s);
#pragma unroll
    for (int pass = 0; pass < WL::PASSES; ++pass) {
      const int l     = WL::lp(wave, pass);
      const BatchLp L = lp[l];
      if (!loop_active(L.ctl)) continue;
      const int cur = L.ctl->cur;
      const double* __restrict__ x   = cur ? L.x1 : L.x0;
      const double* __restrict__ xn  = cur ? L.x0 : L.x1;
      const double* __restrict__ aty = cur ? L.aty1 : L.aty0;
      double* __restrict__ atyn      = cur ? L.aty0 : L.aty1;
      double xv[8], xnv[8], av[8];
#pragma unroll
      for (int j = sub; j < 8; j += WL::NSUB) {
        const int r = b0 + lane + 64 * j, i = r0 + (r < nr ? r : 0);
        xv[j] = x[i], xnv[j] = xn[i], av[j] = aty[i];
      }
#pragma unroll
      for (int j = sub; j < 8; j += WL::NSUB) {
        const int r = b0 + lane + 64 * j;
        if (r < nr) {
          const double v  = S.u.sums[lane + 64 * j][l];
          atyn[r0 + r]    = v;
          const double dx = xnv[j] - xv[j];
          const double t  = v - av[j];
          acc[pass][0][j % VW] += t * dx;
          acc[pass][1][j % VW] += dx * dx;
        }
      }
    }
    __syncthreads();
  }
  batch_block_partials<K, 2, VW>(S, acc, lp, false, W, w);
}

// ---- (2), (3) on the JAGGED layout (kernels_jag.hip, spmv_jag.hpp jag_block): the single kernels' workgroups, waves and passes -------
// A workgroup owns one block of the single layout, a wave its share of the sorted passes, a lane one row of a pass: the lane sums its row
// for all K LPs in diagonal order -- per entry one value and column, then the K values of that column as ONE contiguous piece of the
// interleaved vector (64 bytes at K = 8, 128 at K = 16: a block's column window times K stays in L2), and K sums in registers, each the
// single kernel's chain for its LP.  The LDS cannot hold K interleaved column windows; it holds the K row-sum strips instead (LP-major,
// an odd pitch P >= the block's rows), which is why a layout built for batches of up to L LPs caps its blocks at kJagBatchRows / L rows
// (jag_batch_rows).  The fused epilogue then runs thread <-> row as in jag_block: thread t takes rows t, t + T, ... of each LP in
// ascending order, so its accumulators are jag_block's and block_reduce<Op, K * NQ, WAVES> reduces every LP with jag_block's own tree.
// Blocks with rows longer than kLongRow (their own workgroups, partials after the blocks') and dense segments are not served: the
// batch refuses such a side (pdlpdev_batch_create).
// LDS hazards (round-7 audit, docs/design/10): strip[] is zeroed before barrier B1; every entry is then written by exactly one lane (the
// lane of its row's pass) and read behind B2 by the epilogue's thread of that row, which (A side) overwrites it with the row's y';
// the interleaved copy-out reads the strips behind B3.  red[] (after the strips, never aliased) takes each wave's sums of each LP from
// lane 0 of that wave, one entry per (wave, LP, quantity), and is read behind B4.  No barrier inside the passes.
template <int K, int WAVES>
struct JagBatchGeometry {
  // diagonals requested per round: U x K gathered values in flight per lane (16 waves: half as many, 128 VGPRs a lane)
  static constexpr int U = (WAVES == 16 ? 16 : 32) / K < 1 ? 1 : (WAVES == 16 ? 16 : 32) / K > 8 ? 8 : (WAVES == 16 ? 16 : 32) / K;
};

template <int K, int WAVES>
__device__ __forceinline__ void batch_jag_sums(const JagView& J, int blk, int P, const double* __restrict__ vK, double* strip)
{
  constexpr int U = JagBatchGeometry<K, WAVES>::U;
  const int lane     = threadIdx.x & 63;
  const int wave     = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g        = blk * WAVES + wave;
  const int wbase    = J.win[2 * blk];
  const int wlen     = J.win[2 * blk + 1];
  const int s0       = J.set_ptr[blk];
  int e              = __builtin_amdgcn_readfirstlane(J.tile_e[g]);
  const int sr0      = __builtin_amdgcn_readfirstlane(J.tile_sr[g]);
  const int ns       = __builtin_amdgcn_readfirstlane(J.tile_sr[g + 1]) - sr0;
  for (int p0 = 0; p0 < ns; p0 += 64) {
    const int i      = p0 + lane;
    const bool have  = i < ns;
    const unsigned d = have ? J.sr[sr0 + i] : 0u;
    const int cnt    = have ? (int)(d >> 16) + 1 : 0;
    const int lrow   = (int)(d & 0xFFFFu);
    double sum[K];
#pragma unroll
    for (int l = 0; l < K; ++l) sum[l] = 0.0;
    const int kmax = __builtin_amdgcn_readfirstlane(cnt);  // sorted: lane 0 holds the longest row of the pass
    for (int k0 = 0; k0 < kmax; k0 += U) {
      int at[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {  // diagonal k holds one entry per row longer than k: a prefix of the lanes
        at[u] = e;
        e += __builtin_popcountll(__ballot(cnt > k0 + u));
      }
      double a[U];
      unsigned sl[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        a[u] = 0.0, sl[u] = 0;
        if (cnt > k0 + u) {
          a[u]  = __builtin_nontemporal_load(J.val + at[u] + lane);
          sl[u] = __builtin_nontemporal_load(J.slot + at[u] + lane);
        }
      }
      unsigned col[U];  // the entry's column: the window's base + slot, or the block's column list at the slot
#pragma unroll
      for (int u = 0; u < U; ++u) col[u] = wlen ? (unsigned)wbase + sl[u] : (unsigned)J.set_col[s0 + (int)sl[u]];
      double2 xv[U][K / 2];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const double2* src = (const double2*)(vK + col[u] * (unsigned)K);
#pragma unroll
        for (int h = 0; h < K / 2; ++h) xv[u][h] = cnt > k0 + u ? src[h] : double2{0.0, 0.0};
      }
      // lanes past their row's end add +0.0 * 0.0, as in jag_block: no bit changes
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int h = 0; h < K / 2; ++h) {
          sum[2 * h]     = sum[2 * h] + a[u] * xv[u][h].x;
          sum[2 * h + 1] = sum[2 * h + 1] + a[u] * xv[u][h].y;
        }
    }
    if (have)
#pragma unroll
      for (int l = 0; l < K; ++l) strip[l * P + lrow] = sum[l];
  }
}

// the grid is jag_block's (nlong == 0: the row blocks only); false for the padding workgroups
__device__ __forceinline__ bool batch_jag_block(const JagView& J, int* blk)
{
  if ((int)blockIdx.x >= ((J.nblk + 7) & ~7)) return false;
  *blk = xcd_remap((int)blockIdx.x, J.nblk);
  return *blk < J.nblk;
}

// block_reduce<SumOp, NQ, WAVES> of LP l's accumulators, in two halves: the wave sums go to red[] (its own LDS, after the strips) as the
// epilogue finishes each LP ...
template <int NQ, int K>
__device__ __forceinline__ void batch_jag_wave_sums(double (&acc)[NQ], double* red, int l)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double v = wave_reduce<SumOp>(acc[q]);
    if (lane == 0) red[(wave * K + l) * NQ + q] = v;
  }
}
// ... and, behind a barrier, one thread per (LP, quantity) adds the waves' sums up in block_reduce's order
template <int K, int NQ, int WAVES>
__device__ __forceinline__ void batch_jag_partials(const double* red, const BatchLp* __restrict__ lp, bool a_side, int nparts, int blk)
{
  __syncthreads();  // (B4)
  if ((int)threadIdx.x < K * NQ) {
    const int l = threadIdx.x / NQ, q = threadIdx.x % NQ;
    const BatchLp& L = lp[l];
    if (loop_active(L.ctl)) {
      double total = red[l * NQ + q];
      for (int w = 1; w < WAVES; ++w) total = total + red[(w * K + l) * NQ + q];
      (a_side ? L.part_a : L.part_at)[(size_t)q * nparts + blk] = total;
    }
  }
}

// rows of A for K LPs on the jagged layout: DualEpilogue per LP (kb_a_dual's expressions), y' also interleaved into yK
template <int K, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) kbj_a_dual(JagView J, int P, const BatchLp* __restrict__ lp, const double* __restrict__ xK, double* __restrict__ yK)
{
  extern __shared__ __attribute__((aligned(16))) double kbj_lds[];
  constexpr int T = WAVES * 64;
  double* red = kbj_lds + K * P;
  int blk;
  if (!batch_jag_block(J, &blk)) return;
  const int row0 = J.row0[blk], brows = J.row0[blk + 1] - row0;
  for (int f = threadIdx.x; f < K * P; f += T) kbj_lds[f] = 0.0;  // rows without nonzeros
  __syncthreads();  // (B1)
  batch_jag_sums<K, WAVES>(J, blk, P, xK, kbj_lds);
  __syncthreads();  // (B2: the strips are complete)
  for (int l = 0; l < K; ++l) {
    const BatchLp& L = lp[l];
    if (!loop_active(L.ctl)) continue;
    const int cur      = L.ctl->cur;
    const double sigma = L.ctl->sigma, weight = L.ctl->step_size;
    const bool pend    = L.ctl->pending_avg != 0;
    const double* __restrict__ y = cur ? L.y1 : L.y0;
    double* __restrict__ yn      = cur ? L.y0 : L.y1;
    double acc[1]                = {0.0};
    for (int r = threadIdx.x; r < brows; r += T) {
      const int i = row0 + r;
      if (i >= J.rows) continue;
      const double yi  = y[i];
      const double lo  = L.lo[i], hi = L.hi[i], sy = pend ? L.sumy[i] : 0.0;
      double next      = yi - (sigma * kbj_lds[l * P + r]);
      const double low = next + sigma * lo;
      const double up  = next + sigma * hi;
      next             = dmax(low, dmin(up, 0.0));
      yn[i]            = next;
      kbj_lds[l * P + r] = next;  // (this thread's own entry: read just above)
      const double dy = next - yi;
      acc[0] += dy * dy;
      if (pend) L.sumy[i] = sy + weight * yi;
    }
    batch_jag_wave_sums<1, K>(acc, red, l);
  }
  __syncthreads();  // (B3: y' of every LP in the strips) -> whole entries of the interleaved vector
  for (int f = threadIdx.x; f < brows * K; f += T) yK[(size_t)row0 * K + f] = kbj_lds[(f % K) * P + f / K];
  batch_jag_partials<K, 1, WAVES>(red, lp, true, J.nblk, blk);
}

// rows of A^T for K LPs on the jagged layout: StepEpilogue per LP
template <int K, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) kbj_at_step(JagView J, int P, const BatchLp* __restrict__ lp, const double* __restrict__ yK)
{
  extern __shared__ __attribute__((aligned(16))) double kbj_lds[];
  constexpr int T = WAVES * 64;
  double* red = kbj_lds + K * P;
  int blk;
  if (!batch_jag_block(J, &blk)) return;
  const int row0 = J.row0[blk], brows = J.row0[blk + 1] - row0;
  for (int f = threadIdx.x; f < K * P; f += T) kbj_lds[f] = 0.0;
  __syncthreads();  // (B1)
  batch_jag_sums<K, WAVES>(J, blk, P, yK, kbj_lds);
  __syncthreads();  // (B2)
  for (int l = 0; l < K; ++l) {
    const BatchLp& L = lp[l];
    if (!loop_active(L.ctl)) continue;
    const int cur = L.ctl->cur;
    const double* __restrict__ x   = cur ? L.x1 : L.x0;
    const double* __restrict__ xn  = cur ? L.x0 : L.x1;
    const double* __restrict__ aty = cur ? L.aty1 : L.aty0;
    double* __restrict__ atyn      = cur ? L.aty0 : L.aty1;
    double acc[2]                  = {0.0, 0.0};
    for (int r = threadIdx.x; r < brows; r += T) {
      const int j = row0 + r;
      if (j >= J.rows) continue;
      const double v  = kbj_lds[l * P + r];
      atyn[j]         = v;
      const double dx = xn[j] - x[j];
      const double t  = v - aty[j];
      acc[0] += t * dx;
      acc[1] += dx * dx;
    }
    batch_jag_wave_sums<2, K>(acc, red, l);
  }
  batch_jag_partials<K, 2, WAVES>(red, lp, false, J.nblk, blk);
}

// columns ascending within every row?  (the panels add a row's products slab by slab = by ascending column; the batched products
// walk the CSR row: the same order only then)
__global__ void __launch_bounds__(256) kb_check_sorted(int rows, const int32_t* __restrict__ off, const int32_t* __restrict__ idx, int* __restrict__ bad)
{
  for (int i = blockIdx.x * 256 + threadIdx.x; i < rows; i += gridDim.x * 256)
    for (int k = off[i] + 1; k < off[i + 1]; ++k)
      if (idx[k] <= idx[k - 1]) *bad = 1;
}

}  // namespace

struct pdlpdev_batch {
  int K = 0, device = 0;
  hipStream_t stream = nullptr;
  pdlpdev_ctx* ctx[kBatchMax] = {nullptr};
  BatchLp* lp_dev = nullptr;
  pdlpdev_decision_args* dargs_dev = nullptr;
  std::vector<pdlpdev_decision_args> dargs_host;  // (refreshed with the table: pdlpdev_set_step_params of a member after the batch was made)
  double *xK = nullptr, *yK = nullptr;
  // the row blocks whose partial sums the products reproduce: the panels of the single-LP layout (512 "threads"), or the row blocks
  // of the CSR stream kernels (256)
  // ... or the blocks of the jagged layout (kbj_*: the strips of K LPs, pitch P, `lds` bytes of dynamic LDS)
  struct Side {
    int W = 0;
    const int32_t* row0 = nullptr;
    bool panel = false;
    bool jag = false;
    JagView jv{};
    int P = 0;
    size_t lds = 0;
  } a_side, t_side;
  std::vector<BatchLp> lp_host;  // what lp_dev holds
  // every member in reflected Halpern mode (kernels_batch_halpern.hip): the second per-LP table, kept current as the first is
  bool halpern = false;
  BatchHalpernLp* hl_dev = nullptr;
  std::vector<BatchHalpernLp> hl_host;
  // ... and the third, of the K-wide ray pass (kernels_batch_halpern_ray.hip; pdlpdev_batch_halpern_rays)
  BatchRayLp* ray_dev = nullptr;
  std::vector<BatchRayLp> ray_host;
  int64_t ray_wide = 0, ray_served = 0;  // K-wide passes enqueued, member passes they served
  int64_t ray_single0[kBatchMax] = {0};  // the members' own counts of single passes when they joined
  std::map<int, hipGraphExec_t> graphs;
};

static BatchLp batch_lp_of(const pdlpdev_ctx* c)
{
  return BatchLp{c->ctl, c->y[0], c->y[1], c->sumy, c->lo, c->hi, c->x[0], c->x[1], c->aty[0], c->aty[1], c->sumx, c->c, c->lb, c->ub, c->ubd, c->A.part, c->At.part};
}

static BatchHalpernLp batch_halpern_lp_of(const pdlpdev_ctx* c) { return BatchHalpernLp{c->hal, c->avgx, c->avgy, c->lrx, c->lry, c->lraty}; }

static BatchRayLp batch_ray_lp_of(const pdlpdev_ctx* c)
{
  return BatchRayLp{c->ctl, c->avgx, c->avgy, c->x[0], c->x[1], c->y[0], c->y[1], c->tmp_n, c->tmp_m, c->ax_u[PDLPDEV_CURRENT], c->aty_u[PDLPDEV_CURRENT],
                    c->lo_u, c->hi_u, c->lb_u, c->ub_u, c->part_g, c->scal};
}

// A reset that gives a member row bounds of its own moves its lo / hi (pdlpdev_reset: copy on change): the table the kernels read
// follows (the kernels -- and the captured graphs -- take the table's address, not its contents).
static int batch_refresh_table(pdlpdev_batch* b)
{
  bool changed = false;
  for (int l = 0; l < b->K; ++l) {
    const BatchLp now = batch_lp_of(b->ctx[l]);
    if (memcmp(&now, &b->lp_host[l], sizeof(BatchLp)) != 0) b->lp_host[l] = now, changed = true;
  }
  bool hl_changed = false;
  for (int l = 0; b->halpern && l < b->K; ++l) {
    const BatchHalpernLp now = batch_halpern_lp_of(b->ctx[l]);
    if (memcmp(&now, &b->hl_host[l], sizeof(BatchHalpernLp)) != 0) b->hl_host[l] = now, hl_changed = true;
  }
  if (hl_changed) HIP_TRY(hipMemcpyAsync(b->hl_dev, b->hl_host.data(), b->K * sizeof(BatchHalpernLp), hipMemcpyHostToDevice, b->stream));
  bool ray_changed = false;  // (the ray pass's table: a reset may move a member's unscaled row bounds as well)
  for (int l = 0; b->halpern && l < b->K; ++l) {
    const BatchRayLp now = batch_ray_lp_of(b->ctx[l]);
    if (memcmp(&now, &b->ray_host[l], sizeof(BatchRayLp)) != 0) b->ray_host[l] = now, ray_changed = true;
  }
  if (ray_changed) {
    HIP_TRY(hipMemcpyAsync(b->ray_dev, b->ray_host.data(), b->K * sizeof(BatchRayLp), hipMemcpyHostToDevice, b->stream));
    hl_changed = true;  // (waited for below, as the other tables are)
  }
  bool sp_changed = false;  // (the step-size exponents travel by value in the decision kernel's arguments)
  for (int l = 0; l < b->K; ++l)
    if (memcmp(&b->dargs_host[l].sp, &b->ctx[l]->sp, sizeof(pdlpdev_step_params)) != 0) b->dargs_host[l].sp = b->ctx[l]->sp, sp_changed = true;
  if (changed) HIP_TRY(hipMemcpyAsync(b->lp_dev, b->lp_host.data(), b->K * sizeof(BatchLp), hipMemcpyHostToDevice, b->stream));
  if (sp_changed)  // (the attempt graphs carry the POINTER to this table, not its contents: no re-capture)
    HIP_TRY(hipMemcpyAsync(b->dargs_dev, b->dargs_host.data(), b->K * sizeof(pdlpdev_decision_args), hipMemcpyHostToDevice, b->stream));
  if (changed || sp_changed || hl_changed) HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

static int batch_fetch_ctl(pdlpdev_batch* b)
{
  for (int l = 0; l < b->K; ++l)
    HIP_TRY(hipMemcpyAsync(b->ctx[l]->ctl_h, b->ctx[l]->ctl, sizeof(pdlpdev_ctl), hipMemcpyDeviceToHost, b->stream));
  for (int l = 0; b->halpern && l < b->K; ++l)  // (the Halpern scalars come back with the control block: pdlpdev_get_halpern reads hal_h)
    HIP_TRY(hipMemcpyAsync(b->ctx[l]->hal_h, b->ctx[l]->hal, sizeof(pdlpdev_halpern), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

template <int K>
static const void* batch_jag_kernel(const pdlpdev_batch::Side& S, bool a_side)
{
  if (a_side) return S.jv.waves == 16 ? (const void*)kbj_a_dual<K, 16> : (const void*)kbj_a_dual<K, 8>;
  return S.jv.waves == 16 ? (const void*)kbj_at_step<K, 16> : (const void*)kbj_at_step<K, 8>;
}

// (ev != nullptr: the four dispatches carry start / stop events -- hipExtLaunchKernel's own timestamps, no records between them)
template <int K>
static int batch_enqueue_attempt(pdlpdev_batch* b, hipEvent_t* ev = nullptr)
{
  hipStream_t s   = b->stream;
  pdlpdev_ctx* c0 = b->ctx[0];
  int n           = c0->n;
  int aw = b->a_side.W, tw = b->t_side.W;
  const int32_t *arow0 = b->a_side.row0, *trow0 = b->t_side.row0;
  const bool ap = b->a_side.panel, tp = b->t_side.panel;
  const int pgrid = std::min((n + kBT - 1) / kBT, 4096);
  // per side: the CSR-walking products (panels / CSR stream), or the jagged layout's
  const pdlpdev_batch::Side &A = b->a_side, &T = b->t_side;
  auto jgrid = [](const pdlpdev_batch::Side& S) { return dim3((S.jv.nblk + 7) & ~7); };
  if (b->halpern) {  // kb_primal as it is (pending_avg stays 0), then the Halpern products and the K decisions (never jagged, never timed here)
    kb_primal<K><<<pgrid, kBT, 0, s>>>(b->lp_dev, n, b->xK);
    LAUNCH_CHECK();
    const BatchProductSide ps{aw, arow0, ap, c0->A.hot.off, c0->A.hot.idx, c0->A.hot.val}, pt{tw, trow0, tp, c0->At.hot.off, c0->At.hot.idx, c0->At.hot.val};
    return batch_halpern_enqueue_tail(K, s, ps, pt, b->lp_dev, b->hl_dev, b->xK, b->yK);
  }
  if (ev) {
    JagView ajv = A.jv, tjv = T.jv;
    int aP = A.P, tP = T.P;
    void* a0[] = {&b->lp_dev, &n, &b->xK};
    void* a1[] = {&aw, &arow0, &c0->A.hot.off, &c0->A.hot.idx, &c0->A.hot.val, &b->lp_dev, &b->xK, &b->yK};
    void* a2[] = {&tw, &trow0, &c0->At.hot.off, &c0->At.hot.idx, &c0->At.hot.val, &b->lp_dev, &b->yK};
    void* j1[] = {&ajv, &aP, &b->lp_dev, &b->xK, &b->yK};
    void* j2[] = {&tjv, &tP, &b->lp_dev, &b->yK};
    void* a3[] = {&b->dargs_dev};
    HIP_TRY(hipExtLaunchKernel((const void*)kb_primal<K>, dim3(pgrid), dim3(kBT), a0, 0, s, ev[0], ev[1], 0));
    if (A.jag)
      HIP_TRY(hipExtLaunchKernel(batch_jag_kernel<K>(A, true), jgrid(A), dim3(A.jv.waves * 64), j1, A.lds, s, ev[2], ev[3], 0));
    else
      HIP_TRY(hipExtLaunchKernel(ap ? (const void*)kb_a_dual<K, 8> : (const void*)kb_a_dual<K, 4>, dim3(aw), dim3(kBT), a1, 0, s, ev[2], ev[3], 0));
    if (T.jag)
      HIP_TRY(hipExtLaunchKernel(batch_jag_kernel<K>(T, false), jgrid(T), dim3(T.jv.waves * 64), j2, T.lds, s, ev[4], ev[5], 0));
    else
      HIP_TRY(hipExtLaunchKernel(tp ? (const void*)kb_at_step<K, 8> : (const void*)kb_at_step<K, 4>, dim3(tw), dim3(kBT), a2, 0, s, ev[4], ev[5], 0));
    HIP_TRY(hipExtLaunchKernel((const void*)k_step_decision_batch, dim3(K), dim3(1024), a3, 0, s, ev[6], ev[7], 0));
    return 0;
  }
  kb_primal<K><<<pgrid, kBT, 0, s>>>(b->lp_dev, n, b->xK);
  if (A.jag && A.jv.waves == 16) kbj_a_dual<K, 16><<<jgrid(A), 1024, A.lds, s>>>(A.jv, A.P, b->lp_dev, b->xK, b->yK);
  else if (A.jag) kbj_a_dual<K, 8><<<jgrid(A), 512, A.lds, s>>>(A.jv, A.P, b->lp_dev, b->xK, b->yK);
  else if (ap) kb_a_dual<K, 8><<<aw, kBT, 0, s>>>(aw, arow0, c0->A.hot.off, c0->A.hot.idx, c0->A.hot.val, b->lp_dev, b->xK, b->yK);
  else kb_a_dual<K, 4><<<aw, kBT, 0, s>>>(aw, arow0, c0->A.hot.off, c0->A.hot.idx, c0->A.hot.val, b->lp_dev, b->xK, b->yK);
  if (T.jag && T.jv.waves == 16) kbj_at_step<K, 16><<<jgrid(T), 1024, T.lds, s>>>(T.jv, T.P, b->lp_dev, b->yK);
  else if (T.jag) kbj_at_step<K, 8><<<jgrid(T), 512, T.lds, s>>>(T.jv, T.P, b->lp_dev, b->yK);
  else if (tp) kb_at_step<K, 8><<<tw, kBT, 0, s>>>(tw, trow0, c0->At.hot.off, c0->At.hot.idx, c0->At.hot.val, b->lp_dev, b->yK);
  else kb_at_step<K, 4><<<tw, kBT, 0, s>>>(tw, trow0, c0->At.hot.off, c0->At.hot.idx, c0->At.hot.val, b->lp_dev, b->yK);
  k_step_decision_batch<<<K, 1024, 0, s>>>(b->dargs_dev);
  LAUNCH_CHECK();
  return 0;
}

static int batch_enqueue(pdlpdev_batch* b, hipEvent_t* ev = nullptr)
{
  return b->K == 16  ? batch_enqueue_attempt<16>(b, ev)
         : b->K == 8 ? batch_enqueue_attempt<8>(b, ev)
         : b->K == 4 ? batch_enqueue_attempt<4>(b, ev)
                     : batch_enqueue_attempt<2>(b, ev);
}

static int batch_graph(pdlpdev_batch* b, int attempts, hipGraphExec_t* out)
{
  auto it = b->graphs.find(attempts);
  if (it != b->graphs.end()) {
    *out = it->second;
    return 0;
  }
  hipGraph_t graph;
  HIP_TRY(hipStreamBeginCapture(b->stream, hipStreamCaptureModeThreadLocal));
  int rc = 0;
  for (int i = 0; i < attempts && rc == 0; ++i) rc = batch_enqueue(b);
  hipError_t e = hipStreamEndCapture(b->stream, &graph);
  if (rc != 0) return rc;
  HIP_TRY(e);
  hipGraphExec_t exec;
  HIP_TRY(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
  HIP_TRY(hipGraphDestroy(graph));
  b->graphs[attempts] = exec;
  *out                = exec;
  return 0;
}

// `count` lockstep attempts on the batch's stream, in the single loop's power-of-two chunks: graph replays or plain launches
static int batch_enqueue_attempts(pdlpdev_batch* b, int count)
{
  const bool use_graph = b->ctx[0]->use_graph != 0;
  for (int remaining = count, chunk; remaining > 0; remaining -= chunk) {
    chunk = attempt_chunk(remaining);
    if (use_graph) {
      hipGraphExec_t g;
      TRY(batch_graph(b, chunk, &g));
      HIP_TRY(hipGraphLaunch(g, b->stream));
    } else {
      for (int i = 0; i < chunk; ++i) TRY(batch_enqueue(b));
    }
  }
  return 0;
}

extern "C" {

// A context for ANOTHER LP over the same matrix and objective.  The clone takes the parent's CtxProblem whole -- matrices, layouts, scaling
// vectors, c and the stream are the parent's arrays, which must outlive it -- and starts every other field from its initialiser: what it takes
// from the parent beyond that is carried over below, line by line.  Bounds: own copies of the variable bounds, the parent's row bounds until a
// reset brings others (resets of either side are fine).  pdlpdev_reset(clone, lb, ub, lo, hi) gives it its own bounds and start, bit for bit the
// state of a freshly created context of that LP (tests/test_persistent_resolve_gpu.py pins reset against a fresh solver).
int pdlpdev_clone_shared(pdlpdev_ctx** out, pdlpdev_ctx* parent)
{
  if (!out || !parent) return fail(-1, "pdlpdev_clone_shared: null argument");
  if (!parent->scaled) return fail(-1, "pdlpdev_clone_shared: the parent has not been scaled yet");
  if (parent->comm || parent->small_resident || parent->dense.on) return fail(-7, "pdlpdev_clone_shared: not for sharded, resident or dense-segment contexts");
  HIP_TRY(hipSetDevice(parent->device));
  HIP_TRY(hipStreamSynchronize(parent->stream));
  pdlpdev_ctx* c = new pdlpdev_ctx();
  *out           = c;
  static_cast<CtxProblem&>(*c) = *parent;  // (pointers to the shared arrays, geometry, switches: by value)
  c->shared_with_parent = true;  // (c->parent is set once the row bounds are aliased: a clone that fails before is destroyed without touching the parent's count)
  c->ubd       = parent->ubd;        // the bounds below are the parent's: so is what is known about their uniformity
  c->sp        = parent->sp;         // the step rule's exponents and smoothing (pdlpdev_set_step_params)
  c->use_graph = parent->use_graph;  // pdlpdev_set_graph_mode
  HIP_TRY(hipHostMalloc((void**)&c->scal_h, kScalars * sizeof(double) + sizeof(pdlpdev_ctl)));
  c->ctl_h = (pdlpdev_ctl*)(c->scal_h + kScalars);
  HIP_TRY(hipMalloc((void**)&c->arena, kArenaChunk));
  HIP_TRY(hipMemsetAsync(c->arena, 0, kArenaChunk, c->stream));
  c->first_chunk = c->arena;
  TRY(lp_alloc_slab(c));
  auto own_copy = [&](double** p, const double* src, size_t count) -> int {  // an own buffer holding what the parent's holds
    TRY(dev_alloc(c, p, count));
    HIP_TRY(hipMemcpyAsync(*p, src, count * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return 0;
  };
  const size_t n = (size_t)c->n;
  TRY(own_copy(&c->lb, parent->lb, n)); TRY(own_copy(&c->lb_u, parent->lb_u, n)); TRY(own_copy(&c->ub, parent->ub, n)); TRY(own_copy(&c->ub_u, parent->ub_u, n));
  // lo, hi and their unscaled twins are the parent's until a reset brings other row bounds: pdlpdev_reset makes the copies then
  c->lo = parent->lo, c->hi = parent->hi, c->lo_u = parent->lo_u, c->hi_u = parent->hi_u;
  c->rows_aliased = true, c->parent = parent;
  parent->clones_alive += 1;
  parent->rows_private = false;  // (this clone aliases the parent's CURRENT row bounds)
  TRY(lp_alloc_iterate(c));
  TRY(lp_alloc_partials(c));
  HIP_TRY(hipMemcpyAsync(c->ctl, parent->ctl, sizeof(pdlpdev_ctl), hipMemcpyDeviceToDevice, c->stream));  // step size, primal weight, counters: the parent's
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// K = 2, 4, 8 or 16 contexts over ONE matrix (ctx[0] and its clones, or contexts that alias the same arrays) advance together.  -7: the
// layouts are not the ones whose reduction trees the batched products reproduce (the caller keeps its independent solves).
int pdlpdev_batch_create(pdlpdev_batch** out, pdlpdev_ctx** ctx, int K)
{
  if (!out || !ctx || (K != 2 && K != 4 && K != 8 && K != 16)) return fail(-1, "pdlpdev_batch_create: K must be 2, 4, 8 or 16");
  pdlpdev_ctx* c0 = ctx[0];
  for (int l = 0; l < K; ++l)
    for (int q = 0; q < l; ++q)
      if (ctx[q] == ctx[l]) return fail(-1, "pdlpdev_batch_create: LP %d and LP %d are the same context (two lanes would share one set of iterates)", q, l);
  for (int l = 0; l < K; ++l) {
    pdlpdev_ctx* c = ctx[l];
    if (!c || c->A.hot.off != c0->A.hot.off || c->At.hot.off != c0->At.hot.off || c->A.pan.v.row0 != c0->A.pan.v.row0 || c->A.jag.v.row0 != c0->A.jag.v.row0 ||
        c->At.jag.v.row0 != c0->At.jag.v.row0 || c->A.jag.v.val != c0->A.jag.v.val || c->At.jag.v.val != c0->At.jag.v.val || c->stream != c0->stream)
      return fail(-1, "pdlpdev_batch_create: the contexts do not share one matrix (pdlpdev_clone_shared)");
  }
  // all K in reflected Halpern mode (kernels_batch_halpern.hip) or none; the caller opts in (cuoptamd_settings::halpern_lockstep)
  int nhalpern = 0;
  for (int l = 0; l < K; ++l) nhalpern += ctx[l]->halpern ? 1 : 0;
  if (nhalpern != 0 && nhalpern != K)
    return fail(-7, "pdlpdev_batch_create: not eligible (the batch mixes %d contexts in reflected Halpern mode with %d in the averaging iteration: a lockstep "
                    "attempt runs one of the two)", nhalpern, K - nhalpern);
  const bool halpern = nhalpern == K;
  for (int l = 0; halpern && l < K; ++l)
    if (!ctx[l]->hal || !ctx[l]->hal_h || !ctx[l]->lraty) return fail(-1, "pdlpdev_batch_create: LP %d is in reflected Halpern mode without its anchor (pdlpdev_set_halpern)", l);
  if ((int64_t)std::max(c0->m, c0->n) * K >= ((int64_t)1 << 32))
    return fail(-7, "pdlpdev_batch_create: not eligible (the interleaved vectors are addressed with 32-bit element offsets: max(m, n) * K < 2^32)");
  // per side: the row-sum variant of the panels, the CSR stream layout or the jagged layout -- the three whose rows are summed by one lane
  // and whose per-block reduction the batched products reproduce
  pdlpdev_batch::Side side[2];
  HIP_TRY(hipSetDevice(c0->device));
  const pdlpdev_ctx::MatrixSide* const matrix[2] = {&c0->A, &c0->At};
  for (int t = 0; t < 2; ++t) {
    const pdlpdev_ctx::MatrixSide& M = *matrix[t];
    const pdlpdev_ctx::Panels& P = M.pan;
    const pdlpdev_ctx::Jag& Jg = M.jag;
    const bool jag = Jg.on, pb = M.pb.on;
    const int nlong = M.nlong;
    if (jag && halpern)
      return fail(-7, "pdlpdev_batch_create: not eligible (the %s side is in the jagged layout: the reflected Halpern mode has lockstep products for the "
                      "row-sum panels and the CSR stream layout only)", M.name);
    if (jag && c0->batch_lanes < K)
      return fail(-7, "pdlpdev_batch_create: not eligible (the %s side is in the jagged layout: lockstep batches of %d LPs on it need a parent created "
                      "with batch_lanes >= %d, cuoptamd_settings::batch_lanes; this one has %d)", M.name, K, K, c0->batch_lanes);
    bool ok = !pb && nlong == 0;
    if (ok && jag) {
      if (Jg.v.nlong != 0 || Jg.v.dense_add || Jg.v.nblk <= 0)
        return fail(-7, "pdlpdev_batch_create: not eligible (the %s side is jagged with %d rows of more than %d entries%s: the jagged lockstep "
                        "products serve blocks of short rows only)", M.name, Jg.v.nlong, kLongRow, Jg.v.dense_add ? " and dense segments" : "");
      {  // the strips' pitch: odd (conflict-free transposition), at least the largest block's rows
        std::vector<int32_t> r0((size_t)Jg.v.nblk + 1);
        HIP_TRY(hipMemcpyAsync(r0.data(), Jg.v.row0, r0.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c0->stream));
        HIP_TRY(hipStreamSynchronize(c0->stream));
        int rmax = 1;
        for (int q = 0; q < Jg.v.nblk; ++q) rmax = std::max(rmax, r0[q + 1] - r0[q]);
        pdlpdev_batch::Side S;
        S.W = Jg.v.nblk, S.jag = true, S.jv = Jg.v, S.P = rmax | 1;
        S.lds = sizeof(double) * ((size_t)K * S.P + (size_t)Jg.v.waves * K * 2);  // (the strips, then the wave sums)
        if (S.lds > 160 * 1024) return fail(-1, "pdlpdev_batch_create: %d rows in one jagged block do not leave LDS for %d LPs", rmax, K);
        side[t] = S;
      }
    } else if (ok && P.on) {
      ok      = !P.v.seg && !P.v.own_row && !P.v.any_long && !P.v.dense_add;
      side[t] = pdlpdev_batch::Side{P.v.W, P.v.row0, true};
    } else if (ok) {
      side[t] = pdlpdev_batch::Side{M.nb, M.rb, false};
      ok      = side[t].W > 0 && side[t].row0 != nullptr;
    }
    if (!ok || c0->dense.on || c0->comm || c0->small_resident)
      return fail(-7, "pdlpdev_batch_create: not eligible (%s side: %s; the batched products reproduce the reductions of the row-sum panels, of the CSR stream "
                      "kernels and of the jagged layout: both matrices in one of these layouts, no row of more than %d entries, no dense segments, one "
                      "GPU, not the resident small-LP loop)", M.name,
                      pb ? "gather-free layout" : nlong ? "rows longer than kLongRow" : P.on ? "panels of the long-tail / own-row variant" : "CSR stream", kLongRow);
  }
  {
    struct Flag {  // (released on every way out)
      int* p = nullptr;
      ~Flag() { if (p) (void)hipFree(p); }
    } flag;
    HIP_TRY(hipMalloc((void**)&flag.p, sizeof(int)));
    int* bad = flag.p;
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), c0->stream));
    // (the jagged products walk a row in its CSR order, as the single kernel does: no condition there)
    if (!side[0].jag) kb_check_sorted<<<2048, 256, 0, c0->stream>>>(c0->m, c0->A.hot.off, c0->A.hot.idx, bad);
    if (!side[1].jag) kb_check_sorted<<<2048, 256, 0, c0->stream>>>(c0->n, c0->At.hot.off, c0->At.hot.idx, bad);
    LAUNCH_CHECK();
    int h = 0;
    HIP_TRY(hipMemcpyAsync(&h, bad, sizeof(int), hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream));
    if (h) return fail(-7, "pdlpdev_batch_create: not eligible (column indices are not ascending within the rows)");
  }
  for (int t = 0; t < 2; ++t)  // (the jagged products' strips: dynamic LDS beyond the default limit; the attribute is per kernel and device)
    if (side[t].jag) {
      const void* f = K == 16 ? batch_jag_kernel<16>(side[t], t == 0) : K == 8 ? batch_jag_kernel<8>(side[t], t == 0)
                    : K == 4  ? batch_jag_kernel<4>(side[t], t == 0)  : batch_jag_kernel<2>(side[t], t == 0);
      HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    }
  pdlpdev_batch* b = new pdlpdev_batch();
  *out      = b;
  b->K = K, b->device = c0->device, b->stream = c0->stream;
  b->a_side = side[0], b->t_side = side[1];
  b->halpern = halpern;
  std::vector<BatchLp>& h = b->lp_host;
  h.resize(K);
  std::vector<pdlpdev_decision_args>& dargs = b->dargs_host;
  dargs.resize(K);
  for (int l = 0; l < K; ++l) {
    pdlpdev_ctx* c = ctx[l];
    b->ctx[l]      = c;
    h[l]     = batch_lp_of(c);
    if (halpern) b->hl_host.push_back(batch_halpern_lp_of(c)), b->ray_host.push_back(batch_ray_lp_of(c));
    b->ray_single0[l] = c->stat_single_rays;
    dargs[l] = pdlpdev_decision_args{c->ctl, c->A.part, side[0].W, c->At.part, side[1].W, c->sp};
    c->batches_alive += 1, c->lockstep_batches_alive += 1;
  }
  HIP_TRY(hipMalloc((void**)&b->lp_dev, K * sizeof(BatchLp)));
  HIP_TRY(hipMalloc((void**)&b->xK, ((size_t)c0->n * K + 64) * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&b->yK, ((size_t)c0->m * K + 64) * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&b->dargs_dev, K * sizeof(pdlpdev_decision_args)));
  // everything on the batch's OWN stream (a non-blocking one: work of the null stream -- hipMemset, hipMemcpy -- is not ordered
  // with it, and a memset that the queue scheduler lets wait can land attempts later, in the middle of a product's vectors)
  HIP_TRY(hipMemcpyAsync(b->lp_dev, h.data(), K * sizeof(BatchLp), hipMemcpyHostToDevice, b->stream));
  if (halpern) {
    HIP_TRY(hipMalloc((void**)&b->hl_dev, K * sizeof(BatchHalpernLp)));
    HIP_TRY(hipMemcpyAsync(b->hl_dev, b->hl_host.data(), K * sizeof(BatchHalpernLp), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMalloc((void**)&b->ray_dev, K * sizeof(BatchRayLp)));
    HIP_TRY(hipMemcpyAsync(b->ray_dev, b->ray_host.data(), K * sizeof(BatchRayLp), hipMemcpyHostToDevice, b->stream));
  }
  HIP_TRY(hipMemcpyAsync(b->dargs_dev, dargs.data(), K * sizeof(pdlpdev_decision_args), hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipMemsetAsync(b->xK, 0, ((size_t)c0->n * K + 64) * sizeof(double), b->stream));
  HIP_TRY(hipMemsetAsync(b->yK, 0, ((size_t)c0->m * K + 64) * sizeof(double), b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

void pdlpdev_batch_destroy(pdlpdev_batch* b)
{
  if (!b) return;
  for (int l = 0; l < b->K; ++l)
    if (b->ctx[l]) b->ctx[l]->batches_alive -= 1, b->ctx[l]->lockstep_batches_alive -= 1;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  for (auto& kv : b->graphs) (void)hipGraphExecDestroy(kv.second);
  if (b->lp_dev) (void)hipFree(b->lp_dev);
  if (b->hl_dev) (void)hipFree(b->hl_dev);
  if (b->ray_dev) (void)hipFree(b->ray_dev);
  if (b->dargs_dev) (void)hipFree(b->dargs_dev);
  if (b->xK) (void)hipFree(b->xK);
  if (b->yK) (void)hipFree(b->yK);
  delete b;
}

// Attempts for all K LPs until LP l holds targets[l] accepted steps (targets[l] <= 0: LP l rests; an LP that reaches its target
// rests too: its lanes and its per-LP kernels turn into no-ops).  ctl[l] receives LP l's control block.
int pdlpdev_batch_run(pdlpdev_batch* b, const int32_t* targets, pdlpdev_ctl* ctl)
{
  if (!b || !targets) return fail(-1, "pdlpdev_batch_run: null argument");
  roctx::Range range("pdlp: batched PDHG attempts");
  HIP_TRY(hipSetDevice(b->device));
  TRY(batch_refresh_table(b));
  const int K = b->K;
  for (int l = 0; l < K; ++l) loop_state_touched(b->ctx[l]);  // (the batch's kernels move the contexts' iterates and control blocks)
  for (int l = 0; l < K; ++l)
    if (targets[l] > 0) k_set_target<<<1, 1, 0, b->stream>>>(b->ctx[l]->ctl, targets[l]);
  LAUNCH_CHECK();
  TRY(batch_fetch_ctl(b));
  auto wants = [&](int l) { return targets[l] > 0 && b->ctx[l]->ctl_h->error == 0 && b->ctx[l]->ctl_h->steps_taken < targets[l]; };
  int guard = 0;
  for (;;) {
    int remaining = 0;
    int before[kBatchMax], asked[kBatchMax];
    for (int l = 0; l < K; ++l) {
      before[l] = b->ctx[l]->ctl_h->steps_taken;
      asked[l]  = wants(l) ? targets[l] - before[l] : 0;
      remaining = std::max(remaining, asked[l]);
    }
    if (remaining == 0) break;
    TRY(batch_enqueue_attempts(b, remaining));
    TRY(batch_fetch_ctl(b));
    // (the single loop's rule, per LP: too_many_rejections; a Halpern step is never rejected)
    for (int l = 0; !b->halpern && l < K; ++l) {
      if (asked[l] == 0 || !too_many_rejections(b->ctx[l], before[l], asked[l])) continue;
      k_set_error<<<1, 1, 0, b->stream>>>(b->ctx[l]->ctl);
      LAUNCH_CHECK();
    }
    if (!b->halpern) TRY(batch_fetch_ctl(b));  // (k_set_error may have run; in Halpern mode nothing moved since the fetch above)
    if (++guard > 100000) return fail(-6, "pdlpdev_batch_run: no progress");
  }
  // (the pinned control blocks are what the device holds until something moves a member again: pdlpdev_batch_halpern_rays reads them)
  for (int l = 0; l < K; ++l) b->ctx[l]->batch_ctl_fresh = true;
  if (ctl)
    for (int l = 0; l < K; ++l) ctl[l] = *b->ctx[l]->ctl_h;
  return 0;
}

// Parity hook, the batch twin of pdlpdev_debug_attempts: EXACTLY `count` (1 .. 64) lockstep attempts as one round of pdlpdev_batch_run
// enqueues them (the same power-of-two chunks, graph replay or plain launches), one read-back, that round's rejected_in_a_row
// bookkeeping -- and NO make-up round, so a rejected member's trial iterate is there to be looked at next to the accepted members'.
// Members with on[l] != 0 (on == NULL: all) and no error aim at steps_taken + count; the others REST: a target a resting member still
// holds beyond its steps_taken (a rejection in an earlier round of this hook) is taken back to steps_taken, nothing else of it is
// touched.  ctl[l] receives LP l's control block.  -7: a batch in reflected Halpern mode.
int pdlpdev_debug_batch_attempts(pdlpdev_batch* b, int count, const int32_t* on, pdlpdev_ctl* ctl)
{
  if (!b) return fail(-1, "pdlpdev_debug_batch_attempts: null argument");
  if (b->halpern) return fail(-7, "pdlpdev_debug_batch_attempts: the averaging attempt only (not a batch in reflected Halpern mode)");
  if (count < 1 || count > 64) return fail(-1, "pdlpdev_debug_batch_attempts: count must be 1 .. 64");
  HIP_TRY(hipSetDevice(b->device));
  TRY(batch_refresh_table(b));
  const int K = b->K;
  for (int l = 0; l < K; ++l) loop_state_touched(b->ctx[l]);
  TRY(batch_fetch_ctl(b));
  int before[kBatchMax];
  bool asked[kBatchMax];
  for (int l = 0; l < K; ++l) {
    const pdlpdev_ctl& c = *b->ctx[l]->ctl_h;
    before[l] = c.steps_taken;
    asked[l]  = (!on || on[l] != 0) && c.error == 0;
    if (asked[l]) k_set_target<<<1, 1, 0, b->stream>>>(b->ctx[l]->ctl, before[l] + count);
    else if (c.target_steps > c.steps_taken) k_set_target<<<1, 1, 0, b->stream>>>(b->ctx[l]->ctl, c.steps_taken);
  }
  LAUNCH_CHECK();
  TRY(batch_enqueue_attempts(b, count));
  TRY(batch_fetch_ctl(b));
  for (int l = 0; l < K; ++l) {
    if (!asked[l] || !too_many_rejections(b->ctx[l], before[l], count)) continue;
    k_set_error<<<1, 1, 0, b->stream>>>(b->ctx[l]->ctl);
    LAUNCH_CHECK();
  }
  TRY(batch_fetch_ctl(b));
  for (int l = 0; l < K; ++l) b->ctx[l]->batch_ctl_fresh = true;
  if (ctl)
    for (int l = 0; l < K; ++l) ctl[l] = *b->ctx[l]->ctl_h;
  return 0;
}

// Parity hook: what the products of one side (0: A, 1: A^T) work on.  info = {K, W, layout (0 panels, 1 CSR stream, 2 jagged), rows of
// that side}; row0 (if not NULL) receives the W + 1 block boundaries whose partial sums the product reproduces; vK (if not NULL) a copy
// of the interleaved vector that side GATHERS from: side 0 xK (n * K doubles), side 1 yK (m * K doubles).
int pdlpdev_debug_batch_view(pdlpdev_batch* b, int side, int32_t info[4], int32_t* row0, double* vK)
{
  if (!b || !info || (side != 0 && side != 1)) return fail(-1, "pdlpdev_debug_batch_view: null argument, or a side other than 0 / 1");
  HIP_TRY(hipSetDevice(b->device));
  const pdlpdev_batch::Side& S = side ? b->t_side : b->a_side;
  const pdlpdev_ctx* c0        = b->ctx[0];
  info[0] = b->K, info[1] = S.W, info[2] = S.jag ? 2 : S.panel ? 0 : 1, info[3] = side ? c0->n : c0->m;
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (row0) HIP_TRY(hipMemcpy(row0, S.jag ? S.jv.row0 : S.row0, ((size_t)S.W + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (vK) HIP_TRY(hipMemcpy(vK, side ? b->yK : b->xK, (size_t)(side ? c0->m : c0->n) * b->K * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

static BatchProductSide batch_product_side(const pdlpdev_batch::Side& S, const pdlpdev_ctx::MatrixSide& M)
{
  return BatchProductSide{S.W, S.row0, S.panel, M.hot.off, M.hot.idx, M.hot.val};
}

// The ray pass (enqueue_halpern_ray) for the members with rule[l] >= 0 (the reduced-cost rule, 0 / 1; -1: not in the pass) as ONE K-wide
// pass on the batch's stream behind whatever ran: kernels_batch_halpern_ray.hip.  Nothing is read back and nothing is waited for: the
// member contexts' evaluations run on this same stream (pdlpdev_batch_create refuses contexts on another one), so they are ordered
// behind the pass without an event, and their read-back of scal[0..41) brings the figures along.  A member is served only if its
// control block -- as pdlpdev_batch_run's last read-back left it, nothing having moved the member since -- says error == 0 and at
// least one step; a served context notes the step count and the rule, and its pdlpdev_major_eval then leaves the single pass out.
int pdlpdev_batch_halpern_rays(pdlpdev_batch* b, const int32_t* rule)
{
  if (!b || !rule) return fail(-1, "pdlpdev_batch_halpern_rays: null argument");
  if (!b->halpern) return fail(-7, "pdlpdev_batch_halpern_rays: the batch is not in reflected Halpern mode (the averaging iteration has no ray pass)");
  HIP_TRY(hipSetDevice(b->device));
  TRY(batch_refresh_table(b));
  unsigned on_mask = 0, rule_mask = 0;
  int served = 0;
  for (int l = 0; l < b->K; ++l) {
    pdlpdev_ctx* c = b->ctx[l];
    if (rule[l] < 0 || !c->batch_ctl_fresh || c->ctl_h->error != 0 || c->ctl_h->steps_taken < 1) continue;
    on_mask |= 1u << l, rule_mask |= (rule[l] != 0 ? 1u : 0u) << l;
    served += 1;
  }
  if (on_mask == 0) return 0;
  roctx::Range range("pdlp: K-wide Halpern ray pass");
  pdlpdev_ctx* c0 = b->ctx[0];
  const BatchRayShared sh{c0->n, c0->m, c0->dr, c0->dc, c0->c_u};
  TRY(batch_halpern_enqueue_rays(b->K, b->stream, batch_product_side(b->a_side, c0->A), batch_product_side(b->t_side, c0->At), b->ray_dev, sh, on_mask, rule_mask,
                                 b->xK, b->yK));
  for (int l = 0; l < b->K; ++l)
    if ((on_mask >> l) & 1u) {
      pdlpdev_ctx* c     = b->ctx[l];
      c->ctl_h_current   = true;  // (batch_ctl_fresh: the read-back behind the attempts is what the device holds)
      c->batch_ray_steps = c->ctl_h->steps_taken, c->batch_ray_rule = (int)((rule_mask >> l) & 1u);
    }
  b->ray_wide += 1, b->ray_served += served;
  return 0;
}

// {K-wide passes enqueued, member passes they served, single passes the members' contexts enqueued since they joined the batch, 0}
int pdlpdev_batch_ray_stats(pdlpdev_batch* b, int64_t out[4])
{
  if (!b || !out) return fail(-1, "pdlpdev_batch_ray_stats: null argument");
  out[0] = b->ray_wide, out[1] = b->ray_served, out[2] = 0, out[3] = 0;
  for (int l = 0; l < b->K; ++l) out[2] += b->ctx[l]->stat_single_rays - b->ray_single0[l];
  return 0;
}

// The K-wide plain product as a parity hook, the batch twin of pdlpdev_spmv: out[l] = A in[l] (transpose: A^T in[l]) for the members
// with on[l] != 0 (on == NULL: all) through ONE kb_plain<K>; the other members' outputs are not touched.  The vectors pass through the
// members' tmp_n / tmp_m (where pdlpdev_spmv puts them) and the batch's interleaved vector of that side, all free between runs.
int pdlpdev_batch_spmv(pdlpdev_batch* b, int transpose, const double* const* in, double* const* out, const int32_t* on)
{
  if (!b || !in || !out) return fail(-1, "pdlpdev_batch_spmv: null argument");
  const pdlpdev_batch::Side& S = transpose ? b->t_side : b->a_side;
  if (S.jag) return fail(-7, "pdlpdev_batch_spmv: the %s side is in the jagged layout (the K-wide plain product walks the CSR arrays)", transpose ? "A^T" : "A");
  HIP_TRY(hipSetDevice(b->device));
  pdlpdev_ctx* c0 = b->ctx[0];
  hipStream_t s   = b->stream;
  const int K = b->K, rows = transpose ? c0->n : c0->m, cols = transpose ? c0->m : c0->n;
  unsigned on_mask = 0;
  for (int l = 0; l < K; ++l)
    if (!on || on[l]) {
      if (!in[l] || !out[l]) return fail(-1, "pdlpdev_batch_spmv: member %d is in the product without a vector", l);
      on_mask |= 1u << l;
    }
  if (on_mask == 0) return 0;
  struct Table {  // (the outputs are the members' tmp vectors, not the ray pass's: a table of its own, released on every way out)
    BatchRayLp* p = nullptr;
    ~Table() { if (p) (void)hipFree(p); }
  } table;
  std::vector<BatchRayLp> host(K);
  for (int l = 0; l < K; ++l) {
    host[l]    = batch_ray_lp_of(b->ctx[l]);
    host[l].ax = b->ctx[l]->tmp_m, host[l].aty = b->ctx[l]->tmp_n;
  }
  HIP_TRY(hipMalloc((void**)&table.p, K * sizeof(BatchRayLp)));
  HIP_TRY(hipMemcpyAsync(table.p, host.data(), K * sizeof(BatchRayLp), hipMemcpyHostToDevice, s));
  for (int l = 0; l < K; ++l)
    if ((on_mask >> l) & 1u)
      HIP_TRY(hipMemcpyAsync(transpose ? b->ctx[l]->tmp_m : b->ctx[l]->tmp_n, in[l], (size_t)cols * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));  // (the table and the vectors have left the caller's memory)
  TRY(batch_enqueue_plain(K, s, batch_product_side(S, transpose ? c0->At : c0->A), transpose, cols, table.p, on_mask, transpose ? b->yK : b->xK));
  for (int l = 0; l < K; ++l)
    if ((on_mask >> l) & 1u)
      HIP_TRY(hipMemcpyAsync(out[l], transpose ? b->ctx[l]->tmp_n : b->ctx[l]->tmp_m, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

// Average dispatch durations (ms) of the four kernels of a batched attempt: {primal, A / dual, A^T / step, decisions}, measured as
// pdlpdev_time_kernel measures the single-LP kernels -- whole attempts in the loop's order (each kernel meets the caches as the loop
// leaves them), every LP forced active with its averaging traffic, the dispatches' own timestamps; control blocks and running sums
// are put back afterwards (the "other" iterate buffers are scratch between attempts).
int pdlpdev_batch_time_kernels(pdlpdev_batch* b, int reps, double avg_ms[4])
{
  if (!b || !avg_ms) return fail(-1, "pdlpdev_batch_time_kernels: null argument");
  if (b->halpern)
    return fail(-7, "pdlpdev_batch_time_kernels: not for a batch in reflected Halpern mode (it forces the averaging traffic; take the kernel times from a kernel trace)");
  HIP_TRY(hipSetDevice(b->device));
  TRY(batch_refresh_table(b));
  hipStream_t s = b->stream;
  const int K   = b->K;
  if (reps < 1) reps = 1;
  TRY(batch_fetch_ctl(b));
  pdlpdev_ctl saved[kBatchMax], forced[kBatchMax];
  struct Scratch {  // (copies of the running sums, the dispatches' events: released on every way out)
    double *sx[kBatchMax] = {nullptr}, *sy[kBatchMax] = {nullptr};
    hipEvent_t ev[8] = {nullptr};
    ~Scratch()
    {
      for (double* p : sx) if (p) (void)hipFree(p);
      for (double* p : sy) if (p) (void)hipFree(p);
      for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
  } scratch;
  double **sx = scratch.sx, **sy = scratch.sy;
  hipEvent_t* ev = scratch.ev;
  for (int l = 0; l < K; ++l) {
    pdlpdev_ctx* c = b->ctx[l];
    loop_state_touched(c);
    saved[l] = forced[l] = *c->ctl_h;
    forced[l].pending_avg = 1, forced[l].target_steps = saved[l].steps_taken + 1, forced[l].error = 0;
    HIP_TRY(hipMalloc((void**)&sx[l], std::max<size_t>(c->n, 1) * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&sy[l], std::max<size_t>(c->m, 1) * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(sx[l], c->sumx, (size_t)c->n * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(sy[l], c->sumy, (size_t)c->m * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  auto arm = [&]() -> int {
    for (int l = 0; l < K; ++l) HIP_TRY(hipMemcpyAsync(b->ctx[l]->ctl, &forced[l], sizeof(pdlpdev_ctl), hipMemcpyHostToDevice, s));
    return 0;
  };
  for (int q = 0; q < 8; ++q) HIP_TRY(hipEventCreate(&ev[q]));
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  TRY(arm());
  TRY(batch_enqueue(b));  // warm
  for (int i = 0; i < reps; ++i) {
    TRY(arm());
    TRY(batch_enqueue(b, ev));
    HIP_TRY(hipStreamSynchronize(s));
    for (int q = 0; q < 4; ++q) {
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, ev[2 * q], ev[2 * q + 1]));
      sum[q] += ms;
    }
  }
  for (int q = 0; q < 4; ++q) avg_ms[q] = sum[q] / reps;
  for (int l = 0; l < K; ++l) {
    pdlpdev_ctx* c = b->ctx[l];
    HIP_TRY(hipMemcpyAsync(c->ctl, &saved[l], sizeof(pdlpdev_ctl), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->sumx, sx[l], (size_t)c->n * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->sumy, sy[l], (size_t)c->m * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
