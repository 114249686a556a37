// Shared-matrix lockstep batches in the restarted reflected-Halpern mode (docs/design/04d_halpern_mode.md, "Lockstep batches"): the
// Halpern twins of kb_a_dual / kb_at_step (kernels_batch.hip) and the K decisions.  A translation unit of their own: the averaging
// kernels of kernels_batch.hip are to stay, instruction for instruction, what they were (04d records how easily they move).
//   * the products are the averaging twins' -- batch_block_sums, batch_cross_over, batch_block_partials (batch_common.hpp), the
//     interleaved copy-out, every barrier -- with the epilogue phase replaced: per LP exactly the expressions of
//     HalpernDualEpilogue::apply / HalpernStepEpilogue::apply (pdlp_epilogues.hpp) under HalpernWeights of THAT LP's pdlpdev_halpern
//     block (its k differs from LP to LP once the restarts diverge);
//   * the primal step is kb_primal<K> as it is (pending_avg stays 0 in this mode): kernels_batch.hip launches it, then calls
//     batch_halpern_enqueue_tail for the three launches behind it;
//   * the step is constant and never rejected: every active LP takes exactly one step per batched attempt.  The iterates depend on
//     no reduction, so their bits hinge on the epilogue expressions alone; the three sums of r^2 (restart decisions) reproduce the
//     single kernels' trees as the averaging twins' sums do.
#include <hip/hip_runtime.h>

#include "batch_common.hpp"
#include "halpern_decision.hpp"
#include "pdlp_ctx.hpp"
#include "pdlp_epilogues.hpp"

#define LAUNCH_CHECK() HIP_TRY(hipGetLastError())

namespace {

// rows of A for K LPs: HalpernDualEpilogue per LP.  y' -> the LP's T(z^k) slot (avgy) and, through the LDS tile, interleaved into yK
// (the A^T side gathers y', not y^{k+1}); y^{k+1} = combine(y', y, y^0) -> y[next]; ||y' - y||^2 partials
// LDS: as kb_a_dual -- the epilogue overwrites S.u.sums[row][LP] with y' between the cross-over's second barrier and the barrier in
// front of the copy-out, each entry by the one lane that read it; nothing else is touched (docs/design/10_lds_hazard_audit.md)
template <int K, int VW>
__global__ void __launch_bounds__(kBT) kb_a_halpern(int W, const int32_t* __restrict__ row0, const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                                    const double* __restrict__ val, const BatchLp* __restrict__ lp, const BatchHalpernLp* __restrict__ hl,
                                                    const double* __restrict__ xK, double* __restrict__ yK)
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
      const double sigma = L.ctl->sigma;
      const HalpernWeights hw(hl[l].hal);
      const double* __restrict__ y  = cur ? L.y1 : L.y0;
      double* __restrict__ yn       = cur ? L.y0 : L.y1;
      double* __restrict__ yp       = hl[l].avgy;
      const double* __restrict__ ya = hl[l].lry;  // the anchor
      double yv[8], lov[8], hiv[8], y0v[8];
#pragma unroll
      for (int j = sub; j < 8; j += WL::NSUB) {
        const int r = b0 + lane + 64 * j, i = r0 + (r < nr ? r : 0);
        yv[j] = y[i], lov[j] = L.lo[i], hiv[j] = L.hi[i], y0v[j] = ya[i];
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
          yp[i]            = next;
          S.u.sums[lane + 64 * j][l] = next;
          const double dy = next - yi;
          acc[pass][0][j % VW] += dy * dy;
          yn[i] = hw.combine(next, yi, y0v[j]);
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

// rows of A^T for K LPs: HalpernStepEpilogue per LP.  v = A^T y'; the two sums as in kb_at_step; x^{k+1} over x' in x[next] (read and
// written by the same lane); A^T y^{k+1} = combine(v, A^T y, A^T y^0) -> aty[next]; x' -> the T(z^k) slot (avgx) on the last step of
// the LP's run only (halpern_last_step of ITS control block).  LDS: as kb_at_step, S.u.sums is read only.
template <int K, int VW>
__global__ void __launch_bounds__(kBT) kb_at_halpern(int W, const int32_t* __restrict__ row0, const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                                     const double* __restrict__ val, const BatchLp* __restrict__ lp, const BatchHalpernLp* __restrict__ hl,
                                                     const double* __restrict__ yK)
{
  __shared__ BatchShared<K> S;
  using WL = WaveLps<K>;
  const int w = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, sub = WL::sub(wave);
  const int r0 = row0[w], nr = row0[w + 1] - r0;
  // the epilogue's five operand arrays are requested as one batch in front of the arithmetic -- except at K = 2, where the two anchor
  // streams on top of the twin's three cost the third wave per SIMD (174 VGPRs against kb_at_step<2>'s 140): there they are requested
  // row by row, behind the first three
  constexpr bool kAnchorLate = K == 2;
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
      const HalpernWeights hw(hl[l].hal);
      const double* __restrict__ x   = cur ? L.x1 : L.x0;
      double* xn                     = cur ? L.x0 : L.x1;  // x' on entry, x^{k+1} on exit
      const double* __restrict__ aty = cur ? L.aty1 : L.aty0;
      double* __restrict__ atyn      = cur ? L.aty0 : L.aty1;
      const double* __restrict__ xa  = hl[l].lrx;    // the anchor and its A^T y
      const double* __restrict__ aa  = hl[l].lraty;
      double* __restrict__ xp        = halpern_last_step(L.ctl) ? hl[l].avgx : nullptr;
      double xv[8], xnv[8], av[8], x0v[8], a0v[8];
#pragma unroll
      for (int j = sub; j < 8; j += WL::NSUB) {
        const int r = b0 + lane + 64 * j, i = r0 + (r < nr ? r : 0);
        xv[j] = x[i], xnv[j] = xn[i], av[j] = aty[i];
        if constexpr (!kAnchorLate) x0v[j] = xa[i], a0v[j] = aa[i];
      }
#pragma unroll
      for (int j = sub; j < 8; j += WL::NSUB) {
        const int r = b0 + lane + 64 * j;
        if (r < nr) {
          const int i     = r0 + r;
          if constexpr (kAnchorLate) x0v[j] = xa[i], a0v[j] = aa[i];
          const double v  = S.u.sums[lane + 64 * j][l];
          const double xj = xv[j], xt = xnv[j], a = av[j];
          const double dx = xt - xj;
          const double t  = v - a;
          acc[pass][0][j % VW] += t * dx;
          acc[pass][1][j % VW] += dx * dx;
          if (xp) xp[i] = xt;
          xn[i]   = hw.combine(xt, xj, x0v[j]);
          atyn[i] = hw.combine(v, a, a0v[j]);
        }
      }
    }
    __syncthreads();
  }
  batch_block_partials<K, 2, VW>(S, acc, lp, false, W, w);
}

// The decisions of the K LPs: workgroup <-> LP, each what k_halpern_decision (pdlp_device.hip) does on that LP's control block, Halpern
// block and partials -- the same device function (halpern_decision.hpp: the same summation order, block_sum_fast, the same expressions)
__global__ void __launch_bounds__(kHalpernDecisionThreads) k_halpern_decision_batch(const BatchLp* __restrict__ lp, const BatchHalpernLp* __restrict__ hl, int nb_dy, int nb_t)
{
  halpern_decision_workgroup(lp[blockIdx.x].ctl, hl[blockIdx.x].hal, lp[blockIdx.x].part_a, nb_dy, lp[blockIdx.x].part_at, nb_t);
}

template <int K>
int enqueue_tail(hipStream_t s, const BatchProductSide& A, const BatchProductSide& T, const BatchLp* lp, const BatchHalpernLp* hl, double* xK, double* yK)
{
  if (A.panel) kb_a_halpern<K, 8><<<A.W, kBT, 0, s>>>(A.W, A.row0, A.off, A.idx, A.val, lp, hl, xK, yK);
  else kb_a_halpern<K, 4><<<A.W, kBT, 0, s>>>(A.W, A.row0, A.off, A.idx, A.val, lp, hl, xK, yK);
  if (T.panel) kb_at_halpern<K, 8><<<T.W, kBT, 0, s>>>(T.W, T.row0, T.off, T.idx, T.val, lp, hl, yK);
  else kb_at_halpern<K, 4><<<T.W, kBT, 0, s>>>(T.W, T.row0, T.off, T.idx, T.val, lp, hl, yK);
  k_halpern_decision_batch<<<K, kHalpernDecisionThreads, 0, s>>>(lp, hl, A.W, T.W);
  LAUNCH_CHECK();
  return 0;
}

}  // namespace

int batch_halpern_enqueue_tail(int K, hipStream_t s, const BatchProductSide& A, const BatchProductSide& T, const void* lp_table, const void* halpern_table,
                               double* xK, double* yK)
{
  const BatchLp* lp        = static_cast<const BatchLp*>(lp_table);
  const BatchHalpernLp* hl = static_cast<const BatchHalpernLp*>(halpern_table);
  return K == 16  ? enqueue_tail<16>(s, A, T, lp, hl, xK, yK)
         : K == 8 ? enqueue_tail<8>(s, A, T, lp, hl, xK, yK)
         : K == 4 ? enqueue_tail<4>(s, A, T, lp, hl, xK, yK)
                  : enqueue_tail<2>(s, A, T, lp, hl, xK, yK);
}
