// The decision of a Halpern step for ONE LP by one workgroup of kHalpernDecisionThreads threads: the body of k_halpern_decision
// (pdlp_device.hip) and of k_halpern_decision_batch (kernels_batch_halpern.hip, workgroup <-> LP), so that the two cannot drift apart.
// The partials are added in k_step_decision's order, the fixed-point error of the step is formed in PDHG's metric
//   r_k^2 = (w / eta) ||dx||^2 + 2 dy.(A dx) + ||dy||^2 / (eta w),   dy.(A dx) = dx.(A^T y' - A^T y^k) = StepEpilogue's first sum,
// the counters advance and the buffers flip.  A NaN or an overflow raises the step error like an invalid movement does.
#pragma once
#include "pdlp_kernels.hpp"

constexpr int kHalpernDecisionThreads = 1024;  // (= kDecisionThreads of pdlp_device.hip: one wide workgroup, every partial one independent load)

// The decision itself from three FINISHED sums, by one thread: lc is the thread's copy of the control block, which it stores.  One
// body for the one-LP and the batch decisions (below) and for a sharded solve's, whose sums come out of an all-reduce
// (k_halpern_decision_sums) or out of the peers' landing blocks (k_halpern_decision_p2p), pdlp_device.hip.
__device__ __forceinline__ void halpern_decision_from_sums(pdlpdev_ctl* __restrict__ ctl, pdlpdev_halpern* __restrict__ hal, pdlpdev_ctl& lc, double dy2,
                                                           double interaction, double dx2)
{
  pdlpdev_halpern lh = *hal;
  const double eta = lc.step_size, w = lc.primal_weight;
  const double r2  = (w / eta) * dx2 + 2.0 * interaction + dy2 / (eta * w);
  lc.last_interaction = interaction;
  lc.last_movement    = r2;
  lc.last_dx2         = dx2;
  lc.last_dy2         = dy2;
  lc.attempts += 1;
  if (!(r2 == r2) || !(r2 < 1.0e100)) {
    lc.error = 1;
  } else {
    const double r = sqrt(dmax(r2, 0.0));
    lh.r = r, lh.r2 = r2;
    if (lh.k == 0) lh.r_first = r;
    lh.r2_min = dmin(lh.r2_min, r2);
    lh.k += 1;
    *hal = lh;
  }
  lc.k += 1;
  lc.cur ^= 1;
  lc.steps_taken += 1;
  lc.its_since_restart += 1;
  *ctl = lc;
}

// The scalar part of a restart, by one thread, behind the two squared distances in dist2: their roots in place, the smoothed primal weight
// (theta < 0: the counters only), k <- 0.  The ONE copy: k_halpern_restart_ctl and every restart finish of a resident LP or a burst call it.
__device__ __forceinline__ void halpern_restart_scalars(pdlpdev_ctl* ctl, pdlpdev_halpern* hal, double* dist2, double theta)
{
  const double dx = sqrt(dist2[0]), dy = sqrt(dist2[1]);
  dist2[0] = dx, dist2[1] = dy;
  if (theta >= 0.0 && dx > 1.0e-10 && dy > 1.0e-10) {
    const double w     = exp(theta * log(dy / dx) + (1.0 - theta) * log(ctl->primal_weight));
    ctl->primal_weight = w;
    ctl->tau           = ctl->step_size / w;
    ctl->sigma         = ctl->step_size * w;
  }
  ctl->its_since_restart = 0;
  hal->k                 = 0;
}

__device__ __forceinline__ void halpern_decision_workgroup(pdlpdev_ctl* __restrict__ ctl, pdlpdev_halpern* __restrict__ hal, const double* __restrict__ part_dy,
                                                           int nb_dy, const double* __restrict__ part_t, int nb_t)
{
  __shared__ double red[3 * 16];
  pdlpdev_ctl lc = *ctl;
  if (!(lc.error == 0 && lc.steps_taken < lc.target_steps)) return;
  const int t   = threadIdx.x;
  double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll 4
  for (int i = t; i < nb_dy; i += kHalpernDecisionThreads) acc[0] += part_dy[i];
#pragma unroll 4
  for (int i = t; i < nb_t; i += kHalpernDecisionThreads) {
    acc[1] += part_t[i];
    acc[2] += part_t[nb_t + i];
  }
  block_sum_fast<3, kHalpernDecisionThreads / 64>(acc, red);
  if (t != 0) return;
  halpern_decision_from_sums(ctl, hal, lc, acc[0], acc[1], acc[2]);
}
