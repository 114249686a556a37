// The burst of device-decided major iterations of the reflected-Halpern mode (cuoptamd_settings::halpern_device_major,
// docs/design/04d_halpern_mode.md "Verdict and restart on the device"): what pdlp_device.hip (pdlpdev_run_halpern_burst, the host side
// of a burst) and kernels_halpern_major.hip (the kernels and their launch sites) share, and the host's handling of a burst's ring of
// records (halpern_burst_mark_ring, halpern_burst_collect), which the batch's burst (kernels_resident.hip) uses per member.
#pragma once
#include "halpern_restart_tests.hpp"
#include "pdlp_ctx.hpp"

// The burst's own device block, next to pdlpdev_halpern (whose size does not change): allocated by pdlpdev_set_halpern_device_major,
// armed in front of every burst (k_halpern_major_arm).
struct pdlpdev_halpern_major_state {
  double r_prev;    // the fixed-point error at the previous restart check since the last restart (< 0: none): SolverLoop::halpern_r_prev
  double dist2[2];  // the restart's two distances: squared as finalize_rows leaves them, then their roots
  int32_t stopped;  // 1: a decision of this burst ended it -- every kernel behind it does nothing
  int32_t restart;  // 1: the decision in front asks for the restart (the guard of the three restart kernels)
};

// The decision of a major iteration: halpern_major_head's tests in its order and with its expressions (pdlp_solver.cpp: to_convergence,
// verdict, the iteration limit of check_limits) on the scalars that are on the device, then its three restart tests themselves
// (halpern_restart_due).  k_halpern_major_decide (one LP) and k_halpern_major_decide_batch (one wave per LP) call it: no test forks.
//   sc      the evaluation's nine raw sums (read_eval's input: the scalars' slot 32 on the multi-launch path, the pinned block's on
//           the resident one)
//   target  the period's accepted-step count
//   rec     the record, in pinned host memory
// Stopped: nothing.  The error flag up: a record marked "step error", stopped.  The steps short of the target (a resident launch that
// hit its step cap): "fell short", stopped.  Otherwise the record with the verdict; any verdict but "go on" stops the burst.
__device__ __forceinline__ void halpern_major_decide(const pdlpdev_ctl* __restrict__ ctl, const pdlpdev_halpern* __restrict__ hal,
                                                     pdlpdev_halpern_major_state* __restrict__ st, const double* __restrict__ sc,
                                                     const pdlpdev_halpern_major_params& p, int target, pdlpdev_halpern_major_record* __restrict__ rec)
{
  if (st->stopped) return;
  pdlpdev_halpern_major_record out;
  for (int i = 0; i < PDLPDEV_EV_COUNT; ++i) out.ev[i] = 0.0;
  out.r = hal->r, out.r_first = hal->r_first, out.k = hal->k;
  out.primal_weight = ctl->primal_weight;
  out.dist[0] = out.dist[1] = 0.0, out.new_weight = 0.0;
  out.steps_taken = ctl->steps_taken;
  out.restart = 0;
  st->restart = 0;
  if (ctl->error != 0 || ctl->steps_taken < target) {
    out.verdict = ctl->error != 0 ? PDLPDEV_MAJOR_STEP_ERROR : PDLPDEV_MAJOR_FELL_SHORT;
    st->stopped = 1;
    *rec        = out;
    return;
  }
  // read_eval (pdlp_layouts.hpp)
  double* ev = out.ev;
  ev[PDLPDEV_EV_PRES2]         = sc[0];
  ev[PDLPDEV_EV_DUAL_SUM]      = sc[1] + sc[5];
  ev[PDLPDEV_EV_Y2]            = sc[2];
  ev[PDLPDEV_EV_LINF_PRES_REL] = p.want_linf ? sc[3] : 0.0;
  ev[PDLPDEV_EV_DRES2]         = sc[4];
  ev[PDLPDEV_EV_CX]            = sc[6];
  ev[PDLPDEV_EV_X2]            = sc[7];
  ev[PDLPDEV_EV_LINF_DRES_REL] = p.want_linf ? sc[8] : 0.0;
  // to_convergence
  double pobj = ev[PDLPDEV_EV_CX], dobj = ev[PDLPDEV_EV_DUAL_SUM];
  if (p.objective_scale != 1.0 || p.objective_offset != 0.0) {
    pobj = p.objective_scale * pobj + p.objective_offset;
    dobj = p.objective_scale * dobj + p.objective_offset;
  }
  const double gap = fabs(pobj - dobj), abs_objective = fabs(pobj) + fabs(dobj);
  const double l2_primal = sqrt(ev[PDLPDEV_EV_PRES2]), l2_dual = sqrt(ev[PDLPDEV_EV_DRES2]);
  // verdict: the three inequalities
  const bool gap_ok = gap <= p.absolute_gap_tolerance + p.relative_gap_tolerance * abs_objective;
  bool primal_ok, dual_ok;
  if (p.per_constraint_residual) {
    primal_ok = ev[PDLPDEV_EV_LINF_PRES_REL] <= p.absolute_primal_tolerance;
    dual_ok   = ev[PDLPDEV_EV_LINF_DRES_REL] <= p.absolute_dual_tolerance;
  } else {
    primal_ok = l2_primal <= p.absolute_primal_tolerance + p.relative_primal_tolerance * p.norm_b;
    dual_ok   = l2_dual <= p.absolute_dual_tolerance + p.relative_dual_tolerance * p.norm_c;
  }
  const int total_iterations = p.iteration_offset + ctl->steps_taken;
  int verdict = PDLPDEV_MAJOR_GO_ON;
  if (total_iterations > 1 && dual_ok && primal_ok && gap_ok) verdict = PDLPDEV_MAJOR_OPTIMAL;
  else if (ctl->steps_taken >= p.iteration_limit) verdict = PDLPDEV_MAJOR_ITERATION_LIMIT;  // check_limits: internal_solver_iterations_
  out.verdict = verdict;
  if (verdict != PDLPDEV_MAJOR_GO_ON) {
    st->stopped = 1;
    *rec        = out;
    return;
  }
  const bool restart = halpern_restart_due(hal->r, hal->r_first, st->r_prev, hal->k, total_iterations, p.sufficient_reduction, p.necessary_reduction,
                                           p.artificial_threshold);
  st->r_prev  = restart ? -1.0 : hal->r;  // (halpern_restart_done: no previous check behind a restart)
  st->restart = restart ? 1 : 0;
  out.restart = restart ? 1 : 0;
  *rec        = out;
}

// ---- the host side of a burst's ring: pdlpdev_run_halpern_burst's, and pdlpdev_small_batch_run_halpern_burst's per member (the callers
// count stats->bursts and stats->periods, once per burst).  In front of the launches every slot is "not written": a decision leaves its
// step count there.  Behind the synchronisation the written records go to `records` in order, r_prev is carried forward as the decisions
// left it in the burst's block.  Nonzero: a record was written behind the period that stopped the burst.
static inline void halpern_burst_mark_ring(pdlpdev_halpern_major_record* ring, int count)
{
  for (int j = 0; j < count; ++j) ring[j].steps_taken = -1;
}
static inline int halpern_burst_collect(const pdlpdev_halpern_major_record* ring, int count, double r_prev, pdlpdev_halpern_major_record* records,
                                        int32_t* written, double* r_prev_out, HalpernBurstStats* stats)
{
  int n_written  = 0;
  bool stop_seen = false;
  for (int j = 0; j < count; ++j) {
    const pdlpdev_halpern_major_record& r = ring[j];
    if (r.steps_taken < 0) {
      stop_seen = true;  // (a period behind the stop: its launches were empty)
      stats->empty += 1;
      continue;
    }
    if (stop_seen || n_written != j) return 1;
    records[n_written++] = r;
    if (r.verdict != PDLPDEV_MAJOR_GO_ON) stop_seen = true;
    else r_prev = r.restart ? -1.0 : r.r;
  }
  stats->records += n_written;
  *written = n_written;
  if (r_prev_out) *r_prev_out = r_prev;
  return 0;
}

extern "C" {
// <<<1, 1>>>: stopped <- 0, restart <- 0, r_prev <- the host's
int halpern_major_launch_arm(pdlpdev_ctx* ctx, double r_prev);
// the guarded twin of k_set_target: does nothing once the burst has stopped
int halpern_major_launch_set_target(pdlpdev_ctx* ctx, int32_t target);
// the resident path's steps and evaluation of one period: k_pdhg_resident_halpern's and k_major_small_halpern's bodies behind the guard
int halpern_major_launch_resident_period(pdlpdev_ctx* ctx, int32_t target, int rc_rule_finite_bounds, int want_linf, double eps_rel_primal,
                                         double eps_rel_dual);
// k_halpern_major_decide on the context's own blocks: sc = the nine raw sums of the evaluation (read_eval's input), rec = the record
int halpern_major_launch_decide(pdlpdev_ctx* ctx, const double* sc, const pdlpdev_halpern_major_params& p, int32_t target,
                                pdlpdev_halpern_major_record* rec);
// the guarded restart: distances + anchor (restart_block), A^T y of the anchor, finalize_rows + halpern_restart_scalars.
// mirrors != 0: the control block and the Halpern block also go to their pinned mirrors (the resident path reads no copy back)
int halpern_major_launch_restart(pdlpdev_ctx* ctx, double theta, pdlpdev_halpern_major_record* rec, int mirrors);
}
