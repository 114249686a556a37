// The burst of device-decided major iterations of the reflected-Halpern mode (cuoptamd_settings::halpern_device_major,
// docs/design/04d_halpern_mode.md "Verdict and restart on the device"): what pdlp_device.hip (pdlpdev_run_halpern_burst, the host side
// of a burst) and kernels_halpern_major.hip (the kernels and their launch sites) share.
#pragma once
#include "pdlp_ctx.hpp"

// The burst's own device block, next to pdlpdev_halpern (whose size does not change): allocated by pdlpdev_set_halpern_device_major,
// armed in front of every burst (k_halpern_major_arm).
struct pdlpdev_halpern_major_state {
  double r_prev;    // the fixed-point error at the previous restart check since the last restart (< 0: none): SolverLoop::halpern_r_prev
  double dist2[2];  // the restart's two distances: squared as finalize_rows leaves them, then their roots
  int32_t stopped;  // 1: a decision of this burst ended it -- every kernel behind it does nothing
  int32_t restart;  // 1: the decision in front asks for the restart (the guard of the three restart kernels)
};

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
// the guarded restart: distances + anchor (restart_block), A^T y of the anchor, finalize_rows + k_halpern_restart_ctl's arithmetic.
// mirrors != 0: the control block and the Halpern block also go to their pinned mirrors (the resident path reads no copy back)
int halpern_major_launch_restart(pdlpdev_ctx* ctx, double theta, pdlpdev_halpern_major_record* rec, int mirrors);
}
