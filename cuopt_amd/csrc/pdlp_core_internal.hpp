// What the core's translation units (pdlp_device.hip, pdlp_eval.hip) share beyond the public device ABI: read-backs, the plain products'
// launch sites, and the element-wise kernels both of them enqueue.  Defined in pdlp_device.hip.  (Shared with the lockstep batch as well,
// inline in pdlp_ctx.hpp: attempt_chunk, too_many_rejections, has_guarded_eval, wants_linf.)
#pragma once
#include "pdlp_ctx.hpp"

#define LAUNCH_CHECK() HIP_TRY(hipGetLastError())

extern "C" {
int fetch_scalars(pdlpdev_ctx* ctx, int count);         // scal[0..count) -> scal_h, synchronised
int fetch_ctl(pdlpdev_ctx* ctx, pdlpdev_ctl* out);      // the control block -> ctl_h (and *out)
int fetch_ctl_counted(pdlpdev_ctx* ctx, pdlpdev_ctl* out);  // ... as one of the loop's synchronisations (stat_loop_syncs)
void launch_plain(pdlpdev_ctx* ctx, int transpose, const double* vec, double* out);   // out = A vec / A^T vec in the side's layout
void launch_at_cur(pdlpdev_ctx* ctx, double* out_override, int use_next);             // A^T y of the current (next) iterate
// the kernels of pdlpdev_major_eval, nothing read back (pdlp_eval.hip).  guard != 0: for pdlpdev_run_period -- every kernel is empty unless
// the attempts in front reached their target, and the last one leaves the control block in scal[kCtlSlot ..)
int enqueue_major_eval(pdlpdev_ctx* ctx, int average_mode, int rc_rule_finite_bounds, double eps_rel_primal, double eps_rel_dual, int guard);
void read_major_eval(pdlpdev_ctx* ctx, double* out_current, double* out_average);  // ... and its results out of scal_h
// Halpern mode: the evaluation of T(z^k) (the average slots) alone, results in scal[32 ..), same guard (pdlp_eval.hip)
int enqueue_halpern_eval(pdlpdev_ctx* ctx, int rc_rule_finite_bounds, double eps_rel_primal, double eps_rel_dual, int guard);
void launch_restart_current(pdlpdev_ctx* ctx, int g);  // k_restart(CURRENT, scaled distances) -> part_g
// Halpern mode with pdlpdev_set_halpern_rays: the ray pass behind an evaluation of T(z^k), nothing read back -- raw statistics of the
// displacement T(z^k) - z^k in scal[kRayRows ..), scal[kRayCols ..), step count and rule in scal[kRayMark ..) (pdlp_eval.hip)
int enqueue_halpern_ray(pdlpdev_ctx* ctx, int rc_rule_finite_bounds);
// compute_remaining_stats_kernel on the raw statistics of rows (3) and columns (6) -> the four figures
void compute_remaining_stats(const double* r, const double* c, double out[4]);
}

__global__ void __launch_bounds__(kBlock)
k_flush_average(int n, int m, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ x0, const double* __restrict__ x1, const double* __restrict__ y0,
                const double* __restrict__ y1, double* __restrict__ sumx, double* __restrict__ sumy, int guard);
__global__ void __launch_bounds__(kBlock) k_finalize(const double* __restrict__ part, int nb, int nq, unsigned op_mask, double* __restrict__ out);
__global__ void __launch_bounds__(kBlock) k_div_inplace(int n, double* __restrict__ v, const double* __restrict__ d);
__global__ void __launch_bounds__(kBlock) k_div_to(int n, double* __restrict__ out, const double* __restrict__ v, const double* __restrict__ d);
__global__ void k_restart_ctl(pdlpdev_ctl* ctl);
__global__ void k_clear_pending(pdlpdev_ctl* ctl);

int sync_panel_values(pdlpdev_ctx* c);  // layout value arrays <- the (scaled) CSR values (pdlp_device.hip)
__global__ void __launch_bounds__(kBlock) k_fill(int64_t n, double* __restrict__ d, double v);
__global__ void __launch_bounds__(kBlock) k_scale_vectors(int n, int m, double* __restrict__ c, double* __restrict__ lb, double* __restrict__ ub,
                                                          const double* __restrict__ dc, double* __restrict__ lo, double* __restrict__ hi,
                                                          const double* __restrict__ dr);
// (pdlp_scaling.hip; the owner-computes set-up scales its column block with them too)
__global__ void __launch_bounds__(kBlock) k_scale_matrix(int rows, const int32_t* __restrict__ off, const int32_t* __restrict__ idx, double* __restrict__ val,
                                                         const double* __restrict__ d_self, const double* __restrict__ d_other);
__global__ void __launch_bounds__(kBlock) k_scale_matrix_long(const int32_t* __restrict__ rows_long, const int32_t* __restrict__ off,
                                                              const int32_t* __restrict__ idx, double* __restrict__ val,
                                                              const double* __restrict__ d_self, const double* __restrict__ d_other);
