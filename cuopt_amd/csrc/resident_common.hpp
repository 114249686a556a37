// What the two translation units of the resident small-LP path share (kernels_resident.hip: the averaging loop, its evaluation and the
// K-workgroup batch; kernels_resident_halpern.hip: the reflected-Halpern loop and its evaluation): the row sum every one-workgroup
// kernel uses, the three tiers and the one place that takes a tier to its kernel instantiation (for_resident_tier), and the argument
// record + row walker of the one-workgroup evaluation.
#pragma once
#include <type_traits>

#include "pdlp_ctx.hpp"
#include "pdlp_layouts.hpp"

// prod[a..b) added up strictly left to right; eight LDS reads are in flight before the first add
__device__ __forceinline__ double lds_row_sum(const double* prod, int a, int b)
{
  double acc = 0.0;
  for (int k = a; k < b; k += 8) {
    double p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = prod[k + i < b ? k + i : a];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc = k + i < b ? acc + p[i] : acc;
  }
  return acc;
}

// the three instantiations, smallest first: (lanes, elements per lane, nonzeros per lane)
struct ResidentTier { int T, Q, U; };
constexpr ResidentTier kResidentTiers[3] = {{256, 2, 8}, {512, 2, 16}, {512, 4, 8}};
inline size_t resident_lds_bytes(int tier)
{
  const ResidentTier& r = kResidentTiers[tier];
  return sizeof(double) * (size_t)r.T * (7 * r.Q + r.U);
}
// The one place that takes a tier to its entry of kResidentTiers at compile time: f(std::integral_constant<int, I>) for tier I --
//   [&](auto I) { constexpr ResidentTier r = kResidentTiers[decltype(I)::value]; return launch_resident_kernel(kernel<r.T, r.Q, r.U>, I, ...); }
// -- and none() for a value that is no tier.
template <class F, class None>
static int for_resident_tier(int tier, F&& f, None&& none)
{
  switch (tier) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return none();
  }
}
// `blocks` workgroups of a tier's instantiation of a loop kernel, enqueued on `s`, the kernel's LDS attribute set first
template <class... KArgs, class... Args>
static int launch_resident_kernel(void (*kernel)(KArgs...), int tier, int device, hipStream_t s, int blocks, Args... args)
{
  TRY(allow_dynamic_lds((const void*)kernel, device, resident_lds_bytes(tier)));
  kernel<<<blocks, kResidentTiers[tier].T, resident_lds_bytes(tier), s>>>(args...);
  HIP_TRY(hipGetLastError());
  return 0;
}

// single-workgroup head of a major iteration (pdlpdev_major_eval) for LPs on the resident path
struct MajorSmallArgs {
  int m, n, mode, rule_finite, want_linf;  // mode 0 / 1 / 2: the average k_major_small forms; 3: none, the average slots are evaluated
  double eps_p, eps_d;                     //                 as the Halpern loop left them (k_major_small_halpern)
  const int32_t *a_off, *a_idx, *at_off, *at_idx;
  const double *a_val, *at_val;
  pdlpdev_ctl* ctl;
  double *x0, *x1, *y0, *y1, *sumx, *sumy, *avgx, *avgy;
  const double *dr, *dc, *c_u, *lb_u, *ub_u, *lo_u, *hi_u;
  double *linf_m, *linf_n, *ax_cur, *ax_avg, *aty_cur, *aty_avg, *rc_cur, *rc_avg;
  double* sc;  // current at sc[0..9), average at sc[32..41)  (pinned host memory: no read-back copy)
  int guard_target = -1;  // >= 0 (evaluation enqueued right behind the attempts of a small-LP batch): only if the attempts reached this
                          // accepted-step count or raised the step-size error -- i.e. only if a major iteration is what comes next
  int want_ray = 0;       // mode 3 only (pdlpdev_set_halpern_rays): behind the two passes, the infeasibility information of the displacement
                          // T(z^k) - z^k -- the average slots minus the side of (x0, x1) / (y0, y1) that ctl->cur does not select, where the
                          // loop stored z^k before its last step.  linf_n / linf_m hold the scaled displacement (free behind the l-infinity
                          // reductions).  Raw statistics into free slots of the pinned block below sc[63]: the three of the rows at
                          // sc[kRayRows ..), the six of the columns at sc[kRayCols ..), the step count and the rule at sc[kRayMark ..)
                          // (pdlp_ctx.hpp; sc[16 .. 32) is pdlpdev_eval_infeasibility's, which this mode never calls)
};
constexpr int kMajorThreads = 1024;
// M vec for a matrix of <= 8192 nonzeros: all products in parallel into LDS, then every row is added up left to
// right by one lane (same order as every other SpMV here)
template <class Epi, int NQ>
__device__ __forceinline__ void small_rows(int rows, const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                           const double* __restrict__ val, const double* vec, double* prod, Epi& e,
                                           double (&acc)[NQ])
{
  const int nnz = off[rows];
  for (int k = threadIdx.x; k < nnz; k += kMajorThreads) prod[k] = val[k] * vec[idx[k]];
  __syncthreads();
  for (int r = threadIdx.x; r < rows; r += kMajorThreads) e.row(r, lds_row_sum(prod, off[r], off[r + 1]), acc);
}
inline MajorSmallArgs major_args(const pdlpdev_ctx* ctx, int average_mode, int rc_rule_finite_bounds, int want_linf, double eps_rel_primal, double eps_rel_dual)
{
  MajorSmallArgs A{ctx->m, ctx->n, average_mode, rc_rule_finite_bounds, want_linf, eps_rel_primal, eps_rel_dual,
                        ctx->A.full.off, ctx->A.full.idx, ctx->At.full.off, ctx->At.full.idx, ctx->A.full.val, ctx->At.full.val, ctx->ctl,
                        ctx->x[0], ctx->x[1], ctx->y[0], ctx->y[1], ctx->sumx, ctx->sumy, ctx->avgx, ctx->avgy,
                        ctx->dr, ctx->dc, ctx->c_u, ctx->lb_u, ctx->ub_u, ctx->lo_u, ctx->hi_u, ctx->tmp_m, ctx->tmp_n,
                        ctx->ax_u[PDLPDEV_CURRENT], ctx->ax_u[PDLPDEV_AVERAGE], ctx->aty_u[PDLPDEV_CURRENT],
                        ctx->aty_u[PDLPDEV_AVERAGE], ctx->rc[0], ctx->rc[1], ctx->scal_h};
  A.want_ray = average_mode == 3 && ctx->halpern && ctx->halpern_rays;
  return A;
}

// ---- the reflected-Halpern loop (kernels_resident_halpern.hip); the records of a Halpern small-LP batch sit in the batch object's
// pinned block (kernels_resident.hip), which launches that unit's kernels through the three functions below
struct HalpernSmallView {
  int m, n, nnz;
  const int32_t *a_off, *a_idx, *at_off, *at_idx;
  const double *a_val, *at_val, *c, *lb, *ub, *lo, *hi;
  double *x0, *x1, *y0, *y1, *aty0, *aty1;
  const double *ax, *ay, *aaty;  // the anchor z^0 and its A^T y (lrx, lry, lraty)
  double *tx, *ty;               // T(z^k) of the last step of a run (the average slots)
};
// one LP of k_pdhg_resident_halpern_batch (ResidentArgs' counterpart)
struct HalpernResidentArgs {
  HalpernSmallView V;
  pdlpdev_ctl *ctl, *ctl_host;
  pdlpdev_halpern *hal, *hal_host;
  int target_steps, pad;
};
// one LP of k_halpern_restart_finish_batch
struct HalpernRestartArgs {
  int n, g, clear, pad;
  double theta;  // < 0: the anchor and the counters only
  const double* part;  // k_restart_batch's partials
  const double *aty0, *aty1;
  double* lraty;
  double *dist2, *dist_host;  // the LP's scalar block on the device / its pinned one: the two distances (not squared) at [0], [1]
  pdlpdev_ctl *ctl, *ctl_host;
  pdlpdev_halpern *hal, *hal_host;
};
HalpernSmallView halpern_view(const pdlpdev_ctx* ctx);
int halpern_batch_launch_loop(hipStream_t s, int device, int tier, const HalpernResidentArgs* args, const int* list, int count);
int halpern_batch_launch_eval(hipStream_t s, int device, size_t lds, const MajorSmallArgs* args, const int* list, int count);
int halpern_batch_launch_restart_finish(hipStream_t s, const HalpernRestartArgs* args, const int* list, int count);
