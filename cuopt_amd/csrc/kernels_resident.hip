// The resident small-LP path (BASELINE config 5: LP relaxations of MIP size, re-solved over and over) -- its own translation unit
// since round 6: the one-workgroup PDHG loop, the one-workgroup head of a major iteration, and the BATCH of K such LPs in K
// workgroups of one launch (pdlpdev_small_batch_*: the MI355X-first answer to the reference's thread pool of independent solves,
// cpp/src/linear_programming/utilities/cython_solve.cu:264-296, and to the MIP heuristics' streams of relaxations,
// cpp/src/mip/relaxed_lp/relaxed_lp.cu:53-127 -- one LP keeps ONE of the chip's 256 CUs busy, 256 LPs keep all of them).
#include "pdlp_ctx.hpp"
#include "pdlp_layouts.hpp"
#include "resident_common.hpp"  // lds_row_sum, the tiers, MajorSmallArgs + small_rows: shared with kernels_resident_halpern.hip
#include "halpern_major_batch.hpp"  // the records and launches of a Halpern batch's burst (kernels: kernels_halpern_major.hip)

// ------------------------------------------------------------------------------------------------
// Small LPs (MIP-style repeated re-solves, BASELINE config 5): the whole batch of PDHG attempts between two
// major iterations runs inside ONE workgroup, with the LP on chip.  At this size a 4-launch attempt is pure
// launch latency (~15 us) and even L2 round trips (3-4 dependent ones per phase) cost more than the arithmetic,
// so nothing is re-read from memory inside the loop:
//   * lane t keeps nonzeros t, t+T, ... of A and of A^T (value + column) in registers;
//   * lane t owns rows / columns t, t+T, ...: their CSR extents and every per-element vector
//     (x, A^T y, c, bounds, running sums ...) live in its registers;
//   * the two gathered vectors (xbar, y'), the nonzero products and the constant vectors (c, bounds) sit in LDS.
// Products are val * vec[col] and every row is added up by its owner in CSR order, so x', y', A^T y' are
// bit-identical to the multi-launch kernels (and the oracle); the three step-size sums use a different,
// fixed reduction tree.  T lanes, Q elements and U nonzeros per lane: m, n <= Q*T, nnz <= U*T.
// ------------------------------------------------------------------------------------------------
struct SmallView {
  int m, n, nnz;
  const int32_t *a_off, *a_idx, *at_off, *at_idx;
  const double *a_val, *at_val, *c, *lb, *ub, *lo, *hi;
  double *x0, *x1, *y0, *y1, *aty0, *aty1, *sumx, *sumy;
};
// LDS hazards of the resident loop (round-6 audit), barriers B1 ... B5 of an attempt (B5 sits inside block_sum_fast):
//   xbar_s  written in the primal phase (own columns) before B1, gathered before B2; next written after B5 of the same attempt.
//   prod    written before B2 (A xbar products, own slots) and before B4 (A^T y' products); read by the row sums before B3 / B5;
//           each rewrite is behind the barrier that ends the previous readers (B3 -> B4's writes, B5 -> the next attempt's B2 writes).
//   yn_s    written before B3 (own rows), gathered before B4; next written behind B1 ... B2 of the next attempt.
//   red[2], pw[2]  by attempt parity: written before B5 / B3, read behind B5; the same parity is written again two attempts later,
//           ten barriers on.  Constants (c_s, bounds) are written once before the first B1.
template <int T, int Q, int U>
__device__ __forceinline__ void resident_body(const SmallView& V, pdlpdev_ctl* __restrict__ ctl, pdlpdev_ctl* __restrict__ ctl_host,
                                              const pdlpdev_step_params& sp, int target_steps, int max_attempts, double* lds)
{
  double* xbar_s = lds;               // Q*T
  double* yn_s   = xbar_s + Q * T;    // Q*T
  double* c_s    = yn_s + Q * T;      // constants, read with stride 1 by their owners
  double* lb_s   = c_s + Q * T;
  double* ub_s   = lb_s + Q * T;
  double* lo_s   = ub_s + Q * T;
  double* hi_s   = lo_s + Q * T;
  double* prod   = hi_s + Q * T;      // U*T
  // two sets (attempt parity) of cross-wave partials: a wave may start the next attempt's reduction while a slower
  // one still reads this attempt's table -- the barriers in between only order the *other* buffers
  __shared__ double red[2][3 * 16];
  __shared__ double pw[2][2];  // the two powers of the step-size rule, computed by the last wave while rows are summed
  const int t = threadIdx.x;
  // Every lane keeps its own copy of the control block and repeats the (uniform) step decision: no broadcast
  // through LDS and no barrier between the reduction and the next primal step.
  pdlpdev_ctl lc = *ctl;
  lc.target_steps = target_steps;
  double a_val[U], at_val[U];
  int a_col[U], at_col[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int k  = t + u * T;
    const bool in = k < V.nnz;
    a_val[u]  = in ? V.a_val[k] : 0.0;
    a_col[u]  = in ? V.a_idx[k] : 0;
    at_val[u] = in ? V.at_val[k] : 0.0;
    at_col[u] = in ? V.at_idx[k] : 0;
  }
  const int cur0 = lc.cur;
  int r0[Q], r1[Q], c0[Q], c1[Q];  // CSR extents of the owned rows of A and of A^T (empty when out of range)
  double x[Q], xn[Q], aty[Q], atyn[Q], sumx[Q], y[Q], yn[Q], sumy[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int e = t + q * T;
    const bool row = e < V.m, col = e < V.n;
    r0[q] = row ? V.a_off[e] : 0, r1[q] = row ? V.a_off[e + 1] : 0;
    c0[q] = col ? V.at_off[e] : 0, c1[q] = col ? V.at_off[e + 1] : 0;
    c_s[e] = col ? V.c[e] : 0.0, lb_s[e] = col ? V.lb[e] : 0.0, ub_s[e] = col ? V.ub[e] : 0.0;
    x[q]    = col ? (cur0 ? V.x1 : V.x0)[e] : 0.0;
    aty[q]  = col ? (cur0 ? V.aty1 : V.aty0)[e] : 0.0;
    sumx[q] = col ? V.sumx[e] : 0.0;
    lo_s[e] = row ? V.lo[e] : 0.0, hi_s[e] = row ? V.hi[e] : 0.0;
    y[q]    = row ? (cur0 ? V.y1 : V.y0)[e] : 0.0;
    sumy[q] = row ? V.sumy[e] : 0.0;
    xn[q] = x[q], atyn[q] = aty[q], yn[q] = y[q];
  }
  const int used = (V.nnz + T - 1) / T;  // nonzero slots in use (uniform): tiny LPs skip the empty ones
  for (int attempt = 0; attempt < max_attempts; ++attempt) {
    if (lc.error != 0 || lc.steps_taken >= lc.target_steps) break;  // uniform: every lane holds the same lc
    const int cur       = lc.cur;
    const double tau = lc.tau, sigma = lc.sigma, weight = lc.step_size;
    const bool pend     = lc.pending_avg != 0;
    const double knext  = (double)(lc.k + 1) + 1.0;
    const int par       = attempt & 1;
    // primal projection (utils.cuh:80-95) + deferred averaging
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int j = t + q * T;
      if (j < V.n) {
        const double gradient = c_s[j] - aty[q];
        double next           = x[q] - (tau * gradient);
        next                  = dmax(dmin(next, ub_s[j]), lb_s[j]);
        xn[q]                 = next;
        xbar_s[j]             = next - x[q] + next;
        if (pend) sumx[q] = sumx[q] + weight * x[q];
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (u < used) prod[t + u * T] = a_val[u] * xbar_s[a_col[u]];
    __syncthreads();
    // y' = proj(y - sigma A xbar) (utils.cuh:97-112), ||dy||^2
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = t + q * T;
      if (i < V.m) {
        const double ax = lds_row_sum(prod, r0[q], r1[q]);
        double next      = y[q] - (sigma * ax);
        const double low = next + sigma * lo_s[i];
        const double up  = next + sigma * hi_s[i];
        next             = dmax(low, dmin(up, 0.0));
        yn[q]            = next;
        yn_s[i]          = next;
        const double dy  = next - y[q];
        acc[0] += dy * dy;
        if (pend) sumy[q] = sumy[q] + weight * y[q];
      }
    }
    if (t >= T - 2) pw[par][t - (T - 2)] = pow(knext, t == T - 2 ? -sp.reduction_exponent : -sp.growth_exponent);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (u < used) prod[t + u * T] = at_val[u] * yn_s[at_col[u]];
    __syncthreads();
    // A^T y' + interaction / ||dx||^2 (adaptive_step_size_strategy.cu:278-340)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int j = t + q * T;
      if (j < V.n) {
        const double v = lds_row_sum(prod, c0[q], c1[q]);
        atyn[q]          = v;
        const double dx  = xn[q] - x[q];
        const double dty = v - aty[q];
        acc[1] += dty * dx;
        acc[2] += dx * dx;
      }
    }
    block_sum_fast<3, T / 64>(acc, red[par]);
    apply_step_decision(&lc, acc[0], acc[1], acc[2], sp, pw[par]);
    if (lc.cur != cur) {  // accepted: the candidate becomes the iterate
#pragma unroll
      for (int q = 0; q < Q; ++q) x[q] = xn[q], aty[q] = atyn[q], y[q] = yn[q];
    }
  }
  {
    const int cur = lc.cur;
    double* xo    = cur ? V.x1 : V.x0;
    double* yo    = cur ? V.y1 : V.y0;
    double* atyo  = cur ? V.aty1 : V.aty0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int e = t + q * T;
      if (e < V.n) xo[e] = x[q], atyo[e] = aty[q], V.sumx[e] = sumx[q];
      if (e < V.m) yo[e] = y[q], V.sumy[e] = sumy[q];
    }
  }
  if (t == 0) *ctl = lc, *ctl_host = lc;  // the pinned mirror saves the read-back copy
}
template <int T, int Q, int U>
__global__ void __launch_bounds__(T)
k_pdhg_resident(SmallView V, pdlpdev_ctl* __restrict__ ctl, pdlpdev_ctl* __restrict__ ctl_host, pdlpdev_step_params sp,
                int target_steps, int max_attempts)
{
  extern __shared__ double lds[];
  resident_body<T, Q, U>(V, ctl, ctl_host, sp, target_steps, max_attempts, lds);
}
// K LPs, one workgroup each, ONE launch (round 6): workgroup b runs the loop of LP list[b] exactly as k_pdhg_resident would -- the
// same body, so every LP's trajectory is bit for bit the one of its own launch.  The argument records sit in pinned host memory
// (a workgroup reads ~300 bytes of it once).
struct ResidentArgs {
  SmallView V;
  pdlpdev_ctl *ctl, *ctl_host;
  pdlpdev_step_params sp;
  int target_steps, pad;
};
template <int T, int Q, int U>
__global__ void __launch_bounds__(T) k_pdhg_resident_batch(const ResidentArgs* __restrict__ args, const int* __restrict__ list, int max_attempts)
{
  extern __shared__ double lds[];
  const ResidentArgs& A = args[list[blockIdx.x]];
  resident_body<T, Q, U>(A.V, A.ctl, A.ctl_host, A.sp, A.target_steps, max_attempts, lds);
}
// the three instantiations (kResidentTiers, resident_common.hpp), smallest first
int resident_tier(int m, int n, int64_t nnz)
{
  for (int i = 0; i < 3; ++i) {
    const ResidentTier& r = kResidentTiers[i];
    if (m <= r.Q * r.T && n <= r.Q * r.T && nnz <= (int64_t)r.U * r.T) return i;
  }
  return -1;
}


// single-workgroup head of a major iteration (pdlpdev_major_eval) for LPs on the resident path: MajorSmallArgs, small_rows
// (resident_common.hpp)
// (k_major_small_halpern in kernels_resident_halpern.hip carries a copy of the `which == 1` pass below: a change here is made there too)
__device__ __forceinline__ void major_small_body(const MajorSmallArgs& A, double* prod /* nnz doubles of LDS */)
{
  __shared__ double red[4 * kMajorThreads / 64];
  const int t = threadIdx.x;
  const int cur = A.ctl->cur;
  double* x = cur ? A.x1 : A.x0;
  double* y = cur ? A.y1 : A.y0;
  const bool pend = A.ctl->pending_avg != 0;
  const double w = A.ctl->step_size, sw = A.ctl->sum_weights;
  for (int j = t; j < A.n; j += kMajorThreads) {
    double sx = A.sumx[j];
    if (pend) A.sumx[j] = sx = sx + w * x[j];
    A.avgx[j] = A.mode == 0 ? x[j] : (A.mode == 1 ? 0.0 : sx / sw);
  }
  for (int i = t; i < A.m; i += kMajorThreads) {
    double sy = A.sumy[i];
    if (pend) A.sumy[i] = sy = sy + w * y[i];
    A.avgy[i] = A.mode == 0 ? y[i] : (A.mode == 1 ? 0.0 : sy / sw);
  }
  __syncthreads();  // also orders the global writes above against the reads below (one workgroup)
  if (t == 0) A.ctl->pending_avg = 0;
  for (int which = 0; which < 2; ++which) {
    const double* xv = which ? A.avgx : x;
    const double* yv = which ? A.avgy : y;
    double* sc       = A.sc + 32 * which;
    {
      EvalPrimalEpilogue e{yv, A.dr, A.lo_u, A.hi_u, A.eps_p, A.want_linf ? A.linf_m : nullptr, which ? A.ax_avg : A.ax_cur};
      double acc[3] = {0.0, 0.0, 0.0};
      small_rows(A.m, A.a_off, A.a_idx, A.a_val, xv, prod, e, acc);
      block_sum_fast<3, kMajorThreads / 64>(acc, red);
      if (t == 0) sc[0] = acc[0], sc[1] = acc[1], sc[2] = acc[2];
      __syncthreads();
      if (A.want_linf) {
        double mx[1] = {0.0};
        for (int i = t; i < A.m; i += kMajorThreads) mx[0] = dmax(mx[0], A.linf_m[i]);  // own writes
        block_reduce<MaxOp, 1, kMajorThreads / 64>(mx, red);
        if (t == 0) sc[3] = mx[0];
        __syncthreads();
      }
    }
    {
      EvalDualEpilogue e{EvalDualCore{xv, A.dc, A.c_u, A.lb_u, A.ub_u, A.eps_d, A.rule_finite, which ? A.rc_avg : A.rc_cur,
                                      A.want_linf ? A.linf_n : nullptr, which ? A.aty_avg : A.aty_cur}};
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      small_rows(A.n, A.at_off, A.at_idx, A.at_val, yv, prod, e, acc);
      block_sum_fast<4, kMajorThreads / 64>(acc, red);
      if (t == 0) sc[4] = acc[0], sc[5] = acc[1], sc[6] = acc[2], sc[7] = acc[3];
      __syncthreads();
      if (A.want_linf) {
        double mx[1] = {0.0};
        for (int j = t; j < A.n; j += kMajorThreads) mx[0] = dmax(mx[0], A.linf_n[j]);
        block_reduce<MaxOp, 1, kMajorThreads / 64>(mx, red);
        if (t == 0) sc[8] = mx[0];
        __syncthreads();
      }
    }
  }
}
__global__ void __launch_bounds__(kMajorThreads) k_major_small(MajorSmallArgs A)
{
  extern __shared__ double prod[];
  major_small_body(A, prod);
}
__global__ void __launch_bounds__(kMajorThreads) k_major_small_batch(const MajorSmallArgs* __restrict__ args, const int* __restrict__ list)
{
  extern __shared__ double prod[];
  const MajorSmallArgs& A = args[list[blockIdx.x]];
  if (A.guard_target >= 0 && !(A.ctl->error != 0 || A.ctl->steps_taken >= A.guard_target)) {  // (uniform)
    if (threadIdx.x == 0) A.sc[63] = 0.0;  // "not evaluated"
    return;
  }
  major_small_body(A, prod);
  if (threadIdx.x == 0) A.sc[63] = 1.0;
}

// ---- one LP: the small-LP branches of pdlpdev_run / pdlpdev_major_eval ----------------------------------------------------------------
static SmallView small_view(const pdlpdev_ctx* ctx)
{
  return SmallView{ctx->m, ctx->n, (int)ctx->nnz, ctx->A.full.off, ctx->A.full.idx, ctx->At.full.off, ctx->At.full.idx, ctx->A.full.val, ctx->At.full.val,
                   ctx->c, ctx->lb, ctx->ub, ctx->lo, ctx->hi, ctx->x[0], ctx->x[1], ctx->y[0], ctx->y[1], ctx->aty[0],
                   ctx->aty[1], ctx->sumx, ctx->sumy};
}
static int major_lds_attribute(int device)
{
  TRY(allow_dynamic_lds((const void*)k_major_small, device, 8192 * 8));
  return allow_dynamic_lds((const void*)k_major_small_batch, device, 8192 * 8);
}
// the tier's instantiation of the loop kernel, enqueued (a value that is no tier: nothing, as ever -- resident contexts have one)
static int launch_resident_tier(pdlpdev_ctx* ctx, int tier, const SmallView& V, int32_t target_steps, int max_attempts)
{
  return for_resident_tier(
    tier,
    [&](auto I) {
      constexpr ResidentTier r = kResidentTiers[decltype(I)::value];
      return launch_resident_kernel(k_pdhg_resident<r.T, r.Q, r.U>, I, ctx->device, ctx->stream, 1, V, ctx->ctl, ctx->ctl_h, ctx->sp, target_steps, max_attempts);
    },
    [] { return 0; });
}
// one launch runs attempts until the target is reached (rejected attempts included); the cap only bounds a pathological rejection
// streak, in which case the loop relaunches.  The kernel takes the target as an argument and leaves the control block in pinned host
// memory: one launch + one synchronize per call.
int resident_run(pdlpdev_ctx* ctx, int32_t target_steps)
{
  const SmallView V = small_view(ctx);
  const int tier    = resident_tier(ctx->m, ctx->n, ctx->nnz);
  for (int guard = 0; guard < 1000; ++guard) {
    TRY(launch_resident_tier(ctx, tier, V, target_steps, 1 << 14));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->ctl_h->error != 0 || ctx->ctl_h->steps_taken >= target_steps) break;
  }
  return 0;
}
// pdlpdev_debug_attempts' resident branch: ONE launch that makes at most `count` attempts towards steps_taken + count (ctl_h is current
// on entry: the caller read it back), one synchronisation, no relaunch -- a rejected attempt is not made up for.  The kernel leaves the
// control block in the pinned mirror.
int resident_attempts(pdlpdev_ctx* ctx, int count)
{
  TRY(launch_resident_tier(ctx, resident_tier(ctx->m, ctx->n, ctx->nnz), small_view(ctx), ctx->ctl_h->steps_taken + count, count));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}
int resident_major_eval(pdlpdev_ctx* ctx, int average_mode, int rc_rule_finite_bounds, int want_linf, double eps_rel_primal, double eps_rel_dual)
{
  const MajorSmallArgs A = major_args(ctx, average_mode, rc_rule_finite_bounds, want_linf, eps_rel_primal, eps_rel_dual);
  const size_t lds = sizeof(double) * (size_t)std::max<int64_t>(ctx->nnz, 1);
  TRY(major_lds_attribute(ctx->device));
  k_major_small<<<1, kMajorThreads, lds, ctx->stream>>>(A);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

// ================================================================================================
// K resident LPs at once: one workgroup per LP, one launch per phase of the loop
// ================================================================================================
// The phases of pdlp_solver.cpp's loop that touch the device -- attempts up to the next major iteration, the head of a major
// iteration, a restart, the scalar updates in front of the next attempts, A^T y of a fresh iterate -- each become ONE launch over the
// LPs that are in that phase (lists in pinned host memory), on the batch's own stream, with ONE synchronisation.  Every kernel body
// is the single LP's (resident_body, major_small_body, restart_block + finalize_rows, csr_stream_block), so each LP gets, bit for
// bit, the trajectory of its own solve; LPs of different resident tiers are launched tier by tier.
struct RestartBatchArgs {
  RestartView R;
  int g, pad;
  double* out;  // the LP's pinned scalar block: dist2 at [0], [1]
};
struct CtlOp {
  pdlpdev_ctl* ctl;
  int clear_error, set_weight;
  double weight;
};
__global__ void __launch_bounds__(kBlock) k_restart_batch(const RestartBatchArgs* __restrict__ args, const int2* __restrict__ blk)
{
  __shared__ double red[12];
  const int2 b = blk[blockIdx.x];
  restart_block(args[b.x].R, b.y, args[b.x].g, red);
}
__global__ void __launch_bounds__(kBlock) k_restart_finish_batch(const RestartBatchArgs* __restrict__ args, const int* __restrict__ list)
{
  __shared__ double red[8];
  const RestartBatchArgs& A = args[list[blockIdx.x]];
  finalize_rows(A.R.part, A.g, 2, 0u, A.out, red);
  if (threadIdx.x == 0) {  // k_restart_ctl
    pdlpdev_ctl* ctl       = const_cast<pdlpdev_ctl*>(A.R.ctl);
    ctl->sum_weights       = 0.0;
    ctl->its_since_restart = 0;
    ctl->pending_avg       = 0;
  }
}
__global__ void __launch_bounds__(kBlock) k_ctl_ops_batch(const CtlOp* __restrict__ ops, int n)
{
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  pdlpdev_ctl* ctl = ops[i].ctl;
  if (ops[i].clear_error) ctl->error = 0;  // k_clear_error
  if (ops[i].set_weight) {                 // k_set_step with the step size kept
    const double w     = ops[i].weight;
    ctl->primal_weight = w;
    ctl->tau           = ctl->step_size / w;
    ctl->sigma         = ctl->step_size * w;
  }
}

// The re-solve pattern of the MIP heuristics for K LPs in one launch (relaxed_lp.cu:74-108: other variable bounds, start from the previous
// primal / dual): per LP exactly what pdlpdev_reset(lb, ub) + pdlpdev_set_step + pdlpdev_set_k + pdlpdev_set_initial +
// pdlpdev_project_primal + pdlpdev_get_ctl do one call after the other -- the same expressions, element by element.
struct SmallResetArgs {
  int n, m, k, project;
  int var, warm;          // var >= 0: the bounds of this ONE variable become [var_lb, var_ub] (a branch); warm (PDLPDEV_CURRENT / AVERAGE /
  double var_lb, var_ub;  // BEST, < 0 none): start from that iterate of the LP itself -- unscaled and scaled again like a trip through the host
  const double *bestx, *besty;
  const double *lb_new, *ub_new, *x0, *y0;  // staging (device-visible host memory); NULL: bounds unchanged / start from zero
  double *lb_u, *ub_u, *lb, *ub;
  const double *dc, *dr;
  double *x[2], *aty[2], *rc[2], *y[2], *xbar, *sumx, *avgx, *lrx, *sumy, *avgy, *lry;
  pdlpdev_ctl *ctl, *ctl_host;
  double step, weight;
  const double* weight_dev;  // non-NULL: the weight k_small_objective_finish left on the device (a new objective), not `weight`
};
__global__ void __launch_bounds__(512) k_small_reset_batch(const SmallResetArgs* __restrict__ args, const int* __restrict__ list)
{
  const SmallResetArgs& A = args[list[blockIdx.x]];
  const int cur    = A.ctl->cur;  // (read by every thread before thread 0 rewrites the control block: the loops below end in a barrier-free
  __syncthreads();                //  store by thread 0 only after this barrier)
  const double* wx = A.warm == PDLPDEV_BEST ? A.bestx : A.warm == PDLPDEV_AVERAGE ? A.avgx : A.x[cur];
  const double* wy = A.warm == PDLPDEV_BEST ? A.besty : A.warm == PDLPDEV_AVERAGE ? A.avgy : A.y[cur];
  for (int j = threadIdx.x; j < A.n; j += 512) {
    if (A.lb_new) A.lb_u[j] = A.lb_new[j], A.lb[j] = A.lb_new[j] / A.dc[j];  // k_scale_bounds
    if (A.ub_new) A.ub_u[j] = A.ub_new[j], A.ub[j] = A.ub_new[j] / A.dc[j];
    if (j == A.var) {
      A.lb_u[j] = A.var_lb, A.lb[j] = A.var_lb / A.dc[j];
      A.ub_u[j] = A.var_ub, A.ub[j] = A.var_ub / A.dc[j];
    }
    const double lo = A.lb[j], hi = A.ub[j];
    double x = A.x0 ? A.x0[j] / A.dc[j] : 0.0;  // k_div_inplace (set_initial) on a zeroed iterate
    if (A.warm >= 0) x = (wx[j] * A.dc[j]) / A.dc[j];  // k_unscale (what the caller would have read back), then set_initial
    double avg = 0.0;
    if (A.project) x = dmin(dmax(x, lo), hi), avg = dmin(dmax(avg, lo), hi);  // k_clamp on the iterate and on the average
    A.x[0][j] = x, A.x[1][j] = 0.0, A.aty[0][j] = 0.0, A.aty[1][j] = 0.0, A.rc[0][j] = 0.0, A.rc[1][j] = 0.0;
    A.xbar[j] = 0.0, A.sumx[j] = 0.0, A.avgx[j] = avg, A.lrx[j] = 0.0;
  }
  for (int i = threadIdx.x; i < A.m; i += 512) {
    const double y = A.warm >= 0 ? (wy[i] * A.dr[i]) / A.dr[i] : (A.y0 ? A.y0[i] / A.dr[i] : 0.0);
    A.y[0][i] = y, A.y[1][i] = 0.0;
    A.sumy[i] = 0.0, A.avgy[i] = 0.0, A.lry[i] = 0.0;
  }
  if (threadIdx.x == 0) {
    pdlpdev_ctl c;
    memset(&c, 0, sizeof(c));
    const double w = A.weight_dev ? *A.weight_dev : A.weight;
    c.step_size = A.step, c.primal_weight = w, c.tau = A.step / w, c.sigma = A.step * w;  // k_set_step
    if (A.k >= 0) c.k = A.k;
    *A.ctl = c, *A.ctl_host = c;
  }
}
// New objectives for the LPs of a batch (pdlpdev_small_batch_reset_objectives) in front of k_small_reset_batch, no host in between.
// k_small_objective_batch: workgroup <-> (LP, block of the LP's virtual grid min(grid_for(n), kGenericBlocks)) -- per LP exactly
// k_set_objective's launch, from the staging block.  k_small_objective_finish: workgroup <-> LP -- k_finalize's tree over both rows of
// partials, then the initial primal weight (pdlp.cu:1260-1309) as the host forms it, sqrt and the division being correctly rounded on
// both sides; weight_host >= 0 (cuoptamd_settings::initial_primal_weight) overrides what the reset takes, not what is reported.
struct SmallObjectiveArgs {
  int n, g, unscaled_sum;  // unscaled_sum: the weight's sum is sum c_u^2 (compute_initial_primal_weight_before_scaling), else sum c^2
  const double* src;       // staging: the new objective, minimise sense, the device's column order
  double *c_u, *c;
  const double* dc;
  double *part, *scal, *scal_h;  // scal / scal_h [kObjSums .. +3): sum c_u^2, sum c^2, the computed weight; scal[kObjWeight]: the one to use
  double sum_b, c_scaling, b_scaling, importance, weight_host;
};
constexpr int kObjSums = 42, kObjWeight = 45;
__global__ void __launch_bounds__(kBlock) k_small_objective_batch(const SmallObjectiveArgs* __restrict__ args, const int2* __restrict__ blk)
{
  __shared__ double red[8];
  const int2 w                = blk[blockIdx.x];
  const SmallObjectiveArgs& A = args[w.x];
  set_objective_block(A.n, A.src, A.c_u, A.c, A.dc, A.part, w.y, A.g, red);
}
__global__ void __launch_bounds__(kBlock) k_small_objective_finish(const SmallObjectiveArgs* __restrict__ args, const int* __restrict__ list)
{
  __shared__ double red[8];
  __shared__ double sums[2];
  const SmallObjectiveArgs& A = args[list[blockIdx.x]];
  finalize_rows(A.part, A.g, 2, 0u, sums, red);
  if (threadIdx.x == 0) {
    const double cn = sqrt(A.c_scaling * (A.unscaled_sum ? sums[0] : sums[1]));
    const double bn = sqrt(A.b_scaling * A.sum_b);
    const double w  = (bn > 0.0 && cn > 0.0) ? A.importance * (cn / bn) : A.importance;
    A.scal[kObjSums] = sums[0], A.scal[kObjSums + 1] = sums[1], A.scal[kObjSums + 2] = w;
    A.scal_h[kObjSums] = sums[0], A.scal_h[kObjSums + 1] = sums[1], A.scal_h[kObjSums + 2] = w;
    A.scal[kObjWeight] = A.weight_host >= 0.0 ? A.weight_host : w;
  }
}
// pdlpdev_get_solution for K LPs: x = x^ * D_c, y = y^ * D_r (k_unscale), reduced costs as they are -- straight into the staging block
struct SmallSolutionArgs {
  int n, m, which;
  const pdlpdev_ctl* ctl;
  const double *x0, *x1, *y0, *y1, *avgx, *avgy, *bestx, *besty, *bestrc, *rc0, *rc1, *dc, *dr;
  double *out_x, *out_y, *out_rc;  // NULL: not wanted
};
__global__ void __launch_bounds__(512) k_small_solution_batch(const SmallSolutionArgs* __restrict__ args, const int* __restrict__ list)
{
  const SmallSolutionArgs& A = args[list[blockIdx.x]];
  const int cur   = A.ctl->cur;
  const double* x = A.which == PDLPDEV_BEST ? A.bestx : A.which == PDLPDEV_AVERAGE ? A.avgx : (cur ? A.x1 : A.x0);
  const double* y = A.which == PDLPDEV_BEST ? A.besty : A.which == PDLPDEV_AVERAGE ? A.avgy : (cur ? A.y1 : A.y0);
  const double* r = A.which == PDLPDEV_BEST ? A.bestrc : A.which == PDLPDEV_AVERAGE ? A.rc1 : A.rc0;
  for (int j = threadIdx.x; j < A.n; j += 512) {
    if (A.out_x) A.out_x[j] = x[j] * A.dc[j];
    if (A.out_rc) A.out_rc[j] = r[j];
  }
  if (A.out_y)
    for (int i = threadIdx.x; i < A.m; i += 512) A.out_y[i] = y[i] * A.dr[i];
}

struct pdlpdev_small_batch {
  int device = 0, K = 0;
  hipStream_t stream = nullptr;
  std::vector<pdlpdev_ctx*> ctx;
  std::vector<int> tier;
  size_t major_lds = 8;
  int at_blocks_cap = 0;
  void* pinned = nullptr;  // everything below lives in this one block (device-visible host memory)
  ResidentArgs* run_args = nullptr;
  int* run_list = nullptr;  // 3 * K: one list per tier
  MajorSmallArgs* major = nullptr;
  int* list = nullptr;      // K
  RestartBatchArgs* restart = nullptr;
  int2* blk = nullptr;      // restart / A^T y blocks -> (LP, block of the LP)
  StreamAtCurArgs* at = nullptr;
  CtlOp* ops = nullptr;
  SmallResetArgs* reset = nullptr;
  SmallObjectiveArgs* obj = nullptr;  // pdlpdev_small_batch_reset_objectives: the records and the (LP, block) table of its own (blk is
  int2* obj_blk = nullptr;            // rewritten by a Halpern reset's tail while the objective kernel may still wait in the stream)
  int obj_blocks_cap = 0;
  SmallSolutionArgs* sol = nullptr;
  double* staging = nullptr;  // 4 n + m doubles per LP (new bounds + initial iterate in, solutions out; behind them a new objective), LP l at stage_off[l]
  std::vector<size_t> stage_off;
  // A batch of LPs in reflected Halpern mode (pdlpdev_small_batch_create_halpern): the loop, its evaluation and the restart are
  // kernels_resident_halpern.hip's, their records sit in the same pinned block; blk holds 2 * at_blocks_cap entries (a reset
  // enqueues A^T y of the starting point AND the restart that sets the anchor before its one synchronisation).
  bool halpern = false;
  HalpernResidentArgs* hrun = nullptr;
  HalpernRestartArgs* hrestart = nullptr;
  // launches of the loop kernel / of the evaluation behind it, calls of pdlpdev_small_batch_run, and the synchronisations: one per
  // pass of a run in either mode; for a Halpern batch also restart rounds and resets, and one synchronisation per restart round, reset
  // and separate pdlpdev_small_batch_major_eval
  int64_t stat_loop_launches = 0, stat_eval_launches = 0, stat_periods = 0, stat_restart_rounds = 0, stat_resets = 0, stat_syncs = 0;
  int64_t stat_reset_launches = 0, stat_reset_syncs = 0;  // pdlpdev_small_batch_reset_stats: of every reset call, in either mode
  // pdlpdev_small_batch_set_halpern_device_major: per member a burst block on the device (hmaj[l]); in one pinned block of their own
  // the members' burst records (burst[l]: params, theta, views) and the ring of 16 decision records per member (ring[16 l + j])
  pdlpdev_halpern_major_state* hmaj = nullptr;
  void* burst_pinned = nullptr;
  HalpernBurstMember* burst = nullptr;
  pdlpdev_halpern_major_record* ring = nullptr;
  HalpernBurstStats burst_stats;  // pdlpdev_small_batch_halpern_burst_stats
  pdlpdev_small_batch() = default;
  pdlpdev_small_batch(const pdlpdev_small_batch&) = delete;
  pdlpdev_small_batch& operator=(const pdlpdev_small_batch&) = delete;
  ~pdlpdev_small_batch()  // (also on a failed creation's way out: the stream and the pinned block go with the struct)
  {
    if (stream) (void)hipStreamDestroy(stream);
    if (pinned) (void)hipHostFree(pinned);
    if (burst_pinned) (void)hipHostFree(burst_pinned);
    if (hmaj) (void)hipFree(hmaj);
  }
};

// the tier's instantiation of the averaging loop kernel for the LPs of `list`, enqueued
static int launch_resident_batch(pdlpdev_small_batch* b, int tier, const int* list, int count)
{
  return for_resident_tier(
    tier,
    [&](auto I) {
      constexpr ResidentTier r = kResidentTiers[decltype(I)::value];
      return launch_resident_kernel(k_pdhg_resident_batch<r.T, r.Q, r.U>, I, b->device, b->stream, count, b->run_args, list, 1 << 14);
    },
    [] { return 0; });
}
// the mode's evaluation kernel over b->major for the LPs of b->list[0 .. count), enqueued
static int launch_major_batch(pdlpdev_small_batch* b, int count)
{
  if (b->halpern) return halpern_batch_launch_eval(b->stream, b->device, b->major_lds, b->major, b->list, count);
  k_major_small_batch<<<count, kMajorThreads, b->major_lds, b->stream>>>(b->major, b->list);
  HIP_TRY(hipGetLastError());
  return 0;
}
// k_restart_batch's record of LP c (pdlpdev_restart(which, unscaled)'s view; distances to the LP's pinned scalars) and
// k_spmv_at_cur's (pdlpdev_compute_aty)
static RestartBatchArgs restart_batch_args(const pdlpdev_ctx* c, int which, int unscaled)
{
  return RestartBatchArgs{RestartView{c->n, c->m, which, unscaled, c->dc, c->dr, c->ctl, c->x[0], c->x[1], c->y[0], c->y[1], c->avgx, c->avgy, c->lrx, c->lry,
                                      c->sumx, c->sumy, c->part_g},
                          std::min(grid_for(std::max(c->n, c->m)), kGenericBlocks), 0, c->scal_h};
}
// the record of the restart's finish behind it (halpern_restart_finish_workgroup): ra.g blocks' partials, the distances to the LP's scalars
static HalpernRestartArgs halpern_restart_args(const pdlpdev_ctx* c, const RestartBatchArgs& ra, int clear, double theta)
{
  return HalpernRestartArgs{c->n, ra.g, clear, 0, theta, c->part_g, c->aty[0], c->aty[1], c->lraty, c->scal, c->scal_h, c->ctl, c->ctl_h, c->hal, c->hal_h};
}
static StreamAtCurArgs stream_at_cur_args(const pdlpdev_ctx* c)
{
  return StreamAtCurArgs{c->At.nb, c->At.rb, c->At.hot.off, c->At.hot.idx, c->At.hot.val, c->ctl, c->y[0], c->y[1], c->aty[0], c->aty[1]};
}

// pdlpdev_small_batch_create (halpern == false: the averaging iteration's batch) / pdlpdev_small_batch_create_halpern
static int small_batch_create(pdlpdev_small_batch** out, pdlpdev_ctx** ctx, int K, bool halpern)
{
  const char* const who = halpern ? "pdlpdev_small_batch_create_halpern" : "pdlpdev_small_batch_create";
  if (!out || !ctx || K < 1) return fail(-1, "%s: null argument", who);
  *out = nullptr;
  for (int l = 0; l < K; ++l) {
    const pdlpdev_ctx* c = ctx[l];
    if (!c) return fail(-1, "%s: null context", who);
    if (!c->small_resident || c->comm || c->At.layout() != pdlpdev_ctx::MatrixSide::kStream || c->dense.on)
      return fail(-7, "%s: LP %d is not on the resident small-LP path", who, l);
    if (c->halpern && !halpern)  // (the batch's loop, evaluation and restart are the averaging iteration's)
      return fail(-7, "pdlpdev_small_batch_create: LP %d is in reflected Halpern mode, which has no K-workgroup batch (solve them one after the other)", l);
    if (halpern && c->halpern != ctx[0]->halpern)
      return fail(-7, "%s: LP 0 and LP %d differ: a batch of averaging and reflected Halpern members is not available", who, l);
    if (halpern && !c->halpern) return fail(-7, "%s: LP %d is not in reflected Halpern mode", who, l);
    if (c->device != ctx[0]->device) return fail(-7, "%s: the LPs sit on different devices", who);
    for (int q = 0; q < l; ++q)
      if (ctx[q] == c) return fail(-1, "%s: LP %d and LP %d are the same context", who, q, l);
  }
  std::unique_ptr<pdlpdev_small_batch> b(new pdlpdev_small_batch());
  b->device = ctx[0]->device, b->K = K, b->halpern = halpern;
  b->ctx.assign(ctx, ctx + K);
  HIP_TRY(hipSetDevice(b->device));
  int blocks = 0, obj_blocks = 0;
  for (int l = 0; l < K; ++l) {
    obj_blocks += std::min(grid_for(ctx[l]->n), kGenericBlocks);
    b->tier.push_back(resident_tier(ctx[l]->m, ctx[l]->n, ctx[l]->nnz));
    b->major_lds = std::max(b->major_lds, sizeof(double) * (size_t)std::max<int64_t>(ctx[l]->nnz, 1));
    blocks += std::max(ctx[l]->At.nb, std::min(grid_for(std::max(ctx[l]->n, ctx[l]->m)), kGenericBlocks));
  }
  b->at_blocks_cap = blocks;
  b->obj_blocks_cap = obj_blocks;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_run = 0, o_list3 = o_run + up(sizeof(ResidentArgs) * K), o_major = o_list3 + up(sizeof(int) * 3 * K),
               o_list = o_major + up(sizeof(MajorSmallArgs) * K), o_restart = o_list + up(sizeof(int) * K),
               o_blk = o_restart + up(sizeof(RestartBatchArgs) * K), o_at = o_blk + up(sizeof(int2) * (size_t)blocks * (halpern ? 2 : 1)),
               o_ops = o_at + up(sizeof(StreamAtCurArgs) * K), o_reset = o_ops + up(sizeof(CtlOp) * K), o_sol = o_reset + up(sizeof(SmallResetArgs) * K),
               o_hrun = o_sol + up(sizeof(SmallSolutionArgs) * K), o_hrestart = o_hrun + (halpern ? up(sizeof(HalpernResidentArgs) * K) : 0),
               o_obj = o_hrestart + (halpern ? up(sizeof(HalpernRestartArgs) * K) : 0), o_objblk = o_obj + up(sizeof(SmallObjectiveArgs) * K),
               o_stage = o_objblk + up(sizeof(int2) * (size_t)obj_blocks + sizeof(int) * K);
  size_t total = o_stage;
  for (int l = 0; l < K; ++l) {
    b->stage_off.push_back((total - o_stage) / sizeof(double));
    total += up(sizeof(double) * (4 * (size_t)ctx[l]->n + (size_t)ctx[l]->m));
  }
  HIP_TRY(hipHostMalloc(&b->pinned, total, hipHostMallocDefault));
  char* base  = (char*)b->pinned;
  b->run_args = (ResidentArgs*)(base + o_run), b->run_list = (int*)(base + o_list3), b->major = (MajorSmallArgs*)(base + o_major);
  b->list = (int*)(base + o_list), b->restart = (RestartBatchArgs*)(base + o_restart), b->blk = (int2*)(base + o_blk);
  b->at = (StreamAtCurArgs*)(base + o_at), b->ops = (CtlOp*)(base + o_ops);
  b->reset = (SmallResetArgs*)(base + o_reset), b->sol = (SmallSolutionArgs*)(base + o_sol), b->staging = (double*)(base + o_stage);
  b->obj = (SmallObjectiveArgs*)(base + o_obj), b->obj_blk = (int2*)(base + o_objblk);
  if (halpern) b->hrun = (HalpernResidentArgs*)(base + o_hrun), b->hrestart = (HalpernRestartArgs*)(base + o_hrestart);
  HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
  TRY(major_lds_attribute(b->device));
  for (int l = 0; l < K; ++l) HIP_TRY(hipStreamSynchronize(ctx[l]->stream));  // whatever the set-ups left in flight
  for (int l = 0; l < K; ++l) ctx[l]->batches_alive += 1;
  *out = b.release();
  return 0;
}

// ---- a batch of LPs in reflected Halpern mode: the batched restart and pdlpdev_small_batch_reset's tail (the run and the evaluation are
// pdlpdev_small_batch_run's / _major_eval's own, with the mode's records and kernels) ----
// the restart of the LPs in b->list[0 .. count) (theta[l] < 0: the anchor and the counters only; clear: k_halpern_clear's values first),
// enqueued only: k_restart_batch with the current iterate as the candidate and scaled distances, blocks from b->blk + blk_first, then the
// finishing kernel.  The caller synchronises.
static int halpern_batch_enqueue_restart(pdlpdev_small_batch* b, int count, const double* theta, int clear, int blk_first)
{
  int blocks = blk_first;
  for (int q = 0; q < count; ++q) {
    const int l    = b->list[q];
    pdlpdev_ctx* c = b->ctx[l];
    b->restart[l]  = restart_batch_args(c, PDLPDEV_CURRENT, 0);
    b->hrestart[l] = halpern_restart_args(c, b->restart[l], clear, theta[l]);
    for (int i = 0; i < b->restart[l].g; ++i) b->blk[blocks++] = make_int2(l, i);
  }
  k_restart_batch<<<blocks - blk_first, kBlock, 0, b->stream>>>(b->restart, b->blk + blk_first);
  HIP_TRY(hipGetLastError());
  return halpern_batch_launch_restart_finish(b->stream, b->hrestart, b->list, count);
}
// pdlpdev_small_batch_reset's tail for a Halpern batch (the LPs of b->list, behind k_small_reset_batch): what pdlpdev_reset and the
// solver's start of a run do in this mode -- the Halpern block cleared, A^T y of the starting point, the restart that only sets the anchor
static int halpern_batch_reset_tail(pdlpdev_small_batch* b, int count)
{
  int blocks = 0;
  std::vector<double> theta(b->K, -1.0);
  for (int q = 0; q < count; ++q) {
    pdlpdev_ctx* c   = b->ctx[b->list[q]];
    b->at[b->list[q]] = stream_at_cur_args(c);
    for (int i = 0; i < c->At.nb; ++i) b->blk[blocks++] = make_int2(b->list[q], i);
    loop_state_touched(c);
  }
  TRY(launch_stream_at_cur_batch(b->stream, b->at, b->blk, blocks));
  return halpern_batch_enqueue_restart(b, count, theta.data(), 1, b->at_blocks_cap);
}

extern "C" {

int pdlpdev_small_batch_create(pdlpdev_small_batch** out, pdlpdev_ctx** ctx, int K) { return small_batch_create(out, ctx, K, false); }
int pdlpdev_small_batch_create_halpern(pdlpdev_small_batch** out, pdlpdev_ctx** ctx, int K) { return small_batch_create(out, ctx, K, true); }

int pdlpdev_small_batch_halpern_restart(pdlpdev_small_batch* b, const int32_t* restart, const double* theta, double* dist, pdlpdev_ctl* ctl, pdlpdev_halpern* hal)
{
  if (!b || !b->halpern) return fail(-1, "pdlpdev_small_batch_halpern_restart: not a batch of LPs in reflected Halpern mode");
  HIP_TRY(hipSetDevice(b->device));
  int count = 0;
  for (int l = 0; l < b->K; ++l)
    if (restart[l]) b->list[count++] = l;
  if (!count) return 0;
  TRY(halpern_batch_enqueue_restart(b, count, theta, 0, 0));
  HIP_TRY(hipStreamSynchronize(b->stream));
  b->stat_restart_rounds += 1, b->stat_syncs += 1;
  for (int l = 0; l < b->K; ++l)
    if (restart[l]) {
      const pdlpdev_ctx* c = b->ctx[l];
      if (dist) dist[2 * l] = c->scal_h[0], dist[2 * l + 1] = c->scal_h[1];
      if (ctl) ctl[l] = *c->ctl_h;
      if (hal) hal[l] = *c->hal_h;
    }
  return 0;
}
int pdlpdev_small_batch_get_halpern(pdlpdev_small_batch* b, pdlpdev_halpern* hal)
{
  if (!b || !b->halpern) return fail(-1, "pdlpdev_small_batch_get_halpern: not a batch of LPs in reflected Halpern mode");
  for (int l = 0; l < b->K; ++l) hal[l] = *b->ctx[l]->hal_h;
  return 0;
}
int pdlpdev_small_batch_stats(pdlpdev_small_batch* b, int64_t out[8])
{
  if (!b) return fail(-1, "pdlpdev_small_batch_stats: null batch");
  int tiers = 0;
  for (int t = 0; t < 3; ++t) tiers += std::count(b->tier.begin(), b->tier.end(), t) > 0;
  out[0] = b->halpern, out[1] = tiers, out[2] = b->stat_loop_launches, out[3] = b->stat_eval_launches, out[4] = b->stat_periods;
  out[5] = b->stat_restart_rounds, out[6] = b->stat_resets, out[7] = b->stat_syncs;
  return 0;
}

// ---- bursts of device-decided major iterations for a Halpern batch (kernels: kernels_halpern_major.hip) ----------------------------------
int pdlpdev_small_batch_set_halpern_device_major(pdlpdev_small_batch* b, int on)
{
  if (!b) return fail(-1, "pdlpdev_small_batch_set_halpern_device_major: null batch");
  if (!on) return 0;
  if (!b->halpern) return fail(-7, "pdlpdev_small_batch_set_halpern_device_major: a batch of LPs in reflected Halpern mode only");
  for (int l = 0; l < b->K; ++l)
    if (b->ctx[l]->halpern_rays)
      return fail(-7, "pdlpdev_small_batch_set_halpern_device_major: LP %d evaluates the infeasibility ray, whose verdict is the host's", l);
  HIP_TRY(hipSetDevice(b->device));
  const size_t K = (size_t)b->K;
  if (!b->hmaj) HIP_TRY(hipMalloc((void**)&b->hmaj, sizeof(pdlpdev_halpern_major_state) * K));
  if (!b->burst_pinned) {
    const size_t o_ring = (sizeof(HalpernBurstMember) * K + 255) & ~(size_t)255;
    HIP_TRY(hipHostMalloc(&b->burst_pinned, o_ring + sizeof(pdlpdev_halpern_major_record) * 16 * K, hipHostMallocDefault));
    b->burst = (HalpernBurstMember*)b->burst_pinned;
    b->ring  = (pdlpdev_halpern_major_record*)((char*)b->burst_pinned + o_ring);
  }
  return 0;
}
int pdlpdev_small_batch_halpern_burst_stats(pdlpdev_small_batch* b, int64_t out[4])
{
  if (!b || !out) return fail(-1, "pdlpdev_small_batch_halpern_burst_stats: null argument");
  out[0] = b->burst_stats.bursts, out[1] = b->burst_stats.periods, out[2] = b->burst_stats.records, out[3] = b->burst_stats.empty;
  return 0;
}
// Enqueued in stream order, no kernel waiting for another: the arming kernel; then per period the loop kernel per tier in use, the guarded
// evaluation, the decisions, the guarded restart over the (LP, block) table built once; ONE synchronisation behind the last period.
int pdlpdev_small_batch_run_halpern_burst(pdlpdev_small_batch* b, const int32_t* first_target, int32_t period, int32_t count, const pdlpdev_small_eval* rq,
                                          const pdlpdev_halpern_major_params* params, const double* theta, const double* r_prev,
                                          pdlpdev_halpern_major_record* records, int32_t* written, double* r_prev_out, pdlpdev_ctl* ctl,
                                          pdlpdev_halpern* hal)
{
  roctx::Range range("pdlp: Halpern burst of a small-LP batch (steps + evaluation + decision + restart, P periods)");
  if (!b || !first_target || !rq || !params || !theta || !r_prev || !records || !written)
    return fail(-1, "pdlpdev_small_batch_run_halpern_burst: null argument");
  if (!b->halpern || !b->hmaj || !b->burst) return fail(-7, "pdlpdev_small_batch_run_halpern_burst: call pdlpdev_small_batch_set_halpern_device_major first");
  if (count < 1 || count > 16 || period < 1 || period > (1 << 14))
    return fail(-1, "pdlpdev_small_batch_run_halpern_burst: 1 .. 16 periods of at least one step");
  HIP_TRY(hipSetDevice(b->device));
  const int K = b->K;
  int n = 0, blocks = 0, tier_count[3] = {0, 0, 0};
  for (int l = 0; l < K; ++l) {
    written[l] = 0;
    if (first_target[l] <= 0) continue;
    pdlpdev_ctx* c = b->ctx[l];
    // (the caller holds the control block; where the pinned mirror is known to be the device's, the request is checked against it)
    const bool known = c->ctl_h_current;
    if (c->halpern_rays || (known && (c->ctl_h->error != 0 || c->ctl_h->steps_taken >= first_target[l] || first_target[l] - c->ctl_h->steps_taken > period)))
      return fail(-7, "pdlpdev_small_batch_run_halpern_burst: LP %d: the first period must start inside (step error down, target ahead, at most one period away)", l);
    const int want_linf = wants_linf(rq[l].eps_p, rq[l].eps_d) ? 1 : 0;
    b->major[l]         = major_args(c, 3, rq[l].rule_finite, want_linf, rq[l].eps_p, rq[l].eps_d);  // (guard_target -1: the burst's kernel applies each period's)
    HalpernBurstMember& M = b->burst[l];
    M.run = HalpernResidentArgs{halpern_view(c), c->ctl, c->ctl_h, c->hal, c->hal_h, first_target[l], 0};
    M.st = b->hmaj + l, M.sc = c->scal_h + 32, M.ring = b->ring + 16 * (size_t)l;
    M.p = params[l], M.p.want_linf = want_linf, M.r_prev = r_prev[l];
    const RestartBatchArgs ra = restart_batch_args(c, PDLPDEV_CURRENT, 0);
    M.R = ra.R, M.fin = halpern_restart_args(c, ra, 0, theta[l]);
    halpern_burst_mark_ring(M.ring, count);
    for (int i = 0; i < ra.g; ++i) b->blk[blocks++] = make_int2(l, i);
    b->run_list[b->tier[l] * K + tier_count[b->tier[l]]++] = l;
    b->list[n++] = l;
    loop_state_touched(c);
  }
  if (!n) return 0;
  TRY(halpern_batch_burst_arm(b->stream, b->burst, b->list, n));
  for (int j = 0; j < count; ++j) {
    const int32_t add = j * period;
    for (int tier = 0; tier < 3; ++tier)
      if (tier_count[tier]) {
        TRY(halpern_batch_burst_loop(b->stream, b->device, tier, b->burst, b->run_list + tier * K, tier_count[tier], add));
        b->stat_loop_launches += 1;
      }
    TRY(halpern_batch_burst_eval(b->stream, b->device, b->major_lds, b->major, b->burst, b->list, n, add));
    b->stat_eval_launches += 1;
    TRY(halpern_batch_burst_decide(b->stream, b->burst, b->list, n, j, add));
    TRY(halpern_batch_burst_restart(b->stream, b->burst, b->blk, blocks, b->list, n, j));
  }
  HIP_TRY(hipStreamSynchronize(b->stream));
  b->stat_syncs += 1;
  b->burst_stats.bursts += 1, b->burst_stats.periods += count;
  for (int q = 0; q < n; ++q) {
    const int l    = b->list[q];
    pdlpdev_ctx* c = b->ctx[l];
    c->ctl_h_current = true;
    if (halpern_burst_collect(b->ring + 16 * (size_t)l, count, r_prev[l], records + 16 * (size_t)l, written + l, r_prev_out ? r_prev_out + l : nullptr,
                              &b->burst_stats))
      return fail(-6, "pdlpdev_small_batch_run_halpern_burst: LP %d: a record was written behind the period that stopped it", l);
    if (ctl) ctl[l] = *c->ctl_h;
    if (hal) hal[l] = *c->hal_h;
  }
  return 0;
}

void pdlpdev_small_batch_destroy(pdlpdev_small_batch* b)
{
  if (!b) return;
  for (pdlpdev_ctx* c : b->ctx) c->batches_alive -= 1;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  delete b;
}

// attempts until LP l holds targets[l] accepted steps (<= 0: LP l rests); ctl[l] receives its control block.
// eval_after (optional): the head of the major iteration that follows the attempts is enqueued right behind them for every LP with
// eval_after[l].mode >= 0 -- one synchronisation for both; the evaluation runs only if LP l's attempts reached their target (or raised
// the step-size error), evaluated[l] says whether it did, out_current / out_average then hold its results.
// Per tier in use ONE launch of the mode's loop kernel, behind them ONE launch of the mode's guarded evaluation, ONE synchronisation.
// A Halpern batch evaluates T(z^k) in the average slots (mode 3), whatever mode was asked for, takes a result as resident_halpern_period
// does for one LP (the target reached, no step error, the evaluation ran), and both outputs receive it.
int pdlpdev_small_batch_run(pdlpdev_small_batch* b, const int32_t* targets, pdlpdev_ctl* ctl, const pdlpdev_small_eval* eval_after, double* out_current,
                            double* out_average, int32_t* evaluated)
{
  roctx::Range range("pdlp: PDHG attempts (small-LP batch)");
  HIP_TRY(hipSetDevice(b->device));
  const int K = b->K;
  std::vector<char> todo(K, 0);
  for (int l = 0; l < K; ++l) {
    if (evaluated) evaluated[l] = 0;
    if (targets[l] <= 0) continue;
    pdlpdev_ctx* c = b->ctx[l];
    todo[l]        = 1;
    if (b->halpern) {
      b->hrun[l] = HalpernResidentArgs{halpern_view(c), c->ctl, c->ctl_h, c->hal, c->hal_h, targets[l], 0};
      loop_state_touched(c);
    } else {
      b->run_args[l] = ResidentArgs{small_view(c), c->ctl, c->ctl_h, c->sp, targets[l], 0};
    }
  }
  b->stat_periods += 1;
  for (int guard = 0; guard < 1000; ++guard) {
    int count[3] = {0, 0, 0};
    for (int l = 0; l < K; ++l)
      if (todo[l]) b->run_list[b->tier[l] * K + count[b->tier[l]]++] = l;
    if (count[0] + count[1] + count[2] == 0) break;
    for (int tier = 0; tier < 3; ++tier)
      if (count[tier]) {
        TRY(b->halpern ? halpern_batch_launch_loop(b->stream, b->device, tier, b->hrun, b->run_list + tier * K, count[tier])
                       : launch_resident_batch(b, tier, b->run_list + tier * K, count[tier]));
        b->stat_loop_launches += 1;
      }
    int nev = 0;
    if (guard == 0 && eval_after) {
      for (int l = 0; l < K; ++l)
        if (todo[l] && eval_after[l].mode >= 0) {
          const int want_linf = wants_linf(eval_after[l].eps_p, eval_after[l].eps_d);
          b->major[l] = major_args(b->ctx[l], b->halpern ? 3 : eval_after[l].mode, eval_after[l].rule_finite, want_linf, eval_after[l].eps_p, eval_after[l].eps_d);
          b->major[l].guard_target = targets[l];
          b->list[nev++]           = l;
        }
      if (nev) {
        TRY(launch_major_batch(b, nev));
        b->stat_eval_launches += 1;
      }
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->stat_syncs += 1;
    for (int q = 0; q < nev; ++q) {
      const int l          = b->list[q];
      const pdlpdev_ctx* c = b->ctx[l];
      if (c->scal_h[63] != 1.0) continue;
      if (b->halpern && (c->ctl_h->error != 0 || c->ctl_h->steps_taken < targets[l])) continue;
      const bool want_linf = wants_linf(eval_after[l].eps_p, eval_after[l].eps_d);
      read_eval(c->scal_h + (b->halpern ? 32 : 0), want_linf, out_current + (size_t)l * PDLPDEV_EV_COUNT);
      read_eval(c->scal_h + 32, want_linf, out_average + (size_t)l * PDLPDEV_EV_COUNT);
      if (evaluated) evaluated[l] = 1;
    }
    for (int l = 0; l < K; ++l)
      if (todo[l] && (b->ctx[l]->ctl_h->error != 0 || b->ctx[l]->ctl_h->steps_taken >= targets[l])) todo[l] = 0;
  }
  for (int l = 0; l < K; ++l)
    if (targets[l] > 0) {
      if (b->halpern) b->ctx[l]->ctl_h_current = true;  // (as resident_halpern_run leaves it: the kernel wrote the pinned mirror)
      if (ctl) ctl[l] = *b->ctx[l]->ctl_h;
    }
  return 0;
}

// pdlpdev_major_eval for every LP with req[l].mode >= 0: out_current / out_average hold PDLPDEV_EV_COUNT doubles per LP
int pdlpdev_small_batch_major_eval(pdlpdev_small_batch* b, const pdlpdev_small_eval* req, double* out_current, double* out_average)
{
  roctx::Range range("pdlp: major iteration evaluation (small-LP batch)");
  HIP_TRY(hipSetDevice(b->device));
  int count = 0;
  for (int l = 0; l < b->K; ++l)
    if (req[l].mode >= 0) {
      const int want_linf = wants_linf(req[l].eps_p, req[l].eps_d);
      b->major[l]         = major_args(b->ctx[l], req[l].mode, req[l].rule_finite, want_linf, req[l].eps_p, req[l].eps_d);
      b->list[count++]    = l;
    }
  if (!count) return 0;
  if (b->halpern) {  // the evaluation of T(z^k) in the average slots (mode 3), whatever mode was asked for: both outputs receive it
    for (int q = 0; q < count; ++q) b->major[b->list[q]].mode = 3;
    b->stat_syncs += 1;
  }
  TRY(launch_major_batch(b, count));
  HIP_TRY(hipStreamSynchronize(b->stream));
  for (int l = 0; l < b->K; ++l)
    if (req[l].mode >= 0) {
      const bool want_linf = wants_linf(req[l].eps_p, req[l].eps_d);
      read_eval(b->ctx[l]->scal_h + (b->halpern ? 32 : 0), want_linf, out_current + (size_t)l * PDLPDEV_EV_COUNT);
      read_eval(b->ctx[l]->scal_h + 32, want_linf, out_average + (size_t)l * PDLPDEV_EV_COUNT);
    }
  return 0;
}

// pdlpdev_restart for every LP with which[l] >= 0 (PDLPDEV_CURRENT / PDLPDEV_AVERAGE); dist2[2 l], dist2[2 l + 1]
int pdlpdev_small_batch_restart(pdlpdev_small_batch* b, const int32_t* which, const int32_t* unscaled_distances, double* dist2)
{
  HIP_TRY(hipSetDevice(b->device));
  if (b->halpern) return fail(-7, "pdlpdev_small_batch_restart: the averaging iteration's restart; a batch in reflected Halpern mode takes pdlpdev_small_batch_halpern_restart");
  int count = 0, blocks = 0;
  for (int l = 0; l < b->K; ++l)
    if (which[l] >= 0) {
      b->restart[l] = restart_batch_args(b->ctx[l], which[l], unscaled_distances ? unscaled_distances[l] : 0);
      const int g   = b->restart[l].g;
      for (int q = 0; q < g; ++q) b->blk[blocks++] = make_int2(l, q);
      b->list[count++] = l;
    }
  if (!count) return 0;
  k_restart_batch<<<blocks, kBlock, 0, b->stream>>>(b->restart, b->blk);
  k_restart_finish_batch<<<count, kBlock, 0, b->stream>>>(b->restart, b->list);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(b->stream));
  for (int l = 0; l < b->K; ++l)
    if (which[l] >= 0) dist2[2 * l] = b->ctx[l]->scal_h[0], dist2[2 * l + 1] = b->ctx[l]->scal_h[1];
  return 0;
}

// in front of the next attempts: pdlpdev_clear_error where clear_error[l], pdlpdev_set_step(-1, primal_weight[l]) where
// primal_weight[l] > 0, pdlpdev_compute_aty where compute_aty[l] (any array may be NULL)
int pdlpdev_small_batch_prepare(pdlpdev_small_batch* b, const int32_t* clear_error, const double* primal_weight, const int32_t* compute_aty)
{
  HIP_TRY(hipSetDevice(b->device));
  int nops = 0, blocks = 0, nat = 0;
  for (int l = 0; l < b->K; ++l) {
    const bool ce = clear_error && clear_error[l], sw = primal_weight && primal_weight[l] > 0.0;
    if (ce || sw) b->ops[nops++] = CtlOp{b->ctx[l]->ctl, ce ? 1 : 0, sw ? 1 : 0, sw ? primal_weight[l] : 0.0};
    if (compute_aty && compute_aty[l]) {
      b->at[l] = stream_at_cur_args(b->ctx[l]);
      for (int q = 0; q < b->at[l].nb; ++q) b->blk[blocks++] = make_int2(l, q);
      ++nat;
    }
  }
  if (nops) k_ctl_ops_batch<<<(nops + kBlock - 1) / kBlock, kBlock, 0, b->stream>>>(b->ops, nops);
  if (nat) TRY(launch_stream_at_cur_batch(b->stream, b->at, b->blk, blocks));
  if (nops || nat) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(b->stream));
  }
  return 0;
}

// the re-solve pattern (relaxed_lp.cu:74-108) for every LP with take[l] != 0: new variable bounds (lb[l] / ub[l]: n doubles each, NULL =
// unchanged), the state of a freshly scaled problem, step size / primal weight / k (< 0: 0) as given, the initial iterate x0[l] / y0[l]
// (UNSCALED; NULL = zeros), the projection of the initial primal (project != 0); ctl[l] receives the control block.  What
// pdlpdev_reset(lb, ub, NULL, NULL), pdlpdev_set_step, pdlpdev_set_k, pdlpdev_set_initial, pdlpdev_project_primal and pdlpdev_get_ctl
// do for one LP, bit for bit, in ONE launch.
// (obj != NULL: pdlpdev_small_batch_reset_objectives -- LPs with obj->c[l] get the new objective and the device's weight first)
struct SmallBatchObjectives {
  const double* const* c;
  const double *sum_b, *c_scaling, *b_scaling, *importance;
  const int32_t* unscaled_sum;
  double *sum_cu, *sum_c, *computed_weight;  // out, per LP with an objective
};
static int small_batch_reset_impl(pdlpdev_small_batch* b, const char* who, const SmallBatchObjectives* obj, const int32_t* take, const double* const* lb,
                                  const double* const* ub, const double* const* x0, const double* const* y0, const double* step, const double* weight,
                                  const int32_t* k, int project, pdlpdev_ctl* ctl, const int32_t* var, const double* var_lb, const double* var_ub,
                                  const int32_t* warm)
{
  HIP_TRY(hipSetDevice(b->device));
  int count = 0, nobj = 0, obj_blocks = 0;
  for (int l = 0; l < b->K; ++l) {
    if (!take[l]) continue;
    pdlpdev_ctx* c = b->ctx[l];
    if (!c->scaled) return fail(-1, "%s: LP %d has not been scaled yet", who, l);
    if (c->rows_aliased || c->clones_alive > 0) return fail(-7, "%s: LP %d shares arrays with clones", who, l);
    c->rejected_in_a_row = 0;
    const size_t n = (size_t)c->n, m = (size_t)c->m;
    double* st     = b->staging + b->stage_off[l];
    const double *slb = nullptr, *sub = nullptr, *sx = nullptr, *sy = nullptr;
    if (lb && lb[l]) memcpy(st, lb[l], n * sizeof(double)), slb = st;
    if (ub && ub[l]) memcpy(st + n, ub[l], n * sizeof(double)), sub = st + n;
    if (x0 && x0[l]) memcpy(st + 2 * n, x0[l], n * sizeof(double)), sx = st + 2 * n;
    if (y0 && y0[l]) memcpy(st + 3 * n, y0[l], m * sizeof(double)), sy = st + 3 * n;
    c->note_uniform_bounds(lb ? lb[l] : nullptr, ub ? ub[l] : nullptr);
    const int v = var ? var[l] : -1, wm = warm ? warm[l] : -1;
    if (v >= c->n) return fail(-1, "%s: LP %d has no variable %d", who, l, v);
    if (v >= 0) c->ubd.lb_same = 0, c->ubd.ub_same = 0;  // (one bound differs from the others now, or may)
    if (wm == PDLPDEV_BEST && !c->bestx) return fail(-1, "%s: LP %d saved no best iterate to start from", who, l);
    b->reset[l] = SmallResetArgs{c->n, c->m, k ? k[l] : -1, project, v, wm, v >= 0 ? var_lb[l] : 0.0, v >= 0 ? var_ub[l] : 0.0, c->bestx, c->besty,
                                 slb, sub, sx, sy, c->lb_u, c->ub_u, c->lb, c->ub, c->dc, c->dr,
                                 {c->x[0], c->x[1]}, {c->aty[0], c->aty[1]}, {c->rc[0], c->rc[1]}, {c->y[0], c->y[1]}, c->xbar, c->sumx, c->avgx, c->lrx,
                                 c->sumy, c->avgy, c->lry, c->ctl, c->ctl_h, step[l], weight[l], nullptr};
    if (obj && obj->c[l]) {
      if (c->shared_with_parent || c->lockstep_batches_alive > 0) return fail(-7, "%s: LP %d shares its objective with other contexts", who, l);
      double* sc = st + 3 * n + m;
      memcpy(sc, obj->c[l], n * sizeof(double));
      const int g = std::min(grid_for(c->n), kGenericBlocks);  // (pdlpdev_set_objective's grid for this n)
      b->obj[l]   = SmallObjectiveArgs{c->n, g, obj->unscaled_sum[l], sc, c->c_u, c->c, c->dc, c->part_g, c->scal, c->scal_h,
                                     obj->sum_b[l], obj->c_scaling[l], obj->b_scaling[l], obj->importance[l], weight[l]};
      b->reset[l].weight_dev = c->scal + kObjWeight;
      for (int i = 0; i < g; ++i) b->obj_blk[obj_blocks++] = make_int2(l, i);
      nobj += 1;
    }
    b->list[count++] = l;
  }
  if (!count) return 0;
  if (nobj) {
    int* olist = (int*)(b->obj_blk + b->obj_blocks_cap);  // (the LPs with an objective: K entries behind the table)
    int q = 0;
    for (int i = 0; i < count; ++i)
      if (b->reset[b->list[i]].weight_dev) olist[q++] = b->list[i];
    k_small_objective_batch<<<obj_blocks, kBlock, 0, b->stream>>>(b->obj, b->obj_blk);
    k_small_objective_finish<<<nobj, kBlock, 0, b->stream>>>(b->obj, olist);
    b->stat_reset_launches += 2;
  }
  k_small_reset_batch<<<count, 512, 0, b->stream>>>(b->reset, b->list);
  b->stat_reset_launches += 1;
  HIP_TRY(hipGetLastError());
  if (b->halpern) {
    TRY(halpern_batch_reset_tail(b, count));
    b->stat_resets += 1, b->stat_syncs += 1;
    b->stat_reset_launches += 3;  // (A^T y of the starting points, k_restart_batch, the restart's finish -- halpern_batch_reset_tail)
  }
  HIP_TRY(hipStreamSynchronize(b->stream));
  b->stat_reset_syncs += 1;
  if (ctl)
    for (int l = 0; l < b->K; ++l)
      if (take[l]) ctl[l] = *b->ctx[l]->ctl_h;
  if (obj)
    for (int l = 0; l < b->K; ++l)
      if (take[l] && obj->c[l]) {
        const double* sh = b->ctx[l]->scal_h + kObjSums;
        if (obj->sum_cu) obj->sum_cu[l] = sh[0];
        if (obj->sum_c) obj->sum_c[l] = sh[1];
        if (obj->computed_weight) obj->computed_weight[l] = sh[2];
      }
  return 0;
}
int pdlpdev_small_batch_reset(pdlpdev_small_batch* b, const int32_t* take, const double* const* lb, const double* const* ub, const double* const* x0,
                              const double* const* y0, const double* step, const double* weight, const int32_t* k, int project, pdlpdev_ctl* ctl,
                              const int32_t* var, const double* var_lb, const double* var_ub, const int32_t* warm)
{
  return small_batch_reset_impl(b, "pdlpdev_small_batch_reset", nullptr, take, lb, ub, x0, y0, step, weight, k, project, ctl, var, var_lb, var_ub, warm);
}
// pdlpdev_small_batch_reset with new objectives: c[l] (n doubles, minimise sense, the device's column order; NULL: LP l keeps its
// objective and takes weight[l], exactly pdlpdev_small_batch_reset's path).  An LP with c[l] gets, per LP bit for bit,
// pdlpdev_set_objective(c[l]) and then the initial primal weight formed ON THE DEVICE from the sum that unscaled_sum[l] selects, the
// host's sum_b[l] and the three hyper-parameters; weight[l] >= 0 there is an override the reset takes instead (weight[l] < 0: none).
// No host round trip between objective and reset, launches independent of K, the one synchronisation of pdlpdev_small_batch_reset.
// sum_cu / sum_c / computed_weight (each may be NULL) receive, for the LPs with c[l], both sums and the weight as computed.
int pdlpdev_small_batch_reset_objectives(pdlpdev_small_batch* b, const int32_t* take, const double* const* c, const double* const* lb, const double* const* ub,
                                         const double* const* x0, const double* const* y0, const double* step, const double* weight, const int32_t* k,
                                         int project, pdlpdev_ctl* ctl, const int32_t* var, const double* var_lb, const double* var_ub, const int32_t* warm,
                                         const double* sum_b, const double* c_scaling, const double* b_scaling, const double* importance,
                                         const int32_t* unscaled_sum, double* sum_cu, double* sum_c, double* computed_weight)
{
  const char* const who = "pdlpdev_small_batch_reset_objectives";
  if (!b || !take || !step || !weight) return fail(-1, "%s: null argument", who);
  if (!c) return small_batch_reset_impl(b, who, nullptr, take, lb, ub, x0, y0, step, weight, k, project, ctl, var, var_lb, var_ub, warm);
  if (!sum_b || !c_scaling || !b_scaling || !importance || !unscaled_sum) return fail(-1, "%s: null argument", who);
  const SmallBatchObjectives obj{c, sum_b, c_scaling, b_scaling, importance, unscaled_sum, sum_cu, sum_c, computed_weight};
  return small_batch_reset_impl(b, who, &obj, take, lb, ub, x0, y0, step, weight, k, project, ctl, var, var_lb, var_ub, warm);
}
int pdlpdev_small_batch_reset_stats(pdlpdev_small_batch* b, int64_t out[2])
{
  if (!b || !out) return fail(-1, "pdlpdev_small_batch_reset_stats: null argument");
  out[0] = b->stat_reset_launches, out[1] = b->stat_reset_syncs;
  return 0;
}

// the same without the copies: x_view[l] / y_view[l] / rc_view[l] point INTO the batch's pinned staging block (valid until the next
// pdlpdev_small_batch_reset / _get_solutions / _solution_views call of this batch)
int pdlpdev_small_batch_solution_views(pdlpdev_small_batch* b, const int32_t* which, const double** x_view, const double** y_view, const double** rc_view)
{
  HIP_TRY(hipSetDevice(b->device));
  int count = 0;
  for (int l = 0; l < b->K; ++l) {
    if (x_view) x_view[l] = nullptr;
    if (y_view) y_view[l] = nullptr;
    if (rc_view) rc_view[l] = nullptr;
    if (which[l] < 0) continue;
    pdlpdev_ctx* c = b->ctx[l];
    if (which[l] == PDLPDEV_BEST && !c->bestx) return fail(-1, "pdlpdev_small_batch_solution_views: LP %d saved no best iterate", l);
    const size_t n = (size_t)c->n;
    double* st     = b->staging + b->stage_off[l];
    b->sol[l] = SmallSolutionArgs{c->n, c->m, which[l], c->ctl, c->x[0], c->x[1], c->y[0], c->y[1], c->avgx, c->avgy, c->bestx, c->besty, c->bestrc,
                                  c->rc[0], c->rc[1], c->dc, c->dr, x_view ? st : nullptr, y_view ? st + 2 * n : nullptr, rc_view ? st + n : nullptr};
    if (x_view) x_view[l] = st;
    if (rc_view) rc_view[l] = st + n;
    if (y_view) y_view[l] = st + 2 * n;
    b->list[count++] = l;
  }
  if (!count) return 0;
  k_small_solution_batch<<<count, 512, 0, b->stream>>>(b->sol, b->list);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// pdlpdev_get_solution(which[l]) for every LP with which[l] >= 0: UNSCALED x[l] (n), y[l] (m), reduced costs rc[l] (n); any array or
// entry may be NULL.  One launch, one synchronisation; the copies to the caller's arrays are plain host copies.
int pdlpdev_small_batch_get_solutions(pdlpdev_small_batch* b, const int32_t* which, double* const* x, double* const* y, double* const* rc)
{
  HIP_TRY(hipSetDevice(b->device));
  int count = 0;
  for (int l = 0; l < b->K; ++l) {
    if (which[l] < 0) continue;
    pdlpdev_ctx* c = b->ctx[l];
    if (which[l] == PDLPDEV_BEST && !c->bestx) return fail(-1, "pdlpdev_small_batch_get_solutions: LP %d saved no best iterate", l);
    const size_t n = (size_t)c->n;
    double* st     = b->staging + b->stage_off[l];
    b->sol[l] = SmallSolutionArgs{c->n, c->m, which[l], c->ctl, c->x[0], c->x[1], c->y[0], c->y[1], c->avgx, c->avgy, c->bestx, c->besty, c->bestrc,
                                  c->rc[0], c->rc[1], c->dc, c->dr, (x && x[l]) ? st : nullptr, (y && y[l]) ? st + 2 * n : nullptr, (rc && rc[l]) ? st + n : nullptr};
    b->list[count++] = l;
  }
  if (!count) return 0;
  k_small_solution_batch<<<count, 512, 0, b->stream>>>(b->sol, b->list);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(b->stream));
  for (int l = 0; l < b->K; ++l) {
    if (which[l] < 0) continue;
    const size_t n = (size_t)b->ctx[l]->n, m = (size_t)b->ctx[l]->m;
    const double* st = b->staging + b->stage_off[l];
    if (x && x[l]) memcpy(x[l], st, n * sizeof(double));
    if (rc && rc[l]) memcpy(rc[l], st + n, n * sizeof(double));
    if (y && y[l]) memcpy(y[l], st + 2 * n, m * sizeof(double));
  }
  return 0;
}

}  // extern "C"
