// The restarted reflected-Halpern mode on the resident small-LP path (docs/design/04d_halpern_mode.md, "The resident variant"): a whole
// period of Halpern steps inside ONE workgroup with the LP on chip, and the one-workgroup evaluation of T(z^k) behind it.  A
// translation unit of its own, so that k_pdhg_resident / k_pdhg_resident_batch / k_major_small in kernels_resident.hip keep the
// instructions they had (kernels_halpern.hip was split off kernels_stream.hip for the same reason).
#include "pdlp_ctx.hpp"
#include "pdlp_layouts.hpp"
#include "resident_common.hpp"

// (HalpernSmallView, HalpernResidentArgs: resident_common.hpp -- the batch object in kernels_resident.hip holds the records)
// resident_body's layout, lanes and barriers (B1 ... B5, B5 inside block_sum_fast) with the Halpern epilogues in the two row phases:
//   * registers per owned element: x, x', A^T y, y, y' and the anchor x^0, y^0, A^T y^0 (loaded once; no running sums: no average);
//   * LDS exactly as in resident_body (xbar_s, yn_s, the five constant vectors, prod): nothing is added;
//   * a step: x' and xbar as in the averaging loop -> B1 -> A xbar products -> B2 -> y' (HalpernDualEpilogue's expressions) into yn_s,
//     ||dy||^2, y <- combine(y', y, y^0) -> B3 -> A^T y' products -> B4 -> v = A^T y', HalpernStepEpilogue's two sums,
//     x <- combine(x', x, x^0), A^T y <- combine(v, A^T y, A^T y^0) -> the three sums (B5) -> k_halpern_decision's arithmetic in
//     every lane on its own copy of the two blocks.
// Products are val * vec[col] and every row is added left to right, the combination is HalpernWeights::combine: the iterates are the
// stream layout's multi-launch kernels' bit for bit (the step is constant, so the differently ordered sums never reach an iterate).
// LDS hazards: resident_body's table holds; yn_s is written before B3 by its owners, who form y^{k+1} from the same value in a
// register (no second reader), and gathered before B4.  red[2] by step parity as there; there is no pw.
template <int T, int Q, int U>
__device__ __forceinline__ void resident_halpern_body(const HalpernSmallView& V, pdlpdev_ctl* __restrict__ ctl, pdlpdev_ctl* __restrict__ ctl_host,
                                                      pdlpdev_halpern* __restrict__ hal, pdlpdev_halpern* __restrict__ hal_host,
                                                      int target_steps, int max_steps, double* lds)
{
  double* xbar_s = lds;               // Q*T
  double* yn_s   = xbar_s + Q * T;    // Q*T
  double* c_s    = yn_s + Q * T;      // constants, read with stride 1 by their owners
  double* lb_s   = c_s + Q * T;
  double* ub_s   = lb_s + Q * T;
  double* lo_s   = ub_s + Q * T;
  double* hi_s   = lo_s + Q * T;
  double* prod   = hi_s + Q * T;      // U*T
  __shared__ double red[2][3 * 16];   // (two sets by step parity: see resident_body)
  const int t = threadIdx.x;
  // every lane keeps its own copy of both blocks and repeats the (uniform) bookkeeping of a step
  pdlpdev_ctl lc = *ctl;
  lc.target_steps = target_steps;
  pdlpdev_halpern lh = *hal;
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
  double x[Q], xn[Q], aty[Q], y[Q], yn[Q], ax[Q], ay[Q], aaty[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int e = t + q * T;
    const bool row = e < V.m, col = e < V.n;
    r0[q] = row ? V.a_off[e] : 0, r1[q] = row ? V.a_off[e + 1] : 0;
    c0[q] = col ? V.at_off[e] : 0, c1[q] = col ? V.at_off[e + 1] : 0;
    c_s[e] = col ? V.c[e] : 0.0, lb_s[e] = col ? V.lb[e] : 0.0, ub_s[e] = col ? V.ub[e] : 0.0;
    x[q]    = col ? (cur0 ? V.x1 : V.x0)[e] : 0.0;
    aty[q]  = col ? (cur0 ? V.aty1 : V.aty0)[e] : 0.0;
    ax[q]   = col ? V.ax[e] : 0.0;
    aaty[q] = col ? V.aaty[e] : 0.0;
    lo_s[e] = row ? V.lo[e] : 0.0, hi_s[e] = row ? V.hi[e] : 0.0;
    y[q]    = row ? (cur0 ? V.y1 : V.y0)[e] : 0.0;
    ay[q]   = row ? V.ay[e] : 0.0;
    xn[q] = x[q], yn[q] = y[q];
  }
  const int used = (V.nnz + T - 1) / T;  // nonzero slots in use (uniform): tiny LPs skip the empty ones
  int made = 0;
  for (int step = 0; step < max_steps; ++step) {
    if (lc.error != 0 || lc.steps_taken >= lc.target_steps) break;  // uniform: every lane holds the same lc
    const double tau = lc.tau, sigma = lc.sigma;
    const HalpernWeights hw(&lh);
    const int par = step & 1;
    if (lc.steps_taken + 1 >= lc.target_steps) {
      // the LAST step of the launch: z^k goes where the multi-launch kernels leave it -- the side `cur` selects now, which this step's
      // flip makes the other one.  The ray pass of the evaluation behind the launch forms T(z^k) - z^k from there (uniform branch).
      double* xk = lc.cur ? V.x1 : V.x0;
      double* yk = lc.cur ? V.y1 : V.y0;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int e = t + q * T;
        if (e < V.n) xk[e] = x[q];
        if (e < V.m) yk[e] = y[q];
      }
    }
    // primal projection (utils.cuh:80-95): x' and the extrapolated point
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int j = t + q * T;
      if (j < V.n) {
        const double gradient = c_s[j] - aty[q];
        double next           = x[q] - (tau * gradient);
        next                  = dmax(dmin(next, ub_s[j]), lb_s[j]);
        xn[q]                 = next;
        xbar_s[j]             = next - x[q] + next;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (u < used) prod[t + u * T] = a_val[u] * xbar_s[a_col[u]];
    __syncthreads();
    // HalpernDualEpilogue: y' = proj(y - sigma A xbar) -> yn_s (what the A^T product gathers), ||dy||^2, y^{k+1}
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = t + q * T;
      if (i < V.m) {
        const double v   = lds_row_sum(prod, r0[q], r1[q]);
        const double yi  = y[q];
        double next      = yi - (sigma * v);
        const double low = next + sigma * lo_s[i];
        const double up  = next + sigma * hi_s[i];
        next             = dmax(low, dmin(up, 0.0));
        yn[q]            = next;
        yn_s[i]          = next;
        const double dy  = next - yi;
        acc[0] += dy * dy;
        y[q] = hw.combine(next, yi, ay[q]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (u < used) prod[t + u * T] = at_val[u] * yn_s[at_col[u]];
    __syncthreads();
    // HalpernStepEpilogue: v = A^T y', dx . (v - A^T y^k), ||dx||^2, then x^{k+1} and A^T y^{k+1} by the same combination
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int j = t + q * T;
      if (j < V.n) {
        const double v  = lds_row_sum(prod, c0[q], c1[q]);
        const double xj = x[q], xt = xn[q], a = aty[q];
        const double dx = xt - xj;
        const double d  = v - a;
        acc[1] += d * dx;
        acc[2] += dx * dx;
        x[q]   = hw.combine(xt, xj, ax[q]);
        aty[q] = hw.combine(v, a, aaty[q]);
      }
    }
    block_sum_fast<3, T / 64>(acc, red[par]);
    {  // k_halpern_decision's arithmetic (pdlp_device.hip), in every lane
      const double dy2 = acc[0], interaction = acc[1], dx2 = acc[2];
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
      }
      lc.k += 1;
      lc.cur ^= 1;
      lc.steps_taken += 1;
      lc.its_since_restart += 1;
    }
    made = 1;
  }
  {
    const int cur = lc.cur;
    double* xo    = cur ? V.x1 : V.x0;
    double* yo    = cur ? V.y1 : V.y0;
    double* atyo  = cur ? V.aty1 : V.aty0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int e = t + q * T;
      if (e < V.n) xo[e] = x[q], atyo[e] = aty[q];
      if (e < V.m) yo[e] = y[q];
      if (made) {  // T(z^k) of the last step: what the multi-launch kernels leave in the average slots (a launch without a step keeps them)
        if (e < V.n) V.tx[e] = xn[q];
        if (e < V.m) V.ty[e] = yn[q];
      }
    }
  }
  if (t == 0) *ctl = lc, *ctl_host = lc, *hal = lh, *hal_host = lh;  // the pinned mirrors save the read-back copies
}
template <int T, int Q, int U>
__global__ void __launch_bounds__(T)
k_pdhg_resident_halpern(HalpernSmallView V, pdlpdev_ctl* __restrict__ ctl, pdlpdev_ctl* __restrict__ ctl_host, pdlpdev_halpern* __restrict__ hal,
                        pdlpdev_halpern* __restrict__ hal_host, int target_steps, int max_steps)
{
  extern __shared__ double lds[];
  resident_halpern_body<T, Q, U>(V, ctl, ctl_host, hal, hal_host, target_steps, max_steps, lds);
}
// p, which points to global memory, as a pointer the compiler knows that of (the empty statement keeps the two casts from cancelling
// and names a scalar register: the value is uniform)
template <class P>
__device__ __forceinline__ P* as_global(P* p)
{
  __attribute__((address_space(1))) P* g = (__attribute__((address_space(1))) P*)p;
  asm("" : "+s"(g));
  return (P*)g;
}
// K LPs, one workgroup each, ONE launch: workgroup b runs the Halpern loop of LP list[b] exactly as k_pdhg_resident_halpern would -- the
// same body, so every LP's iterates, scalars and counters are bit for bit those of its own launch (k_pdhg_resident_batch's arrangement).
template <int T, int Q, int U>
__global__ void __launch_bounds__(T) k_pdhg_resident_halpern_batch(const HalpernResidentArgs* __restrict__ args, const int* __restrict__ list, int max_steps)
{
  extern __shared__ double lds[];
  const HalpernResidentArgs& A = args[list[blockIdx.x]];
  // A pointer read from memory is a generic one to the compiler, a kernel argument is known to point to global memory.  as_global
  // says so for the record's pointers: the two blocks are then read with scalar loads and the vectors with global ones, as in
  // k_pdhg_resident_halpern (145 / 193 / 195 VGPRs; with generic pointers both blocks sit in vector registers: 168 / 219 / 223).
  const HalpernSmallView& S = A.V;
  const HalpernSmallView V{S.m, S.n, S.nnz, as_global(S.a_off), as_global(S.a_idx), as_global(S.at_off), as_global(S.at_idx), as_global(S.a_val),
                           as_global(S.at_val), as_global(S.c), as_global(S.lb), as_global(S.ub), as_global(S.lo), as_global(S.hi), as_global(S.x0),
                           as_global(S.x1), as_global(S.y0), as_global(S.y1), as_global(S.aty0), as_global(S.aty1), as_global(S.ax), as_global(S.ay),
                           as_global(S.aaty), as_global(S.tx), as_global(S.ty)};
  resident_halpern_body<T, Q, U>(V, as_global(A.ctl), as_global(A.ctl_host), as_global(A.hal), as_global(A.hal_host), A.target_steps, max_steps, lds);
}

// MajorSmallArgs::mode == 3, served by a kernel of its own: no average is formed and nothing is flushed; the average slots are
// evaluated as the loop left them (T(z^k) of the period's last step), results in sc[32..41) as k_major_small leaves the average's.
// KEEP IN STEP with major_small_body (kernels_resident.hip): what follows the guard is its `which == 1` pass, statement for
// statement (epilogues, reduction trees, slots of sc).  It is a copy and not a shared helper because both ways of sharing it were
// tried and both change k_major_small / k_major_small_batch: a mode-3 branch inside major_small_body, and a __forceinline__
// per-point helper called by both bodies (1206 lines of llvm-objdump -d of kernels_resident's gfx950 code object differ) -- and
// the existing kernels are to keep the instructions they had.  guard_target as in
// k_major_small_batch; sc[63] says whether the evaluation ran.
__device__ __forceinline__ void major_small_halpern_body(const MajorSmallArgs& A, double* prod /* nnz doubles of LDS */)
{
  __shared__ double red[4 * kMajorThreads / 64];
  const int t = threadIdx.x;
  if (A.guard_target >= 0 && !(A.ctl->error != 0 || A.ctl->steps_taken >= A.guard_target)) {  // (uniform)
    if (t == 0) A.sc[63] = 0.0;  // "not evaluated"
    return;
  }
  double* sc = A.sc + 32;
  {
    EvalPrimalEpilogue e{A.avgy, A.dr, A.lo_u, A.hi_u, A.eps_p, A.want_linf ? A.linf_m : nullptr, A.ax_avg};
    double acc[3] = {0.0, 0.0, 0.0};
    small_rows(A.m, A.a_off, A.a_idx, A.a_val, A.avgx, prod, e, acc);
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
    EvalDualEpilogue e{EvalDualCore{A.avgx, A.dc, A.c_u, A.lb_u, A.ub_u, A.eps_d, A.rule_finite, A.rc_avg, A.want_linf ? A.linf_n : nullptr, A.aty_avg}};
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    small_rows(A.n, A.at_off, A.at_idx, A.at_val, A.avgy, prod, e, acc);
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
  if (A.want_ray) {
    // Infeasibility detection: the infeasibility information with the displacement of the last step in the iterate's place
    // (k_halpern_ray_rows / _cols of pdlp_eval.hip as epilogues).  T(z^k) is what the two passes above evaluated; z^k is in the side
    // of the ping-pong pairs `cur` does not select.  The scaled displacement goes to linf_n / linf_m for the products to gather
    // (written here, read behind small_rows' barrier by the same workgroup); prod is free behind the barriers above.
    __shared__ double rred[6 * kMajorThreads / 64];
    const int cur    = A.ctl->cur;
    const double* xk = cur ? A.x0 : A.x1;
    const double* yk = cur ? A.y0 : A.y1;
    for (int j = t; j < A.n; j += kMajorThreads) A.linf_n[j] = A.avgx[j] - xk[j];
    for (int i = t; i < A.m; i += kMajorThreads) A.linf_m[i] = A.avgy[i] - yk[i];
    __syncthreads();
    {
      RayRowsEpilogue e{A.avgy, yk, A.dr, A.lo_u, A.hi_u};
      double acc[3] = {0.0, 0.0, 0.0};
      small_rows(A.m, A.a_off, A.a_idx, A.a_val, A.linf_n, prod, e, acc);
      double mx[2] = {acc[0], acc[1]}, sm[1] = {acc[2]};
      block_reduce<MaxOp, 2, kMajorThreads / 64>(mx, rred);
      __syncthreads();
      block_reduce<SumOp, 1, kMajorThreads / 64>(sm, rred + 2 * (kMajorThreads / 64));
      if (t == 0) A.sc[kRayRows] = mx[0], A.sc[kRayRows + 1] = mx[1], A.sc[kRayRows + 2] = sm[0];
      __syncthreads();
    }
    {
      RayColsEpilogue e{A.avgx, xk, A.dc, A.c_u, A.lb_u, A.ub_u, A.rule_finite};
      double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      small_rows(A.n, A.at_off, A.at_idx, A.at_val, A.linf_m, prod, e, acc);
      double mx[4] = {acc[0], acc[1], acc[2], acc[3]}, sm[2] = {acc[4], acc[5]};
      block_reduce<MaxOp, 4, kMajorThreads / 64>(mx, rred);
      __syncthreads();
      block_reduce<SumOp, 2, kMajorThreads / 64>(sm, rred + 4 * (kMajorThreads / 64));
      if (t == 0) {
        for (int q = 0; q < 4; ++q) A.sc[kRayCols + q] = mx[q];
        A.sc[kRayCols + 4] = sm[0], A.sc[kRayCols + 5] = sm[1];
        A.sc[kRayMark] = (double)A.ctl->steps_taken, A.sc[kRayMark + 1] = A.rule_finite != 0 ? 1.0 : 0.0;
      }
    }
  }
  if (t == 0) A.sc[63] = 1.0;
}
__global__ void __launch_bounds__(kMajorThreads) k_major_small_halpern(MajorSmallArgs A)
{
  extern __shared__ double prod[];
  major_small_halpern_body(A, prod);
}
// the same for the LPs of a batch: workgroup b evaluates LP list[b] (its own guard_target, its own sc[63])
__global__ void __launch_bounds__(kMajorThreads) k_major_small_halpern_batch(const MajorSmallArgs* __restrict__ args, const int* __restrict__ list)
{
  extern __shared__ double prod[];
  major_small_halpern_body(args[list[blockIdx.x]], prod);
}

// Behind k_restart_batch (candidate = the current iterate, scaled distances) for the LPs of a Halpern batch: what pdlpdev_halpern_restart
// enqueues behind k_restart for one LP -- k_finalize's two sums (finalize_rows: the same tree), k_copy_current of A^T y into the anchor's,
// k_halpern_restart_ctl's arithmetic with this LP's theta -- in one workgroup per LP; both blocks go to their pinned mirrors and the two
// distances to the LP's pinned scalars.  clear != 0 (a reset): k_halpern_clear's values first.
__global__ void __launch_bounds__(kBlock) k_halpern_restart_finish_batch(const HalpernRestartArgs* __restrict__ args, const int* __restrict__ list)
{
  __shared__ double red[8];
  const HalpernRestartArgs& A = args[list[blockIdx.x]];
  const int cur = A.ctl->cur;  // (read by every thread in front of finalize_rows' barriers; thread 0 rewrites the block behind them)
  finalize_rows(A.part, A.g, 2, 0u, A.dist2, red);
  const double* __restrict__ v = cur ? A.aty1 : A.aty0;
  for (int i = threadIdx.x; i < A.n; i += kBlock) A.lraty[i] = v[i];
  if (threadIdx.x == 0) {
    pdlpdev_ctl* ctl     = A.ctl;
    pdlpdev_halpern* hal = A.hal;
    if (A.clear) {  // k_halpern_clear
      hal->r = hal->r_first = hal->r2 = 0.0;
      hal->r2_min = __builtin_huge_val();
      hal->k = 0, hal->reserved = 0;
    }
    const double dx = sqrt(A.dist2[0]), dy = sqrt(A.dist2[1]);  // k_halpern_restart_ctl
    A.dist2[0] = dx, A.dist2[1] = dy;
    A.dist_host[0] = dx, A.dist_host[1] = dy;
    if (A.theta >= 0.0 && dx > 1.0e-10 && dy > 1.0e-10) {
      const double w     = exp(A.theta * log(dy / dx) + (1.0 - A.theta) * log(ctl->primal_weight));
      ctl->primal_weight = w;
      ctl->tau           = ctl->step_size / w;
      ctl->sigma         = ctl->step_size * w;
    }
    ctl->its_since_restart = 0;
    hal->k                 = 0;
    *A.ctl_host = *ctl, *A.hal_host = *hal;  // the pinned mirrors save the read-back copies
  }
}

HalpernSmallView halpern_view(const pdlpdev_ctx* ctx)
{
  return HalpernSmallView{ctx->m, ctx->n, (int)ctx->nnz, ctx->A.full.off, ctx->A.full.idx, ctx->At.full.off, ctx->At.full.idx, ctx->A.full.val, ctx->At.full.val,
                          ctx->c, ctx->lb, ctx->ub, ctx->lo, ctx->hi, ctx->x[0], ctx->x[1], ctx->y[0], ctx->y[1], ctx->aty[0],
                          ctx->aty[1], ctx->lrx, ctx->lry, ctx->lraty, ctx->avgx, ctx->avgy};
}
static int enqueue_resident_halpern(pdlpdev_ctx* ctx, int32_t target_steps)
{
  const HalpernSmallView V = halpern_view(ctx);
  return for_resident_tier(
    resident_tier(ctx->m, ctx->n, ctx->nnz),
    [&](auto I) {
      constexpr ResidentTier r = kResidentTiers[decltype(I)::value];
      return launch_resident_kernel(k_pdhg_resident_halpern<r.T, r.Q, r.U>, I, ctx->device, ctx->stream, 1, V, ctx->ctl, ctx->ctl_h, ctx->hal, ctx->hal_h,
                                    target_steps, 1 << 14);
    },
    [] { return fail(-1, "resident Halpern loop: the LP fits no tier"); });
}
static int enqueue_resident_halpern_eval(pdlpdev_ctx* ctx, int rc_rule_finite_bounds, int want_linf, double eps_rel_primal, double eps_rel_dual, int guard_target)
{
  TRY(allow_dynamic_lds((const void*)k_major_small_halpern, ctx->device, 8192 * 8));
  MajorSmallArgs A = major_args(ctx, 3, rc_rule_finite_bounds, want_linf, eps_rel_primal, eps_rel_dual);
  A.guard_target   = guard_target;
  const size_t lds = sizeof(double) * (size_t)std::max<int64_t>(ctx->nnz, 1);
  k_major_small_halpern<<<1, kMajorThreads, lds, ctx->stream>>>(A);
  HIP_TRY(hipGetLastError());
  return 0;
}

// pdlpdev_run's branch: one launch runs the steps up to the target (a step never fails; the cap of a launch only bounds its length),
// both blocks come back through their pinned mirrors: one launch + one synchronisation per call
int resident_halpern_run(pdlpdev_ctx* ctx, int32_t target_steps)
{
  for (int guard = 0; guard < 1000; ++guard) {
    TRY(enqueue_resident_halpern(ctx, target_steps));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->stat_loop_syncs += 1;
    if (ctx->ctl_h->error != 0 || ctx->ctl_h->steps_taken >= target_steps) break;
  }
  ctx->ctl_h_current = true;
  return 0;
}
// pdlpdev_major_eval's branch: the evaluation of the average slots, results in scal_h[32..41)
int resident_halpern_eval(pdlpdev_ctx* ctx, int rc_rule_finite_bounds, int want_linf, double eps_rel_primal, double eps_rel_dual)
{
  TRY(enqueue_resident_halpern_eval(ctx, rc_rule_finite_bounds, want_linf, eps_rel_primal, eps_rel_dual, -1));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ctx->stat_loop_syncs += 1;
  return 0;
}
// pdlpdev_run_period's branch: the loop kernel, the evaluation right behind it (it runs only if the steps reached the target or raised
// the error), ONE synchronisation.  *evaluated = 1: scal_h[32..41) holds the evaluation of the period's last T(z^k).
int resident_halpern_period(pdlpdev_ctx* ctx, int32_t target_steps, int rc_rule_finite_bounds, int want_linf, double eps_rel_primal, double eps_rel_dual,
                            int32_t* evaluated)
{
  *evaluated = 0;
  TRY(enqueue_resident_halpern(ctx, target_steps));
  TRY(enqueue_resident_halpern_eval(ctx, rc_rule_finite_bounds, want_linf, eps_rel_primal, eps_rel_dual, target_steps));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ctx->stat_loop_syncs += 1;
  ctx->ctl_h_current = true;
  if (ctx->ctl_h->error == 0 && ctx->ctl_h->steps_taken >= target_steps) {
    *evaluated = ctx->scal_h[63] == 1.0 ? 1 : 0;
    return 0;
  }
  if (ctx->ctl_h->error != 0) return 0;  // (the caller's major iteration evaluates the present way and reports the error)
  return resident_halpern_run(ctx, target_steps);  // a launch that hit its cap: the rest of the period, no evaluation
}

// ---- K LPs in K workgroups: the launches of a Halpern small-LP batch (the batch object and its host code: kernels_resident.hip) ----------
int halpern_batch_launch_loop(hipStream_t s, int device, int tier, const HalpernResidentArgs* args, const int* list, int count)
{
  return for_resident_tier(
    tier,
    [&](auto I) {
      constexpr ResidentTier r = kResidentTiers[decltype(I)::value];
      return launch_resident_kernel(k_pdhg_resident_halpern_batch<r.T, r.Q, r.U>, I, device, s, count, args, list, 1 << 14);
    },
    [&] { return fail(-1, "resident Halpern batch: no tier %d", tier); });
}
int halpern_batch_launch_eval(hipStream_t s, int device, size_t lds, const MajorSmallArgs* args, const int* list, int count)
{
  TRY(allow_dynamic_lds((const void*)k_major_small_halpern_batch, device, 8192 * 8));
  k_major_small_halpern_batch<<<count, kMajorThreads, lds, s>>>(args, list);
  HIP_TRY(hipGetLastError());
  return 0;
}
int halpern_batch_launch_restart_finish(hipStream_t s, const HalpernRestartArgs* args, const int* list, int count)
{
  k_halpern_restart_finish_batch<<<count, kBlock, 0, s>>>(args, list);
  HIP_TRY(hipGetLastError());
  return 0;
}
