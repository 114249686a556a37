// The three one-workgroup bodies of the reflected-Halpern mode on the resident small-LP path: the loop (resident_halpern_body), the
// evaluation of T(z^k) (major_small_halpern_body) and the finish of a restart (halpern_restart_finish_workgroup).  In a header since
// kernels_halpern_major.hip wraps all three in kernels of its own (the burst of device-decided major iterations,
// cuoptamd_settings::halpern_device_major); kernels_resident_halpern.hip instantiates the first two exactly as while they stood there.
#pragma once
#include "pdlp_ctx.hpp"
#include "pdlp_layouts.hpp"
#include "resident_common.hpp"
#include "halpern_decision.hpp"

// p, which points to global memory, as a pointer the compiler knows that of (the empty statement keeps the two casts from cancelling
// and names a scalar register: the value is uniform)
template <class P>
__device__ __forceinline__ P* as_global(P* p)
{
  __attribute__((address_space(1))) P* g = (__attribute__((address_space(1))) P*)p;
  asm("" : "+s"(g));
  return (P*)g;
}

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

// MajorSmallArgs::mode == 3, served by a kernel of its own: no average is formed and nothing is flushed; the average slots are
// evaluated as the loop left them (T(z^k) of the period's last step), results in sc[32..41) as k_major_small leaves the average's.
// KEEP IN STEP with major_small_body (kernels_resident.hip): what follows the guard is its `which == 1` pass, statement for
// statement (epilogues, reduction trees, slots of sc).  It is a copy and not a shared helper because both ways of sharing it were
// tried and both change k_major_small / k_major_small_batch: a mode-3 branch inside major_small_body, and a __forceinline__
// per-point helper called by both bodies (1206 lines of llvm-objdump -d of kernels_resident's gfx950 code object differ) -- and
// the existing kernels are to keep the instructions they had.  guard_target as in
// k_major_small_batch; sc[63] says whether the evaluation ran.  Guarded by
// tests/test_halpern_resident_steps_gpu.py::test_major_small_halpern_against_the_reference (this copy against tests/eval_reference.py,
// as tests/test_resident_attempts_gpu.py holds the original).
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

// The finish of the restart of ONE resident LP by one workgroup of kBlock threads, behind k_restart_batch's blocks: what
// pdlpdev_halpern_restart enqueues behind k_restart for one LP -- k_finalize's two sums (finalize_rows: the same tree) into dist2,
// k_copy_current of A^T y into the anchor's, halpern_restart_scalars with this LP's theta; the distances also go to dist_out, both blocks
// to their pinned mirrors.  A.clear != 0 (a reset): k_halpern_clear's values first.  red: 8 doubles of LDS.
__device__ __forceinline__ void halpern_restart_finish_workgroup(const HalpernRestartArgs& A, double* dist2, double* dist_out, double* red)
{
  const int cur = A.ctl->cur;  // (read by every thread in front of finalize_rows' barriers; thread 0 rewrites the block behind them)
  finalize_rows(A.part, A.g, 2, 0u, dist2, red);
  const double* __restrict__ v = cur ? A.aty1 : A.aty0;
  for (int i = threadIdx.x; i < A.n; i += kBlock) A.lraty[i] = v[i];
  if (threadIdx.x != 0) return;
  pdlpdev_halpern* hal = A.hal;
  if (A.clear) {  // k_halpern_clear
    hal->r = hal->r_first = hal->r2 = 0.0;
    hal->r2_min = __builtin_huge_val();
    hal->k = 0, hal->reserved = 0;
  }
  double d[2] = {dist2[0], dist2[1]};  // (in registers: a store to the blocks may alias dist2, and each reload behind one is a round trip)
  halpern_restart_scalars(A.ctl, hal, d, A.theta);
  dist2[0] = dist_out[0] = d[0], dist2[1] = dist_out[1] = d[1];
  *A.ctl_host = *A.ctl, *A.hal_host = *hal;
}
