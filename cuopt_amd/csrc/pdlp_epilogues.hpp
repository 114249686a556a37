// Device-side pieces shared by the kernel translation units (kernels_stream / _panel / _jag / _pb / _dense .hip) and the core
// (pdlp_device.hip): the direct peer transport's device structs, the fused epilogues of the SpMV skeletons, the dense-segment view.
#pragma once
#include "pdlp_kernels.hpp"

using namespace pdlp;

namespace p2pdev {
struct Peers {
  char* base[16];
};
constexpr int kKinds = 3;  // exchanges per attempt: xbar slices, y' row blocks, step-size scalars
__device__ __forceinline__ bool active(const pdlpdev_ctl* ctl) { return ctl->error == 0 && ctl->steps_taken < ctl->target_steps; }

// What a PRODUCING kernel (primal step, dual step, packing of the step-size sums) needs to store its results straight into
// every rank's landing block and to raise this rank's flag there; lives in device memory (one per exchange), kernels take a
// pointer (null: no peer transport) and read the table with scalar loads.
struct Push {
  Peers P;
  int world, rank, kind;
  size_t dst_off, flag_off;  // bytes inside every rank's block: this rank's slot of the exchange / the flag area
  unsigned long long* epoch;
  // halo exchange through the peer stores (round 6): rank q needs the entries [lo[q], hi[q]) of this rank's share only -- what its rows
  // (kind 0: xbar) or columns (kind 1: y') reference, found at set-up (halo_setup); everything: [0, INT_MAX)
  int lo[16], hi[16];
  __device__ __forceinline__ double* slot(int q) const { return reinterpret_cast<double*>(P.base[q] + dst_off); }
  __device__ __forceinline__ bool wants(int q, int i) const { return q != rank && i >= lo[q] && i < hi[q]; }
};
// A producing kernel's store into a landing block: system scope = write-through, so that no cache write-back is needed before the
// flag goes up
__device__ __forceinline__ void put(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
// Called once per workgroup at the end of a producing kernel: ONE thread of the grid counts the exchange.  The flag itself is raised
// by the first workgroup of the NEXT kernel of the stream (raise, below): a kernel boundary is what guarantees that every store of
// the producer has landed, for nothing.  (Round 3 published from the producer's tail -- every thread waited for its own stores, the
// workgroup took a ticket, the last one raised the flags: at one rank that made k_primal 31.8 us instead of 13.)
__device__ __forceinline__ void count_exchange(const Push* T)
{
  if (blockIdx.x == 0 && threadIdx.x == 0) T->epoch[T->kind] = T->epoch[T->kind] + 1;
}
// first thread of the consuming kernel: this rank's flag of the exchange goes up in every rank's block
__device__ __forceinline__ void raise(const Push* T)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned long long e = T->epoch[T->kind];
  for (int q = 0; q < T->world; ++q) {
    unsigned long long* flag = reinterpret_cast<unsigned long long*>(T->P.base[q] + T->flag_off) + (size_t)T->kind * T->world + T->rank;
    __hip_atomic_store(flag, e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
// lane q waits for rank q's flag of exchange `kind` (relaxed polls), then ONE lane acquires for the workgroup; false when
// patience ran out (5 s: a peer died)
__device__ __forceinline__ bool wait_flags(const unsigned long long* flags, int world, int kind, const unsigned long long* epoch)
{
  bool ok = true;
  if ((int)threadIdx.x < world) {
    const unsigned long long want = epoch[kind];
    const unsigned long long* f   = flags + (size_t)kind * world + threadIdx.x;
    const unsigned long long t0   = wall_clock64();
    while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < want) {
      __builtin_amdgcn_s_sleep(8);
      if (wall_clock64() - t0 > 500000000ull) {  // 100 MHz
        ok = false;
        break;
      }
    }
  }
  ok = __syncthreads_and(ok);
  if (threadIdx.x == 0) __threadfence_system();
  __syncthreads();
  return ok;
}
}  // namespace p2pdev

// ---- the fused epilogues ---------------------------------------------------------------------------------------------------------
// A product's HEAD -- which buffer of a ping-pong pair is the current iterate and which the next, which scalars of the control block
// the epilogue carries -- is written once, in the `make` next to the epilogue's fields; the product's kernel in each layout
// (kernels_stream / _halpern / _panel / _jag / _pb .hip) calls it with its own pointers.  The kernels keep their guard
// (loop_active, period_guard_skips), the choice of the vector their walker gathers, and the walker's call.

// (2) rows of A: v = A xbar (stream SpMV) -> dual projection (utils.cuh:97-112) -> ||dy||^2 partial,
//     plus the deferred dual averaging.
struct DualEpilogue {
  static constexpr int NQ = 1;
  using Op = SumOp;
  const double* __restrict__ y;
  double* __restrict__ yn;
  const double* __restrict__ lo;
  const double* __restrict__ hi;
  double* __restrict__ sumy;
  double sigma, weight;
  bool pend;
  double* __restrict__ copy = nullptr;  // sharded solves, owner-computes dataflow: y' also goes to this rank's slot of the gathered dual
  const p2pdev::Push* __restrict__ push = nullptr;  // ... or, with the direct peer transport, into every rank's landing block
  // the row's operands, separable from the arithmetic so that a layout can request them before its row sums are ready
  struct Ops {
    double y, lo, hi, sum;
  };
  __device__ __forceinline__ Ops load(int i) const { return Ops{y[i], lo[i], hi[i], pend ? sumy[i] : 0.0}; }
  __device__ __forceinline__ void apply(int i, double v, const Ops& o, double (&acc)[1])
  {
    const double yi = o.y;
    double next     = yi - (sigma * v);
    const double low = next + sigma * o.lo;
    const double up  = next + sigma * o.hi;
    next            = dmax(low, dmin(up, 0.0));
    yn[i]           = next;
    if (copy) copy[i] = next;
    if (push)
      for (int q = 0; q < push->world; ++q)
        if (push->wants(q, i)) p2pdev::put(push->slot(q) + i, next);  // (this rank's own rows: `copy`, an ordinary store)
    const double dy = next - yi;
    acc[0] += dy * dy;
    if (pend) sumy[i] = o.sum + weight * yi;
  }
  __device__ __forceinline__ void row(int i, double v, double (&acc)[1]) { apply(i, v, load(i), acc); }
  static __device__ __forceinline__ DualEpilogue make(const pdlpdev_ctl* ctl, double* y0, double* y1, const double* lo, const double* hi,
                                                      double* sumy, double* ycopy, const p2pdev::Push* push)
  {
    const int cur = ctl->cur;
    return DualEpilogue{cur ? y1 : y0, cur ? y0 : y1, lo, hi, sumy, ctl->sigma, ctl->step_size, ctl->pending_avg != 0, ycopy, push};
  }
};

// (3) rows of A^T: AtY' = A^T y' (stream SpMV) fused with the step-size statistics
//     interaction = dx . (AtY' - AtY), ||dx||^2  (adaptive_step_size_strategy.cu:278-340)
struct StepEpilogue {
  static constexpr int NQ = 2;
  using Op = SumOp;
  const double* __restrict__ x;
  const double* __restrict__ xn;
  const double* __restrict__ aty;
  double* __restrict__ atyn;
  struct Ops {
    double x, xn, aty;
  };
  __device__ __forceinline__ Ops load(int j) const { return Ops{x[j], xn[j], aty[j]}; }
  __device__ __forceinline__ void apply(int j, double v, const Ops& o, double (&acc)[2])
  {
    atyn[j]         = v;
    const double dx = o.xn - o.x;
    const double t  = v - o.aty;
    acc[0] += t * dx;
    acc[1] += dx * dx;
  }
  __device__ __forceinline__ void row(int j, double v, double (&acc)[2]) { apply(j, v, load(j), acc); }
  static __device__ __forceinline__ StepEpilogue make(const pdlpdev_ctl* ctl, const double* x0, const double* x1, double* aty0, double* aty1)
  {
    const int cur = ctl->cur;
    return StepEpilogue{cur ? x1 : x0, cur ? x0 : x1, cur ? aty1 : aty0, cur ? aty0 : aty1};
  }
};

// ---- restarted reflected-Halpern mode (docs/design/04d_halpern_mode.md): the same two products, the epilogues carry the combination
//      z^{k+1} = w (2 T(z^k) - z^k) + (1 - w) z^0.  Every added access is one coalesced 8-byte stream per row next to the ones
//      above (no LDS, nothing gathered).
struct HalpernWeights {
  double w, w0;  // w_k = (k + 1) / (k + 2) and 1 - w_k
  __device__ __forceinline__ explicit HalpernWeights(const pdlpdev_halpern* hal)
  {
    const double k = (double)hal->k;
    w              = (k + 1.0) / (k + 2.0);
    w0             = 1.0 - w;
  }
  __device__ __forceinline__ double combine(double t, double z, double z0) const { return w * (2.0 * t - z) + w0 * z0; }
};
// what the kernels of a Halpern step take besides their twins' arguments (by value: a handful of pointers)
struct HalpernArgs {
  const pdlpdev_halpern* __restrict__ hal;
  double* __restrict__ tx;          // T(z^k), primal half (the AVERAGE slot)
  double* __restrict__ ty;          // T(z^k), dual half: what the A^T product gathers
  const double* __restrict__ x0;    // the anchor
  const double* __restrict__ y0;
  const double* __restrict__ aty0;
};
// x' is kept on the last step of a run only (the evaluation behind it reads it; every other step would store 8 n bytes for nobody)
__device__ __forceinline__ bool halpern_last_step(const pdlpdev_ctl* ctl) { return ctl->steps_taken + 1 >= ctl->target_steps; }
// (2h) rows of A: y' as in DualEpilogue -> yp (the vector the A^T product gathers, and the dual half of T(z^k)), ||dy||^2 partial,
//      y^{k+1} -> yn
struct HalpernDualEpilogue {
  static constexpr int NQ = 1;
  using Op = SumOp;
  const double* __restrict__ y;
  double* __restrict__ yn;
  double* __restrict__ yp;
  const double* __restrict__ y0;
  const double* __restrict__ lo;
  const double* __restrict__ hi;
  double sigma;
  HalpernWeights hw;
  // the row's operands (as in DualEpilogue: a layout may request them before its row sums are ready)
  struct Ops {
    double y, lo, hi, y0;
  };
  __device__ __forceinline__ Ops load(int i) const { return Ops{y[i], lo[i], hi[i], y0[i]}; }
  __device__ __forceinline__ void apply(int i, double v, const Ops& o, double (&acc)[1])
  {
    const double yi  = o.y;
    double next      = yi - (sigma * v);
    const double low = next + sigma * o.lo;
    const double up  = next + sigma * o.hi;
    next             = dmax(low, dmin(up, 0.0));
    yp[i]            = next;
    const double dy  = next - yi;
    acc[0] += dy * dy;
    yn[i] = hw.combine(next, yi, o.y0);
  }
  // (row() keeps its own wording -- y0[i] read behind the store to yp[i] -- so that the layouts that call it compile to the
  // instructions they had: written as apply(load()) it moved 30 to 170 instructions in each of their Halpern kernels)
  __device__ __forceinline__ void row(int i, double v, double (&acc)[1])
  {
    const double yi  = y[i];
    double next      = yi - (sigma * v);
    const double low = next + sigma * lo[i];
    const double up  = next + sigma * hi[i];
    next             = dmax(low, dmin(up, 0.0));
    yp[i]            = next;
    const double dy  = next - yi;
    acc[0] += dy * dy;
    yn[i] = hw.combine(next, yi, y0[i]);
  }
  static __device__ __forceinline__ HalpernDualEpilogue make(const pdlpdev_ctl* ctl, double* y0, double* y1, const double* lo, const double* hi,
                                                             const HalpernArgs& h)
  {
    const int cur = ctl->cur;
    return HalpernDualEpilogue{cur ? y1 : y0, cur ? y0 : y1, h.ty, h.y0, lo, hi, ctl->sigma, HalpernWeights(h.hal)};
  }
};
// (2hs) the same on a rank of a sharded solve, owner-computes dataflow (cuoptamd_settings::halpern_sharded): y' of the rank's rows also
//       goes to this rank's slot of the gathered dual (copy), which the column block's A^T product gathers, and -- direct peer
//       transport -- into every other rank's landing block (push), as DualEpilogue's copy / push do.  One more coalesced 8-byte
//       stream per row; no LDS.  An epilogue of its own: HalpernDualEpilogue and the kernels built on it keep their instructions.
struct HalpernShardedDualEpilogue {
  static constexpr int NQ = 1;
  using Op = SumOp;
  const double* __restrict__ y;
  double* __restrict__ yn;
  double* __restrict__ yp;
  const double* __restrict__ y0;
  const double* __restrict__ lo;
  const double* __restrict__ hi;
  double sigma;
  HalpernWeights hw;
  double* __restrict__ copy;
  const p2pdev::Push* __restrict__ push;
  struct Ops {
    double y, lo, hi, y0;
  };
  __device__ __forceinline__ Ops load(int i) const { return Ops{y[i], lo[i], hi[i], y0[i]}; }
  __device__ __forceinline__ void apply(int i, double v, const Ops& o, double (&acc)[1])
  {
    const double yi  = o.y;
    double next      = yi - (sigma * v);
    const double low = next + sigma * o.lo;
    const double up  = next + sigma * o.hi;
    next             = dmax(low, dmin(up, 0.0));
    yp[i]            = next;
    copy[i]          = next;
    if (push)
      for (int q = 0; q < push->world; ++q)
        if (push->wants(q, i)) p2pdev::put(push->slot(q) + i, next);
    const double dy = next - yi;
    acc[0] += dy * dy;
    yn[i] = hw.combine(next, yi, o.y0);
  }
  __device__ __forceinline__ void row(int i, double v, double (&acc)[1]) { apply(i, v, load(i), acc); }
  static __device__ __forceinline__ HalpernShardedDualEpilogue make(const pdlpdev_ctl* ctl, double* y0, double* y1, const double* lo, const double* hi,
                                                                    const HalpernArgs& h, double* ycopy, const p2pdev::Push* push)
  {
    const int cur = ctl->cur;
    return HalpernShardedDualEpilogue{cur ? y1 : y0, cur ? y0 : y1, h.ty, h.y0, lo, hi, ctl->sigma, HalpernWeights(h.hal), ycopy, push};
  }
};
// (3h) rows of A^T: v = A^T y' with StepEpilogue's two sums (dx . (A^T y' - A^T y^k) = dy . A dx, ||dx||^2), then x^{k+1} over x'
//      (read and written by the same lane) and A^T y^{k+1} by the same linear combination; xp (null except on the last step of a
//      run): x', the primal half of T(z^k), survives there
struct HalpernStepEpilogue {
  static constexpr int NQ = 2;
  using Op = SumOp;
  const double* __restrict__ x;
  double* __restrict__ xn;
  const double* __restrict__ aty;
  double* __restrict__ atyn;
  const double* __restrict__ x0;
  const double* __restrict__ aty0;
  double* __restrict__ xp;
  HalpernWeights hw;
  // the row's operands (xn[j] is x', read here and overwritten in apply by the same lane)
  struct Ops {
    double x, xn, aty, x0, aty0;
  };
  __device__ __forceinline__ Ops load(int j) const { return Ops{x[j], xn[j], aty[j], x0[j], aty0[j]}; }
  __device__ __forceinline__ void apply(int j, double v, const Ops& o, double (&acc)[2])
  {
    const double xj = o.x, xt = o.xn, a = o.aty;
    const double dx = xt - xj;
    const double t  = v - a;
    acc[0] += t * dx;
    acc[1] += dx * dx;
    if (xp) xp[j] = xt;
    xn[j]   = hw.combine(xt, xj, o.x0);
    atyn[j] = hw.combine(v, a, o.aty0);
  }
  // (row() in its own wording, as in HalpernDualEpilogue: x0[j] and aty0[j] read where they are used)
  __device__ __forceinline__ void row(int j, double v, double (&acc)[2])
  {
    const double xj = x[j], xt = xn[j], a = aty[j];
    const double dx = xt - xj;
    const double t  = v - a;
    acc[0] += t * dx;
    acc[1] += dx * dx;
    if (xp) xp[j] = xt;
    xn[j]   = hw.combine(xt, xj, x0[j]);
    atyn[j] = hw.combine(v, a, aty0[j]);
  }
  static __device__ __forceinline__ HalpernStepEpilogue make(const pdlpdev_ctl* ctl, double* x0, double* x1, double* aty0, double* aty1,
                                                             const HalpernArgs& h)
  {
    const int cur = ctl->cur;
    return HalpernStepEpilogue{cur ? x1 : x0, cur ? x0 : x1, cur ? aty1 : aty0, cur ? aty0 : aty1, h.x0, h.aty0,
                               halpern_last_step(ctl) ? h.tx : nullptr, HalpernWeights(h.hal)};
  }
};

// (plain SpMV: A^T y at start / after restart-to-average; parity hook; multi-GPU partial products)
struct StoreEpilogue {
  static constexpr int NQ = 0;
  using Op = SumOp;
  double* __restrict__ out;
  __device__ __forceinline__ void row(int r, double v, double (&)[1]) { out[r] = v; }
  // A^T y of the iterate on side `side` of the ping-pong pairs (ctl->cur: the current one, flipped: the trial iterate) into that
  // side's buffer, or into `out_override`; the kernel gathers the same side of y
  static __device__ __forceinline__ StoreEpilogue iterate(int side, double* aty0, double* aty1, double* out_override)
  {
    return StoreEpilogue{out_override ? out_override : (side ? aty1 : aty0)};
  }
};

// The iterate an evaluation looks at: the running average, or the current side of a ping-pong pair (x and y alike).  It also picks
// the current side of a pair that has no average, the A^T y buffers of k_panel_eval_dual_from_aty: `which` is PDLPDEV_CURRENT there
// and `avg` null, never read.
__device__ __forceinline__ const double* evaluated(int cur, int which, const double* v0, const double* v1, const double* avg)
{
  return which == PDLPDEV_AVERAGE ? avg : (cur ? v1 : v0);
}

// Convergence information, primal side (convergence_information.cu:221-248 + row part of :323-366):
// rows of the SCALED A against the SCALED iterate; (A x)_i = (A^ x^)_i / D_r,i and y_i = y^_i D_r,i
// recover the unscaled quantities without a second copy of the matrix.
struct EvalPrimalEpilogue {
  static constexpr int NQ = 3;
  using Op = SumOp;
  const double* __restrict__ yhat;
  const double* __restrict__ dr;
  const double* __restrict__ lo_u;
  const double* __restrict__ hi_u;
  double eps_rel;
  double* __restrict__ linf_rows;  // per-row r_p,i - eps*bcomb_i (max-reduced by a second pass)
  double* __restrict__ ax_out;     // (A x)_i of the unscaled problem, kept for the infeasibility pass
  __device__ __forceinline__ void row(int i, double v, double (&acc)[3])
  {
    const double d  = dr[i];
    const double ax = v / d;
    ax_out[i]       = ax;
    const double yi = yhat[i] * d;
    const double lo = lo_u[i], hi = hi_u[i];
    const double rp = violation(ax, lo, hi);
    acc[0] += rp * rp;
    acc[1] += bound_value_product(yi, lo, hi);
    acc[2] += yi * yi;
    if (linf_rows) linf_rows[i] = rp - eps_rel * combine_bounds(lo, hi);  // relative_residual_t, utils.cuh:385-409
  }
};

// dual side (convergence_information.cu:261-320,369-422): one column j per lane
struct EvalDualCore {
  const double* __restrict__ xhat;
  const double* __restrict__ dc;
  const double* __restrict__ c_u;
  const double* __restrict__ lb_u;
  const double* __restrict__ ub_u;
  double eps_rel;
  int rule_finite;
  double* __restrict__ rc_out;
  double* __restrict__ linf_rows;
  double* __restrict__ aty_out;  // (A^T y)_j of the unscaled problem, kept for the infeasibility pass
  // acc: 0 ||r_d||^2, 1 sum B(rc,lb,ub), 2 c.x, 3 ||x||^2
  __device__ __forceinline__ void col(int j, double aty_scaled, double (&acc)[4])
  {
    const double d    = dc[j];
    const double aty  = aty_scaled / d;
    aty_out[j]        = aty;
    const double cj   = c_u[j];
    const double g    = cj - aty;
    const double xj   = xhat[j] * d;
    const double lb   = lb_u[j], ub = ub_u[j];
    const double bv   = g > 0.0 ? lb : ub;  // bound_value_gradient, utils.cuh:195-202
    double rc;
    if (g == 0.0)
      rc = g;
    else if (rule_finite)  // copy_gradient_if_finite_bounds, utils.cuh:231-239
      rc = dfinite(bv) ? g : 0.0;
    else  // copy_gradient_if_should_be_reduced_cost, utils.cuh:221-229
      rc = fabs(xj - bv) <= fabs(xj) ? g : 0.0;
    const double rd = g - rc;
    rc_out[j]       = rc;
    acc[0] += rd * rd;
    acc[1] += bound_value_product(rc, lb, ub);
    acc[2] += cj * xj;
    acc[3] += xj * xj;
    if (linf_rows) linf_rows[j] = rd - eps_rel * cj;  // the dual "rhs" is c_j itself (signed), :204-208
  }
};

struct EvalDualEpilogue {
  static constexpr int NQ = 4;
  using Op = SumOp;
  EvalDualCore core;
  __device__ __forceinline__ void row(int j, double v, double (&acc)[4]) { core.col(j, v, acc); }
};

// Infeasibility detection in reflected Halpern mode, the one-workgroup evaluation (kernels_resident_halpern.hip): the statistics of
// k_halpern_ray_rows / k_halpern_ray_cols (pdlp_eval.hip) as epilogues of the two products formed from the scaled displacement
// T(z^k) - z^k.  t: T(z^k) (the average slot), zk: z^k.  Maxima and sums share one accumulator array; the caller reduces them apart.
struct RayRowsEpilogue {
  static constexpr int NQ = 3;
  const double* __restrict__ t;
  const double* __restrict__ zk;
  const double* __restrict__ dr;
  const double* __restrict__ lo_u;
  const double* __restrict__ hi_u;
  // acc: 0 max homogeneous primal residual, 1 ||dy||_inf, 2 sum B(dy, lo, hi)
  __device__ __forceinline__ void row(int i, double v, double (&acc)[3])
  {
    const double d  = dr[i];
    const double lo = lo_u[i], hi = hi_u[i];
    const double hl = dfinite(lo) ? 0.0 : lo, hu = dfinite(hi) ? 0.0 : hi;  // zero_if_is_finite
    const double r  = fabs(violation(v / d, hl, hu));
    const double yi = (t[i] - zk[i]) * d;
    acc[0] = r > acc[0] ? r : acc[0];
    acc[1] = fabs(yi) > acc[1] ? fabs(yi) : acc[1];
    acc[2] += bound_value_product(yi, lo, hi);
  }
};
struct RayColsEpilogue {
  static constexpr int NQ = 6;
  const double* __restrict__ t;
  const double* __restrict__ zk;
  const double* __restrict__ dc;
  const double* __restrict__ c_u;
  const double* __restrict__ lb_u;
  const double* __restrict__ ub_u;
  int rule_finite;
  // acc: 0 max homogeneous dual residual, 1 ||rc||_inf, 2 ||dx||_inf, 3 max bound violation, 4 sum B(rc, lb, ub), 5 c . dx
  __device__ __forceinline__ void row(int j, double v, double (&acc)[6])
  {
    const double d  = dc[j];
    const double g  = -1.0 * (v / d);
    const double xj = (t[j] - zk[j]) * d;
    const double lb = lb_u[j], ub = ub_u[j];
    const double bv = g > 0.0 ? lb : ub;
    double rc;
    if (g == 0.0)
      rc = g;
    else if (rule_finite)
      rc = dfinite(bv) ? g : 0.0;
    else
      rc = fabs(xj - bv) <= fabs(xj) ? g : 0.0;
    const double rd = fabs(g - rc);
    double viol     = 0.0;
    if (dfinite(lb)) viol = dmax(viol, -xj);
    if (dfinite(ub)) viol = dmax(viol, xj);
    acc[0] = rd > acc[0] ? rd : acc[0];
    acc[1] = fabs(rc) > acc[1] ? fabs(rc) : acc[1];
    acc[2] = fabs(xj) > acc[2] ? fabs(xj) : acc[2];
    acc[3] = viol > acc[3] ? viol : acc[3];
    acc[4] += bound_value_product(rc, lb, ub);
    acc[5] += c_u[j] * xj;
  }
};

// ---- dense row segments: index-free storage (pdlpdev_ctx::Dense) ---------------------------------------------------------
struct DenseView {
  const int32_t* __restrict__ row;
  const int32_t* __restrict__ row_seg;
  const int32_t* __restrict__ seg_row;
  const int32_t* __restrict__ seg_c0;
  const int32_t* __restrict__ seg_len;
  const int32_t* __restrict__ seg_ptr;
  const int32_t* __restrict__ tile_ptr;
  const int32_t* __restrict__ tile_seg;
  const int32_t* __restrict__ tile_id;  // the 256-column tiles some segment overlaps
  const double* __restrict__ val;
  const int32_t* __restrict__ ch_seg;   // chunks of <= kDenseChunk entries of a segment: one workgroup each ...
  const int32_t* __restrict__ ch_k0;
  const int32_t* __restrict__ row_ch;   // ... and per owning row its chunk range (added up in this order)
  double* __restrict__ ch_part;
};

constexpr int kDenseChunk = 4096;

// Which vector a product gathers, where a kernel is told so by its `mode` argument and picks it on the device (phase P of the
// gather-free layout, the dense segments' kernels).  ONE encoding for the host (Gathered, pdlp_launch.hpp) and the device; the values
// are those the kernels have always been launched with.
enum GatherMode : int {
  kGatherFixed   = 0,  // v0, as it is
  kGatherTrial   = 1,  // of the ping-pong pair (v0, v1) the trial iterate, which the step in flight wrote: cur ? v0 : v1
  kGatherCurrent = 2,  // ... the current iterate: cur ? v1 : v0
};
static_assert(kGatherFixed == 0 && kGatherTrial == 1 && kGatherCurrent == 2, "the values of the kernels' `mode` argument");
__device__ __forceinline__ const double* pick_vector(const pdlpdev_ctl* ctl, const double* v0, const double* v1, int mode)
{
  if (mode == kGatherFixed) return v0;
  const bool cur = ctl->cur != 0;
  return (cur == (mode == kGatherTrial)) ? v0 : v1;
}
