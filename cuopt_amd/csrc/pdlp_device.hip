#include "pdlp_ctx.hpp"
#include "pdlp_layouts.hpp"
#include "pdlp_setup.hpp"
#include "halpern_decision.hpp"


// ================================================================================================
// kernels: element-wise helpers of the set-up (the scaling kernels live in pdlp_scaling.hip)
// ================================================================================================
__global__ void __launch_bounds__(kBlock) k_fill(int64_t n, double* __restrict__ d, double v)
{
  for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    d[i] = v;
}
__global__ void __launch_bounds__(kBlock) k_scale_vectors(int n, int m, double* __restrict__ c,
                                                          double* __restrict__ lb,
                                                          double* __restrict__ ub,
                                                          const double* __restrict__ dc,
                                                          double* __restrict__ lo,
                                                          double* __restrict__ hi,
                                                          const double* __restrict__ dr)
{
  const int tot = n > m ? n : m;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < tot; i += gridDim.x * kBlock) {
    if (i < n) {
      c[i]  = c[i] * dc[i];
      lb[i] = lb[i] / dc[i];
      ub[i] = ub[i] / dc[i];
    }
    if (i < m) {
      lo[i] = lo[i] * dr[i];
      hi[i] = hi[i] * dr[i];
    }
  }
}
// the bound part of k_scale_vectors alone (pdlpdev_reset): same expressions, so a re-solve with new bounds is
// bit-identical to a fresh solver; NULL = that vector is unchanged
__global__ void __launch_bounds__(kBlock) k_scale_bounds(int n, int m, double* lb, double* ub,
                                                         const double* __restrict__ dc, double* lo, double* hi,
                                                         const double* __restrict__ dr)
{
  const int tot = n > m ? n : m;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < tot; i += gridDim.x * kBlock) {
    if (i < n) {
      if (lb) lb[i] = lb[i] / dc[i];
      if (ub) ub[i] = ub[i] / dc[i];
    }
    if (i < m) {
      if (lo) lo[i] = lo[i] * dr[i];
      if (hi) hi[i] = hi[i] * dr[i];
    }
  }
}
__global__ void __launch_bounds__(kBlock) k_div_inplace(int n, double* __restrict__ v,
                                                        const double* __restrict__ d)
{
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) v[i] = v[i] / d[i];
}
__global__ void __launch_bounds__(kBlock) k_div_to(int n, double* __restrict__ out, const double* __restrict__ v,
                                                   const double* __restrict__ d)
{
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) out[i] = v[i] / d[i];
}
__global__ void __launch_bounds__(kBlock) k_clamp(int n, double* __restrict__ x,
                                                  const double* __restrict__ lb,
                                                  const double* __restrict__ ub)
{
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
    x[i] = dmin(dmax(x[i], lb[i]), ub[i]);  // clamp, utils.cuh:131-137
}

// generic grid-stride reductions -> part[q * gridDim + block]
// mode 0: max |v| ; 1: sum v^2 ; 2: sum combine_bounds(a,b)^2 ; 3: sum (a-b)^2
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_reduce(int64_t n, const double* __restrict__ a,
                                                   const double* __restrict__ b,
                                                   double* __restrict__ part)
{
  __shared__ double red[8];
  double acc[1] = {0.0};
  for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    if (MODE == 0) {
      const double v = fabs(a[i]);
      acc[0] = v > acc[0] ? v : acc[0];
    } else if (MODE == 1) {
      acc[0] += a[i] * a[i];
    } else if (MODE == 2) {
      const double v = combine_bounds(a[i], b[i]);
      acc[0] += v * v;
    } else {
      const double v = a[i] - b[i];
      acc[0] += v * v;
    }
  }
  if (MODE == 0)
    block_reduce<MaxOp, 1>(acc, red);
  else
    block_reduce<SumOp, 1>(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
}
__global__ void __launch_bounds__(kBlock) k_dot(int64_t n, const double* __restrict__ a, const double* __restrict__ b,
                                                double* __restrict__ part)
{
  __shared__ double red[8];
  double acc[1] = {0.0};
  for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) acc[0] += a[i] * b[i];
  block_reduce<SumOp, 1>(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
}
// out[q] = reduce(part[q*nb .. q*nb+nb)) ; op_mask bit q set => max
__global__ void __launch_bounds__(kBlock) k_finalize(const double* __restrict__ part, int nb, int nq,
                                                     unsigned op_mask, double* __restrict__ out)
{
  __shared__ double red[8];
  finalize_rows(part, nb, nq, op_mask, out, red);
}

// ================================================================================================
// kernels: the PDHG attempt (4 launches, no host interaction)
// ================================================================================================
// (1) primal projection + extrapolation (primal_projection functor, utils.cuh:80-95) fused with the
//     deferred averaging of the previously accepted iterate (weighted_average_solution.cu:73-108).
// primal_body<false> is k_primal as it was, argument list included; <true> (k_primal_zs) also writes the bitmap of xbar's non-zeros and
// counts them.
// One column of the step: the projected x' into xn, the extrapolated xbar (returned) and, ZS, the wave's ballot of its non-zeros.
// (xmask: one bit per column, set where xbar is not 0.0 -- what the panels of A need to skip the gathers of zeros.  A wave's 64
//  columns are consecutive and start at a multiple of 64, so its ballot is one whole word of the bitmap; lanes beyond n are not in the
//  call and count as zeros.  -0.0 compares equal to 0.0: clear; NaN and infinities: set.  nz: the set bits the wave has seen.)
template <bool ZS>
__device__ __forceinline__ double primal_column(int j, double xj, double cj, double atyj, double lbj, double ubj, double tau, double* __restrict__ xn,
                                                double* __restrict__ xbar, unsigned long long* __restrict__ xmask, int& nz)
{
  const double gradient = cj - atyj;
  double next           = xj - (tau * gradient);
  next                  = dmax(dmin(next, ubj), lbj);
  xn[j]                 = next;
  const double xb       = next - xj + next;
  xbar[j]               = xb;
  if constexpr (ZS) {
    const unsigned long long bits = __ballot(xb != 0.0);
    if ((threadIdx.x & 63) == 0) xmask[j >> 6] = bits;
    nz += __popcll(bits);
  }
  return xb;
}
// zcount, with xmask: the set bits per workgroup of WAVES waves, an exact integer that the decision adds up for the density guard
// (lane 0 of a wave is in every call its wave makes, so its count is the wave's)
template <int WAVES>
__device__ __forceinline__ void primal_store_zcount(int nz, int* __restrict__ zcount)
{
  __shared__ int wave_nz[WAVES];
  if ((threadIdx.x & 63) == 0) wave_nz[threadIdx.x >> 6] = nz;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) sum += wave_nz[w];
    zcount[blockIdx.x] = sum;
  }
}
template <bool ZS>
__device__ __forceinline__ void
primal_body(int n, const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ x0, double* __restrict__ x1,
         const double* __restrict__ aty0, const double* __restrict__ aty1,
         const double* __restrict__ c, const double* __restrict__ lb, const double* __restrict__ ub,
         double* __restrict__ xbar, double* __restrict__ sumx, const p2pdev::Push* __restrict__ push, pdlpdev_ctx::UniformBounds ubd,
         unsigned long long* __restrict__ xmask, int* __restrict__ zcount)
{
  [[maybe_unused]] int nz = 0;
  // (ubd: every lower / upper bound is the same 0 or infinity -- x >= 0 is the usual LP -- so the bound arrays, 16 of the kernel's
  //  72 bytes per column, are not read at all; scaling keeps 0 and infinity what they are)
  if (!loop_active(ctl)) return;
  const int cur       = ctl->cur;
  const double tau    = ctl->tau;
  const double weight = ctl->step_size;
  const bool pend     = ctl->pending_avg != 0;
  const double* __restrict__ x   = cur ? x1 : x0;
  double* __restrict__ xn        = cur ? x0 : x1;
  const double* __restrict__ aty = cur ? aty1 : aty0;
  for (int j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
    const double xj = x[j];
    const double xb = primal_column<ZS>(j, xj, c[j], aty[j], ubd.lb_same ? ubd.lb : lb[j], ubd.ub_same ? ubd.ub : ub[j], tau, xn, xbar, xmask, nz);
    if (push)  // sharded solve, direct peer transport: this rank's slice of xbar lands in every OTHER rank's block (its own copy is
               // the ordinary store above: write-through stores cost 17 us per attempt at C3 and buy nothing at home)
      for (int q = 0; q < push->world; ++q)
        if (push->wants(q, j)) p2pdev::put(push->slot(q) + j, xb);
    if (pend) sumx[j] = sumx[j] + weight * xj;
  }
  if constexpr (ZS) primal_store_zcount<kBlock / 64>(nz, zcount);
  if (push) p2pdev::count_exchange(push);
}
__global__ void __launch_bounds__(kBlock)
k_primal(int n, const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ x0, double* __restrict__ x1,
         const double* __restrict__ aty0, const double* __restrict__ aty1,
         const double* __restrict__ c, const double* __restrict__ lb, const double* __restrict__ ub,
         double* __restrict__ xbar, double* __restrict__ sumx, const p2pdev::Push* __restrict__ push, pdlpdev_ctx::UniformBounds ubd)
{
  primal_body<false>(n, ctl, x0, x1, aty0, aty1, c, lb, ub, xbar, sumx, push, ubd, nullptr, nullptr);
}
__global__ void __launch_bounds__(kBlock)
k_primal_zs(int n, const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ x0, double* __restrict__ x1,
            const double* __restrict__ aty0, const double* __restrict__ aty1,
            const double* __restrict__ c, const double* __restrict__ lb, const double* __restrict__ ub,
            double* __restrict__ xbar, double* __restrict__ sumx, pdlpdev_ctx::UniformBounds ubd,
            unsigned long long* __restrict__ xmask, int* __restrict__ zcount)
{
  primal_body<true>(n, ctl, x0, x1, aty0, aty1, c, lb, ub, xbar, sumx, nullptr, ubd, xmask, zcount);
}



// multi-GPU variant of (3): after the all-reduce of the A^T y' partial products
__global__ void __launch_bounds__(kBlock)
k_step_stats(int n, int nbg, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ reduced,
             const double* __restrict__ x0, const double* __restrict__ x1, double* __restrict__ aty0,
             double* __restrict__ aty1, double* __restrict__ part)
{
  __shared__ double red[12];
  if (!loop_active(ctl)) return;
  const int cur = ctl->cur;
  const double* __restrict__ x   = cur ? x1 : x0;
  const double* __restrict__ xn  = cur ? x0 : x1;
  const double* __restrict__ aty = cur ? aty1 : aty0;
  double* __restrict__ atyn      = cur ? aty0 : aty1;
  double acc[2] = {0.0, 0.0};
  for (int j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
    const double v  = reduced[j];
    atyn[j]         = v;
    const double dx = xn[j] - x[j];
    const double t  = v - aty[j];
    acc[0] += t * dx;
    acc[1] += dx * dx;
  }
  block_reduce<SumOp, 2>(acc, red);
  if (threadIdx.x == 0) {
    part[blockIdx.x]       = acc[0];
    part[nbg + blockIdx.x] = acc[1];
  }
}

constexpr int kDecisionThreads = 1024;  // one wide workgroup: every partial is one independent load
static_assert(kDecisionThreads == kHalpernDecisionThreads, "k_halpern_decision runs halpern_decision_workgroup");
// Latency is all that matters here (one workgroup on the critical path of every attempt): the control block is
// read once into registers (uniform -> scalar loads) and written back once, the two pow() of the step-size rule
// are evaluated by the last wave while the others fetch partials, the sums use DPP lane permutes.
// ZS (k_step_decision_zs): the density guard of the zero skip rides along -- the non-zeros of xbar that k_primal's workgroups counted
// are added up as a fourth sum (integers below 2^31 as doubles: exact in any order) and set the flag the NEXT attempt's A product
// reads: up at 25 % zeros or more, down at 13 % or fewer (measured break-even on the 1e6 x 1e6 LP: docs/design/09_next.md item
// 9), unchanged in between; zmode 2 keeps it up.  The flag never changes a result, only which code path forms it.
//
// step_decision_form is the decision without its loads and stores of the control block: `lc` comes in as the block the attempt ran with
// (loop active) and leaves as the decided one -- in thread 0, or, EVERY, in every thread (the sums end in every lane, each thread then
// applies the rule to the same values: k_primal_decide, whose workgroups all go on with the decided block).
// step_decision_workgroup reads the block at `in` and stores the decided one at `out`.  in == out: the loop's own block, nothing is
// stored when the attempt was empty (the loop is not active).  in != out (the end of a chunk of attempts that went from scratch block
// to scratch block, enqueue_single_chunk): `out` always ends up current -- an empty attempt copies the block through.
// Each thread's FIRST partial of every sum is requested up front, then `ahead()` runs (k_primal_decide: its operand requests, which
// thereby stand BEHIND the partials in the order the loads return and are not waited for by the sums), then the sums are formed in the
// order they always were: thread t adds partials t, t + 1024, ... to 0.0.
template <bool ZS, bool EVERY, class Ahead>
__device__ __forceinline__ void step_decision_form(pdlpdev_ctl& lc, const double* __restrict__ part_dy, int nb_dy, const double* __restrict__ part_t, int nb_t,
                                                   const double* __restrict__ dy2_reduced, const pdlpdev_step_params& sp, const int* __restrict__ zcount,
                                                   int nb_z, int zn, int zmode, Ahead&& ahead)
{
  __shared__ double red[(ZS ? 4 : 3) * 16];
  __shared__ double pw[2];
  const int t = threadIdx.x;
  // (a thread beyond an array's end requests the last entry and leaves it unused: the requests stay one straight run of loads, which the
  //  compiler does not tie to the sums' conditions)
  const bool has_dy = dy2_reduced == nullptr && t < nb_dy, has_t = t < nb_t, has_z = ZS && t < nb_z;
  const int i_t = min(t, nb_t - 1);
  const double first_dy = dy2_reduced == nullptr && nb_dy > 0 ? part_dy[min(t, nb_dy - 1)] : 0.0;
  const double first_t0 = nb_t > 0 ? part_t[i_t] : 0.0, first_t1 = nb_t > 0 ? part_t[nb_t + i_t] : 0.0;
  [[maybe_unused]] int first_z = 0;
  if constexpr (ZS) first_z = nb_z > 0 ? zcount[min(t, nb_z - 1)] : 0;
  ahead();
  if (t >= kDecisionThreads - 2) {
    const double knext = (double)(lc.k + 1) + 1.0;
    pw[t - (kDecisionThreads - 2)] = pow(knext, t == kDecisionThreads - 2 ? -sp.reduction_exponent : -sp.growth_exponent);
  }
  // (the sums start from a zero the compiler cannot see through: it would otherwise form "0.0 + first" right behind each request, in
  //  front of ahead(), and wait for the partial there)
  double zero = 0.0;
  int izero   = 0;
  asm volatile("" : "+v"(zero), "+v"(izero));
  double acc[ZS ? 4 : 3] = {zero, zero, zero};
  if (dy2_reduced == nullptr) {
    if (has_dy) acc[0] += first_dy;
#pragma unroll 4
    for (int i = t + kDecisionThreads; i < nb_dy; i += kDecisionThreads) acc[0] += part_dy[i];
  }
  if (has_t) acc[1] += first_t0, acc[2] += first_t1;
#pragma unroll 4
  for (int i = t + kDecisionThreads; i < nb_t; i += kDecisionThreads) {
    acc[1] += part_t[i];
    acc[2] += part_t[nb_t + i];
  }
  if constexpr (ZS) {
    acc[3] = zero;
    if (has_z) acc[3] += (double)(first_z + izero);
#pragma unroll 2
    for (int i = t + kDecisionThreads; i < nb_z; i += kDecisionThreads) acc[3] += (double)zcount[i];
  }
  block_sum_fast<ZS ? 4 : 3, kDecisionThreads / 64>(acc, red);
  if (!EVERY && t != 0) return;
  apply_step_decision(&lc, dy2_reduced ? dy2_reduced[0] : acc[0], acc[1], acc[2], sp, pw);
  if constexpr (ZS) {
    const long long nonzeros = (long long)acc[3];
    lc.zs_nonzeros           = (int32_t)nonzeros;
    if (zmode == 2 || nonzeros * 4 <= 3ll * zn) lc.zskip = 1;
    else if (nonzeros * 100 >= 87ll * zn) lc.zskip = 0;
  }
}
// one thread's store of a control block
template <bool ZS>
__device__ __forceinline__ void store_ctl(pdlpdev_ctl* out, const pdlpdev_ctl& lc)
{
  if constexpr (ZS) {
    *out = lc;
  } else {
    // (the decision without the guard neither reads nor writes the guard's two fields at the block's end: the loads and stores of this
    //  latency-bound kernel are the ones it had before the block grew)
    __builtin_memcpy(out, &lc, offsetof(pdlpdev_ctl, zskip));
  }
}
template <bool ZS = false>
__device__ __forceinline__ void step_decision_workgroup(const pdlpdev_ctl* in, pdlpdev_ctl* out, const double* __restrict__ part_dy, int nb_dy,
                                                        const double* __restrict__ part_t, int nb_t, const double* __restrict__ dy2_reduced,
                                                        const pdlpdev_step_params& sp, const int* __restrict__ zcount = nullptr, int nb_z = 0,
                                                        int zn = 0, int zmode = 0)
{
  pdlpdev_ctl lc = *in;
  if (!(lc.error == 0 && lc.steps_taken < lc.target_steps)) {
    if (in != out && threadIdx.x == 0) store_ctl<ZS>(out, lc);
    return;
  }
  step_decision_form<ZS, false>(lc, part_dy, nb_dy, part_t, nb_t, dy2_reduced, sp, zcount, nb_z, zn, zmode, [] {});
  if (threadIdx.x == 0) store_ctl<ZS>(out, lc);
}
// (in: the block the attempt ran with; out: where the decided one goes -- the same block everywhere but at the end of a chunk)
__global__ void __launch_bounds__(kDecisionThreads)
k_step_decision(const pdlpdev_ctl* in, pdlpdev_ctl* out, const double* __restrict__ part_dy, int nb_dy,
                const double* __restrict__ part_t, int nb_t, const double* __restrict__ dy2_reduced,
                pdlpdev_step_params sp)
{
  step_decision_workgroup(in, out, part_dy, nb_dy, part_t, nb_t, dy2_reduced, sp);
}
// (single GPU, averaging modes, with the bitmap of xbar in use: attempt_xmask)
__global__ void __launch_bounds__(kDecisionThreads)
k_step_decision_zs(const pdlpdev_ctl* in, pdlpdev_ctl* out, const double* __restrict__ part_dy, int nb_dy,
                   const double* __restrict__ part_t, int nb_t, pdlpdev_step_params sp, const int* __restrict__ zcount, int nb_z, int zn, int zmode)
{
  step_decision_workgroup<true>(in, out, part_dy, nb_dy, part_t, nb_t, nullptr, sp, zcount, nb_z, zn, zmode);
}

// ---- the decision of the PREVIOUS attempt at the head of the primal step (attempts 2 .. N of a chunk: enqueue_single_chunk) ---------
// k_primal's 56 bytes per column take their 10 us in any order, and more than 98 % of the 1e6 x 1e6 LP's attempts are accepted.  So
// every workgroup (1) reads the block the previous attempt ran with and REQUESTS the operands of its first kPrimalDecideCols columns per
// thread as if that attempt was accepted -- the flipped side of x and A^T y, c, sum_x, the bounds unless they are uniform --, (2) forms
// the decision while they are in flight: step_decision_form, the association and the pow() calls of the one-workgroup kernel, so the
// same bits in every workgroup, (3) after a rejection loads x and A^T y again from the side the decision names (rare, slower),
// (4, 5) and goes through its columns with the decided tau, step size, pending_avg and cur, unless the decided block ends the loop.
// Workgroup 0 stores the decided block at `out`: the block this attempt's two products and the next decision read.  `in` is never
// written by this kernel and `zcount_in` (the previous primal step's counts) is not the buffer this one writes: a workgroup may be done
// before another has started.  An empty previous attempt (loop not active at `in`) copies the block through and leaves the columns alone.
constexpr int kPrimalDecideCols = 4;     // columns per thread requested ahead of the decision: 245 workgroups at n = 1e6, one per CU
constexpr int kPrimalDecideMaxGrid = 512;  // (every workgroup reads all partials: a few hundred of them keep that traffic negligible)
// (cap: kPrimalDecideMaxGrid, or what CUOPT_AMD_TUNE=primal_decide_grid asks for -- tests reach the grid-stride remainder with a small LP)
static inline int primal_decide_grid(int n, int cap)
{
  const int per = kDecisionThreads * kPrimalDecideCols;
  return std::max(1, std::min((n + per - 1) / per, cap));
}
template <bool ZS>
__device__ __forceinline__ void
primal_decide_body(int n, const pdlpdev_ctl* in, pdlpdev_ctl* out, double* __restrict__ x0, double* __restrict__ x1,
                   const double* __restrict__ aty0, const double* __restrict__ aty1, const double* __restrict__ c, const double* __restrict__ lb,
                   const double* __restrict__ ub, double* __restrict__ xbar, double* __restrict__ sumx, pdlpdev_ctx::UniformBounds ubd,
                   unsigned long long* __restrict__ xmask, int* __restrict__ zcount_out, const double* __restrict__ part_dy, int nb_dy,
                   const double* __restrict__ part_t, int nb_t, const pdlpdev_step_params& sp, const int* __restrict__ zcount_in, int nb_z, int zmode)
{
  constexpr int U = kPrimalDecideCols, T = kDecisionThreads;
  [[maybe_unused]] int nz = 0;
  pdlpdev_ctl lc = *in;
  if (!(lc.error == 0 && lc.steps_taken < lc.target_steps)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) store_ctl<ZS>(out, lc);
    return;
  }
  // (1) the first columns' operands, as if accepted: requested right behind the decision's partials, (2) the decision
  const int ahead = lc.cur ^ 1;
  const int j0    = blockIdx.x * (U * T) + threadIdx.x;
  double xj[U], tj[U], cj[U], sj[U], lbj[U], ubj[U];
  step_decision_form<ZS, true>(lc, part_dy, nb_dy, part_t, nb_t, nullptr, sp, zcount_in, nb_z, n, zmode, [&] {
    // (a thread beyond column n - 1 requests that column and leaves it unused, n > 0: one straight run of loads behind the partials', so
    //  that the sums' wait counts them and lets them fly)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = min(j0 + u * T, n - 1);
      xj[u]  = (ahead ? x1 : x0)[j];
      tj[u]  = (ahead ? aty1 : aty0)[j];
      cj[u]  = c[j];
      sj[u]  = sumx[j];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) lbj[u] = ubd.lb_same ? ubd.lb : lb[min(j0 + u * T, n - 1)];
#pragma unroll
    for (int u = 0; u < U; ++u) ubj[u] = ubd.ub_same ? ubd.ub : ub[min(j0 + u * T, n - 1)];
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) store_ctl<ZS>(out, lc);
  if (!(lc.error == 0 && lc.steps_taken < lc.target_steps)) return;  // (4)
  const int cur       = __builtin_amdgcn_readfirstlane(lc.cur);  // (the same in every thread: scalar)
  const bool pend     = __builtin_amdgcn_readfirstlane(lc.pending_avg) != 0;
  const double tau    = lc.tau;
  const double weight = lc.step_size;
  const double* __restrict__ x   = cur ? x1 : x0;
  double* __restrict__ xn        = cur ? x0 : x1;
  const double* __restrict__ aty = cur ? aty1 : aty0;
  // (3) rejected: the iterate did not flip
  if (cur != ahead) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * T;
      if (j < n) xj[u] = x[j], tj[u] = aty[j];
    }
  }
  // (5) the columns: k_primal's expressions
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = j0 + u * T;
    if (j < n) {
      primal_column<ZS>(j, xj[u], cj[u], tj[u], lbj[u], ubj[u], tau, xn, xbar, xmask, nz);
      if (pend) sumx[j] = sj[u] + weight * xj[u];
    }
  }
  // (an LP of more columns than the grid's first pass holds: the rest as k_primal takes them)
  for (long long base = ((long long)blockIdx.x + gridDim.x) * (U * T); base < n; base += (long long)gridDim.x * (U * T)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long jj = base + threadIdx.x + u * T;
      if (jj < n) {
        const int j = (int)jj;
        const double xv = x[j];
        primal_column<ZS>(j, xv, c[j], aty[j], ubd.lb_same ? ubd.lb : lb[j], ubd.ub_same ? ubd.ub : ub[j], tau, xn, xbar, xmask, nz);
        if (pend) sumx[j] = sumx[j] + weight * xv;
      }
    }
  }
  if constexpr (ZS) primal_store_zcount<T / 64>(nz, zcount_out);
}
__global__ void __launch_bounds__(kDecisionThreads)
k_primal_decide(int n, const pdlpdev_ctl* in, pdlpdev_ctl* out, double* __restrict__ x0, double* __restrict__ x1,
                const double* __restrict__ aty0, const double* __restrict__ aty1, const double* __restrict__ c, const double* __restrict__ lb,
                const double* __restrict__ ub, double* __restrict__ xbar, double* __restrict__ sumx, pdlpdev_ctx::UniformBounds ubd,
                const double* __restrict__ part_dy, int nb_dy, const double* __restrict__ part_t, int nb_t, pdlpdev_step_params sp)
{
  primal_decide_body<false>(n, in, out, x0, x1, aty0, aty1, c, lb, ub, xbar, sumx, ubd, nullptr, nullptr, part_dy, nb_dy, part_t, nb_t, sp, nullptr, 0, 0);
}
__global__ void __launch_bounds__(kDecisionThreads)
k_primal_decide_zs(int n, const pdlpdev_ctl* in, pdlpdev_ctl* out, double* __restrict__ x0, double* __restrict__ x1,
                   const double* __restrict__ aty0, const double* __restrict__ aty1, const double* __restrict__ c, const double* __restrict__ lb,
                   const double* __restrict__ ub, double* __restrict__ xbar, double* __restrict__ sumx, pdlpdev_ctx::UniformBounds ubd,
                   unsigned long long* __restrict__ xmask, int* __restrict__ zcount_out, const double* __restrict__ part_dy, int nb_dy,
                   const double* __restrict__ part_t, int nb_t, pdlpdev_step_params sp, const int* __restrict__ zcount_in, int nb_z, int zmode)
{
  primal_decide_body<true>(n, in, out, x0, x1, aty0, aty1, c, lb, ub, xbar, sumx, ubd, xmask, zcount_out, part_dy, nb_dy, part_t, nb_t, sp, zcount_in, nb_z,
                           zmode);
}
// the decisions of the K LPs of a shared-matrix batch (kernels_batch.hip): workgroup <-> LP, each exactly k_step_decision
__global__ void __launch_bounds__(kDecisionThreads)
k_step_decision_batch(const pdlpdev_decision_args* __restrict__ args)
{
  const pdlpdev_decision_args a = args[blockIdx.x];
  step_decision_workgroup(a.ctl, a.ctl, a.part_dy, a.nb_dy, a.part_t, a.nb_t, nullptr, a.sp);
}

// The decision of a Halpern step (docs/design/04d_halpern_mode.md): nothing to decide -- a step never fails -- but the same one workgroup
// on the critical path: the partials are added in k_step_decision's order, the fixed-point error of the step is formed in PDHG's metric
//   r_k^2 = (w / eta) ||dx||^2 + 2 dy.(A dx) + ||dy||^2 / (eta w),   dy.(A dx) = dx.(A^T y' - A^T y^k) = StepEpilogue's first sum,
// the counters advance and the buffers flip.  A NaN or an overflow raises the step error like an invalid movement does.
__global__ void __launch_bounds__(kDecisionThreads)
k_halpern_decision(pdlpdev_ctl* __restrict__ ctl, pdlpdev_halpern* __restrict__ hal, const double* __restrict__ part_dy, int nb_dy,
                   const double* __restrict__ part_t, int nb_t)
{
  halpern_decision_workgroup(ctl, hal, part_dy, nb_dy, part_t, nb_t);  // (halpern_decision.hpp: shared with the lockstep batch's K decisions)
}
__global__ void k_halpern_clear(pdlpdev_halpern* hal)
{
  hal->r = hal->r_first = hal->r2 = 0.0;
  hal->r2_min = __builtin_huge_val();
  hal->k = 0, hal->reserved = 0;
}
// behind k_restart + k_finalize (dist2 = the two squared distances): the smoothed primal weight on the device, the anchor's A^T y, k <- 0
__global__ void k_halpern_restart_ctl(pdlpdev_ctl* ctl, pdlpdev_halpern* hal, double* dist2, double theta)
{
  halpern_restart_scalars(ctl, hal, dist2, theta);  // (halpern_decision.hpp: shared with every other restart of the mode)
}
__global__ void __launch_bounds__(kBlock)
k_copy_current(int n, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ v0, const double* __restrict__ v1, double* __restrict__ out)
{
  const double* __restrict__ v = ctl->cur ? v1 : v0;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) out[i] = v[i];
}
// power iteration (pdlpdev_spectral_norm): out = v / d
__global__ void __launch_bounds__(kBlock) k_div_by_scalar(int n, double* __restrict__ out, const double* __restrict__ v, double d)
{
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) out[i] = v[i] / d;
}

// The scalar exchange of the direct peer transport, by ONE workgroup of kBlock threads (the body of k_step_decision_p2p and of
// k_halpern_decision_p2p, so that the flag / wait protocol exists once): this rank's three sums from the partials of the two SpMV
// kernels, write-through stores into every rank's block, the flag, the bounded wait for the others, the landed sums added in rank
// order -- the same bits on every rank.  true: thread 0 (and only it) goes on with `sum`; false: every other thread, and every
// thread when the wait ran out (then the fault flag and the step error are up).
__device__ __forceinline__ bool p2p_exchange_step_sums(pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ part_dy, int nb_dy,
                                                       const double* __restrict__ part_t, int nb_t, const double* __restrict__ landed,
                                                       const unsigned long long* __restrict__ flags, int world,
                                                       const unsigned long long* __restrict__ epoch, int* __restrict__ fault,
                                                       const p2pdev::Push* __restrict__ push, double (&sum)[3])
{
  {
    __shared__ double red[3 * 8];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nb_dy; i += kBlock) acc[0] += part_dy[i];
    for (int i = threadIdx.x; i < nb_t; i += kBlock) {
      acc[1] += part_t[i];
      acc[2] += part_t[nb_t + i];
    }
    block_reduce<SumOp, 3>(acc, red);
    if (threadIdx.x == 0) {
      for (int q = 0; q < push->world; ++q) {
        double* d = push->slot(q);
        p2pdev::put(d, acc[0]), p2pdev::put(d + 1, acc[1]), p2pdev::put(d + 2, acc[2]);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      push->epoch[push->kind] = push->epoch[push->kind] + 1;
      p2pdev::raise(push);
    }
    __syncthreads();
  }
  if (!p2pdev::wait_flags(flags, world, 2, epoch)) {
    if (threadIdx.x == 0) *fault = 1, ctl->error = 1;
    return false;
  }
  if (threadIdx.x != 0) return false;
  sum[0] = sum[1] = sum[2] = 0.0;
  for (int q = 0; q < world; ++q)
    for (int k = 0; k < 3; ++k) sum[k] += __hip_atomic_load(landed + 4 * q + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return true;
}

// direct peer transport of a sharded solve: wait for every rank's three step-size sums (landed in this rank's block), add them
// up in rank order -- the same bits on every rank -- and take the decision
// (one workgroup, so the whole scalar exchange lives in this kernel: its own three sums from the partials of the two SpMV kernels,
// write-through stores into every rank's block, the flag, the wait for the others -- no ticket, no kernel boundary in between)
__global__ void __launch_bounds__(kBlock)
k_step_decision_p2p(pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ part_dy, int nb_dy, const double* __restrict__ part_t, int nb_t,
                    const double* __restrict__ landed, const unsigned long long* __restrict__ flags, int world,
                    const unsigned long long* __restrict__ epoch, int* __restrict__ fault, pdlpdev_step_params sp, const p2pdev::Push* __restrict__ push)
{
  if (!loop_active(ctl)) return;
  double sum[3];
  if (!p2p_exchange_step_sums(ctl, part_dy, nb_dy, part_t, nb_t, landed, flags, world, epoch, fault, push, sum)) return;
  pdlpdev_ctl lc = *ctl;
  apply_step_decision(&lc, sum[0], sum[1], sum[2], sp);
  *ctl = lc;
}
// ---- the decision of a sharded Halpern step (cuoptamd_settings::halpern_sharded; owner-computes dataflow) ----
// collective transport: the three sums arrive all-reduced (k_pack_step_sums -> allreduce(3)): the same bits on every rank, so every
// rank takes the same decision -- the step error of a NaN or an overflow included -- through the one body of halpern_decision.hpp
__global__ void k_halpern_decision_sums(pdlpdev_ctl* __restrict__ ctl, pdlpdev_halpern* __restrict__ hal, const double* __restrict__ sums)
{
  pdlpdev_ctl lc = *ctl;
  if (!(lc.error == 0 && lc.steps_taken < lc.target_steps)) return;
  halpern_decision_from_sums(ctl, hal, lc, sums[0], sums[1], sums[2]);
}
// direct peer transport: the twin of k_step_decision_p2p -- the same scalar exchange (p2p_exchange_step_sums), the Halpern decision
__global__ void __launch_bounds__(kBlock)
k_halpern_decision_p2p(pdlpdev_ctl* __restrict__ ctl, pdlpdev_halpern* __restrict__ hal, const double* __restrict__ part_dy, int nb_dy,
                       const double* __restrict__ part_t, int nb_t, const double* __restrict__ landed, const unsigned long long* __restrict__ flags,
                       int world, const unsigned long long* __restrict__ epoch, int* __restrict__ fault, const p2pdev::Push* __restrict__ push)
{
  if (!loop_active(ctl)) return;
  double sum[3];
  if (!p2p_exchange_step_sums(ctl, part_dy, nb_dy, part_t, nb_t, landed, flags, world, epoch, fault, push, sum)) return;
  pdlpdev_ctl lc = *ctl;
  halpern_decision_from_sums(ctl, hal, lc, sum[0], sum[1], sum[2]);
}

__global__ void __launch_bounds__(kBlock)
k_permute_pad(int64_t n, const int32_t* __restrict__ perm, const double* __restrict__ src, double* __restrict__ dst)
{
  for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int32_t k = perm[i];
    dst[i]          = k >= 0 ? src[k] : 0.0;
  }
}
__global__ void __launch_bounds__(kBlock)
k_permute(int64_t n, const int32_t* __restrict__ perm, const double* __restrict__ src, double* __restrict__ dst)
{
  for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    dst[i] = src[perm[i]];
}

// deferred averaging made explicit (called before a major iteration consumes the sums)
__global__ void __launch_bounds__(kBlock)
k_flush_average(int n, int m, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ x0,
                const double* __restrict__ x1, const double* __restrict__ y0,
                const double* __restrict__ y1, double* __restrict__ sumx, double* __restrict__ sumy, int guard)
{
  if (ctl->pending_avg == 0 || (guard && !period_reached(ctl))) return;
  const int cur           = ctl->cur;
  const double w          = ctl->step_size;
  const double* __restrict__ x = cur ? x1 : x0;
  const double* __restrict__ y = cur ? y1 : y0;
  const int tot = n > m ? n : m;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < tot; i += gridDim.x * kBlock) {
    if (i < n) sumx[i] = sumx[i] + w * x[i];
    if (i < m) sumy[i] = sumy[i] + w * y[i];
  }
}
__global__ void k_clear_pending(pdlpdev_ctl* ctl) { ctl->pending_avg = 0; }

__global__ void __launch_bounds__(kBlock)
k_sum_partials_to(const double* __restrict__ part, int nb, double* __restrict__ out)
{
  __shared__ double red[8];
  double acc[1] = {0.0};
  for (int i = threadIdx.x; i < nb; i += kBlock) acc[0] += part[i];
  block_reduce<SumOp, 1>(acc, red);
  if (threadIdx.x == 0) out[0] = acc[0];
}

// sliced-primal dataflow: this rank's three step-size partial sums, side by side, for ONE small all-reduce
__global__ void __launch_bounds__(kBlock)
k_pack_step_sums(const double* __restrict__ part_dy, int nb_dy, const double* __restrict__ part_t, int nb_t, double* __restrict__ out)
{
  __shared__ double red[3 * 8];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nb_dy; i += kBlock) acc[0] += part_dy[i];
  for (int i = threadIdx.x; i < nb_t; i += kBlock) {
    acc[1] += part_t[i];
    acc[2] += part_t[nb_t + i];
  }
  block_reduce<SumOp, 3>(acc, red);
  if (threadIdx.x == 0) {
    out[0] = acc[0], out[1] = acc[1], out[2] = acc[2];
  }
}

__global__ void k_restart_ctl(pdlpdev_ctl* ctl)
{
  ctl->sum_weights       = 0.0;
  ctl->its_since_restart = 0;
  ctl->pending_avg       = 0;
}
__global__ void k_set_step(pdlpdev_ctl* ctl, double step, double w)
{
  if (step >= 0.0) ctl->step_size = step;
  ctl->primal_weight = w;
  ctl->tau           = ctl->step_size / w;
  ctl->sigma         = ctl->step_size * w;
}
__global__ void k_set_target(pdlpdev_ctl* ctl, int target) { ctl->target_steps = target; }
__global__ void k_set_k(pdlpdev_ctl* ctl, int k) { ctl->k = k; }
__global__ void k_clear_error(pdlpdev_ctl* ctl) { ctl->error = 0; }
__global__ void k_set_error(pdlpdev_ctl* ctl) { ctl->error = 1; }
__global__ void k_set_loop_state(pdlpdev_ctl* ctl, double sum_weights, int its_since_restart, int k)
{
  ctl->sum_weights       = sum_weights;
  ctl->its_since_restart = its_since_restart;
  ctl->k                 = k;
  ctl->pending_avg       = 0;
}

// unscale for output: x = x^ * D_c, y = y^ * D_r (unscale_solutions, initial_scaling.cu:460-484)
__global__ void __launch_bounds__(kBlock)
k_unscale(int n, const double* __restrict__ v, const double* __restrict__ d, double* __restrict__ out)
{
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) out[i] = v[i] * d[i];
}






// Every hot-loop launch goes through here so that pdlpdev_time_kernel can ask for the dispatch's own start / stop
// timestamps (hipExtLaunchKernel) without putting event records between the kernels of an attempt.
#include "pdlp_launch.hpp"
#include "pdlp_core_internal.hpp"
#include "halpern_major.hpp"

// panel values <- current CSR values (after upload and again after scale_problem)
int sync_panel_values(pdlpdev_ctx* c)
{
  // first the hot copies of the matrices and the segments' values, from the full (just scaled) CSR
  if (c->A.hot.val != c->A.full.val) k_permute<<<grid_for(c->A.hot_nnz), kBlock, 0, c->stream>>>(c->A.hot_nnz, c->dense.s_perm_a, c->A.full.val, c->A.hot.val);
  if (c->At.hot.val != c->At.full.val) k_permute<<<grid_for(c->At.hot_nnz), kBlock, 0, c->stream>>>(c->At.hot_nnz, c->dense.s_perm_at, c->At.full.val, c->At.hot.val);
  if (c->dense.on) k_permute<<<grid_for(c->dense.nent), kBlock, 0, c->stream>>>(c->dense.nent, c->dense.perm, c->A.full.val, c->dense.val);
  // then each layout's values from its side's hot CSR: panels of A, A^T, jagged rows of A, A^T, gather-free of A, A^T, the column block's
  const pdlpdev_ctx::MatrixSide* sides[] = {&c->A, &c->At};
  for (const auto* s : sides)
    if (s->pan.on) k_permute<<<grid_for(s->pan.nent), kBlock, 0, c->stream>>>(s->pan.nent, s->pan.perm, s->hot.val, s->pan.val);
  for (const auto* s : sides)
    if (s->jag.on) k_permute<<<grid_for(s->jag.nent), kBlock, 0, c->stream>>>(s->jag.nent, s->jag.perm, s->hot.val, s->jag.val);
  for (const auto* s : sides)
    if (s->pb.on) k_permute_pad<<<grid_for(s->pb.np), kBlock, 0, c->stream>>>(s->pb.np, s->pb.perm, s->hot.val, s->pb.val);
  if (c->Oc.pan.on) k_permute<<<grid_for(c->Oc.pan.nent), kBlock, 0, c->stream>>>(c->Oc.pan.nent, c->Oc.pan.perm, c->Oc.hot.val, c->Oc.pan.val);
  if (c->Oc.jag.on) k_permute<<<grid_for(c->Oc.jag.nent), kBlock, 0, c->stream>>>(c->Oc.jag.nent, c->Oc.jag.perm, c->Oc.hot.val, c->Oc.jag.val);
  HIP_TRY(hipGetLastError());
  return 0;
}


// per slice of the gathered vector: the smallest and largest index this matrix references there (halo exchange, pdlp_ctx.hpp Halo)
__global__ void __launch_bounds__(kBlock) k_slice_ranges(int64_t nnz, const int32_t* __restrict__ idx, int32_t slice, int world,
                                                         int32_t* __restrict__ lo, int32_t* __restrict__ hi)
{
  __shared__ int32_t slo[16], shi[16];
  if (threadIdx.x < 16) slo[threadIdx.x] = 0x7fffffff, shi[threadIdx.x] = -1;
  __syncthreads();
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * kBlock) {
    const int32_t j = idx[k];
    const int q     = min(j / slice, world - 1);
    if (j < slo[q]) atomicMin(&slo[q], j);
    if (j > shi[q]) atomicMax(&shi[q], j);
  }
  __syncthreads();
  if ((int)threadIdx.x < world && shi[threadIdx.x] >= 0) atomicMin(&lo[threadIdx.x], slo[threadIdx.x]), atomicMax(&hi[threadIdx.x], shi[threadIdx.x]);
}

// the columns a rank of a sliced dataflow (rsag, owner-computes) steps: `len` from `cs` on -- equal slices, the last ranks' clipped at n
struct ColSlice { size_t cs; int len; };
static ColSlice rank_slice(const pdlpdev_ctx* ctx)
{
  const size_t cs = (size_t)ctx->rank * ctx->slice;
  return {cs, (int)std::max<int64_t>(0, std::min<int64_t>(ctx->slice, (int64_t)ctx->n - (int64_t)cs))};
}

extern "C" {

int pdlpdev_owner_slice(pdlpdev_ctx* ctx, int32_t* col_begin, int32_t* ncols)
{
  if (!ctx->owner) return fail(-1, "pdlpdev_owner_slice: the solver does not run the owner-computes dataflow");
  const ColSlice sl = rank_slice(ctx);
  *col_begin        = (int32_t)std::min<int64_t>((int64_t)sl.cs, ctx->n);
  *ncols            = sl.len;
  return 0;
}
int pdlpdev_shard_slice(pdlpdev_ctx* ctx, int32_t* col_begin, int32_t* ncols)
{
  const int64_t cs = ctx->rsag ? (int64_t)ctx->rank * ctx->slice : 0, len = ctx->rsag ? ctx->slice : ctx->n;
  *col_begin       = (int32_t)std::min<int64_t>(cs, ctx->n);
  *ncols           = (int32_t)std::max<int64_t>(0, std::min<int64_t>(len, (int64_t)ctx->n - cs));
  return 0;
}
int pdlpdev_owner_layout_info(pdlpdev_ctx* ctx, int32_t out[3])
{
  if (!ctx->owner || !ctx->Oc.hot.off) return fail(-1, "pdlpdev_owner_layout_info: no column block (the owner-computes dataflow behind pdlpdev_owner_setup only)");
  ctx->Oc.info(out);
  return 0;
}
// The column block of the owner-computes dataflow: rows [col_begin, col_begin + ncols) of the GLOBAL A^T (column indices =
// global row numbers of A, ascending: every column is then summed over the rows in the order one GPU uses), unscaled
// values; row_bounds[world + 1] = the ranks' row blocks.  Call after pdlpdev_scale_problem: the values are scaled here with
// this rank's D_c and the gathered D_r, by the expression the transposed copy of an unsharded solve goes through.
int pdlpdev_owner_setup(pdlpdev_ctx* ctx, const int32_t* off, const int32_t* idx, const double* val, const int32_t* row_bounds)
{
  if (!ctx->owner) return fail(-1, "pdlpdev_owner_setup: the solver does not run the owner-computes dataflow");
  if (!ctx->scaled) return fail(-1, "pdlpdev_owner_setup: call after pdlpdev_scale_problem");
  HIP_TRY(hipSetDevice(ctx->device));
  int32_t cb = 0, nc = 0;
  TRY(pdlpdev_owner_slice(ctx, &cb, &nc));
  if (row_bounds[ctx->rank + 1] - row_bounds[ctx->rank] != ctx->m) return fail(-1, "pdlpdev_owner_setup: row bounds disagree with this rank's block");
  int maxrows = 0;
  for (int q = 0; q < ctx->world; ++q) maxrows = std::max(maxrows, row_bounds[q + 1] - row_bounds[q]);
  ctx->ypad = (maxrows + 15) & ~15;
  const int64_t gcols = (int64_t)ctx->world * ctx->ypad;
  if (gcols >= ((int64_t)1 << 31)) return fail(-1, "pdlpdev_owner_setup: gathered dual too long");
  const int64_t nnz = nc > 0 ? off[nc] : 0;
  ctx->Oc.name = "column block", ctx->Oc.rows = nc, ctx->Oc.cols = (int32_t)gcols, ctx->Oc.hot_nnz = nnz;
  // global row -> position in the gathered dual (rank q's rows at [q * ypad, ...))
  std::vector<int32_t> ridx((size_t)std::max<int64_t>(nnz, 1));
  {
    std::vector<int32_t> shift(ctx->world);
    for (int q = 0; q < ctx->world; ++q) shift[q] = q * ctx->ypad - row_bounds[q];
    for (int32_t r = 0; r < nc; ++r) {
      int q = 0;
      for (int k = off[r]; k < off[r + 1]; ++k) {  // ascending rows: the owner only moves forward
        while (idx[k] >= row_bounds[q + 1]) ++q;
        ridx[k] = idx[k] + shift[q];
      }
    }
  }
  TRY(upload_i32(ctx, &ctx->Oc.hot.off, off, (size_t)nc + 1));
  TRY(upload_i32(ctx, &ctx->Oc.hot.idx, ridx.data(), (size_t)nnz, 8));
  TRY(upload_f64(ctx, &ctx->Oc.hot.val, val, (size_t)nnz, 8));
  ctx->Oc.full = ctx->Oc.hot;
  TRY(dev_alloc(ctx, &ctx->ygather, (size_t)gcols + kSlicePad));
  std::vector<int32_t> longs;
  for (int32_t r = 0; r < nc; ++r)
    if (off[r + 1] - off[r] > kLongRow) longs.push_back(r);
  ctx->Oc.nlong = (int)longs.size();
  if (ctx->Oc.nlong) TRY(upload_i32(ctx, &ctx->Oc.longs, longs.data(), longs.size()));
  std::vector<int32_t> rb = build_row_blocks(nc, off);
  ctx->Oc.nb = (int)rb.size() / 2 - 1;
  TRY(upload_i32(ctx, &ctx->Oc.rb, rb.data(), rb.size()));
  // scaling: D_r of every rank's rows in the gathered layout (ygather doubles as the staging buffer), then (val * D_c[j]) * D_r[i]
  hipStream_t s = ctx->stream;
  HIP_TRY(hipMemcpyAsync(ctx->ygather + (size_t)ctx->rank * ctx->ypad, ctx->dr, (size_t)ctx->m * sizeof(double), hipMemcpyDeviceToDevice, s));
  TRY(all_gather(ctx, ctx->ygather, (size_t)ctx->ypad));
  k_scale_matrix<<<grid_for(nc), kBlock, 0, s>>>(nc, ctx->Oc.hot.off, ctx->Oc.hot.idx, ctx->Oc.hot.val, ctx->dc + cb, ctx->ygather);
  if (ctx->Oc.nlong) k_scale_matrix_long<<<ctx->Oc.nlong, kBlock, 0, s>>>(ctx->Oc.longs, ctx->Oc.hot.off, ctx->Oc.hot.idx, ctx->Oc.hot.val, ctx->dc + cb, ctx->ygather);
  HIP_TRY(hipGetLastError());
  // layouts, by the policy of the two other matrices with two candidates: jagged rows, then panels (timed mode counts as auto here)
  {
    LayoutPolicy P;
    TRY(layout_policy(&P));
    const LayoutPolicy::Mode mode = P.mode == LayoutPolicy::kTimed ? LayoutPolicy::kAuto : P.mode;
    if (nc > 0 && (mode == LayoutPolicy::kAuto || mode == LayoutPolicy::kJag)) {
      JagHost j = build_jag(nc, (int32_t)gcols, off, ridx.data(), mode == LayoutPolicy::kJag ? 1 : 0, ctx->cus);
      TRY(upload_jag(ctx, &ctx->Oc.jag, j, ctx->Oc.hot.off, ctx->Oc.hot.idx, ctx->Oc.hot.val));
    }
    const bool panels = mode == LayoutPolicy::kPanel ||
                        (mode == LayoutPolicy::kAuto && gcols * 8 > P.ws_limit && gather_working_set(nc, (int32_t)gcols, off, ridx.data()) > P.ws_limit);
    if (nc > 0 && !ctx->Oc.jag.on && panels) {
      PanelHost h = build_panels(nc, (int32_t)gcols, off, ridx.data(), P.slab_bytes, true);
      TRY(upload_panels(ctx, &ctx->Oc.pan, h, ctx->Oc.hot.off, ctx->Oc.hot.idx, ctx->Oc.hot.val));
    }
  }
  TRY(dev_alloc(ctx, &ctx->Oc.part, (size_t)8 * std::max(ctx->Oc.partials(), 1)));
  {
    const char* tr = getenv("CUOPT_AMD_SHARD_TRANSPORT");
    if (tr && std::string(tr) == "p2p") TRY(p2p_setup(ctx));
    else if (tr && std::string(tr) != "collective") return fail(-1, "CUOPT_AMD_SHARD_TRANSPORT must be collective or p2p");
  }
  if (ctx->Oc.pan.on) k_permute<<<grid_for(ctx->Oc.pan.nent), kBlock, 0, s>>>(ctx->Oc.pan.nent, ctx->Oc.pan.perm, ctx->Oc.hot.val, ctx->Oc.pan.val);
  if (ctx->Oc.jag.on) k_permute<<<grid_for(ctx->Oc.jag.nent), kBlock, 0, s>>>(ctx->Oc.jag.nent, ctx->Oc.jag.perm, ctx->Oc.hot.val, ctx->Oc.jag.val);
  HIP_TRY(hipGetLastError());
  {
    // what this rank references outside its own slice / rows: per peer one range of xbar (the rank's rows of A, on the device) and
    // one of the gathered y' (the column block, here on the host)
    const int W = ctx->world;
    std::vector<int32_t> need((size_t)4 * W, 0), xl(W, 0x7fffffff), xh(W, -1);
    int32_t *d_lo = nullptr, *d_hi = nullptr;
    TRY(dev_alloc(ctx, &d_lo, 16));
    TRY(dev_alloc(ctx, &d_hi, 16));
    HIP_TRY(hipMemcpyAsync(d_lo, xl.data(), W * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_hi, xh.data(), W * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (ctx->nnz > 0) k_slice_ranges<<<grid_for(ctx->nnz, 8), kBlock, 0, s>>>(ctx->nnz, ctx->A.full.idx, ctx->slice, W, d_lo, d_hi);
    HIP_TRY(hipMemcpyAsync(xl.data(), d_lo, W * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(xh.data(), d_hi, W * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<int32_t> yl(W, 0x7fffffff), yh(W, -1);
    for (int64_t k = 0; k < nnz; ++k) {
      const int32_t pos = ridx[(size_t)k];
      const int q       = pos / ctx->ypad;
      yl[q] = std::min(yl[q], pos), yh[q] = std::max(yh[q], pos);
    }
    for (int q = 0; q < W; ++q) {
      need[(size_t)4 * q + 0] = xh[q] >= 0 ? xl[q] : 0, need[(size_t)4 * q + 1] = xh[q] >= 0 ? xh[q] + 1 : 0;
      need[(size_t)4 * q + 2] = yh[q] >= 0 ? yl[q] : 0, need[(size_t)4 * q + 3] = yh[q] >= 0 ? yh[q] + 1 : 0;
    }
    TRY(halo_setup(ctx, need.data()));
  }
  HIP_TRY(hipStreamSynchronize(s));  // the host arrays are the caller's
  return 0;
}

// ---- helpers --------------------------------------------------------------------------------------
int fetch_scalars(pdlpdev_ctx* ctx, int count)
{
  HIP_TRY(hipMemcpyAsync(ctx->scal_h, ctx->scal, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}
int fetch_ctl(pdlpdev_ctx* ctx, pdlpdev_ctl* out)
{
  HIP_TRY(hipMemcpyAsync(ctx->ctl_h, ctx->ctl, sizeof(pdlpdev_ctl), hipMemcpyDeviceToHost, ctx->stream));
  if (ctx->halpern) HIP_TRY(hipMemcpyAsync(ctx->hal_h, ctx->hal, sizeof(pdlpdev_halpern), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ctx->ctl_h_current = true;
  if (out) *out = *ctx->ctl_h;
  return 0;
}
int fetch_ctl_counted(pdlpdev_ctx* ctx, pdlpdev_ctl* out)
{
  TRY(fetch_ctl(ctx, out));
  ctx->stat_loop_syncs += 1;
  return 0;
}

static int reduce_vec(pdlpdev_ctx* ctx, int mode, int64_t n, const double* a, const double* b, int slot)
{
  const int g = std::min(grid_for(n), kGenericBlocks);
  switch (mode) {
    case 0: k_reduce<0><<<g, kBlock, 0, ctx->stream>>>(n, a, b, ctx->part_g); break;
    case 1: k_reduce<1><<<g, kBlock, 0, ctx->stream>>>(n, a, b, ctx->part_g); break;
    case 2: k_reduce<2><<<g, kBlock, 0, ctx->stream>>>(n, a, b, ctx->part_g); break;
    default: k_reduce<3><<<g, kBlock, 0, ctx->stream>>>(n, a, b, ctx->part_g); break;
  }
  k_finalize<<<1, kBlock, 0, ctx->stream>>>(ctx->part_g, g, 1, mode == 0 ? 1u : 0u, ctx->scal + slot);
  LAUNCH_CHECK();
  return 0;
}

// max over the ranks of one host scalar (identity without a communicator): lets every rank of a sharded solve
// take the same wall-clock decision (time limit), which they must -- the collectives have to match up
int pdlpdev_agree_max(pdlpdev_ctx* ctx, double* value)
{
  if (!ctx->comm) return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(ctx->scal + 60, value, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  TRY(allreduce(ctx, ctx->scal + 60, 1, rccl::kMax));
  HIP_TRY(hipMemcpyAsync(ctx->scal_h + 60, ctx->scal + 60, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  *value = ctx->scal_h[60];
  return 0;
}

int pdlpdev_init_norms(pdlpdev_ctx* ctx, double out[3])
{
  HIP_TRY(hipSetDevice(ctx->device));
  TRY(reduce_vec(ctx, 0, ctx->nnz, ctx->A.full.val, nullptr, 0));
  TRY(reduce_vec(ctx, 1, ctx->n, ctx->c, nullptr, 1));
  TRY(reduce_vec(ctx, 2, ctx->m, ctx->lo, ctx->hi, 2));
  TRY(allreduce(ctx, ctx->scal + 0, 1, rccl::kMax));
  TRY(allreduce(ctx, ctx->scal + 2, 1, rccl::kSum));
  TRY(fetch_scalars(ctx, 3));
  out[0] = ctx->scal_h[0], out[1] = ctx->scal_h[1], out[2] = ctx->scal_h[2];
  return 0;
}

// New bounds for the SAME matrix and objective, iterate and all loop state back to their values right after
// pdlpdev_scale_problem: what a MIP heuristic needs between two relaxations (relaxed_lp.cu:53-127 builds a whole
// new pdlp_solver_t instead).  D_r, D_c depend on A only (initial_scaling.cu:125-307), so nothing is rescaled.
int pdlpdev_reset(pdlpdev_ctx* ctx, const double* lb, const double* ub, const double* lo, const double* hi)
{
  HIP_TRY(hipSetDevice(ctx->device));
  if (!ctx->scaled) return fail(-1, "pdlpdev_reset: the problem has not been scaled yet");
  ctx->rejected_in_a_row = 0;
  ctx->spare_attempts    = 0;
  loop_state_touched(ctx);
  hipStream_t s = ctx->stream;
  const size_t nb = (size_t)ctx->n * sizeof(double), mb = (size_t)ctx->m * sizeof(double);
  auto put = [&](const double* src, double* unscaled, double* scaled, size_t bytes) -> int {
    if (!src || bytes == 0) return 0;
    HIP_TRY(hipMemcpyAsync(unscaled, src, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(scaled, unscaled, bytes, hipMemcpyDeviceToDevice, s));
    return 0;
  };
  TRY(put(lb, ctx->lb_u, ctx->lb, nb));
  TRY(put(ub, ctx->ub_u, ctx->ub, nb));
  {
    const pdlpdev_ctx::UniformBounds before = ctx->ubd;
    ctx->note_uniform_bounds(lb, ub);
    const pdlpdev_ctx::UniformBounds& now = ctx->ubd;
    if (before.lb_same != now.lb_same || before.ub_same != now.ub_same || (now.lb_same && before.lb != now.lb) || (now.ub_same && before.ub != now.ub)) {
      // the attempt graphs carry k_primal's arguments by value: captured again on the next run
      for (auto& kv : ctx->graphs) (void)hipGraphExecDestroy(kv.second);
      ctx->graphs.clear();
    }
  }
  if ((lo || hi) && (ctx->rows_aliased || (ctx->clones_alive > 0 && !ctx->rows_private))) {
    // row bounds shared with clones (or with the parent): this context gets arrays of its own first; the others keep the old ones
    for (double** v : {&ctx->lo, &ctx->lo_u, &ctx->hi, &ctx->hi_u}) {
      const double* src = *v;
      TRY(dev_alloc(ctx, v, (size_t)ctx->m));
      HIP_TRY(hipMemcpyAsync(*v, src, mb, hipMemcpyDeviceToDevice, s));
    }
    ctx->rows_aliased = false;
    ctx->rows_private = true;  // (until pdlpdev_clone_shared makes another clone of this context: that one aliases the new arrays)
    for (auto& kv : ctx->graphs) (void)hipGraphExecDestroy(kv.second);  // (the attempt graphs carry the old arrays' addresses)
    ctx->graphs.clear();
  }
  TRY(put(lo, ctx->lo_u, ctx->lo, mb));
  TRY(put(hi, ctx->hi_u, ctx->hi, mb));
  if (lb || ub || lo || hi)
    k_scale_bounds<<<grid_for(std::max(ctx->m, ctx->n)), kBlock, 0, s>>>(ctx->n, ctx->m, lb ? ctx->lb : nullptr, ub ? ctx->ub : nullptr,
                                                                      ctx->dc, lo ? ctx->lo : nullptr, hi ? ctx->hi : nullptr, ctx->dr);
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(hipMemsetAsync(ctx->x[i], 0, nb, s));
    HIP_TRY(hipMemsetAsync(ctx->aty[i], 0, nb, s));
    HIP_TRY(hipMemsetAsync(ctx->rc[i], 0, nb, s));
    HIP_TRY(hipMemsetAsync(ctx->y[i], 0, mb, s));
  }
  for (double* v : {ctx->xbar, ctx->sumx, ctx->avgx, ctx->lrx}) HIP_TRY(hipMemsetAsync(v, 0, nb, s));
  for (double* v : {ctx->sumy, ctx->avgy, ctx->lry}) HIP_TRY(hipMemsetAsync(v, 0, mb, s));
  HIP_TRY(hipMemsetAsync(ctx->ctl, 0, sizeof(pdlpdev_ctl), s));
  if (ctx->halpern) {  // (the mode stays; its anchor and scalars go back to their state after scaling)
    HIP_TRY(hipMemsetAsync(ctx->lraty, 0, nb, s));
    k_halpern_clear<<<1, 1, 0, s>>>(ctx->hal);
  }
  LAUNCH_CHECK();
  return 0;
}
// A new objective for the SAME matrix and bounds (the feasibility pump's distance objectives, feasibility_pump.cu:145-249): one upload
// into c_u, one kernel that scales it into c (k_scale_vectors' expression) and leaves the partials of both sums of squares, one
// k_finalize.  Both arrays are overwritten in place -- every kernel argument list and captured graph keeps reading the same addresses --
// and D_c depends on A only, so nothing else of the context moves.  sums = {sum c_u^2, sum c^2}: the bits reduce_vec(1, n, c_u / c) gives.
__global__ void __launch_bounds__(kBlock) k_set_objective(int n, double* c_u, double* c, const double* __restrict__ dc, double* __restrict__ part)
{
  __shared__ double red[8];
  set_objective_block(n, c_u, c_u, c, dc, part, blockIdx.x, gridDim.x, red);
}
int pdlpdev_set_objective(pdlpdev_ctx* ctx, const double* c, double sums[2])
{
  if (!ctx || !c) return fail(-1, "pdlpdev_set_objective: null argument");
  // c and c_u belong to the part a clone shares: refused, before anything is written, wherever they are not this context's alone
  if (ctx->clones_alive > 0) return fail(-7, "pdlpdev_set_objective: %d live clone(s) share this context's objective", ctx->clones_alive);
  if (ctx->shared_with_parent) return fail(-7, "pdlpdev_set_objective: a clone shares its parent's objective");
  if (ctx->lockstep_batches_alive > 0) return fail(-7, "pdlpdev_set_objective: a member of a lockstep batch (pdlpdev_batch_*) shares the batch's objective");
  if (ctx->comm) return fail(-7, "pdlpdev_set_objective: sharded contexts are not supported");
  if (!ctx->scaled) return fail(-1, "pdlpdev_set_objective: the problem has not been scaled yet");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int n   = ctx->n;
  if (n > 0) HIP_TRY(hipMemcpyAsync(ctx->c_u, c, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
  const int g = std::min(grid_for(n), kGenericBlocks);  // (reduce_vec's grid: the same partials)
  k_set_objective<<<g, kBlock, 0, s>>>(n, ctx->c_u, ctx->c, ctx->dc, ctx->part_g);
  k_finalize<<<1, kBlock, 0, s>>>(ctx->part_g, g, 2, 0u, ctx->scal);
  LAUNCH_CHECK();
  TRY(fetch_scalars(ctx, 2));
  if (sums) sums[0] = ctx->scal_h[0], sums[1] = ctx->scal_h[1];
  return 0;
}
// out[0] = sum c_j^2, out[1] = sum bcomb_i^2 of the scaled (unscaled != 0: the user's) problem
int pdlpdev_weight_norms(pdlpdev_ctx* ctx, int unscaled, double out[2])
{
  HIP_TRY(hipSetDevice(ctx->device));
  TRY(reduce_vec(ctx, 1, ctx->n, unscaled ? ctx->c_u : ctx->c, nullptr, 1));
  TRY(reduce_vec(ctx, 2, ctx->m, unscaled ? ctx->lo_u : ctx->lo, unscaled ? ctx->hi_u : ctx->hi, 2));
  TRY(allreduce(ctx, ctx->scal + 2, 1, rccl::kSum));
  TRY(fetch_scalars(ctx, 3));
  out[0] = ctx->scal_h[1], out[1] = ctx->scal_h[2];
  return 0;
}


int pdlpdev_problem_norms(pdlpdev_ctx* ctx, double* norm_c, double* norm_b)
{
  HIP_TRY(hipSetDevice(ctx->device));
  TRY(reduce_vec(ctx, 1, ctx->n, ctx->c_u, nullptr, 0));
  TRY(reduce_vec(ctx, 2, ctx->m, ctx->lo_u, ctx->hi_u, 1));
  TRY(allreduce(ctx, ctx->scal + 1, 1, rccl::kSum));
  TRY(fetch_scalars(ctx, 2));
  if (norm_c) *norm_c = sqrt(ctx->scal_h[0]);
  if (norm_b) *norm_b = sqrt(ctx->scal_h[1]);
  return 0;
}

int pdlpdev_set_step_params(pdlpdev_ctx* ctx, const pdlpdev_step_params* p)
{
  ctx->sp = *p;
  for (auto& kv : ctx->graphs) (void)hipGraphExecDestroy(kv.second);  // parameters are baked in
  ctx->graphs.clear();
  return 0;
}
int pdlpdev_set_step(pdlpdev_ctx* ctx, double step_size, double primal_weight)
{
  HIP_TRY(hipSetDevice(ctx->device));
  ctx->ctl_h_current = false;
  k_set_step<<<1, 1, 0, ctx->stream>>>(ctx->ctl, step_size, primal_weight);
  LAUNCH_CHECK();
  return 0;
}
int pdlpdev_set_k(pdlpdev_ctx* ctx, int32_t k)
{
  HIP_TRY(hipSetDevice(ctx->device));
  ctx->ctl_h_current = false;
  k_set_k<<<1, 1, 0, ctx->stream>>>(ctx->ctl, k);
  LAUNCH_CHECK();
  return 0;
}
int pdlpdev_set_initial(pdlpdev_ctx* ctx, const double* x, const double* y)
{
  HIP_TRY(hipSetDevice(ctx->device));
  TRY(fetch_ctl(ctx, nullptr));
  ctx->aty_valid = false;
  const int cur = ctx->ctl_h->cur;
  if (x) {
    HIP_TRY(hipMemcpyAsync(ctx->x[cur], x, (size_t)ctx->n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    k_div_inplace<<<grid_for(ctx->n), kBlock, 0, ctx->stream>>>(ctx->n, ctx->x[cur], ctx->dc);
  }
  if (y) {
    HIP_TRY(hipMemcpyAsync(ctx->y[cur], y, (size_t)ctx->m * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    k_div_inplace<<<grid_for(ctx->m), kBlock, 0, ctx->stream>>>(ctx->m, ctx->y[cur], ctx->dr);
  }
  LAUNCH_CHECK();
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}
}  // extern "C"
extern "C" {
// update_step_size_on_initial_solution (pdlp.cu:878-948): the quantities of one compute_step_sizes call with
// delta_primal = x0, delta_dual = y' = y0 and a zero A^T y.  out = {interaction x0.(A^T y0), ||x0||^2, ||y0||^2, max|x0|,
// max|y0|}.
//   x0_unscaled == y0_unscaled == nullptr: on the SCALED iterate that set_initial left in the current buffers; leaves A^T y0
//     in the current A^T y buffer (which is what the loop needs next anyway).
//   both given (compute_initial_step_size_before_scaling, pdlp.cu:929-947): the caller's vectors as they came, against the
//     SCALED matrix; they pass through the next-iterate buffers, which the first attempt overwrites before it reads them,
//     and the current A^T y buffer is left alone.
int pdlpdev_initial_solution_stats(pdlpdev_ctx* ctx, double out[5], const double* x0_unscaled, const double* y0_unscaled)
{
  HIP_TRY(hipSetDevice(ctx->device));
  if ((x0_unscaled == nullptr) != (y0_unscaled == nullptr)) return fail(-1, "initial_solution_stats: both unscaled vectors or none");
  hipStream_t s = ctx->stream;
  const int n = ctx->n, m = ctx->m;
  TRY(fetch_ctl(ctx, nullptr));
  const int cur = ctx->ctl_h->cur;
  const double *xv = ctx->x[cur], *yv = ctx->y[cur], *atyv = ctx->aty[cur];
  if (x0_unscaled) {
    const int nxt = 1 - cur;
    HIP_TRY(hipMemcpyAsync(ctx->x[nxt], x0_unscaled, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ctx->y[nxt], y0_unscaled, (size_t)m * sizeof(double), hipMemcpyHostToDevice, s));
    double* prod = ctx->comm ? ctx->ar_buf : ctx->aty[nxt];
    launch_plain(ctx, 1, ctx->y[nxt], prod);
    LAUNCH_CHECK();
    if (ctx->comm) TRY(allreduce(ctx, prod, (size_t)n, rccl::kSum));
    xv = ctx->x[nxt], yv = ctx->y[nxt], atyv = prod;
  } else {
    TRY(pdlpdev_compute_aty(ctx));
  }
  const int g = std::min(grid_for(n), kGenericBlocks);
  k_dot<<<g, kBlock, 0, s>>>(n, xv, atyv, ctx->part_g);
  k_finalize<<<1, kBlock, 0, s>>>(ctx->part_g, g, 1, 0u, ctx->scal + 48);
  TRY(reduce_vec(ctx, 1, n, xv, nullptr, 49));
  TRY(reduce_vec(ctx, 1, m, yv, nullptr, 50));
  TRY(reduce_vec(ctx, 0, n, xv, nullptr, 51));
  TRY(reduce_vec(ctx, 0, m, yv, nullptr, 52));
  LAUNCH_CHECK();
  if (ctx->comm) {  // the dual side is sharded
    TRY(allreduce(ctx, ctx->scal + 50, 1, rccl::kSum));
    TRY(allreduce(ctx, ctx->scal + 52, 1, rccl::kMax));
  }
  HIP_TRY(hipMemcpyAsync(ctx->scal_h + 48, ctx->scal + 48, 5 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int i = 0; i < 5; ++i) out[i] = ctx->scal_h[48 + i];
  return 0;
}

int pdlpdev_project_primal(pdlpdev_ctx* ctx)
{
  HIP_TRY(hipSetDevice(ctx->device));
  TRY(fetch_ctl(ctx, nullptr));
  const int cur = ctx->ctl_h->cur;
  k_clamp<<<grid_for(ctx->n), kBlock, 0, ctx->stream>>>(ctx->n, ctx->x[cur], ctx->lb, ctx->ub);
  k_clamp<<<grid_for(ctx->n), kBlock, 0, ctx->stream>>>(ctx->n, ctx->avgx, ctx->lb, ctx->ub);
  LAUNCH_CHECK();
  return 0;
}

// ---- hot loop -------------------------------------------------------------------------------------
}  // extern "C"
extern "C" {
int pdlpdev_compute_aty(pdlpdev_ctx* ctx)
{
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (!ctx->comm) {
    launch_at_cur(ctx, nullptr, 0);
    LAUNCH_CHECK();
  } else {
    launch_at_cur(ctx, ctx->ar_buf, 0);
    LAUNCH_CHECK();
    TRY(allreduce(ctx, ctx->ar_buf, (size_t)ctx->n, rccl::kSum));
    TRY(fetch_ctl(ctx, nullptr));
    HIP_TRY(hipMemcpyAsync(ctx->aty[ctx->ctl_h->cur], ctx->ar_buf, (size_t)ctx->n * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  return 0;
}


// the products of an attempt and the plain ones, each in its side's layout (launch_product)
static inline HalpernArgs halpern_args(const pdlpdev_ctx* ctx) { return HalpernArgs{ctx->hal, ctx->avgx, ctx->avgy, ctx->lrx, ctx->lry, ctx->lraty}; }
// (Halpern mode: the twins' kernels; its A^T product gathers y' from its own buffer, which the kernels take inside HalpernArgs)
// Zero skip (CUOPT_AMD_TUNE=zero_skip, pdlp_ctx.hpp): the bitmap of xbar's non-zeros that k_primal writes and k_panel_a_dual<false> reads in
// the attempts of a single-GPU context in the averaging modes whose A is in the row-sum panels (of any slab width: the layout is
// the one it would be without the bitmap); null everywhere else (sharded dataflows hand k_primal slices, Halpern mode has its own products).  Both launches of an
// attempt ask here, so the bits a product reads are always those of the xbar it gathers.
static unsigned long long* attempt_xmask(const pdlpdev_ctx* ctx)
{
  const pdlpdev_ctx::Panels& pn = ctx->A.pan;
  if (!ctx->xmask || ctx->comm || ctx->owner || ctx->rsag || ctx->halpern) return nullptr;
  if (ctx->A.layout() != pdlpdev_ctx::MatrixSide::kPanel || pn.v.seg) return nullptr;
  return ctx->xmask;
}
// k_primal on a slice of the columns; push (direct peer transport): xbar of the slice also lands in the peers' blocks
static void launch_primal_slice(pdlpdev_ctx* ctx, const ColSlice& sl, const p2pdev::Push* push)
{
  launch_k(ctx, k_primal, grid_for(sl.len), kBlock, 0, sl.len, ctx->ctl, ctx->x[0] + sl.cs, ctx->x[1] + sl.cs, ctx->aty[0] + sl.cs, ctx->aty[1] + sl.cs, ctx->c + sl.cs,
           ctx->lb + sl.cs, ctx->ub + sl.cs, ctx->xbar + sl.cs, ctx->sumx + sl.cs, push, ctx->ubd);
}
// the primal step of all columns: with the bitmap where the A product reads it (single GPU), else the kernel as it always was
static void launch_primal(pdlpdev_ctx* ctx)
{
  const int n = ctx->n;
  if (unsigned long long* xmask = attempt_xmask(ctx))
    return launch_k(ctx, k_primal_zs, grid_for(n), kBlock, 0, n, ctx->ctl, ctx->x[0], ctx->x[1], ctx->aty[0], ctx->aty[1], ctx->c, ctx->lb, ctx->ub, ctx->xbar, ctx->sumx, ctx->ubd, xmask, ctx->zcount);
  launch_primal_slice(ctx, ColSlice{0, n}, nullptr);
}
static void launch_a_dual(pdlpdev_ctx* ctx, double* ycopy = nullptr, const p2pdev::Push* push = nullptr)
{
  ctx->A.pan.v.zmask = attempt_xmask(ctx), ctx->A.pan.v.zcols = ctx->n, ctx->A.pan.v.zforce = ctx->zs_mode == 2;  // (the view travels by value with every launch)
  const Gathered g = Gathered::fixed(ctx->xbar, true);
  const auto pre  = std::make_tuple(ctx->ctl);
  const auto vecs = std::make_tuple(ctx->xbar);
  if (ctx->halpern && ycopy)  // (a rank of a sharded Halpern solve: y' also into the gathered dual and, with `push`, the peers' blocks)
    (void)launch_product(ctx, ctx->A, products::a_halpern_sharded, g, pre, vecs, std::make_tuple(ctx->y[0], ctx->y[1], ctx->lo, ctx->hi, halpern_args(ctx), ctx->A.part, ycopy, push));
  else if (ctx->halpern) (void)launch_product(ctx, ctx->A, products::a_halpern, g, pre, vecs, std::make_tuple(ctx->y[0], ctx->y[1], ctx->lo, ctx->hi, halpern_args(ctx), ctx->A.part));
  else (void)launch_product(ctx, ctx->A, products::a_dual, g, pre, vecs, std::make_tuple(ctx->y[0], ctx->y[1], ctx->lo, ctx->hi, ctx->sumy, ctx->A.part, ycopy, push));
}
static void launch_at_step(pdlpdev_ctx* ctx)
{
  const auto pre = std::make_tuple(ctx->ctl);
  if (ctx->halpern)
    (void)launch_product(ctx, ctx->At, products::at_halpern, Gathered::fixed(ctx->avgy, true), pre, std::make_tuple(),
                         std::make_tuple(ctx->x[0], ctx->x[1], ctx->aty[0], ctx->aty[1], halpern_args(ctx), ctx->At.part));
  else  // y' = the trial dual
    (void)launch_product(ctx, ctx->At, products::at_step, Gathered::trial(ctx->y[0], ctx->y[1], true), pre, std::make_tuple(ctx->y[0], ctx->y[1]),
                         std::make_tuple(ctx->x[0], ctx->x[1], ctx->aty[0], ctx->aty[1], ctx->At.part));
}
void launch_at_cur(pdlpdev_ctx* ctx, double* out_override, int use_next)
{
  (void)launch_product(ctx, ctx->At, products::at_cur, use_next ? Gathered::trial(ctx->y[0], ctx->y[1]) : Gathered::current(ctx->y[0], ctx->y[1]), std::make_tuple(ctx->ctl),
                       std::make_tuple(ctx->y[0], ctx->y[1]), std::make_tuple(ctx->aty[0], ctx->aty[1], out_override, use_next));
}
// plain y = A x (transpose = 0) or y = A^T x through the layout the solver iterates with
void launch_plain(pdlpdev_ctx* ctx, int transpose, const double* vec, double* out)
{
  (void)launch_product(ctx, transpose ? ctx->At : ctx->A, products::plain, Gathered::fixed(vec), std::make_tuple(), std::make_tuple(vec), std::make_tuple(out));
}
// the decision of the attempt that ran with the block at ctx->ctl, into `out`; zc: the counts its primal step left, nb_z of them
static void launch_decision_into(pdlpdev_ctx* ctx, pdlpdev_ctl* out, const int* zc, int nb_z)
{
  if (attempt_xmask(ctx))
    return launch_k(ctx, k_step_decision_zs, 1, kDecisionThreads, 0, ctx->ctl, out, ctx->A.part, ctx->A.partials(), ctx->At.part, ctx->At.partials(), ctx->sp, zc, nb_z,
                    ctx->n, ctx->zs_mode);
  launch_k(ctx, k_step_decision, 1, kDecisionThreads, 0, ctx->ctl, out, ctx->A.part, ctx->A.partials(), ctx->At.part, ctx->At.partials(), nullptr, ctx->sp);
}
static void launch_decision(pdlpdev_ctx* ctx)
{
  if (ctx->halpern) return launch_k(ctx, k_halpern_decision, 1, kDecisionThreads, 0, ctx->ctl, ctx->hal, ctx->A.part, ctx->A.partials(), ctx->At.part, ctx->At.partials());
  launch_decision_into(ctx, ctx->ctl, ctx->zcount, grid_for(ctx->n));
}
// the primal step of all columns behind the decision of the attempt that ran with the block at `in` (k_primal_decide); the decided block
// goes to `out`, this step's counts to zc_out
static void launch_primal_decide(pdlpdev_ctx* ctx, const pdlpdev_ctl* in, pdlpdev_ctl* out, const int* zc_in, int nb_z, int* zc_out)
{
  const int n = ctx->n;
  if (unsigned long long* xmask = attempt_xmask(ctx))
    return launch_k(ctx, k_primal_decide_zs, primal_decide_grid(n, ctx->primal_decide_grid_cap), kDecisionThreads, 0, n, in, out, ctx->x[0], ctx->x[1], ctx->aty[0], ctx->aty[1], ctx->c, ctx->lb, ctx->ub,
                    ctx->xbar, ctx->sumx, ctx->ubd, xmask, zc_out, ctx->A.part, ctx->A.partials(), ctx->At.part, ctx->At.partials(), ctx->sp, zc_in, nb_z, ctx->zs_mode);
  launch_k(ctx, k_primal_decide, primal_decide_grid(n, ctx->primal_decide_grid_cap), kDecisionThreads, 0, n, in, out, ctx->x[0], ctx->x[1], ctx->aty[0], ctx->aty[1], ctx->c, ctx->lb, ctx->ub, ctx->xbar,
           ctx->sumx, ctx->ubd, ctx->A.part, ctx->A.partials(), ctx->At.part, ctx->At.partials(), ctx->sp);
}

// owner-computes dataflow: A^T y' of this rank's columns from the gathered y' (complete sums) + the step statistics of the slice
static void launch_oc_step(pdlpdev_ctx* ctx, const ColSlice& sl)
{
  const size_t cs = sl.cs;
  double *x0 = ctx->x[0] + cs, *x1 = ctx->x[1] + cs, *t0 = ctx->aty[0] + cs, *t1 = ctx->aty[1] + cs;
  const double* yg = ctx->ygather;  // the trial dual of every rank, whichever ping-pong buffer it lives in
  if (ctx->halpern) {
    // the Halpern twin gathers y' of every rank from the gathered dual; T(z^k)'s primal half (x' of a run's last step), the anchor and its A^T y are offset
    // by the slice like the x / A^T y pairs.  Complete column sums on the owner: A^T y^{k+1} of a column is the linear combination
    // of the bits an unsharded step combines.
    const HalpernArgs h{ctx->hal, ctx->ar_buf + cs /* run_epilogue takes it to the average slot */, const_cast<double*>(yg), ctx->lrx + cs, ctx->lry, ctx->lraty + cs};
    (void)launch_product(ctx, ctx->Oc, products::at_halpern, Gathered::fixed(yg, true), std::make_tuple(ctx->ctl), std::make_tuple(),
                         std::make_tuple(x0, x1, t0, t1, h, ctx->Oc.part));
    return;
  }
  (void)launch_product(ctx, ctx->Oc, products::at_step, Gathered::trial(yg, yg, true), std::make_tuple(ctx->ctl), std::make_tuple(yg, yg),
                       std::make_tuple(x0, x1, t0, t1, ctx->Oc.part));
}

// k_step_decision on sums a collective has reduced (the same bits on every rank): ||dy||^2 at dy2, the other two as nb_t partials at part_t
static void launch_decision_reduced(pdlpdev_ctx* ctx, const double* part_t, int nb_t, const double* dy2)
{
  launch_k(ctx, k_step_decision, 1, kDecisionThreads, 0, ctx->ctl, ctx->ctl, nullptr, 0, part_t, nb_t, dy2, ctx->sp);
}

// ---- one attempt, per dataflow.  Halpern mode (single GPU and owner-computes only): the launch helpers pick the twins' kernels, k_primal is the
// same, pending_avg stays 0.  Single GPU: 4 launches, the stages (id: PDLPDEV_K_*) in stream order; pdlpdev_time_kernel walks the same list.
struct AttemptStage { int id; void (*launch)(pdlpdev_ctx*); };
static const AttemptStage kSingleStages[4] = {{PDLPDEV_K_PRIMAL, launch_primal}, {PDLPDEV_K_SPMV_A_DUAL, [](pdlpdev_ctx* c) { launch_a_dual(c); }},
                                              {PDLPDEV_K_SPMV_AT_STEP, launch_at_step}, {PDLPDEV_K_STEP_DECISION, launch_decision}};
static int enqueue_single(pdlpdev_ctx* ctx)
{
  for (const AttemptStage& st : kSingleStages) st.launch(ctx);
  LAUNCH_CHECK();
  return 0;
}
// A chunk of N attempts on the single GPU in the averaging modes (CUOPT_AMD_TUNE=primal_decides, pdlp_ctx.hpp): 3 N + 1 launches,
//     primal,        a_dual, at_step        attempt 1: reads ctx->ctl, like the attempt above
//     primal_decide, a_dual, at_step        attempts 2 .. N: the decision of the attempt before at the head of the primal step
//     decision                              the last attempt's, into ctx->ctl
// N = 1 is the attempt above, launch for launch.  The decided blocks go from one of the two scratch blocks to the other: attempt k's
// primal_decide reads the block attempt k - 1 ran with and writes the other one, which its own products and the next decision read;
// nothing outside the chunk ever sees them, and the last decision always leaves ctx->ctl current (step_decision_workgroup).  The counts
// of xbar's non-zeros alternate between two buffers the same way: a primal step reads the previous one's for the decision while its
// own workgroups write theirs.  Stream order between the kernels is all the synchronisation there is.
// (While the chunk is enqueued ctx->ctl points at the block the launches of the attempt in hand read -- the launch helpers, the dense
//  prologue and phase P of the gather-free layout all take it from there --; ChunkBlocks puts the loop's own block back.)
static bool chunk_decides_in_primal(const pdlpdev_ctx* ctx) { return ctx->primal_decides && !ctx->halpern && !ctx->comm && !ctx->small_resident && ctx->n > 0; }
// the chunk's scratch blocks and second count buffer: on first use, never inside a stream capture
static int chunk_blocks_ready(pdlpdev_ctx* ctx)
{
  if (!chunk_decides_in_primal(ctx) || ctx->chunk_ctl[0]) return 0;
  TRY(dev_alloc(ctx, &ctx->chunk_ctl[0], 1));
  TRY(dev_alloc(ctx, &ctx->chunk_ctl[1], 1));
  if (ctx->zcount) {  // (primal_decide_grid(n, cap) <= grid_for(n))
    TRY(dev_alloc(ctx, &ctx->zcount_alt, (size_t)grid_for(ctx->n)));
  }
  return 0;
}
static int enqueue_single_chunk(pdlpdev_ctx* ctx, int attempts)
{
  if (!chunk_decides_in_primal(ctx) || attempts == 1) {
    for (int k = 0; k < attempts; ++k) TRY(enqueue_single(ctx));
    return 0;
  }
  if (!ctx->chunk_ctl[0]) return fail(-1, "enqueue_single_chunk: chunk_blocks_ready was not called");
  struct ChunkBlocks {
    pdlpdev_ctx* c;
    pdlpdev_ctl* const home;
    ~ChunkBlocks() { c->ctl = home; }
  } blocks{ctx, ctx->ctl};
  int* const zc[2] = {ctx->zcount, ctx->zcount_alt};
  int nb_z         = grid_for(ctx->n);  // the counts the primal step in hand leaves in zc[k & 1]
  for (int k = 0; k < attempts; ++k) {
    if (k == 0) {
      launch_primal(ctx);
    } else {
      pdlpdev_ctl* const decided = ctx->chunk_ctl[k & 1];
      launch_primal_decide(ctx, ctx->ctl, decided, zc[(k - 1) & 1], nb_z, zc[k & 1]);
      ctx->ctl = decided;
      nb_z     = primal_decide_grid(ctx->n, ctx->primal_decide_grid_cap);
    }
    launch_a_dual(ctx);
    launch_at_step(ctx);
  }
  launch_decision_into(ctx, blocks.home, zc[(attempts - 1) & 1], nb_z);
  LAUNCH_CHECK();
  return 0;
}
// Replicated primal: partial A^T y' of this row block -> ar_buf[0..n), ||dy||^2 partial -> ar_buf[n]; ONE all-reduce.  (Here and below a
// LAUNCH_CHECK stands in front of every collective: it decides what a failed capture leaves on the stream.)
static int enqueue_replicated(pdlpdev_ctx* ctx)
{
  const int n = ctx->n, g = std::min(grid_for(n), kGenericBlocks);
  launch_primal(ctx);
  launch_a_dual(ctx);
  launch_at_cur(ctx, ctx->ar_buf, 1);
  launch_k(ctx, k_sum_partials_to, 1, kBlock, 0, ctx->A.part, ctx->A.partials(), ctx->ar_buf + n);
  LAUNCH_CHECK();
  TRY(allreduce(ctx, ctx->ar_buf, (size_t)n + 1, rccl::kSum));
  launch_k(ctx, k_step_stats, g, kBlock, 0, n, g, ctx->ctl, ctx->ar_buf, ctx->x[0], ctx->x[1], ctx->aty[0], ctx->aty[1], ctx->part_g);
  launch_decision_reduced(ctx, ctx->part_g, g, ctx->ar_buf + n);
  LAUNCH_CHECK();
  return 0;
}
// Sliced primal (rsag): primal step on this rank's columns -> all-gather(xbar) -> local rows of A -> partial A^T y' ->
// reduce-scatter -> this rank's columns of A^T y' and of the step-size sums -> ONE 3-scalar all-reduce -> the same
// decision on every rank.  Same wire bytes as the all-reduce of the replicated dataflow, 1/world of its element-wise work.
static int enqueue_rsag(pdlpdev_ctx* ctx)
{
  const ColSlice sl = rank_slice(ctx);
  const int g       = std::min(grid_for(sl.len), kGenericBlocks);
  launch_primal_slice(ctx, sl, nullptr);
  LAUNCH_CHECK();
  TRY(all_gather(ctx, ctx->xbar, (size_t)ctx->slice));
  launch_a_dual(ctx);
  launch_at_cur(ctx, ctx->ar_buf, 1);
  LAUNCH_CHECK();
  TRY(reduce_scatter(ctx, ctx->ar_buf, ctx->rs_buf, (size_t)ctx->slice));
  launch_k(ctx, k_step_stats, g, kBlock, 0, sl.len, g, ctx->ctl, ctx->rs_buf, ctx->x[0] + sl.cs, ctx->x[1] + sl.cs, ctx->aty[0] + sl.cs, ctx->aty[1] + sl.cs, ctx->part_g);
  launch_k(ctx, k_pack_step_sums, 1, kBlock, 0, ctx->A.part, ctx->A.partials(), ctx->part_g, g, ctx->rs_scal);
  LAUNCH_CHECK();
  TRY(allreduce(ctx, ctx->rs_scal, 3, rccl::kSum));
  launch_decision_reduced(ctx, ctx->rs_scal + 1, 1, ctx->rs_scal);
  LAUNCH_CHECK();
  return 0;
}
// Owner-computes over collectives: xbar and y' travel whole or, on a structured LP, as the ranges the rows / columns reference (halo exchange)
static int enqueue_owner_collective(pdlpdev_ctx* ctx)
{
  const ColSlice sl = rank_slice(ctx);
  launch_primal_slice(ctx, sl, nullptr);
  LAUNCH_CHECK();
  TRY(ctx->halo.on ? halo_exchange(ctx, 0, ctx->xbar) : all_gather(ctx, ctx->xbar, (size_t)ctx->slice));
  launch_a_dual(ctx, ctx->ygather + (size_t)ctx->rank * ctx->ypad);
  LAUNCH_CHECK();
  TRY(ctx->halo.on ? halo_exchange(ctx, 1, ctx->ygather) : all_gather(ctx, ctx->ygather, (size_t)ctx->ypad));
  launch_oc_step(ctx, sl);
  launch_k(ctx, k_pack_step_sums, 1, kBlock, 0, ctx->A.part, ctx->A.partials(), ctx->Oc.part, ctx->Oc.partials(), ctx->rs_scal);
  LAUNCH_CHECK();
  TRY(allreduce(ctx, ctx->rs_scal, 3, rccl::kSum));
  if (ctx->halpern) launch_k(ctx, k_halpern_decision_sums, 1, 1, 0, ctx->ctl, ctx->hal, ctx->rs_scal);
  else launch_decision_reduced(ctx, ctx->rs_scal + 1, 1, ctx->rs_scal);
  LAUNCH_CHECK();
  return 0;
}
// Owner-computes over the direct peer transport: peer stores + epoch flags instead of collectives.  The producing kernels (primal step, dual
// step, decision with its step-size sums) store into every rank's landing block and raise this rank's flag from their last workgroup; a
// consumer waits for the world flags and copies the landed vector into ordinary memory.  Six launches, nothing between them but stream order.
static const unsigned long long* p2p_flags(const pdlpdev_ctx::P2P& P) { return reinterpret_cast<const unsigned long long*>(P.base + P.off_f); }
// what landed of kind 0 (xbar) / 1 (the gathered y') -> dst: the other ranks' per_rank entries or, with the halo exchange, the stored ranges only
static void p2p_pull(pdlpdev_ctx* ctx, int kind, double* dst, size_t land_off, int per_rank)
{
  pdlpdev_ctx::P2P& P = ctx->p2p;
  const double* land  = reinterpret_cast<const double*>(P.base + land_off);
  if (ctx->halo.on) {
    p2pdev::PullRanges R{};
    int most = 0;
    for (int q = 0; q < ctx->world; ++q) R.off[q] = ctx->halo.recv_off[kind][q], R.cnt[q] = ctx->halo.recv_cnt[kind][q], most = std::max(most, R.cnt[q]);
    return launch_k(ctx, p2pdev::k_pull_ranges, std::max(1, std::min((most + 255) / 256, 64)), 256, 0, ctx->ctl, dst, land, R, p2p_flags(P), ctx->world, kind, P.epoch,
                    P.fault, P.push_dev + kind);
  }
  const int count = ctx->world * per_rank, remote = count - per_rank;  // (this rank's own entries: the producing kernel's ordinary store)
  const int g     = std::max(1, std::min((remote + 4095) / 4096, 1024));
  launch_k(ctx, p2pdev::k_pull, g, 256, 0, ctx->ctl, dst, land, count, ctx->rank * per_rank, per_rank, p2p_flags(P), ctx->world, kind, P.epoch, P.fault, P.push_dev + kind);
}
static int enqueue_owner_p2p(pdlpdev_ctx* ctx)
{
  pdlpdev_ctx::P2P& P = ctx->p2p;
  const ColSlice sl   = rank_slice(ctx);
  const double* sums  = reinterpret_cast<const double*>(P.base + P.off_s);
  launch_primal_slice(ctx, sl, P.push_dev);
  LAUNCH_CHECK();
  p2p_pull(ctx, 0, ctx->xbar, P.off_x, ctx->slice);
  launch_a_dual(ctx, ctx->ygather + (size_t)ctx->rank * ctx->ypad, P.push_dev + 1);
  p2p_pull(ctx, 1, ctx->ygather, P.off_y, ctx->ypad);
  launch_oc_step(ctx, sl);
  if (ctx->halpern) launch_k(ctx, k_halpern_decision_p2p, 1, kBlock, 0, ctx->ctl, ctx->hal, ctx->A.part, ctx->A.partials(), ctx->Oc.part, ctx->Oc.partials(), sums, p2p_flags(P),
                             ctx->world, P.epoch, P.fault, P.push_dev + 2);
  else launch_k(ctx, k_step_decision_p2p, 1, kBlock, 0, ctx->ctl, ctx->A.part, ctx->A.partials(), ctx->Oc.part, ctx->Oc.partials(), sums, p2p_flags(P), ctx->world, P.epoch,
                P.fault, ctx->sp, P.push_dev + 2);
  LAUNCH_CHECK();
  return 0;
}

// one PDHG attempt on ctx->stream: the sequence of the context's dataflow
static int enqueue_attempt(pdlpdev_ctx* ctx)
{
  if (ctx->halpern && ctx->comm && !ctx->owner) return fail(-7, "reflected Halpern mode: behind a communicator the owner-computes dataflow only");
  if (ctx->owner && !ctx->Oc.hot.off) return fail(-1, "owner-computes dataflow: pdlpdev_owner_setup was not called");
  if (ctx->owner) return ctx->p2p.on ? enqueue_owner_p2p(ctx) : enqueue_owner_collective(ctx);
  if (ctx->rsag) return enqueue_rsag(ctx);
  return ctx->comm ? enqueue_replicated(ctx) : enqueue_single(ctx);
}
// a chunk of attempts that go out together (one graph, or the plain launches of a round): the single GPU has a sequence for the chunk
static int enqueue_chunk(pdlpdev_ctx* ctx, int attempts)
{
  if (!ctx->comm && !ctx->owner && !ctx->rsag) return enqueue_single_chunk(ctx, attempts);
  for (int i = 0; i < attempts; ++i) TRY(enqueue_attempt(ctx));
  return 0;
}

static int get_graph(pdlpdev_ctx* ctx, int attempts, hipGraphExec_t* out)
{
  auto it = ctx->graphs.find(attempts);
  if (it != ctx->graphs.end()) {
    *out = it->second;
    return 0;
  }
  TRY(chunk_blocks_ready(ctx));
  hipGraph_t graph;
  HIP_TRY(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
  const int rc = enqueue_chunk(ctx, attempts);
  hipError_t e = hipStreamEndCapture(ctx->stream, &graph);
  if (rc != 0) return rc;
  HIP_TRY(e);
  hipGraphExec_t exec;
  HIP_TRY(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
  HIP_TRY(hipGraphDestroy(graph));
  ctx->graphs[attempts] = exec;
  *out                  = exec;
  return 0;
}

// `count` attempts on ctx->stream: replays of the attempt graphs (powers of two up to 64) or plain launches
static int enqueue_attempts(pdlpdev_ctx* ctx, int remaining)
{
  // Sharded solves over RCCL replay attempt graphs too: the collectives are captured with the kernels around them (round 4:
  // tools/rccl_capture_repro.cpp captures ncclAllGather + ncclAllReduce in every capture mode with both RCCL builds of this image,
  // and bench.py --force-comm runs the owner dataflow through captured graphs at one rank; round 3's crash inside the capture did
  // not reproduce after the prune).  A capture that fails is remembered and the solver goes on with plain launches -- the same
  // sequence of collectives, so ranks that took different paths still meet.  The in-process communicator synchronises on the
  // host and can never be captured; the direct peer transport is kernels only.
  const bool rccl_graphs = ctx->comm && !ctx->p2p.on && !ctx->soft && !ctx->graph_comm_failed;
  bool replayed = false;
  if (rccl_graphs && ctx->use_graph && !ctx->comm_warm) {
    // the very first attempt of a solver over RCCL goes out as plain launches: whatever a collective sets up lazily on its first call
    // (channels, proxies) must not happen inside a stream capture
    TRY(enqueue_attempt(ctx));
    ctx->comm_warm = true;
    remaining -= 1;
  }
  if (ctx->use_graph && (!ctx->comm || ctx->p2p.on || rccl_graphs)) {
    replayed = true;
    while (remaining > 0) {
      const int chunk = attempt_chunk(remaining);
      hipGraphExec_t g;
      const int grc = get_graph(ctx, chunk, &g);
      if (grc != 0 && rccl_graphs) {  // (nothing of this chunk was enqueued: a failed capture leaves the stream empty)
        ctx->graph_comm_failed = true;
        (void)hipGetLastError();
        replayed = false;
        break;
      }
      TRY(grc);
      HIP_TRY(hipGraphLaunch(g, ctx->stream));
      remaining -= chunk;
    }
  }
  if (!replayed && remaining > 0) {  // (plain launches: what is left of the round is one chunk)
    TRY(chunk_blocks_ready(ctx));
    TRY(enqueue_chunk(ctx, remaining));
  }
  return 0;
}

// what `enqueued` attempts behind `before` accepted steps and `attempts_before` attempts left, from the fresh ctl_h (a Halpern burst asks too)
static void note_attempts(pdlpdev_ctx* ctx, int before, int attempts_before, int enqueued)
{
  const pdlpdev_ctl& c = *ctx->ctl_h;
  const int made       = c.attempts - attempts_before;  // an attempt that found the target reached (or an error raised) did nothing
  if (!ctx->comm) ctx->stat_empty_attempts += enqueued - made;
  if (c.steps_taken > before && c.error == 0 && !ctx->comm) ctx->aty_valid = true;  // k_*_at_step stored A^T y' and the decision flipped to it
  if (c.error != 0) ctx->aty_valid = false;
}
static int after_round(pdlpdev_ctx* ctx, int before, int attempts_before, int enqueued, int counted /* towards the 64-in-a-row rule */)
{
  note_attempts(ctx, before, attempts_before, enqueued);
  if (ctx->p2p.on && ctx->ctl_h->error != 0) {  // a wait of the direct peer transport ran out of patience: a peer is gone
    int fault = 0;
    HIP_TRY(hipMemcpy(&fault, ctx->p2p.fault, sizeof(int), hipMemcpyDeviceToHost));
    if (fault) return fail(-6, "direct peer transport: rank %d waited 5 s for another rank's data (a peer failed or is stuck)", ctx->rank);
  }
  if (too_many_rejections(ctx, before, counted)) {
    k_set_error<<<1, 1, 0, ctx->stream>>>(ctx->ctl);
    LAUNCH_CHECK();
    TRY(fetch_ctl_counted(ctx, nullptr));
    ctx->aty_valid = false;
  }
  return 0;
}
// one round: `enqueue` attempts, ONE counted read-back of the control block, after_round; ctl_h is current on entry and on return
static int run_round(pdlpdev_ctx* ctx, int attempts_before, int enqueue, int counted)
{
  const int before = ctx->ctl_h->steps_taken;
  TRY(enqueue_attempts(ctx, enqueue));
  TRY(fetch_ctl_counted(ctx, nullptr));
  return after_round(ctx, before, attempts_before, enqueue, counted);
}

// rounds of attempts until the target is reached or the error flag is up; ctl_h is current on entry and on return
static int run_rounds(pdlpdev_ctx* ctx, int32_t target_steps, int* rounds)
{
  // Each attempt accepts at most one step, so `remaining` attempts can never overshoot; rejected
  // attempts are made up for in the next round (one control-block read per round, not per step).
  int guard = 0;
  while (ctx->ctl_h->error == 0 && ctx->ctl_h->steps_taken < target_steps) {
    const int asked = target_steps - ctx->ctl_h->steps_taken;
    TRY(run_round(ctx, ctx->ctl_h->attempts, asked, asked));
    if (++guard > 100000) return fail(-6, "pdlpdev_run: no progress");
  }
  if (rounds) *rounds += guard;
  return 0;
}
static int run_epilogue(pdlpdev_ctx* ctx, int rounds, pdlpdev_ctl* ctl)
{
  if (ctx->rsag && rounds > 0) {
    // back to replicated primal vectors for everything outside the loop (major iterations, snapshots, the solution): the
    // current x, its A^T y and the running sum are complete on their owners' slices only
    const int cur = ctx->ctl_h->cur;
    TRY(all_gather(ctx, ctx->x[cur], (size_t)ctx->slice));
    TRY(all_gather(ctx, ctx->aty[cur], (size_t)ctx->slice));
    if (ctx->halpern) {
      // (owner dataflow: the mode has no running sum.  x' of the run's last step -- the primal half of T(z^k), which the evaluation reads
      //  from the average slot -- is valid on the owners' slices only; it travels through ar_buf, which has the spare entries equal
      //  slices need and is free between attempts, and lands in the average slot, which has none: launch_oc_step)
      TRY(all_gather(ctx, ctx->ar_buf, (size_t)ctx->slice));
      HIP_TRY(hipMemcpyAsync(ctx->avgx, ctx->ar_buf, (size_t)ctx->n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    } else {
      TRY(all_gather(ctx, ctx->sumx, (size_t)ctx->slice));
    }
  }
  if (ctl) *ctl = *ctx->ctl_h;
  return 0;
}
// k_set_target, and the control block on the host: read back, unless the pinned copy is known to be what the device holds
static int set_target(pdlpdev_ctx* ctx, int32_t target_steps)
{
  k_set_target<<<1, 1, 0, ctx->stream>>>(ctx->ctl, target_steps);
  LAUNCH_CHECK();
  if (ctx->ctl_h_current && !ctx->comm) {
    ctx->ctl_h->target_steps = target_steps;
    return 0;
  }
  return fetch_ctl_counted(ctx, nullptr);
}

int pdlpdev_run(pdlpdev_ctx* ctx, int32_t target_steps, pdlpdev_ctl* ctl)
{
  roctx::Range range("pdlp: PDHG attempts");
  HIP_TRY(hipSetDevice(ctx->device));
  if (ctx->small_resident && !ctx->comm) {  // the whole loop inside one workgroup (kernels_resident.hip)
    TRY(ctx->halpern ? resident_halpern_run(ctx, target_steps) : resident_run(ctx, target_steps));
    if (ctl) *ctl = *ctx->ctl_h;
    return 0;
  }
  TRY(set_target(ctx, target_steps));
  int rounds = 0;
  TRY(run_rounds(ctx, target_steps, &rounds));
  return run_epilogue(ctx, rounds, ctl);
}

// Parity hook: `count` attempts as pdlpdev_run enqueues them (same kernels, graph replay or plain launches), one read-back, after_round's
// bookkeeping -- and NO make-up round, so a rejected attempt is there to be looked at: the trial iterate in the other side of the
// ping-pong pairs, the decision's inputs in the control block.  On the resident small-LP path: one launch of the one-workgroup loop
// capped at `count` attempts (resident_attempts); a rejected trial iterate stays in that kernel's registers.  On a sharded context
// every rank calls it with the same count; run_epilogue behind the round replicates the current side again (sliced dataflows).
int pdlpdev_debug_attempts(pdlpdev_ctx* ctx, int count, pdlpdev_ctl* ctl)
{
  HIP_TRY(hipSetDevice(ctx->device));
  const bool resident = ctx->small_resident && !ctx->comm && !ctx->halpern;
  if (ctx->halpern) return fail(-7, "pdlpdev_debug_attempts: the averaging attempt only, multi-launch, sharded or resident (not Halpern mode)");
  if (count < 1 || count > 64) return fail(-1, "pdlpdev_debug_attempts: count must be 1 .. 64");
  TRY(fetch_ctl(ctx, nullptr));  // (not one of the loop's synchronisations: the hook's own)
  if (resident) {
    TRY(resident_attempts(ctx, count));
    if (ctl) *ctl = *ctx->ctl_h;
    return 0;
  }
  TRY(set_target(ctx, ctx->ctl_h->steps_taken + count));
  int rounds = 0;
  if (ctx->ctl_h->error == 0) {  // (all-reduced scalars decide the error: every rank of a sharded context sees the same)
    TRY(run_round(ctx, ctx->ctl_h->attempts, count, count));
    rounds = 1;
  }
  return run_epilogue(ctx, rounds, ctl);
}

// One major-iteration period with ONE synchronisation: the attempts up to `target_steps`, a few spare ones (empty launches unless an
// attempt in front of them was rejected), and behind them the head of the major iteration that is due at the target (pdlpdev_major_eval's
// kernels, each of which does nothing unless the target was reached), then one read-back of the scalars and the control block.
// *evaluated = 1: the period was reached and out_current / out_average hold what pdlpdev_major_eval(rq) would have returned.
// *evaluated = 0: the attempts are done as pdlpdev_run does them (make-up rounds included) and NOTHING of the major iteration has
// happened -- the context is not eligible (sharded, resident in an averaging mode, a layout without guarded evaluation kernels,
// l-infinity residuals asked for, a control block the host does not hold), the period fell short, or the step error is up; the caller
// goes on the present way.
// A resident context in Halpern mode is always eligible and takes a branch of its own: the one-workgroup loop kernel with its target,
// the one-workgroup evaluation of T(z^k) guarded behind it (l-infinity residuals included), one synchronisation; *evaluated = 1 unless
// the step error came up or a launch hit its step cap.
int pdlpdev_run_period(pdlpdev_ctx* ctx, int32_t target_steps, const pdlpdev_small_eval* rq, pdlpdev_ctl* ctl,
                       double out_current[PDLPDEV_EV_COUNT], double out_average[PDLPDEV_EV_COUNT], int32_t* evaluated)
{
  *evaluated = 0;
  HIP_TRY(hipSetDevice(ctx->device));
  if (ctx->halpern && ctx->small_resident && !ctx->comm) {
    // the resident Halpern loop: the loop kernel with its target, the one-workgroup evaluation of T(z^k) right behind it (it computes
    // the l-infinity residuals itself, so that request stays on this path), one synchronisation for both
    roctx::Range range("pdlp: Halpern steps + evaluation (resident)");
    const bool want_linf = wants_linf(rq->eps_p, rq->eps_d);
    TRY(resident_halpern_period(ctx, target_steps, rq->rule_finite, want_linf ? 1 : 0, rq->eps_p, rq->eps_d, evaluated));
    if (*evaluated) {
      read_eval(ctx->scal_h + 32, want_linf, out_current);
      read_eval(ctx->scal_h + 32, want_linf, out_average);
    }
    if (ctl) *ctl = *ctx->ctl_h;
    return 0;
  }
  const bool eligible = !ctx->comm && has_guarded_eval(ctx) && ctx->ctl_h_current && !wants_linf(rq->eps_p, rq->eps_d) && ctx->ctl_h->error == 0 &&
                        ctx->ctl_h->steps_taken < target_steps;
  if (!eligible) return pdlpdev_run(ctx, target_steps, ctl);
  roctx::Range range("pdlp: PDHG attempts + major iteration evaluation");
  TRY(set_target(ctx, target_steps));
  const int before = ctx->ctl_h->steps_taken, attempts_before = ctx->ctl_h->attempts, asked = target_steps - before;
  const int spare = ctx->halpern ? 0 : ctx->spare_attempts;  // (a Halpern step never fails: a period is exactly `asked` steps)
  TRY(enqueue_attempts(ctx, asked));
  if (spare > 0) TRY(enqueue_attempts(ctx, spare));
  if (ctx->halpern) {
    TRY(enqueue_halpern_eval(ctx, rq->rule_finite, rq->eps_p, rq->eps_d, 1));
    if (ctx->halpern_rays) TRY(enqueue_halpern_ray(ctx, rq->rule_finite));  // (its scalars sit in front of kCtlSlot: the same read-back)
    HIP_TRY(hipMemcpyAsync(ctx->hal_h, ctx->hal, sizeof(pdlpdev_halpern), hipMemcpyDeviceToHost, ctx->stream));
  } else {
    TRY(enqueue_major_eval(ctx, rq->mode, rq->rule_finite, rq->eps_p, rq->eps_d, 1));
  }
  HIP_TRY(hipMemcpyAsync(ctx->scal_h, ctx->scal, kCtlSlot * sizeof(double) + sizeof(pdlpdev_ctl), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ctx->stat_loop_syncs += 1;
  memcpy(ctx->ctl_h, ctx->scal_h + kCtlSlot, sizeof(pdlpdev_ctl));
  ctx->ctl_h_current = true;
  // (a period with an accepted step and rejections: the attempts made beyond the accepted ones are the rejections)
  const int rejected  = (ctx->ctl_h->attempts - attempts_before) - (ctx->ctl_h->steps_taken - before);
  ctx->spare_attempts = std::max(0, std::min(rejected, 4));
  TRY(after_round(ctx, before, attempts_before, asked + spare, asked));
  int rounds = 1;
  if (ctx->ctl_h->error == 0 && ctx->ctl_h->steps_taken >= target_steps) {
    *evaluated = 1;
    read_major_eval(ctx, out_current, out_average);
  } else {
    if (ctx->ctl_h->error == 0 && ctx->ctl_h->steps_taken == before && spare > 0 && spare < asked) {
      // nothing was accepted: the spare attempts were the first ones of the make-up round pdlpdev_run would enqueue now; the rest of
      // that round follows, so that the 64-in-a-row rule sees the rounds -- and stops after the number of attempts -- it always did
      TRY(run_round(ctx, attempts_before + asked + spare, asked - spare, asked));
      rounds += 1;
    }
    TRY(run_rounds(ctx, target_steps, &rounds));
  }
  return run_epilogue(ctx, rounds, ctl);
}

// ---- bursts of device-decided major iterations (cuoptamd_settings::halpern_device_major; kernels: kernels_halpern_major.hip) ----------
int pdlpdev_set_halpern_device_major(pdlpdev_ctx* ctx, int on)
{
  HIP_TRY(hipSetDevice(ctx->device));
  if (!on) return 0;
  if (!ctx->halpern || ctx->comm) return fail(-7, "pdlpdev_set_halpern_device_major: reflected Halpern mode on one GPU only");
  if (!ctx->hmaj) TRY(dev_alloc(ctx, &ctx->hmaj, 1));
  if (!ctx->hmaj_ring) HIP_TRY(hipHostMalloc((void**)&ctx->hmaj_ring, 16 * sizeof(pdlpdev_halpern_major_record)));
  return 0;
}
int pdlpdev_halpern_burst_eligible(pdlpdev_ctx* ctx, const pdlpdev_small_eval* rq)
{
  if (!ctx->halpern || ctx->comm || ctx->halpern_rays) return 0;
  if (ctx->small_resident) return 1;
  return has_guarded_eval(ctx) && !wants_linf(rq->eps_p, rq->eps_d) ? 1 : 0;
}
int pdlpdev_halpern_burst_stats(pdlpdev_ctx* ctx, int64_t out[4])
{
  out[0] = ctx->burst_stats.bursts, out[1] = ctx->burst_stats.periods, out[2] = ctx->burst_stats.records, out[3] = ctx->burst_stats.empty;
  return 0;
}
// Per period, in stream order: the steps to the period's target (multi-launch: the guarded twin of k_set_target, then the attempt graphs
// as pdlpdev_run_period replays them; resident: the loop kernel's body behind the guard), the guarded evaluation of T(z^k) that
// pdlpdev_run_period enqueues, k_halpern_major_decide, the guarded restart.  One synchronisation behind the last period.
int pdlpdev_run_halpern_burst(pdlpdev_ctx* ctx, int32_t first_target, int32_t period, int32_t count, const pdlpdev_small_eval* rq,
                              const pdlpdev_halpern_major_params* params, double theta, double r_prev,
                              pdlpdev_halpern_major_record* records, int32_t* written, double* r_prev_out, pdlpdev_ctl* ctl)
{
  roctx::Range range("pdlp: Halpern burst (steps + evaluation + decision + restart, P periods)");
  *written = 0;
  HIP_TRY(hipSetDevice(ctx->device));
  if (count < 1 || count > 16 || period < 1) return fail(-1, "pdlpdev_run_halpern_burst: 1 .. 16 periods of at least one step");
  if (!ctx->hmaj || !ctx->hmaj_ring) return fail(-7, "pdlpdev_run_halpern_burst: call pdlpdev_set_halpern_device_major first");
  if (!pdlpdev_halpern_burst_eligible(ctx, rq)) return fail(-7, "pdlpdev_run_halpern_burst: the context has no burst (the resident Halpern loop, or panels on both sides without an l-infinity request)");
  const bool resident = ctx->small_resident;
  // (something moved the control block behind the loop's back -- a cleared step error: read it, as set_target does)
  if (!ctx->ctl_h_current) TRY(fetch_ctl_counted(ctx, nullptr));
  const int before = ctx->ctl_h->steps_taken, attempts_before = ctx->ctl_h->attempts;
  if (ctx->ctl_h->error != 0 || before >= first_target || first_target - before > period || (resident && period > (1 << 14)))
    return fail(-7, "pdlpdev_run_halpern_burst: the first period must start inside (step error down, target ahead, at most one period away)");
  const bool want_linf = wants_linf(rq->eps_p, rq->eps_d);
  pdlpdev_halpern_major_params p = *params;
  p.want_linf = want_linf ? 1 : 0;
  halpern_burst_mark_ring(ctx->hmaj_ring, count);
  TRY(halpern_major_launch_arm(ctx, r_prev));
  int enqueued = 0;
  for (int j = 0; j < count; ++j) {
    const int32_t target = first_target + j * period;
    if (resident) {
      // (the one-workgroup evaluation writes the pinned block: scal_h is what the decision reads, and the host afterwards)
      TRY(halpern_major_launch_resident_period(ctx, target, rq->rule_finite, want_linf ? 1 : 0, rq->eps_p, rq->eps_d));
      TRY(halpern_major_launch_decide(ctx, ctx->scal_h + 32, p, target, ctx->hmaj_ring + j));
    } else {
      const int asked = j == 0 ? first_target - before : period;
      TRY(halpern_major_launch_set_target(ctx, target));
      TRY(enqueue_attempts(ctx, asked));
      enqueued += asked;
      TRY(enqueue_halpern_eval(ctx, rq->rule_finite, rq->eps_p, rq->eps_d, 1));
      TRY(halpern_major_launch_decide(ctx, ctx->scal + 32, p, target, ctx->hmaj_ring + j));
    }
    TRY(halpern_major_launch_restart(ctx, theta, ctx->hmaj_ring + j, resident ? 1 : 0));
  }
  if (!resident) {
    HIP_TRY(hipMemcpyAsync(ctx->hal_h, ctx->hal, sizeof(pdlpdev_halpern), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->ctl_h, ctx->ctl, sizeof(pdlpdev_ctl), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ctx->stat_loop_syncs += 1;
  ctx->ctl_h_current = true;
  ctx->burst_stats.bursts += 1, ctx->burst_stats.periods += count;
  if (halpern_burst_collect(ctx->hmaj_ring, count, r_prev, records, written, r_prev_out, &ctx->burst_stats))
    return fail(-6, "pdlpdev_run_halpern_burst: a record was written behind the period that stopped the burst");
  if (!resident) {
    note_attempts(ctx, before, attempts_before, enqueued);  // (k_*_at_halpern stored A^T y of z^{k+1})
    ctx->rejected_in_a_row = 0;                             // (a Halpern step never fails)
  }
  if (ctl) *ctl = *ctx->ctl_h;
  return 0;
}

int pdlpdev_loop_stats(pdlpdev_ctx* ctx, int64_t out[4])
{
  out[0] = ctx->stat_eval_reused, out[1] = ctx->stat_eval_product, out[2] = ctx->stat_loop_syncs, out[3] = ctx->stat_empty_attempts;
  return 0;
}

// The reference accepts host OR device arrays at the C API (cuopt_c.cpp:119,261-403 copy with raft::copy).  The
// front end (plain C++, no HIP header) asks here: device / managed memory is copied down, anything else -- also when no
// HIP device or runtime is usable -- is an ordinary host pointer.
int pdlpdev_copy_in(void* dst, const void* src, size_t bytes)
{
  if (bytes == 0) return 0;
  if (!dst || !src) return fail(-1, "pdlpdev_copy_in: null pointer");
  hipPointerAttribute_t attr;
  memset(&attr, 0, sizeof(attr));
  const hipError_t e = hipPointerGetAttributes(&attr, src);
  if (e == hipSuccess && (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged)) {
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
  }
  (void)hipGetLastError();  // "invalid value" for plain host memory is the normal case
  memcpy(dst, src, bytes);
  return 0;
}

void pdlpdev_range_push(const char* name)
{
  roctx::load();
  if (roctx::Push) roctx::Push(name);
}
void pdlpdev_range_pop(void)
{
  if (roctx::Pop) roctx::Pop();
}

int pdlpdev_prepare_graphs(pdlpdev_ctx* ctx)
{
  HIP_TRY(hipSetDevice(ctx->device));
  if (!ctx->use_graph || (ctx->comm && !ctx->p2p.on) || ctx->small_resident) return 0;
  for (int chunk = 1; chunk <= 64; chunk *= 2) {
    hipGraphExec_t g;
    TRY(get_graph(ctx, chunk, &g));
  }
  return 0;
}

int pdlpdev_get_ctl(pdlpdev_ctx* ctx, pdlpdev_ctl* ctl)
{
  HIP_TRY(hipSetDevice(ctx->device));
  return fetch_ctl(ctx, ctl);
}
int pdlpdev_clear_error(pdlpdev_ctx* ctx)
{
  HIP_TRY(hipSetDevice(ctx->device));
  ctx->ctl_h_current = false;
  k_clear_error<<<1, 1, 0, ctx->stream>>>(ctx->ctl);
  LAUNCH_CHECK();
  return 0;
}
int pdlpdev_set_graph_mode(pdlpdev_ctx* ctx, int use_graph)
{
  ctx->use_graph = use_graph;
  return 0;
}

// ---- results ----------------------------------------------------------------------------------------
int pdlpdev_get_solution(pdlpdev_ctx* ctx, int which, double* x, double* y, double* rc)
{
  HIP_TRY(hipSetDevice(ctx->device));
  TRY(fetch_ctl(ctx, nullptr));
  const int cur = ctx->ctl_h->cur;
  hipStream_t s = ctx->stream;
  if (which == PDLPDEV_BEST) {
    if (!ctx->bestx) return fail(-1, "pdlpdev_get_solution(BEST): nothing was saved");
    if (x) {
      k_unscale<<<grid_for(ctx->n), kBlock, 0, s>>>(ctx->n, ctx->bestx, ctx->dc, ctx->tmp_n);
      HIP_TRY(hipMemcpyAsync(x, ctx->tmp_n, (size_t)ctx->n * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    if (y) {
      k_unscale<<<grid_for(ctx->m), kBlock, 0, s>>>(ctx->m, ctx->besty, ctx->dr, ctx->tmp_m);
      HIP_TRY(hipMemcpyAsync(y, ctx->tmp_m, (size_t)ctx->m * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    if (rc) HIP_TRY(hipMemcpyAsync(rc, ctx->bestrc, (size_t)ctx->n * sizeof(double), hipMemcpyDeviceToHost, s));
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
  }
  if (x) {
    k_unscale<<<grid_for(ctx->n), kBlock, 0, s>>>(ctx->n, which == PDLPDEV_AVERAGE ? ctx->avgx : ctx->x[cur], ctx->dc, ctx->tmp_n);
    HIP_TRY(hipMemcpyAsync(x, ctx->tmp_n, (size_t)ctx->n * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  if (y) {
    k_unscale<<<grid_for(ctx->m), kBlock, 0, s>>>(ctx->m, which == PDLPDEV_AVERAGE ? ctx->avgy : ctx->y[cur], ctx->dr, ctx->tmp_m);
    HIP_TRY(hipMemcpyAsync(y, ctx->tmp_m, (size_t)ctx->m * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  if (rc)
    HIP_TRY(hipMemcpyAsync(rc, ctx->rc[which == PDLPDEV_AVERAGE ? 1 : 0], (size_t)ctx->n * sizeof(double), hipMemcpyDeviceToHost, s));
  LAUNCH_CHECK();
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

static int64_t locate_buffer(pdlpdev_ctx* ctx, int id, double** ptr)
{
  if (hipSetDevice(ctx->device) != hipSuccess) return -2;
  if (fetch_ctl(ctx, nullptr) != 0) return -2;
  const int cur = ctx->ctl_h->cur;
  double* src   = nullptr;
  int64_t count = 0;
  const int64_t n = ctx->n, m = ctx->m, nnz = ctx->nnz;
  switch (id) {
    case PDLPDEV_BUF_X: src = ctx->x[cur], count = n; break;
    case PDLPDEV_BUF_Y: src = ctx->y[cur], count = m; break;
    case PDLPDEV_BUF_X_OTHER: src = ctx->x[cur ^ 1], count = n; break;
    case PDLPDEV_BUF_Y_OTHER: src = ctx->y[cur ^ 1], count = m; break;
    case PDLPDEV_BUF_ATY: src = ctx->aty[cur], count = n; break;
    case PDLPDEV_BUF_ATY_OTHER: src = ctx->aty[cur ^ 1], count = n; break;
    case PDLPDEV_BUF_XBAR: src = ctx->xbar, count = n; break;
    case PDLPDEV_BUF_SUM_X: src = ctx->sumx, count = n; break;
    case PDLPDEV_BUF_SUM_Y: src = ctx->sumy, count = m; break;
    case PDLPDEV_BUF_AVG_X: src = ctx->avgx, count = n; break;
    case PDLPDEV_BUF_AVG_Y: src = ctx->avgy, count = m; break;
    case PDLPDEV_BUF_DROW: src = ctx->dr, count = m; break;
    case PDLPDEV_BUF_DCOL: src = ctx->dc, count = n; break;
    case PDLPDEV_BUF_A_VALUES: src = ctx->A.full.val, count = nnz; break;
    case PDLPDEV_BUF_AT_VALUES: src = ctx->At.full.val, count = nnz; break;
    case PDLPDEV_BUF_C: src = ctx->c, count = n; break;
    case PDLPDEV_BUF_LB: src = ctx->lb, count = n; break;
    case PDLPDEV_BUF_UB: src = ctx->ub, count = n; break;
    case PDLPDEV_BUF_LO: src = ctx->lo, count = m; break;
    case PDLPDEV_BUF_HI: src = ctx->hi, count = m; break;
    case PDLPDEV_BUF_RC_CURRENT: src = ctx->rc[0], count = n; break;
    case PDLPDEV_BUF_RC_AVERAGE: src = ctx->rc[1], count = n; break;
    case PDLPDEV_BUF_LAST_RESTART_X: src = ctx->lrx, count = n; break;
    case PDLPDEV_BUF_LAST_RESTART_Y: src = ctx->lry, count = m; break;
    case PDLPDEV_BUF_ATY_U_CURRENT: src = ctx->aty_u[PDLPDEV_CURRENT], count = n; break;
    case PDLPDEV_BUF_ATY_U_AVERAGE: src = ctx->aty_u[PDLPDEV_AVERAGE], count = n; break;
    case PDLPDEV_BUF_LAST_RESTART_ATY:
      if (!ctx->lraty) { fail(-1, "buffer %d exists in Halpern mode only", id); return -1; }
      src = ctx->lraty, count = n;
      break;
    case PDLPDEV_BUF_AX_U_CURRENT: src = ctx->ax_u[PDLPDEV_CURRENT], count = m; break;
    case PDLPDEV_BUF_AX_U_AVERAGE: src = ctx->ax_u[PDLPDEV_AVERAGE], count = m; break;
    case PDLPDEV_BUF_PART_A: src = ctx->A.part, count = ctx->A.partials(); break;
    case PDLPDEV_BUF_PART_AT:  // (a sharded Halpern step's A^T product runs on the owner-computes column block, whose partials these are;
                               //  every other context answers as it always did)
      if (ctx->halpern && ctx->owner && ctx->Oc.part) src = ctx->Oc.part, count = 2 * (int64_t)ctx->Oc.partials();
      else src = ctx->At.part, count = 2 * (int64_t)ctx->At.partials();
      break;
    case PDLPDEV_BUF_ZS_LAUNCHES:
      if (!ctx->xmask) { fail(-1, "buffer %d: this context has no bitmap of xbar (CUOPT_AMD_TUNE=zero_skip=0, or A is not in the row-sum panels)", id); return -1; }
      src = reinterpret_cast<double*>(ctx->xmask + 2 * (((size_t)n + 127) / 128)), count = 1;
      break;
    case PDLPDEV_BUF_XBAR_MASK:  // (64-bit words, the size of the doubles the hook copies; all zero where no attempt writes it)
      if (!ctx->xmask) { fail(-1, "buffer %d: this context has no bitmap of xbar (CUOPT_AMD_TUNE=zero_skip=0, or A is not in the row-sum panels)", id); return -1; }
      src = reinterpret_cast<double*>(ctx->xmask), count = (n + 63) / 64;
      break;
    case PDLPDEV_BUF_AX_U_LAST_RESTART: src = ctx->ax_u[PDLPDEV_LAST_RESTART], count = m; break;
    case PDLPDEV_BUF_ATY_U_LAST_RESTART: src = ctx->aty_u[PDLPDEV_LAST_RESTART], count = n; break;
    default: fail(-1, "unknown buffer %d", id); return -1;
  }
  *ptr = src;
  return count;
}

int64_t pdlpdev_download(pdlpdev_ctx* ctx, int id, void* host, int64_t max_elements)
{
  double* src   = nullptr;
  int64_t count = locate_buffer(ctx, id, &src);
  if (count < 0) return count;
  count = std::min(count, max_elements);
  if (count > 0) {
    if (hipMemcpyAsync(host, src, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return -2;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return -2;
  }
  return count;
}

int64_t pdlpdev_upload(pdlpdev_ctx* ctx, int id, const void* host, int64_t elements)
{
  double* dst   = nullptr;
  int64_t count = locate_buffer(ctx, id, &dst);
  if (count < 0) return count;
  if (id == PDLPDEV_BUF_A_VALUES || id == PDLPDEV_BUF_AT_VALUES) {
    fail(-1, "matrix values cannot be overwritten");
    return -1;
  }
  if (id == PDLPDEV_BUF_XBAR_MASK || id == PDLPDEV_BUF_ZS_LAUNCHES || id == PDLPDEV_BUF_PART_A || id == PDLPDEV_BUF_PART_AT) {
    fail(-1, "the bitmap of xbar and the reduction partials are written by the attempt's kernels alone");
    return -1;
  }
  if (id == PDLPDEV_BUF_AX_U_LAST_RESTART || id == PDLPDEV_BUF_ATY_U_LAST_RESTART) {
    fail(-1, "the products at the last-restart anchors are written by the evaluation and the trust region alone");
    return -1;
  }
  count = std::min(count, elements);
  ctx->aty_valid = false;  // (an iterate or its A^T y may be what is overwritten)
  if ((id == PDLPDEV_BUF_LB && ctx->ubd.lb_same) || (id == PDLPDEV_BUF_UB && ctx->ubd.ub_same)) {
    // bounds written behind the solver's back: the arrays are read again (and the attempt graphs, which carry the flags by value,
    // are captured again)
    if (id == PDLPDEV_BUF_LB) ctx->ubd.lb_same = 0;
    else ctx->ubd.ub_same = 0;
    for (auto& kv : ctx->graphs) (void)hipGraphExecDestroy(kv.second);
    ctx->graphs.clear();
  }
  if (count > 0) {
    if (hipMemcpyAsync(dst, host, (size_t)count * sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return -2;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return -2;
  }
  return count;
}

int pdlpdev_set_loop_state(pdlpdev_ctx* ctx, double sum_weights, int32_t its_since_restart, int32_t k)
{
  HIP_TRY(hipSetDevice(ctx->device));
  loop_state_touched(ctx);
  k_set_loop_state<<<1, 1, 0, ctx->stream>>>(ctx->ctl, sum_weights, its_since_restart, k);
  LAUNCH_CHECK();
  return 0;
}

// ---- restarted reflected-Halpern mode ----------------------------------------------------------------------
static void drop_graphs(pdlpdev_ctx* ctx)
{
  for (auto& kv : ctx->graphs) (void)hipGraphExecDestroy(kv.second);
  ctx->graphs.clear();
}
int pdlpdev_set_halpern(pdlpdev_ctx* ctx, int on)
{
  HIP_TRY(hipSetDevice(ctx->device));
  if ((on != 0) == ctx->halpern) return 0;
  if (on) {
    // behind a communicator: the owner-computes dataflow only (the step's twins run on its column block; the solver's
    // cuoptamd_settings::halpern_sharded is the public gate above this layer).  The anchors lrx / lry / lraty: replicated / this
    // rank's rows / replicated.
    if (ctx->comm && !ctx->owner)
      return fail(-7, "reflected Halpern mode: a sharded solver runs it on the owner-computes dataflow only, not on CUOPT_AMD_SHARD_DATAFLOW=%s",
                  ctx->rsag ? "rsag" : "allreduce");
    // (a context on the resident small-LP path runs the mode inside one workgroup: kernels_resident_halpern.hip)
    if (!ctx->scaled) return fail(-1, "pdlpdev_set_halpern: call after pdlpdev_scale_problem");
    if (!ctx->lraty) TRY(dev_alloc(ctx, &ctx->lraty, (size_t)ctx->n));
    if (!ctx->hal) TRY(dev_alloc(ctx, &ctx->hal, 1));
    if (!ctx->hal_h) HIP_TRY(hipHostMalloc((void**)&ctx->hal_h, sizeof(pdlpdev_halpern)));
    k_halpern_clear<<<1, 1, 0, ctx->stream>>>(ctx->hal);
    LAUNCH_CHECK();
    *ctx->hal_h        = pdlpdev_halpern{};
    ctx->hal_h->r2_min = HUGE_VAL;
  }
  ctx->halpern = on != 0;
  loop_state_touched(ctx);
  drop_graphs(ctx);  // (the attempt graphs hold the other mode's kernels)
  return 0;
}
int pdlpdev_get_halpern(pdlpdev_ctx* ctx, pdlpdev_halpern* out)
{
  if (!ctx->halpern) return fail(-1, "pdlpdev_get_halpern: the context is not in Halpern mode");
  *out = *ctx->hal_h;
  return 0;
}
int pdlpdev_spectral_norm(pdlpdev_ctx* ctx, double rel_tol, int32_t max_products, double* sigma_max, int32_t* products)
{
  HIP_TRY(hipSetDevice(ctx->device));
  // (a resident context keeps its stream-layout arrays: launch_plain runs the layout's plain products on it, as pdlpdev_compute_aty does)
  // A sharded context: A v on this rank's rows, the partial A^T (A v) into ar_buf, one all-reduce as in pdlpdev_compute_aty, the norm
  // and the next v from the replicated result -- every rank holds the same bits and returns the same sigma_max.  xbar is not borrowed.
  hipStream_t s = ctx->stream;
  const int n   = ctx->n;
  double* v = ctx->tmp_n;  // the normalised iterate; A v -> tmp_m; A^T A v -> xbar (sharded: ar_buf)
  double* const atav = ctx->comm ? ctx->ar_buf : ctx->xbar;
  k_fill<<<grid_for(n), kBlock, 0, s>>>(n, v, 1.0 / sqrt((double)n));
  double est = 0.0;
  int done   = 0;
  while (done < max_products) {
    launch_plain(ctx, 0, v, ctx->tmp_m);
    launch_plain(ctx, 1, ctx->tmp_m, atav);
    if (ctx->comm) {
      LAUNCH_CHECK();
      TRY(allreduce(ctx, atav, (size_t)n, rccl::kSum));
    }
    TRY(reduce_vec(ctx, 1, n, atav, nullptr, 0));
    TRY(fetch_scalars(ctx, 1));
    done += 1;
    const double s2 = sqrt(ctx->scal_h[0]);  // ||A^T A v||, v of unit length: the estimate of sigma_max^2 (from below)
    if (!(s2 > 0.0)) {
      est = 0.0;
      break;
    }
    k_div_by_scalar<<<grid_for(n), kBlock, 0, s>>>(n, v, atav, s2);  // v <- A^T A v / s2
    LAUNCH_CHECK();
    const bool settled = fabs(s2 - est) <= rel_tol * s2;
    est                = s2;
    if (settled) break;
  }
  if (!ctx->comm) HIP_TRY(hipMemsetAsync(ctx->xbar, 0, (size_t)n * sizeof(double), s));
  if (sigma_max) *sigma_max = sqrt(est);
  if (products) *products = done;
  return 0;
}
int pdlpdev_halpern_restart(pdlpdev_ctx* ctx, double theta, double dist[2], pdlpdev_ctl* ctl)
{
  HIP_TRY(hipSetDevice(ctx->device));
  if (!ctx->halpern) return fail(-1, "pdlpdev_halpern_restart: the context is not in Halpern mode");
  hipStream_t s = ctx->stream;
  const int g   = std::min(grid_for(std::max(ctx->n, ctx->m)), kGenericBlocks);
  // distances to the anchor and anchor <- iterate: the KKT restart's kernel with the current iterate as the candidate
  launch_restart_current(ctx, g);
  k_finalize<<<1, kBlock, 0, s>>>(ctx->part_g, g, 2, 0u, ctx->scal);
  k_copy_current<<<grid_for(ctx->n), kBlock, 0, s>>>(ctx->n, ctx->ctl, ctx->aty[0], ctx->aty[1], ctx->lraty);
  if (ctx->comm) {  // (the dual distance is a sum over the row blocks, as in pdlpdev_restart: every rank forms the same weight)
    LAUNCH_CHECK();
    TRY(allreduce(ctx, ctx->scal + 1, 1, rccl::kSum));
  }
  k_halpern_restart_ctl<<<1, 1, 0, s>>>(ctx->ctl, ctx->hal, ctx->scal, theta);
  LAUNCH_CHECK();
  HIP_TRY(hipMemcpyAsync(ctx->scal_h, ctx->scal, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  TRY(fetch_ctl_counted(ctx, ctl));  // (the weight changed on the device; aty[cur] is untouched, so aty_valid keeps its value)
  if (dist) dist[0] = ctx->scal_h[0], dist[1] = ctx->scal_h[1];
  return 0;
}

// ---- measurement / parity hooks ------------------------------------------------------------------------
int pdlpdev_spmv(pdlpdev_ctx* ctx, int transpose, const double* x, double* y)
{
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s  = ctx->stream;
  const int rows = transpose ? ctx->n : ctx->m, cols = transpose ? ctx->m : ctx->n;
  double* in     = transpose ? ctx->tmp_m : ctx->tmp_n;
  double* outv   = transpose ? ctx->tmp_n : ctx->tmp_m;
  HIP_TRY(hipMemcpyAsync(in, x, (size_t)cols * sizeof(double), hipMemcpyHostToDevice, s));
  launch_plain(ctx, transpose, in, outv);
  LAUNCH_CHECK();
  HIP_TRY(hipMemcpyAsync(y, outv, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

int pdlpdev_time_kernel(pdlpdev_ctx* ctx, int kernel_id, int reps, double* avg_ms)
{
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (reps < 1) reps = 1;
  const bool loop_kernel = kernel_id == PDLPDEV_K_PRIMAL || kernel_id == PDLPDEV_K_SPMV_A_DUAL || kernel_id == PDLPDEV_K_SPMV_AT_STEP || kernel_id == PDLPDEV_K_STEP_DECISION;
  if (!loop_kernel && kernel_id != PDLPDEV_K_SPMV_A_PLAIN && kernel_id != PDLPDEV_K_SPMV_AT_PLAIN) return fail(-1, "pdlpdev_time_kernel: unknown kernel %d", kernel_id);
  // save what the timed launches may touch: control block and the running sums
  TRY(fetch_ctl(ctx, nullptr));
  loop_state_touched(ctx);  // (forced attempts run on the solver's own buffers)
  pdlpdev_ctl saved = *ctx->ctl_h;
  pdlpdev_ctl forced = saved;
  forced.pending_avg  = ctx->halpern ? 0 : 1;    // time the kernels WITH their averaging traffic (Halpern mode has none)
  forced.target_steps = saved.steps_taken + (ctx->halpern ? 2 : 1);  // and not as no-ops (Halpern: nor as the last step of a run, the
  forced.error        = 0;                                            //  only one that stores x')
  const pdlpdev_halpern saved_hal = ctx->halpern ? *ctx->hal_h : pdlpdev_halpern{};
  // (Halpern mode: no sums are touched; what the forced steps overwrite is T(z^k) in the average slots -- y' on every step, x' on none
  //  of them, both saved so that an evaluation behind the hook still sees the point of the last real step)
  double* const keep_n = ctx->halpern ? ctx->avgx : ctx->sumx;
  double* const keep_m = ctx->halpern ? ctx->avgy : ctx->sumy;
  double *sx = nullptr, *sy = nullptr;
  HIP_TRY(hipMalloc((void**)&sx, std::max<size_t>(ctx->n, 1) * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&sy, std::max<size_t>(ctx->m, 1) * sizeof(double)));
  HIP_TRY(hipMemcpyAsync(sx, keep_n, (size_t)ctx->n * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(sy, keep_m, (size_t)ctx->m * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(ctx->ctl, &forced, sizeof(forced), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (hipEvent_t& e : ctx->prof_ev) HIP_TRY(hipEventCreate(&e));
  // The kernels of an attempt evict each other's streams from L2 and the 256 MiB Infinity Cache; timing one of them
  // in a tight loop of its own would let its matrix sit in those caches and flatter it.  So every repetition enqueues
  // the whole single-GPU attempt, stage by stage as the solver does, and brackets only the kernel of interest with events.
  // a plain SpMV takes the place of its fused twin
  const int slot = loop_kernel ? kernel_id : (kernel_id == PDLPDEV_K_SPMV_A_PLAIN ? PDLPDEV_K_SPMV_A_DUAL : PDLPDEV_K_SPMV_AT_STEP);
  auto attempt = [&](bool timed) -> int {
    for (const AttemptStage& st : kSingleStages) {
      const bool mine = st.id == slot;
      ctx->prof_armed = mine && timed;
      if (ctx->prof_armed) ctx->prof_used = 0;
      if (!mine || loop_kernel) st.launch(ctx);
      else if (kernel_id == PDLPDEV_K_SPMV_A_PLAIN) launch_plain(ctx, 0, ctx->xbar, ctx->tmp_m);
      else launch_plain(ctx, 1, ctx->y[saved.cur], ctx->tmp_n);
      ctx->prof_armed = false;
      if (st.id == PDLPDEV_K_STEP_DECISION)  // the decision ended the forced step: arm the next repetition
        HIP_TRY(hipMemcpyAsync(ctx->ctl, &forced, sizeof(forced), hipMemcpyHostToDevice, s));
    }
    return 0;
  };
  TRY(attempt(false));  // warm
  float ms = 0.f;
  for (int i = 0; i < reps; ++i) {
    TRY(attempt(true));
    HIP_TRY(hipStreamSynchronize(s));
    for (int q = 0; q < ctx->prof_used; ++q) {  // the launches of the call site: their own durations, added up
      float one_ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&one_ms, ctx->prof_ev[2 * q], ctx->prof_ev[2 * q + 1]));
      ms += one_ms;
    }
  }
  if (avg_ms) *avg_ms = (double)ms / reps;
  // restore
  HIP_TRY(hipMemcpyAsync(keep_n, sx, (size_t)ctx->n * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(keep_m, sy, (size_t)ctx->m * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(ctx->ctl, &saved, sizeof(saved), hipMemcpyHostToDevice, s));
  if (ctx->halpern) HIP_TRY(hipMemcpyAsync(ctx->hal, &saved_hal, sizeof(saved_hal), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (hipEvent_t& e : ctx->prof_ev) (void)hipEventDestroy(e), e = nullptr;
  (void)hipFree(sx), (void)hipFree(sy);
  return 0;
}

int pdlpdev_synchronize(pdlpdev_ctx* ctx)
{
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}
int64_t pdlpdev_device_bytes(pdlpdev_ctx* ctx) { return ctx->bytes; }
int pdlpdev_shard_dataflow(pdlpdev_ctx* ctx) { return !ctx->comm ? 0 : ctx->owner ? 3 : ctx->rsag ? 2 : 1; }
int pdlpdev_shard_transport(pdlpdev_ctx* ctx) { return ctx->p2p.on ? 1 : 0; }
int pdlpdev_shard_wire_bytes(pdlpdev_ctx* ctx, int64_t out[3])
{
  out[0] = ctx->halo.on ? 1 : 0, out[1] = ctx->halo.on ? ctx->halo.bytes : ctx->halo.bytes_allgather, out[2] = ctx->halo.bytes_allgather;
  return 0;
}
int pdlpdev_dense_info(pdlpdev_ctx* ctx, int64_t out[3])
{
  out[0] = ctx->dense.on ? 1 : 0, out[1] = ctx->dense.nseg, out[2] = ctx->dense.nent;
  return 0;
}
int pdlpdev_layout_info(pdlpdev_ctx* ctx, int32_t out[8])
{
  // per matrix: layout (0 CSR stream, 1 slab-major panels, 2 resident single-workgroup loop, 3 jagged rows + LDS column
  // sets), workgroups, slabs (panels) or percent of the global gathers the LDS sets save (jagged)
  ctx->A.info(out), ctx->At.info(out + 3);
  out[6] = ctx->A.pan.on && ctx->A.pan.v.seg, out[7] = ctx->At.pan.on && ctx->At.pan.v.seg;  // panels: the long-tail variant (row sums by nonzero)
  if (ctx->small_resident) out[0] = out[3] = 2;
  return 0;
}

// FNV-1a of a device array (parity tests: the device-side set-up must produce the host constructions' arrays bit for bit)
static uint64_t checksum_device(pdlpdev_ctx* ctx, const void* dev, size_t bytes)
{
  if (!dev || bytes == 0) return 0;
  std::vector<unsigned char> h(bytes);
  if (hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return ~0ull;
  uint64_t f = 1469598103934665603ull;
  for (unsigned char b : h) f = (f ^ b) * 1099511628211ull;
  (void)ctx;
  return f;
}
int pdlpdev_debug_panel_words(pdlpdev_ctx* ctx, int side, int64_t info[5], int32_t* tile_ptr, int32_t* col)
{
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const pdlpdev_ctx::Panels& P = side ? ctx->At.pan : ctx->A.pan;
  if (!P.on) return fail(-1, "side %d is not in panels", side);
  const int NP = P.v.NP ? P.v.NP : P.v.W;
  info[0] = NP, info[1] = P.v.S, info[2] = P.nent, info[3] = P.v.sorted, info[4] = P.v.slab_w;
  if (tile_ptr) HIP_TRY(hipMemcpy(tile_ptr, P.v.tile_ptr, ((size_t)NP * P.v.S + 1) * 4, hipMemcpyDeviceToHost));
  if (col) HIP_TRY(hipMemcpy(col, P.v.col, (size_t)P.nent * 4, hipMemcpyDeviceToHost));
  return 0;
}
int pdlpdev_debug_layout_checksums(pdlpdev_ctx* ctx, uint64_t out[16])
{
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 16; ++i) out[i] = 0;
  const size_t nnz = (size_t)ctx->nnz;
  out[0] = checksum_device(ctx, ctx->At.full.off, ((size_t)ctx->n + 1) * 4);
  out[1] = checksum_device(ctx, ctx->At.full.idx, nnz * 4);
  out[2] = checksum_device(ctx, ctx->At.full.val, nnz * 8);
  auto panels = [&](const pdlpdev_ctx::Panels& P, int32_t rows, uint64_t* o) {
    if (!P.on) return;
    const int NP = P.v.NP ? P.v.NP : P.v.W;
    o[0] = checksum_device(ctx, P.v.row0, ((size_t)NP + 1) * 4);
    o[1] = checksum_device(ctx, P.v.tile_ptr, ((size_t)NP * P.v.S + 1) * 4);
    o[2] = P.v.seg ? 0 : checksum_device(ctx, P.v.rowptr, (size_t)P.v.S * ((size_t)rows + NP) * 2);
    o[3] = checksum_device(ctx, P.v.col, (size_t)P.nent * 4);
    o[4] = checksum_device(ctx, P.perm, (size_t)P.nent * 4);
  };
  panels(ctx->A.pan, ctx->m, out + 3);
  panels(ctx->At.pan, ctx->n, out + 8);
  auto gather_free = [&](const pdlpdev_ctx::Pb& P, int64_t side_nnz, uint64_t* o) {  // (a side is in ONE layout: the panels' slots)
    if (!P.on) return;
    const PbView& v = P.v;
    o[0] = checksum_device(ctx, P.perm, (size_t)P.np * 4);
    o[1] = checksum_device(ctx, v.lidx, (size_t)P.np * 2);
    o[2] = checksum_device(ctx, v.piece_dst, (size_t)(P.np >> v.gshift) * 4);
    o[4] = checksum_device(ctx, v.wg_e0, ((size_t)v.nwg + 1) * 4) ^ (checksum_device(ctx, v.wg_panel, (size_t)v.nwg * 4) * 3) ^
           (checksum_device(ctx, v.bin_row0, ((size_t)v.B + 1) * 4) * 5) ^ (checksum_device(ctx, v.bin_e0, ((size_t)v.B + 1) * 4) * 7) ^
           (uint64_t)v.S * 17 ^ (uint64_t)v.gshift * 19 ^ (uint64_t)v.panel_shift * 23 ^ (uint64_t)P.p_threads * 29 ^ (uint64_t)v.wide * 31;
    if (v.wide) {  // the slot words and the steps' levels instead of the rows by length and the jagged diagonals
      o[3] = checksum_device(ctx, v.rib, (size_t)P.np * 2) ^ (checksum_device(ctx, v.step_lv, (size_t)(P.np >> 10)) * 3) ^ (uint64_t)v.nser * 37;
      if (v.nser) {
        int32_t ser_nnz = 0;
        (void)hipMemcpy(&ser_nnz, v.ser_eptr + v.nser, sizeof(int32_t), hipMemcpyDeviceToHost);
        o[3] ^= (checksum_device(ctx, v.ser_ptr, ((size_t)v.B + 1) * 4) * 5) ^ (checksum_device(ctx, v.ser_row, (size_t)v.nser * 4) * 7) ^
                (checksum_device(ctx, v.ser_eptr, ((size_t)v.nser + 1) * 4) * 11) ^ (checksum_device(ctx, v.ser_slot, (size_t)ser_nnz * 4) * 13);
      }
      return;
    }
    int32_t groups = 0;
    (void)hipMemcpy(&groups, v.bin_grp + v.B, sizeof(int32_t), hipMemcpyDeviceToHost);
    o[3] = checksum_device(ctx, v.pos, (size_t)side_nnz * 2) ^ (checksum_device(ctx, v.sr, (size_t)v.rows * 4) * 3);
    o[4] ^= (checksum_device(ctx, v.bin_grp, ((size_t)v.B + 1) * 4) * 11) ^ (checksum_device(ctx, v.grp_pos, ((size_t)groups + 1) * 4) * 13);
  };
  gather_free(ctx->A.pb, ctx->dense.on ? ctx->A.hot_nnz : ctx->nnz, out + 3);
  gather_free(ctx->At.pb, ctx->dense.on ? ctx->At.hot_nnz : ctx->nnz, out + 8);
  auto jag = [&](const pdlpdev_ctx::Jag& J) -> uint64_t {
    if (!J.on) return 0;
    int32_t nsr = 0, nset = 0;
    (void)hipMemcpy(&nsr, J.v.tile_sr + J.v.ngroups, sizeof(int32_t), hipMemcpyDeviceToHost);
    (void)hipMemcpy(&nset, J.v.set_ptr + J.v.nblk, sizeof(int32_t), hipMemcpyDeviceToHost);
    return checksum_device(ctx, J.v.slot, (size_t)J.nent * 2) ^ (checksum_device(ctx, J.perm, (size_t)J.nent * 4) * 3) ^
           (checksum_device(ctx, J.v.row0, ((size_t)J.v.nblk + 1) * 4) * 5) ^ (checksum_device(ctx, J.v.sr, (size_t)nsr * 4) * 7) ^
           (checksum_device(ctx, J.v.tile_e, ((size_t)J.v.ngroups + 1) * 4) * 11) ^ (checksum_device(ctx, J.v.tile_sr, ((size_t)J.v.ngroups + 1) * 4) * 13) ^
           (checksum_device(ctx, J.v.win, (size_t)J.v.nblk * 8) * 17) ^ (checksum_device(ctx, J.v.set_ptr, ((size_t)J.v.nblk + 1) * 4) * 19) ^
           (checksum_device(ctx, J.v.set_col, (size_t)nset * 4) * 23) ^ (checksum_device(ctx, J.v.lr_ptr, ((size_t)J.v.nblk + 1) * 4) * 29) ^
           (checksum_device(ctx, J.v.lr_row, (size_t)J.v.nlong * 4) * 31) ^ (uint64_t)J.v.waves * 37;
  };
  out[13] = jag(ctx->A.jag), out[14] = jag(ctx->At.jag);
  out[15] = (uint64_t)ctx->A.pan.on | (uint64_t)ctx->At.pan.on << 1 | (uint64_t)ctx->A.jag.on << 2 | (uint64_t)ctx->At.jag.on << 3 |
            (uint64_t)(ctx->A.pan.on && ctx->A.pan.v.seg) << 4 | (uint64_t)(ctx->At.pan.on && ctx->At.pan.v.seg) << 5 | (uint64_t)ctx->A.pb.on << 6 |
            (uint64_t)ctx->At.pb.on << 7 | (uint64_t)(ctx->A.pan.v.dn_own_seg != nullptr) << 8 | (uint64_t)(ctx->At.pan.v.dn_pan_ptr != nullptr) << 9 |
            (uint64_t)ctx->Oc.jag.on << 10 | (uint64_t)ctx->Oc.pan.on << 11;
  return 0;
}

}  // extern "C"
