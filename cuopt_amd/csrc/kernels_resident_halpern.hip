// The restarted reflected-Halpern mode on the resident small-LP path (docs/design/04d_halpern_mode.md, "The resident variant"): a whole
// period of Halpern steps inside ONE workgroup with the LP on chip, and the one-workgroup evaluation of T(z^k) behind it.  A
// translation unit of its own, so that k_pdhg_resident / k_pdhg_resident_batch / k_major_small in kernels_resident.hip keep the
// instructions they had (kernels_halpern.hip was split off kernels_stream.hip for the same reason).
#include "pdlp_ctx.hpp"
#include "pdlp_layouts.hpp"
#include "resident_common.hpp"

#include "resident_halpern_bodies.hpp"

// (resident_halpern_body, major_small_halpern_body: resident_halpern_bodies.hpp)
template <int T, int Q, int U>
__global__ void __launch_bounds__(T)
k_pdhg_resident_halpern(HalpernSmallView V, pdlpdev_ctl* __restrict__ ctl, pdlpdev_ctl* __restrict__ ctl_host, pdlpdev_halpern* __restrict__ hal,
                        pdlpdev_halpern* __restrict__ hal_host, int target_steps, int max_steps)
{
  extern __shared__ double lds[];
  resident_halpern_body<T, Q, U>(V, ctl, ctl_host, hal, hal_host, target_steps, max_steps, lds);
}
// (as_global: resident_halpern_bodies.hpp)
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

// Behind k_restart_batch for the LPs of a Halpern batch: halpern_restart_finish_workgroup (resident_halpern_bodies.hpp), one workgroup
// per LP; the two distances go to the LP's scalar block on the device and to its pinned one.
__global__ void __launch_bounds__(kBlock) k_halpern_restart_finish_batch(const HalpernRestartArgs* __restrict__ args, const int* __restrict__ list)
{
  __shared__ double red[8];
  const HalpernRestartArgs& A = args[list[blockIdx.x]];
  halpern_restart_finish_workgroup(A, A.dist2, A.dist_host, red);
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
