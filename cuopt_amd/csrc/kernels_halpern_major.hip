// gfx950 kernels of the burst of device-decided major iterations in reflected-Halpern mode (cuoptamd_settings::halpern_device_major;
// docs/design/04d_halpern_mode.md, "Verdict and restart on the device").  A translation unit of its own: the four layout units, the
// two resident units and the core's restart kernels (k_restart, k_finalize, k_copy_current, k_halpern_restart_ctl) compile as before.
// Every kernel here asks the burst's block first and does nothing once a decision has stopped the burst; no kernel waits for another
// -- the order is the stream's.
#include "halpern_major.hpp"
#include "pdlp_launch.hpp"
#include "resident_halpern_bodies.hpp"

namespace {

constexpr int kDecideThreads = 64;  // one wave; thread 0 decides (a handful of comparisons on scalars: nothing to share out)

__global__ void k_halpern_major_arm(pdlpdev_halpern_major_state* st, double r_prev)
{
  st->r_prev = r_prev;
  st->dist2[0] = st->dist2[1] = 0.0;
  st->stopped = 0, st->restart = 0;
}
// the guarded twin of k_set_target
__global__ void k_halpern_major_set_target(pdlpdev_ctl* ctl, const pdlpdev_halpern_major_state* st, int target)
{
  if (st->stopped) return;
  ctl->target_steps = target;
}

// The resident path's two kernels of a period behind the guard: k_pdhg_resident_halpern's body with the period's target, and
// k_major_small_halpern's body with its guard_target.
template <int T, int Q, int U>
__global__ void __launch_bounds__(T)
k_pdhg_resident_halpern_burst(HalpernSmallView V, pdlpdev_ctl* __restrict__ ctl, pdlpdev_ctl* __restrict__ ctl_host, pdlpdev_halpern* __restrict__ hal,
                              pdlpdev_halpern* __restrict__ hal_host, const pdlpdev_halpern_major_state* __restrict__ st, int target_steps, int max_steps)
{
  extern __shared__ double lds[];
  if (st->stopped) return;  // (uniform)
  resident_halpern_body<T, Q, U>(V, ctl, ctl_host, hal, hal_host, target_steps, max_steps, lds);
}
__global__ void __launch_bounds__(kMajorThreads) k_major_small_halpern_burst(MajorSmallArgs A, const pdlpdev_halpern_major_state* __restrict__ st)
{
  extern __shared__ double prod[];
  if (st->stopped) return;  // (uniform)
  major_small_halpern_body(A, prod);
}

// The decision of a major iteration, one workgroup: halpern_major_head's tests in its order and with its expressions (pdlp_solver.cpp:
// to_convergence, verdict, the iteration limit of check_limits, the three restart tests) on the scalars that are on the device.
//   sc      the evaluation's nine raw sums (read_eval's input: the scalars' slot 32 on the multi-launch path, the pinned block's on
//           the resident one)
//   target  the period's accepted-step count
//   rec     the record, in pinned host memory
// Stopped: nothing.  The error flag up: a record marked "step error", stopped.  The steps short of the target (a resident launch that
// hit its step cap): "fell short", stopped.  Otherwise the record with the verdict; any verdict but "go on" stops the burst.
__global__ void __launch_bounds__(kDecideThreads)
k_halpern_major_decide(const pdlpdev_ctl* __restrict__ ctl, const pdlpdev_halpern* __restrict__ hal, pdlpdev_halpern_major_state* __restrict__ st,
                       const double* __restrict__ sc, pdlpdev_halpern_major_params p, int target, pdlpdev_halpern_major_record* __restrict__ rec)
{
  if (threadIdx.x != 0) return;
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
  // the three restart tests
  const double r = hal->r, r_first = hal->r_first, r_prev = st->r_prev;
  bool restart = false;
  if (r <= p.sufficient_reduction * r_first) restart = true;
  else if (r <= p.necessary_reduction * r_first && r_prev >= 0.0 && r > r_prev) restart = true;
  else if ((double)hal->k >= p.artificial_threshold * (double)total_iterations) restart = true;
  st->r_prev  = restart ? -1.0 : r;  // (halpern_restart_done: no previous check behind a restart)
  st->restart = restart ? 1 : 0;
  out.restart = restart ? 1 : 0;
  *rec        = out;
}

// ---- the restart, guarded by the decision: twins of k_restart (candidate = the current iterate, scaled distances), k_copy_current
// (A^T y -> the anchor's) and k_finalize + k_halpern_restart_ctl (the two sums by finalize_rows' tree, the smoothed weight, k <- 0)
__global__ void __launch_bounds__(kBlock) k_halpern_major_restart(RestartView R, const pdlpdev_halpern_major_state* __restrict__ st)
{
  __shared__ double red[12];
  if (st->stopped || !st->restart) return;  // (uniform)
  restart_block(R, blockIdx.x, gridDim.x, red);
}
__global__ void __launch_bounds__(kBlock)
k_halpern_major_copy_current(int n, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ v0, const double* __restrict__ v1, double* __restrict__ out,
                             const pdlpdev_halpern_major_state* __restrict__ st)
{
  if (st->stopped || !st->restart) return;
  const double* __restrict__ v = ctl->cur ? v1 : v0;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) out[i] = v[i];
}
__global__ void __launch_bounds__(kBlock)
k_halpern_major_restart_finish(const double* __restrict__ part, int g, pdlpdev_ctl* ctl, pdlpdev_halpern* hal, pdlpdev_halpern_major_state* st, double theta,
                               pdlpdev_halpern_major_record* rec, pdlpdev_ctl* ctl_host, pdlpdev_halpern* hal_host)
{
  __shared__ double red[8];
  if (st->stopped || !st->restart) return;  // (uniform; the flag is the decision's to write)
  finalize_rows(part, g, 2, 0u, st->dist2, red);
  if (threadIdx.x != 0) return;
  const double dx = sqrt(st->dist2[0]), dy = sqrt(st->dist2[1]);  // k_halpern_restart_ctl
  st->dist2[0] = dx, st->dist2[1] = dy;
  if (theta >= 0.0 && dx > 1.0e-10 && dy > 1.0e-10) {
    const double w     = exp(theta * log(dy / dx) + (1.0 - theta) * log(ctl->primal_weight));
    ctl->primal_weight = w;
    ctl->tau           = ctl->step_size / w;
    ctl->sigma         = ctl->step_size * w;
  }
  ctl->its_since_restart = 0;
  hal->k                 = 0;
  rec->dist[0] = dx, rec->dist[1] = dy, rec->new_weight = ctl->primal_weight;
  if (ctl_host) *ctl_host = *ctl, *hal_host = *hal;
}

}  // namespace

extern "C" {

int halpern_major_launch_arm(pdlpdev_ctx* ctx, double r_prev)
{
  k_halpern_major_arm<<<1, 1, 0, ctx->stream>>>(ctx->hmaj, r_prev);
  HIP_TRY(hipGetLastError());
  return 0;
}
int halpern_major_launch_set_target(pdlpdev_ctx* ctx, int32_t target)
{
  k_halpern_major_set_target<<<1, 1, 0, ctx->stream>>>(ctx->ctl, ctx->hmaj, target);
  HIP_TRY(hipGetLastError());
  return 0;
}
int halpern_major_launch_resident_period(pdlpdev_ctx* ctx, int32_t target, int rc_rule_finite_bounds, int want_linf, double eps_rel_primal,
                                         double eps_rel_dual)
{
  const HalpernSmallView V = halpern_view(ctx);
  TRY(for_resident_tier(
    pdlpdev_resident_tier(ctx->m, ctx->n, ctx->nnz),
    [&](auto I) {
      constexpr ResidentTier r = kResidentTiers[decltype(I)::value];
      return launch_resident_kernel(k_pdhg_resident_halpern_burst<r.T, r.Q, r.U>, I, ctx->device, ctx->stream, 1, V, ctx->ctl, ctx->ctl_h, ctx->hal,
                                    ctx->hal_h, (const pdlpdev_halpern_major_state*)ctx->hmaj, target, 1 << 14);
    },
    [] { return fail(-1, "resident Halpern burst: the LP fits no tier"); }));
  TRY(allow_dynamic_lds((const void*)k_major_small_halpern_burst, ctx->device, 8192 * 8));
  MajorSmallArgs A = major_args(ctx, 3, rc_rule_finite_bounds, want_linf, eps_rel_primal, eps_rel_dual);
  A.guard_target   = target;
  const size_t lds = sizeof(double) * (size_t)std::max<int64_t>(ctx->nnz, 1);
  k_major_small_halpern_burst<<<1, kMajorThreads, lds, ctx->stream>>>(A, ctx->hmaj);
  HIP_TRY(hipGetLastError());
  return 0;
}
int halpern_major_launch_decide(pdlpdev_ctx* ctx, const double* sc, const pdlpdev_halpern_major_params& p, int32_t target,
                                pdlpdev_halpern_major_record* rec)
{
  k_halpern_major_decide<<<1, kDecideThreads, 0, ctx->stream>>>(ctx->ctl, ctx->hal, ctx->hmaj, sc, p, target, rec);
  HIP_TRY(hipGetLastError());
  return 0;
}
int halpern_major_launch_restart(pdlpdev_ctx* ctx, double theta, pdlpdev_halpern_major_record* rec, int mirrors)
{
  hipStream_t s = ctx->stream;
  const int g   = std::min(grid_for(std::max(ctx->n, ctx->m)), kGenericBlocks);  // (pdlpdev_halpern_restart's grid: the same partials)
  const RestartView R{ctx->n, ctx->m, PDLPDEV_CURRENT, 0, ctx->dc, ctx->dr, ctx->ctl, ctx->x[0], ctx->x[1], ctx->y[0], ctx->y[1],
                      ctx->avgx, ctx->avgy, ctx->lrx, ctx->lry, ctx->sumx, ctx->sumy, ctx->part_g};
  k_halpern_major_restart<<<g, kBlock, 0, s>>>(R, ctx->hmaj);
  k_halpern_major_copy_current<<<grid_for(ctx->n), kBlock, 0, s>>>(ctx->n, ctx->ctl, ctx->aty[0], ctx->aty[1], ctx->lraty, ctx->hmaj);
  k_halpern_major_restart_finish<<<1, kBlock, 0, s>>>(ctx->part_g, g, ctx->ctl, ctx->hal, ctx->hmaj, theta, rec, mirrors ? ctx->ctl_h : nullptr,
                                                      mirrors ? ctx->hal_h : nullptr);
  HIP_TRY(hipGetLastError());
  return 0;
}

int pdlpdev_debug_halpern_major_decide(int device, const double ev[PDLPDEV_EV_COUNT], const pdlpdev_ctl* ctl, const pdlpdev_halpern* hal,
                                       double r_prev, int32_t stopped, int32_t target, const pdlpdev_halpern_major_params* params,
                                       pdlpdev_halpern_major_record* record, double* r_prev_out, int32_t* stopped_out, int32_t* restart_out)
{
  if (!ev || !ctl || !hal || !params || !record) return fail(-1, "pdlpdev_debug_halpern_major_decide: null argument");
  HIP_TRY(hipSetDevice(device));
  // one device block for everything the kernel reads and writes: [state | control block | Halpern block | nine raw sums | record]
  struct Blocks {
    pdlpdev_halpern_major_state st;
    pdlpdev_ctl ctl;
    pdlpdev_halpern hal;
    double sc[9];
    pdlpdev_halpern_major_record rec;
  } h{}, *d = nullptr;
  h.st.r_prev = r_prev, h.st.stopped = stopped, h.st.restart = 0;
  h.ctl = *ctl, h.hal = *hal, h.rec = *record;
  // (read_eval's input from its output: the dual objective's two halves as the sum and a zero)
  h.sc[0] = ev[PDLPDEV_EV_PRES2], h.sc[1] = ev[PDLPDEV_EV_DUAL_SUM], h.sc[2] = ev[PDLPDEV_EV_Y2], h.sc[3] = ev[PDLPDEV_EV_LINF_PRES_REL];
  h.sc[4] = ev[PDLPDEV_EV_DRES2], h.sc[5] = 0.0, h.sc[6] = ev[PDLPDEV_EV_CX], h.sc[7] = ev[PDLPDEV_EV_X2], h.sc[8] = ev[PDLPDEV_EV_LINF_DRES_REL];
  HIP_TRY(hipMalloc((void**)&d, sizeof(Blocks)));
  hipError_t e = hipMemcpy(d, &h, sizeof(Blocks), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    k_halpern_major_decide<<<1, kDecideThreads>>>(&d->ctl, &d->hal, &d->st, d->sc, *params, target, &d->rec);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof(Blocks), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  HIP_TRY(e);
  *record = h.rec;
  if (r_prev_out) *r_prev_out = h.st.r_prev;
  if (stopped_out) *stopped_out = h.st.stopped;
  if (restart_out) *restart_out = h.st.restart;
  return 0;
}

}  // extern "C"
