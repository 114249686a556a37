// gfx950 kernels of the burst of device-decided major iterations in reflected-Halpern mode (cuoptamd_settings::halpern_device_major;
// docs/design/04d_halpern_mode.md, "Verdict and restart on the device").  A translation unit of its own: the four layout units, the
// two resident units and the core's restart kernels (k_restart, k_finalize, k_copy_current) compile as before.
// Every kernel here asks the burst's block first and does nothing once a decision has stopped the burst; no kernel waits for another
// -- the order is the stream's.  The second half serves the K LPs of a Halpern small-LP batch (cuoptamd_batch_set_halpern_device_major;
// "Bursts of a K-workgroup batch"): the same bodies with a workgroup per LP, each behind that LP's own block.
// A restart's scalars are halpern_restart_scalars (halpern_decision.hpp), a resident LP's restart finish is halpern_restart_finish_workgroup
// (resident_halpern_bodies.hpp), the decision's three restart tests are the host's (halpern_restart_tests.hpp): nothing is restated here.
#include "halpern_major.hpp"
#include "halpern_major_batch.hpp"
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

// The decision of a major iteration, one workgroup: thread 0 runs halpern_major_decide (halpern_major.hpp) on the context's own blocks.
__global__ void __launch_bounds__(kDecideThreads)
k_halpern_major_decide(const pdlpdev_ctl* __restrict__ ctl, const pdlpdev_halpern* __restrict__ hal, pdlpdev_halpern_major_state* __restrict__ st,
                       const double* __restrict__ sc, pdlpdev_halpern_major_params p, int target, pdlpdev_halpern_major_record* __restrict__ rec)
{
  if (threadIdx.x != 0) return;
  halpern_major_decide(ctl, hal, st, sc, p, target, rec);
}

// ---- the restart, guarded by the decision: twins of k_restart (candidate = the current iterate, scaled distances), k_copy_current
// (A^T y -> the anchor's, over a grid) and k_finalize + k_halpern_restart_ctl (finalize_rows' tree, then halpern_restart_scalars)
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
  halpern_restart_scalars(ctl, hal, st->dist2, theta);
  rec->dist[0] = st->dist2[0], rec->dist[1] = st->dist2[1], rec->new_weight = ctl->primal_weight;
  if (ctl_host) *ctl_host = *ctl, *hal_host = *hal;
}

// ---- the burst of a Halpern small-LP batch (halpern_major_batch.hpp): every kernel above once more with one workgroup (the restart:
// its blocks) per LP, each behind that LP's own flags.  A member that has stopped rests; the others go on.
__global__ void __launch_bounds__(kDecideThreads) k_halpern_major_arm_batch(const HalpernBurstMember* __restrict__ mem, const int* __restrict__ list, int count)
{
  const int i = blockIdx.x * kDecideThreads + threadIdx.x;
  if (i >= count) return;
  const HalpernBurstMember& M     = mem[list[i]];
  pdlpdev_halpern_major_state* st = M.st;
  st->r_prev   = M.r_prev;
  st->dist2[0] = st->dist2[1] = 0.0;
  st->stopped = 0, st->restart = 0;
}
// workgroup b serves LP list[b]: k_pdhg_resident_halpern_batch's arrangement (the record's pointers through as_global, so that the two
// blocks stay in scalar registers) behind the guard, to the period's target
template <int T, int Q, int U>
__global__ void __launch_bounds__(T)
k_pdhg_resident_halpern_burst_batch(const HalpernBurstMember* __restrict__ mem, const int* __restrict__ list, int add_target, int max_steps)
{
  extern __shared__ double lds[];
  const HalpernBurstMember& M = mem[list[blockIdx.x]];
  if (as_global(M.st)->stopped) return;  // (uniform)
  const HalpernResidentArgs& A = M.run;
  const HalpernSmallView& S    = A.V;
  const HalpernSmallView V{S.m, S.n, S.nnz, as_global(S.a_off), as_global(S.a_idx), as_global(S.at_off), as_global(S.at_idx), as_global(S.a_val),
                           as_global(S.at_val), as_global(S.c), as_global(S.lb), as_global(S.ub), as_global(S.lo), as_global(S.hi), as_global(S.x0),
                           as_global(S.x1), as_global(S.y0), as_global(S.y1), as_global(S.aty0), as_global(S.aty1), as_global(S.ax), as_global(S.ay),
                           as_global(S.aaty), as_global(S.tx), as_global(S.ty)};
  resident_halpern_body<T, Q, U>(V, as_global(A.ctl), as_global(A.ctl_host), as_global(A.hal), as_global(A.hal_host), A.target_steps + add_target, max_steps,
                                 lds);
}
// workgroup b evaluates LP list[b] behind the same guard, with that period's guard_target
__global__ void __launch_bounds__(kMajorThreads)
k_major_small_halpern_burst_batch(const MajorSmallArgs* __restrict__ args, const HalpernBurstMember* __restrict__ mem, const int* __restrict__ list, int add_target)
{
  extern __shared__ double prod[];
  const int l = list[blockIdx.x];
  if (mem[l].st->stopped) return;  // (uniform)
  // major_small_halpern_body's guard with the period's target (the record's own guard_target is -1: the body asks nothing more)
  const MajorSmallArgs& A = args[l];
  const int guard_target  = mem[l].run.target_steps + add_target;
  if (!(A.ctl->error != 0 || A.ctl->steps_taken >= guard_target)) {  // (uniform)
    if (threadIdx.x == 0) A.sc[63] = 0.0;  // "not evaluated"
    return;
  }
  major_small_halpern_body(A, prod);
}
// one wave per LP, thread 0 decides: ring slot [l][j]
__global__ void __launch_bounds__(kDecideThreads)
k_halpern_major_decide_batch(const HalpernBurstMember* __restrict__ mem, const int* __restrict__ list, int j, int add_target)
{
  if (threadIdx.x != 0) return;
  const HalpernBurstMember& M = mem[list[blockIdx.x]];
  halpern_major_decide(M.run.ctl, M.run.hal, M.st, M.sc, M.p, M.run.target_steps + add_target, M.ring + j);
}
// the twin of k_restart_batch: the (LP, block) table covers every member of the burst; a block returns unless its LP asked for a restart
__global__ void __launch_bounds__(kBlock) k_halpern_major_restart_batch(const HalpernBurstMember* __restrict__ mem, const int2* __restrict__ blk)
{
  __shared__ double red[12];
  const int2 b                = blk[blockIdx.x];
  const HalpernBurstMember& M = mem[b.x];
  if (M.st->stopped || !M.st->restart) return;  // (uniform)
  restart_block(M.R, b.y, M.fin.g, red);
}
// k_halpern_restart_finish_batch's body behind the member's guard; the distances go to the member's block, they and the new weight to the record
__global__ void __launch_bounds__(kBlock) k_halpern_major_restart_finish_batch(const HalpernBurstMember* __restrict__ mem, const int* __restrict__ list, int j)
{
  __shared__ double red[8];
  const HalpernBurstMember& M = mem[list[blockIdx.x]];
  if (M.st->stopped || !M.st->restart) return;  // (uniform; the flag is the decision's to write)
  pdlpdev_halpern_major_record* rec = M.ring + j;
  halpern_restart_finish_workgroup(M.fin, M.st->dist2, rec->dist, red);
  if (threadIdx.x == 0) rec->new_weight = M.fin.ctl->primal_weight;
}

// the two debug entry points: read_eval's input from its output (the dual objective's two halves as the sum and a zero)
void raw_sums_of(const double* ev, double sc[9])
{
  sc[0] = ev[PDLPDEV_EV_PRES2], sc[1] = ev[PDLPDEV_EV_DUAL_SUM], sc[2] = ev[PDLPDEV_EV_Y2], sc[3] = ev[PDLPDEV_EV_LINF_PRES_REL];
  sc[4] = ev[PDLPDEV_EV_DRES2], sc[5] = 0.0, sc[6] = ev[PDLPDEV_EV_CX], sc[7] = ev[PDLPDEV_EV_X2], sc[8] = ev[PDLPDEV_EV_LINF_DRES_REL];
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

// ---- the launches of a batch burst (pdlpdev_small_batch_run_halpern_burst, kernels_resident.hip) ----
int halpern_batch_burst_arm(hipStream_t s, const HalpernBurstMember* mem, const int* list, int count)
{
  k_halpern_major_arm_batch<<<(count + kDecideThreads - 1) / kDecideThreads, kDecideThreads, 0, s>>>(mem, list, count);
  HIP_TRY(hipGetLastError());
  return 0;
}
int halpern_batch_burst_loop(hipStream_t s, int device, int tier, const HalpernBurstMember* mem, const int* tier_list, int count, int32_t add_target)
{
  return for_resident_tier(
    tier,
    [&](auto I) {
      constexpr ResidentTier r = kResidentTiers[decltype(I)::value];
      return launch_resident_kernel(k_pdhg_resident_halpern_burst_batch<r.T, r.Q, r.U>, I, device, s, count, mem, tier_list, add_target, 1 << 14);
    },
    [&] { return fail(-1, "resident Halpern batch burst: no tier %d", tier); });
}
int halpern_batch_burst_eval(hipStream_t s, int device, size_t lds, const MajorSmallArgs* args, const HalpernBurstMember* mem, const int* list, int count,
                             int32_t add_target)
{
  TRY(allow_dynamic_lds((const void*)k_major_small_halpern_burst_batch, device, 8192 * 8));
  k_major_small_halpern_burst_batch<<<count, kMajorThreads, lds, s>>>(args, mem, list, add_target);
  HIP_TRY(hipGetLastError());
  return 0;
}
int halpern_batch_burst_decide(hipStream_t s, const HalpernBurstMember* mem, const int* list, int count, int32_t j, int32_t add_target)
{
  k_halpern_major_decide_batch<<<count, kDecideThreads, 0, s>>>(mem, list, j, add_target);
  HIP_TRY(hipGetLastError());
  return 0;
}
int halpern_batch_burst_restart(hipStream_t s, const HalpernBurstMember* mem, const int2* blk, int blocks, const int* list, int count, int32_t j)
{
  k_halpern_major_restart_batch<<<blocks, kBlock, 0, s>>>(mem, blk);
  k_halpern_major_restart_finish_batch<<<count, kBlock, 0, s>>>(mem, list, j);
  HIP_TRY(hipGetLastError());
  return 0;
}

int pdlpdev_debug_halpern_major_decide_batch(int device, int32_t count, const double* ev, const pdlpdev_ctl* ctl, const pdlpdev_halpern* hal,
                                             const double* r_prev, const int32_t* stopped, const int32_t* target,
                                             const pdlpdev_halpern_major_params* params, pdlpdev_halpern_major_record* records, double* r_prev_out,
                                             int32_t* stopped_out, int32_t* restart_out)
{
  if (!ev || !ctl || !hal || !r_prev || !stopped || !target || !params || !records || count < 1)
    return fail(-1, "pdlpdev_debug_halpern_major_decide_batch: null argument");
  HIP_TRY(hipSetDevice(device));
  // per member what pdlpdev_debug_halpern_major_decide holds for its one case, plus the member's record of the burst and the list
  struct Blocks {
    pdlpdev_halpern_major_state st;
    pdlpdev_ctl ctl;
    pdlpdev_halpern hal;
    double sc[9];
    pdlpdev_halpern_major_record rec;
    HalpernBurstMember mem;
    int list;
  };
  std::vector<Blocks> h((size_t)count);
  Blocks* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, sizeof(Blocks) * (size_t)count));
  for (int l = 0; l < count; ++l) {
    Blocks& b = h[l];
    memset(&b, 0, sizeof(b));
    b.st.r_prev = r_prev[l], b.st.stopped = stopped[l], b.st.restart = 0;
    b.ctl = ctl[l], b.hal = hal[l], b.rec = records[l];
    raw_sums_of(ev + (size_t)l * PDLPDEV_EV_COUNT, b.sc);
    b.mem.run.ctl = &d[l].ctl, b.mem.run.hal = &d[l].hal, b.mem.run.target_steps = target[l];
    b.mem.st = &d[l].st, b.mem.sc = d[l].sc, b.mem.ring = &d[l].rec, b.mem.p = params[l];
    b.list = count - 1 - l;  // (workgroup w serves member count - 1 - w: the list is looked at)
  }
  hipError_t e = hipMemcpy(d, h.data(), sizeof(Blocks) * (size_t)count, hipMemcpyHostToDevice);
  // the member records and the list, each contiguous as the kernel indexes them
  HalpernBurstMember* dmem = nullptr;
  int* dlist               = nullptr;
  if (e == hipSuccess) e = hipMalloc((void**)&dmem, sizeof(HalpernBurstMember) * (size_t)count);
  if (e == hipSuccess) e = hipMalloc((void**)&dlist, sizeof(int) * (size_t)count);
  for (int l = 0; e == hipSuccess && l < count; ++l) {
    e = hipMemcpy(dmem + l, &h[l].mem, sizeof(HalpernBurstMember), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dlist + l, &h[l].list, sizeof(int), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) {
    k_halpern_major_decide_batch<<<count, kDecideThreads>>>(dmem, dlist, 0, 0);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(h.data(), d, sizeof(Blocks) * (size_t)count, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (dmem) (void)hipFree(dmem);
  if (dlist) (void)hipFree(dlist);
  HIP_TRY(e);
  for (int l = 0; l < count; ++l) {
    records[l] = h[l].rec;
    if (r_prev_out) r_prev_out[l] = h[l].st.r_prev;
    if (stopped_out) stopped_out[l] = h[l].st.stopped;
    if (restart_out) restart_out[l] = h[l].st.restart;
  }
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
  raw_sums_of(ev, h.sc);
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
