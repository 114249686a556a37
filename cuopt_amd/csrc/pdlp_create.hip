// Context creation and destruction of the device layer (pdlp_device.h: pdlpdev_create*, pdlpdev_destroy): uploads (or adoption of an
// analysed matrix's device arrays), the choice and construction of the SpMV layouts of both matrices, the vectors' slab.  The kernels,
// the loop and everything that runs after creation: pdlp_device.hip.
#include "pdlp_ctx.hpp"
#include "pdlp_layouts.hpp"
#include "pdlp_setup.hpp"

// (defined in pdlp_device.hip)
__global__ void k_fill(int64_t n, double* __restrict__ d, double v);
int sync_panel_values(pdlpdev_ctx* c);
int resident_tier(int m, int n, int64_t nnz);

static thread_local int g_create_sharded = 0;  // pdlpdev_create_hint: the next context will run behind a communicator
static thread_local int g_create_no_resident = 0;  // pdlpdev_create_no_resident: the next context stays off the resident small-LP path
static thread_local int g_create_batch_lanes = 0;  // pdlpdev_create_batch_lanes: the next context's jagged layouts serve batches that wide

static int create_impl(pdlpdev_ctx** out, int device, int32_t m, int32_t n, const int32_t* a_offsets,
                       const int32_t* a_indices, const double* a_values, const int32_t* at_offsets,
                       const int32_t* at_indices, const double* at_values,
                       void (*transpose_ready)(void*), void* user, const double* c, const double* lo,
                       const double* hi, const double* lb, const double* ub, pdlpdev_analysis* an);

extern "C" {

const char* pdlpdev_last_error(void) { return g_err.c_str(); }
void pdlpdev_create_hint(int sharded) { g_create_sharded = sharded; }
void pdlpdev_create_no_resident(int no_resident) { g_create_no_resident = no_resident; }
void pdlpdev_create_batch_lanes(int lanes) { g_create_batch_lanes = lanes; }
static thread_local pdlpdev_ctx* g_create_stream_donor = nullptr;
void pdlpdev_create_share_stream(pdlpdev_ctx* donor) { g_create_stream_donor = donor; }
int pdlpdev_resident_size(int32_t m, int32_t n, int64_t nnz) { return resident_tier(m, n, nnz) >= 0 ? 1 : 0; }
int pdlpdev_resident_tier(int32_t m, int32_t n, int64_t nnz) { return resident_tier(m, n, nnz); }

int pdlpdev_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int pdlpdev_device_info(int dev, char* name, int len, int* compute_units, int64_t* hbm_bytes)
{
  hipDeviceProp_t p;
  HIP_TRY(hipGetDeviceProperties(&p, dev));
  if (name && len > 0) snprintf(name, (size_t)len, "%s (%s)", p.name, p.gcnArchName);
  if (compute_units) *compute_units = p.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
  return 0;
}

int pdlpdev_create(pdlpdev_ctx** out, int device, int32_t m, int32_t n, const int32_t* a_offsets,
                   const int32_t* a_indices, const double* a_values, const int32_t* at_offsets,
                   const int32_t* at_indices, const double* at_values, const double* c,
                   const double* lo, const double* hi, const double* lb, const double* ub)
{
  return pdlpdev_create_overlapped(out, device, m, n, a_offsets, a_indices, a_values, at_offsets, at_indices, at_values,
                                   nullptr, nullptr, c, lo, hi, lb, ub);
}

int pdlpdev_create_overlapped(pdlpdev_ctx** out, int device, int32_t m, int32_t n, const int32_t* a_offsets,
                              const int32_t* a_indices, const double* a_values, const int32_t* at_offsets,
                              const int32_t* at_indices, const double* at_values,
                              void (*transpose_ready)(void*), void* user, const double* c, const double* lo,
                              const double* hi, const double* lb, const double* ub)
{
  if (!a_offsets || !at_offsets) return fail(-1, "pdlpdev_create: bad argument");
  return create_impl(out, device, m, n, a_offsets, a_indices, a_values, at_offsets, at_indices, at_values, transpose_ready, user, c, lo,
                     hi, lb, ub, nullptr);
}

// The context of an analysed matrix (pdlpdev_analyze): A and A^T are already on the device (the analysis' arrays are adopted, nothing
// of the matrix crosses PCIe again), the layouts are built from them -- panels on the device, the others on the host from the
// structure it holds or fetches.  c / lo / hi / lb / ub are in the order of the matrices the device holds (the caller applies
// pdlpdev_analysis_maps when the analysis permuted them).  The analysis must be destroyed afterwards (pdlpdev_analysis_destroy).
int pdlpdev_create_from_analysis(pdlpdev_ctx** out, pdlpdev_analysis* an, const double* c, const double* lo, const double* hi,
                                 const double* lb, const double* ub)
{
  if (!an || an->adopted) return fail(-1, "pdlpdev_create_from_analysis: no (or an already consumed) analysis");
  const int32_t* a_off = analysis_host_off(an);
  // (a permuted matrix's indices live on the device: they come to the host only if a host construction asks for them -- 88 MB at 1e7
  // nonzeros; the caller's own array otherwise)
  const int32_t* a_idx = an->permuted ? nullptr : analysis_host_idx(an);
  const int32_t* t_off = analysis_host_t_off(an);
  return create_impl(out, an->device, an->m, an->n, a_off, a_idx, nullptr, t_off, nullptr, nullptr, nullptr, nullptr, c, lo, hi, lb, ub, an);
}
}  // extern "C"

int layout_policy(LayoutPolicy* p)
{
  static const char* const names[] = {"auto", "stream", "panel", "jag", "pb", "timed"};  // (LayoutPolicy::Mode's order)
  const char* mode = getenv("CUOPT_AMD_SPMV_LAYOUT");
  const auto* it   = std::find_if(std::begin(names), std::end(names), [&](const char* s) { return strcmp(s, mode ? mode : "auto") == 0; });
  if (it == std::end(names)) return fail(-1, "CUOPT_AMD_SPMV_LAYOUT must be auto, stream, panel, jag, pb or timed");
  p->mode = (LayoutPolicy::Mode)(it - std::begin(names));
  // 1.33 MiB of the gathered vector per slab: measured optimum on the 1e6 x 1e6 random LP (6 slabs: 71 us per
  // SpMV; 8 slabs of 1 MiB: 74 us; 4 slabs of 2 MiB: 75 us) -- fewer tiles per panel against L2 capacity
  p->slab_bytes = std::max<int64_t>(64, cuopt_amd::tune_int("slab_bytes", 1398102));
  p->ws_limit   = cuopt_amd::tune_int("panel_ws_bytes", kPanelWorkingSetBytes);
  p->pb_device  = cuopt_amd::tune_int("pb_device", 1) != 0;
  p->jag_device = cuopt_amd::tune_int("jag_device", 1) != 0;
  return 0;
}

namespace {
// One matrix as the layout walk sees it (A: m x n, A^T: n x m).  The walk runs on the host alone when `device` is false: then it
// neither allocates from the context nor enqueues on its stream, and may run on a thread of its own.
struct LayoutSide {
  const char* name = "";
  int32_t rows = 0, cols = 0;
  const int32_t* off = nullptr;  // the hot CSR on the host: offsets, and the indices once the host holds them
  const int32_t* idx = nullptr;
  pdlpdev_analysis* an = nullptr;  // (null indices: an analysed matrix's, fetched from it on first use)
  bool transposed = false;
  const int32_t *d_off = nullptr, *d_idx = nullptr;  // the hot CSR on the device
  const double* d_val = nullptr;
  bool device = false;    // an analysed matrix without dense segments: the live gather set is counted and the layouts built there
  bool skip_jag = false;  // the analysis' sampled estimate already rules the jagged layout out
  const std::vector<int32_t>* first_seg = nullptr;  // A's dense segments (host panels)
  pdlpdev_ctx::MatrixSide* side = nullptr;  // the context's side: its layout slots are what the walk fills
  std::function<void(const std::string&)> lap;
  // what the walk leaves: the host constructions (upload_side takes them to the device), the live gather set once counted, and why
  // the gather-free layout turned the matrix away
  JagHost jh;
  PbHost pbh;
  PanelHost ph;
  int64_t ws = -1;
  std::string why;
  const int32_t* host_idx()
  {
    if (!idx) idx = transposed ? analysis_host_t_idx(an) : analysis_host_idx(an);
    return idx;
  }
};

// Panels when the CSR stream kernel's live gather set overflows what an XCD's L2 keeps of it (auto); counted once per side, on the
// device where the indices are, else on the host -- from the four windows alone when the host does not hold the indices.
int want_panels(pdlpdev_ctx* ctx, const LayoutPolicy& P, LayoutSide& s, bool* want)
{
  const bool timed = P.mode == LayoutPolicy::kTimed, timing = getenv("CUOPT_AMD_TIMING") != nullptr;
  *want = P.mode == LayoutPolicy::kPanel || (timed && !timing);
  if (*want || (!timed && (P.mode != LayoutPolicy::kAuto || (int64_t)s.cols * 8 <= P.ws_limit))) return 0;
  if (s.ws < 0) {
    int64_t ws = 0;
    const int rc = s.device ? gather_working_set_device(ctx, s.d_idx, s.off[s.rows], s.cols, &ws) : 1;
    if (rc < 0) return rc;
    if (rc == 1 && s.idx) {
      ws = gather_working_set(s.rows, s.cols, s.off, s.idx);
    } else if (rc == 1) {  // (beyond ~2e7 columns the device's bitmap leaves the LDS)
      std::vector<int32_t> sparse;
      std::vector<std::pair<int64_t, int64_t>> windows;
      if (analysis_fetch_idx_windows(s.an, s.transposed ? 1 : 0, (int64_t)s.off[s.rows], &sparse, &windows) != 0) return 0;
      ws = gather_working_set_windows(s.cols, sparse.data(), windows);
    }
    s.ws = ws;
    if (timing)
      fprintf(stderr, "[cuopt_amd setup]   layout %-3s: live gather set of the stream kernel %.2f MiB (limit %.2f) -> %s\n", s.name,
              ws / 1048576.0, P.ws_limit / 1048576.0, ws > P.ws_limit ? "panels" : "stream");
  }
  *want = timed || s.ws > P.ws_limit;
  return 0;
}

// One construction per layout: the device builder where it applies (kernels_layout_build.hip: < 0 error, 0 done -- dst->on says
// whether the layout was built --, 1 the host must build it), else the host construction, which upload_side takes to the device.
int side_jag(pdlpdev_ctx* ctx, const LayoutPolicy& P, LayoutSide& s)
{
  const int mode = P.mode == LayoutPolicy::kJag ? 1 : 0;
  const int rc   = s.device && P.jag_device ? build_jag_device(ctx, &s.side->jag, s.rows, s.cols, s.off, s.d_off, s.d_idx, s.d_val, mode, ctx->cus, ctx->batch_lanes) : 1;
  if (rc == 1) s.jh = build_jag(s.rows, s.cols, s.off, s.host_idx(), mode, ctx->cus, ctx->batch_lanes);
  s.lap(std::string("jag ") + s.name);
  return rc < 0 ? rc : 0;
}

int side_pb(pdlpdev_ctx* ctx, const LayoutPolicy& P, LayoutSide& s)
{
  const bool forced = P.mode == LayoutPolicy::kPb;
  const int rc      = s.device && P.pb_device ? build_pb_device(ctx, &s.side->pb, s.rows, s.cols, s.off, s.d_off, s.d_idx, ctx->cus, forced, &s.why) : 1;
  if (rc == 1) {
    s.pbh = build_pb(s.rows, s.cols, s.off, s.host_idx(), ctx->cus, forced);
    s.why = s.pbh.why;
  }
  s.lap(std::string("gather-free ") + s.name);
  return rc < 0 ? rc : 0;
}

int side_panels(pdlpdev_ctx* ctx, const LayoutPolicy& P, LayoutSide& s)
{
  const bool force = P.mode != LayoutPolicy::kTimed;  // (timed: only where the panels apply at all; pick_layout times them)
  const int rc     = s.device ? build_panels_device(ctx, &s.side->pan, s.rows, s.cols, s.off, s.d_off, s.d_idx, s.d_val, P.slab_bytes, force) : 1;
  if (rc == 1) s.ph = build_panels(s.rows, s.cols, s.off, s.host_idx(), P.slab_bytes, force, s.first_seg);
  s.lap(std::string("panels ") + s.name);
  return rc < 0 ? rc : 0;
}

// The candidates of one side, in order: jagged rows, the gather-free layout, slab-major panels; the CSR stream when none is built.
int layout_walk(pdlpdev_ctx* ctx, const LayoutPolicy& P, LayoutSide& s)
{
  if (P.try_jag() && !s.skip_jag) TRY(side_jag(ctx, P, s));
  if (s.jh.ok || s.side->jag.on) return 0;
  bool panels = false;
  if (P.want_pb(s.cols)) {
    if (P.mode != LayoutPolicy::kPb) TRY(want_panels(ctx, P, s, &panels));
    if (P.mode == LayoutPolicy::kPb || panels) TRY(side_pb(ctx, P, s));
    if (s.pbh.ok || s.side->pb.on) return 0;
  }
  if (P.mode == LayoutPolicy::kStream || P.mode == LayoutPolicy::kJag || P.mode == LayoutPolicy::kPb) return 0;
  TRY(want_panels(ctx, P, s, &panels));
  return panels ? side_panels(ctx, P, s) : 0;
}

// the walk's host constructions to the device (on the main thread, after the walk wherever it ran)
int upload_side(pdlpdev_ctx* ctx, const LayoutPolicy& P, LayoutSide& s)
{
  if (s.jh.ok) TRY(upload_jag(ctx, &s.side->jag, s.jh, s.d_off, s.d_idx, s.d_val));
  TRY(upload_pb(ctx, &s.side->pb, s.pbh));
  if (P.mode == LayoutPolicy::kPb && !s.side->pb.on) return fail(-1, "CUOPT_AMD_SPMV_LAYOUT=pb: %s does not fit the gather-free layout (%s)", s.name, s.why.c_str());
  return upload_panels(ctx, &s.side->pan, s.ph, s.d_off, s.d_idx, s.d_val);
}

// A's panels with dense segments: the segments of the own rows (a workgroup each), in own-row order -- those workgroups add them
int own_segments(pdlpdev_ctx* ctx, const DenseHost& DH, const PanelHost& ha)
{
  // (the rows that own segments are a subset of the own rows and both lists ascend)
  std::vector<int32_t> own_seg(ha.own_row.size() + 1, 0);
  for (size_t i = 0; i < ha.own_row.size(); ++i) {
    const int32_t f = DH.first_seg[ha.own_row[i]];
    int32_t cnt     = 0;
    for (int32_t q = f; f >= 0 && q < (int32_t)DH.seg_row.size() && DH.seg_row[q] == ha.own_row[i]; ++q) ++cnt;
    own_seg[i + 1] = own_seg[i] + cnt;
  }
  int32_t* d_own_seg = nullptr;
  TRY(upload_i32(ctx, &d_own_seg, own_seg.data(), own_seg.size()));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  PanelView& v = ctx->A.pan.v;
  v.dn_own_seg = d_own_seg, v.dn_seg_c0 = ctx->dense.seg_c0, v.dn_seg_len = ctx->dense.seg_len, v.dn_seg_ptr = ctx->dense.seg_ptr;
  v.dn_seg_row = ctx->dense.seg_row, v.dn_val = ctx->dense.val;
  return 0;
}

// A^T's panels with dense segments: per panel the segments that reach into its column range (ascending rows = segment numbers), for
// the column epilogue -- when no panel meets more than kPanelDenseSegs and there are no own rows (else k_dense_cols in front, as for
// the other layouts)
int column_segments(pdlpdev_ctx* ctx, const DenseHost& DH, const PanelHost& hat)
{
  const std::vector<int32_t>& row0 = hat.row0;
  std::vector<int32_t> pan_ptr(row0.size(), 0), pan_seg;
  bool fits = true;
  for (size_t w = 0; w + 1 < row0.size(); ++w) {
    for (size_t q = 0; q < DH.seg_row.size(); ++q)
      if (DH.seg_c0[q] < row0[w + 1] && DH.seg_c0[q] + DH.seg_len[q] > row0[w]) pan_seg.push_back((int32_t)q);
    pan_ptr[w + 1] = (int32_t)pan_seg.size();
    fits           = fits && pan_ptr[w + 1] - pan_ptr[w] <= kPanelDenseSegs;
  }
  if (!fits || !hat.own_row.empty()) return 0;
  int32_t *d_ptr = nullptr, *d_seg = nullptr;
  TRY(upload_i32(ctx, &d_ptr, pan_ptr.data(), pan_ptr.size()));
  TRY(upload_i32(ctx, &d_seg, pan_seg.data(), pan_seg.size()));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  PanelView& v = ctx->At.pan.v;
  v.dn_pan_ptr = d_ptr, v.dn_pan_seg = d_seg;
  v.dn_seg_c0 = ctx->dense.seg_c0, v.dn_seg_len = ctx->dense.seg_len, v.dn_seg_ptr = ctx->dense.seg_ptr;
  v.dn_seg_row = ctx->dense.seg_row, v.dn_val = ctx->dense.val;
  return 0;
}
}  // namespace

static int create_impl(pdlpdev_ctx** out, int device, int32_t m, int32_t n, const int32_t* a_offsets,
                       const int32_t* a_indices, const double* a_values, const int32_t* at_offsets,
                       const int32_t* at_indices, const double* at_values,
                       void (*transpose_ready)(void*), void* user, const double* c, const double* lo,
                       const double* hi, const double* lb, const double* ub, pdlpdev_analysis* an)
{
  roctx::Range range("pdlp: device set-up (upload, layouts)");
  const int batch_lanes = g_create_batch_lanes;
  g_create_batch_lanes  = 0;
  if (batch_lanes != 0 && batch_lanes != 2 && batch_lanes != 4 && batch_lanes != 8 && batch_lanes != 16)
    return fail(-1, "pdlpdev_create: batch_lanes must be 0, 2, 4, 8 or 16 (got %d)", batch_lanes);
  if (!out || m < 0 || n < 0 || !a_offsets || !at_offsets) return fail(-1, "pdlpdev_create: bad argument");
  if (pdlpdev_device_count() <= device)
    return fail(-5, "pdlpdev_create: no HIP device %d visible (this solver has no CPU fallback)", device);
  HIP_TRY(hipSetDevice(device));
  const bool timing = getenv("CUOPT_AMD_TIMING") != nullptr;
  auto tlast = std::chrono::steady_clock::now();
  pdlpdev_ctx* ctx = nullptr;
  auto lap = [&](const std::string& what) {
    if (!timing) return;
    // (the context's own stream: a device-wide synchronisation would break a graph capture another thread's solver is in the middle of)
    if (ctx && ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    else (void)hipDeviceSynchronize();
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[cuopt_amd setup]   dev: %-22s %8.2f ms\n", what.c_str(), 1e3 * std::chrono::duration<double>(now - tlast).count());
    tlast = now;
  };
  ctx         = new pdlpdev_ctx();
  ctx->device = device;
  ctx->batch_lanes = batch_lanes;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ctx->cus = cus;
  }
  ctx->m = m, ctx->n = n, ctx->nnz = a_offsets[m];
  ctx->A.name = "A", ctx->A.rows = m, ctx->A.cols = n;
  ctx->At.name = "A^T", ctx->At.rows = n, ctx->At.cols = m;
  *out = ctx;
  {
    Recycled r;
    if (an && an->bundle_owned && an->stream && an->pinned && an->chunk) {  // the analysis' stream, pinned block and chunk move here
      ctx->stream = an->stream, ctx->scal_h = an->pinned, ctx->arena = an->chunk, ctx->first_chunk = an->chunk;
      an->bundle_owned = false;
      HIP_TRY(hipMemsetAsync(ctx->arena, 0, kArenaChunk, ctx->stream));
    } else if (g_create_stream_donor && g_create_stream_donor->device == device) {  // pdlpdev_create_share_stream
      ctx->stream = g_create_stream_donor->stream, ctx->stream_borrowed = true;
      g_create_stream_donor = nullptr;
      HIP_TRY(hipHostMalloc((void**)&ctx->scal_h, kScalars * sizeof(double) + sizeof(pdlpdev_ctl)));
      HIP_TRY(hipMalloc((void**)&ctx->arena, kArenaChunk));
      HIP_TRY(hipMemsetAsync(ctx->arena, 0, kArenaChunk, ctx->stream));
      ctx->first_chunk = ctx->arena;
    } else if (take_recycled(device, &r)) {
      ctx->stream = r.stream, ctx->scal_h = r.pinned, ctx->arena = r.chunk, ctx->first_chunk = r.chunk;
      HIP_TRY(hipMemsetAsync(ctx->arena, 0, kArenaChunk, ctx->stream));
    } else {
      HIP_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
      HIP_TRY(hipHostMalloc((void**)&ctx->scal_h, kScalars * sizeof(double) + sizeof(pdlpdev_ctl)));  // one pinned block
      HIP_TRY(hipMalloc((void**)&ctx->arena, kArenaChunk));
      HIP_TRY(hipMemsetAsync(ctx->arena, 0, kArenaChunk, ctx->stream));
      ctx->first_chunk = ctx->arena;
    }
    ctx->ctl_h = (pdlpdev_ctl*)(ctx->scal_h + kScalars);
  }
  const size_t nnz = (size_t)ctx->nnz;
  // Everything that needs A only comes first; the caller may still be transposing on other threads (A^T is not
  // touched before transpose_ready returns).
  if (an) {
    // adopted: both matrices are the analysis' device arrays (allocated with the 8 spare entries the stream kernel may over-read)
    ctx->A.full  = pdlpdev_ctx::Csr{an->A.off, an->A.idx, an->A.val};
    ctx->At.full = pdlpdev_ctx::Csr{an->At.off, an->At.idx, an->At.val};
    for (void* p : {(void*)an->A.off, (void*)an->A.idx, (void*)an->A.val, (void*)an->At.off, (void*)an->At.idx, (void*)an->At.val}) {
      an->owned.erase(std::remove(an->owned.begin(), an->owned.end(), p), an->owned.end());
      ctx->allocs.push_back(p);
    }
    an->adopted = true;
    ctx->bytes += (int64_t)(2 * (nnz + 8) * 12 + ((size_t)m + n + 2) * 4);
  } else {
    TRY(upload_i32(ctx, &ctx->A.full.off, a_offsets, (size_t)m + 1));
    TRY(upload_i32(ctx, &ctx->A.full.idx, a_indices, nnz, 8));  // +8: the vector loads of the stream kernel may over-read
    TRY(upload_f64(ctx, &ctx->A.full.val, a_values, nnz, 8));
  }
  lap("alloc + upload A");
  auto long_rows = [](int32_t rows, const int32_t* off) {
    constexpr int kParts = 16;
    std::vector<int32_t> part[kParts], v;
    cuopt_amd::parallel_tasks(kParts, [&](int t) {
      const int32_t a = (int32_t)((int64_t)rows * t / kParts), b = (int32_t)((int64_t)rows * (t + 1) / kParts);
      for (int32_t r = a; r < b; ++r)
        if (off[r + 1] - off[r] > kLongRow) part[t].push_back(r);
    }, (int64_t)rows * 8);
    for (int t = 0; t < kParts; ++t) v.insert(v.end(), part[t].begin(), part[t].end());
    return v;
  };
  std::vector<int32_t> la = long_rows(m, a_offsets), lat;  // alive until the stream is synchronised at the end
  ctx->A.nlong = (int)la.size();
  if (ctx->A.nlong) TRY(upload_i32(ctx, &ctx->A.longs, la.data(), la.size()));
  // dense row segments leave the hot loop's copy of the matrix (single-GPU solves)
  const bool one_gpu = !g_create_sharded;
  g_create_sharded   = 0;
  DenseHost DH;
  std::vector<int32_t> hA_off, hA_idx, hA_perm, hT_off, hT_idx, hT_perm;  // the hot CSRs where they differ from the full ones
  lap("long rows A");
  auto a_idx_host = [&]() -> const int32_t* { return a_indices ? a_indices : (an ? analysis_host_idx(an) : nullptr); };
  if (one_gpu) {
    // (the scan reads the indices of rows with at least kDenseMin entries only: none of them, no indices needed)
    std::vector<int32_t> candidates;
    for (int32_t r : la)
      if (a_offsets[r + 1] - a_offsets[r] >= kDenseMin) candidates.push_back(r);
    // (no candidate: no segment can exist, and the pass over 1e6 rows was 0.26 ms.  A permuted matrix's indices live on the device:
    //  a few candidate rows -- the linking rows of a block-angular LP -- come over on their own instead of the whole 40 MB array)
    if (!candidates.empty()) {
      const int32_t* scan_idx = a_indices ? a_indices : (an && candidates.size() <= 64 ? analysis_host_idx_rows(an, a_offsets, candidates) : a_idx_host());
      find_dense_segments(m, n, a_offsets, scan_idx, &DH);
      if (DH.on && !a_indices) {  // (segments found after all: the host constructions behind them read every row)
        DenseHost again;
        find_dense_segments(m, n, a_offsets, a_idx_host(), &again);
        DH = std::move(again);
      }
    }
  }
  lap("dense scan");
  if (DH.on) hA_off.swap(DH.s_off), hA_idx.swap(DH.s_idx), hA_perm.swap(DH.s_perm);
  const bool hot_a     = !hA_off.empty();
  const int32_t* A_off = hot_a ? hA_off.data() : a_offsets;
  const int32_t* A_idx = hot_a ? hA_idx.data() : a_indices;  // (null: an analysed, permuted matrix whose indices stayed on the device)
  ctx->A.hot = ctx->A.full;
  ctx->A.hot_nnz = (int64_t)A_off[m];
  if (hot_a) {
    TRY(upload_i32(ctx, &ctx->A.hot.off, A_off, (size_t)m + 1));
    TRY(upload_i32(ctx, &ctx->A.hot.idx, A_idx, (size_t)ctx->A.hot_nnz, 8));
    TRY(dev_alloc(ctx, &ctx->A.hot.val, (size_t)ctx->A.hot_nnz + 8));
    TRY(upload_i32(ctx, &ctx->dense.s_perm_a, hA_perm.data(), hA_perm.size()));
  }
  if (DH.on) {
    pdlpdev_ctx::Dense& D = ctx->dense;
    D.nrows = (int)DH.row.size(), D.nseg = (int)DH.seg_row.size(), D.ntiles = (int)DH.tile_id.size(), D.nent = DH.nent;
    TRY(upload_i32(ctx, &D.row, DH.row.data(), DH.row.size()));
    TRY(upload_i32(ctx, &D.row_seg, DH.row_seg.data(), DH.row_seg.size()));
    TRY(upload_i32(ctx, &D.seg_row, DH.seg_row.data(), DH.seg_row.size()));
    TRY(upload_i32(ctx, &D.seg_c0, DH.seg_c0.data(), DH.seg_c0.size()));
    TRY(upload_i32(ctx, &D.seg_len, DH.seg_len.data(), DH.seg_len.size()));
    TRY(upload_i32(ctx, &D.seg_ptr, DH.seg_ptr.data(), DH.seg_ptr.size()));
    TRY(upload_i32(ctx, &D.tile_id, DH.tile_id.data(), DH.tile_id.size()));
    TRY(upload_i32(ctx, &D.tile_ptr, DH.tile_ptr.data(), DH.tile_ptr.size()));
    TRY(upload_i32(ctx, &D.tile_seg, DH.tile_seg.data(), DH.tile_seg.size()));
    TRY(upload_i32(ctx, &D.perm, DH.perm.data(), DH.perm.size()));
    D.nchunks = (int)DH.ch_seg.size();
    TRY(upload_i32(ctx, &D.ch_seg, DH.ch_seg.data(), DH.ch_seg.size()));
    TRY(upload_i32(ctx, &D.ch_k0, DH.ch_k0.data(), DH.ch_k0.size()));
    TRY(upload_i32(ctx, &D.row_ch, DH.row_ch.data(), DH.row_ch.size()));
    TRY(dev_alloc(ctx, &D.ch_part, (size_t)D.nchunks + 8));
    TRY(dev_alloc(ctx, &D.val, (size_t)D.nent + 8));
    D.on = true;
    if (timing) fprintf(stderr, "[cuopt_amd setup]   dense: %d segments in %d rows, %lld of %lld nonzeros stored index-free\n", D.nseg, D.nrows, (long long)D.nent, (long long)ctx->nnz);
  }
  if (DH.on) TRY(dev_alloc(ctx, &ctx->A.dense_add, (size_t)m));
  std::vector<int32_t> rba = build_row_blocks(m, A_off);
  lap("row blocks A");
  ctx->A.nb = (int)rba.size() / 2 - 1;
  TRY(upload_i32(ctx, &ctx->A.rb, rba.data(), rba.size()));
  TRY(lp_alloc_slab(ctx));  // (a large LP: the vectors below out of one zero-filled allocation)
  // every problem vector crosses PCIe once: the unscaled copy is made on the device, and a bound vector that is one value
  // throughout (all lower bounds 0, all upper bounds +inf: most LPs) is not uploaded at all
  lap("slab");
  ctx->note_uniform_bounds(lb, ub);
  lap("uniform bounds");
  auto upload_pair = [&](double** work, double** keep, const double* src, size_t count, bool uniform, double value) -> int {
    TRY(dev_alloc(ctx, work, count));
    TRY(dev_alloc(ctx, keep, count));
    if (count == 0) return 0;
    if (uniform) {
      k_fill<<<grid_for((int64_t)count), kBlock, 0, ctx->stream>>>((int64_t)count, *work, value);
    } else if (const double* on_device = an ? an->prefetched(src) : nullptr) {  // (sent ahead while the analysis ran: kernels_setup.hip)
      HIP_TRY(hipMemcpyAsync(*work, on_device, count * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    } else {
      HIP_TRY(hipMemcpyAsync(*work, src, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(hipMemcpyAsync(*keep, *work, count * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
  };
  TRY(upload_pair(&ctx->c, &ctx->c_u, c, (size_t)n, false, 0.0));
  TRY(upload_pair(&ctx->lb, &ctx->lb_u, lb, (size_t)n, ctx->ubd.lb_same != 0, ctx->ubd.lb));
  TRY(upload_pair(&ctx->ub, &ctx->ub_u, ub, (size_t)n, ctx->ubd.ub_same != 0, ctx->ubd.ub));
  TRY(upload_pair(&ctx->lo, &ctx->lo_u, lo, (size_t)m, false, 0.0));
  TRY(upload_pair(&ctx->hi, &ctx->hi_u, hi, (size_t)m, false, 0.0));
  lap("vector uploads");
  TRY(dev_alloc(ctx, &ctx->dr, m)); TRY(dev_alloc(ctx, &ctx->dc, n));
  TRY(lp_alloc_iterate(ctx));
  const size_t slab_rest = ctx->slab_cap - ctx->slab_used;  // (kept for the n-sized buffers allocated after the layouts)
  ctx->slab_cap = ctx->slab_used;
  LayoutPolicy P;
  TRY(layout_policy(&P));
  lap("row blocks + vectors");
  {
    // One walk per side (layout_walk).  A^T's runs on a thread of its own, next to the A side, when no device construction applies
    // to it (the caller's matrices, or dense segments): the caller's transposition, the hot CSR and the constructions are host work
    // then, and the main thread uploads what it built after the join.  An analysed matrix has nothing to wait for and little left to
    // do on the host: its A^T side runs inline, after A^T's uploads (a thread of its own took 3 ms to do 0.5 ms of work next to the
    // main thread's HIP calls).
    const bool at_thread = !an || DH.on;
    auto init_side = [&](LayoutSide& s, pdlpdev_ctx::MatrixSide* side, int t) {
      s.side = side, s.name = side->name, s.rows = side->rows, s.cols = side->cols, s.an = an, s.transposed = t != 0;
      s.device   = an && !DH.on;
      s.skip_jag = an && an->estimated && !an->permuted && P.mode != LayoutPolicy::kJag && an->saving_natural[t] < 0.35;
    };
    LayoutSide T;
    init_side(T, &ctx->At, 1);
    T.off = at_offsets, T.idx = at_indices;  // (the device's hot CSR once it is uploaded, below)
    const auto w0 = std::chrono::steady_clock::now();
    auto wlap = [&](const std::string& what) {
      if (timing) fprintf(stderr, "[cuopt_amd setup]   A^T thread: %-22s at %6.2f ms\n", what.c_str(), 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count());
    };
    if (at_thread) T.lap = wlap;
    else T.lap = lap;
    std::vector<int32_t> rbt;
    int at_rc = 0;
    auto at_side = [&](bool walk) {
      if (transpose_ready) transpose_ready(user);
      if ((int64_t)at_offsets[n] != ctx->nnz) return;  // (reported below)
      lat = long_rows(n, at_offsets);
      wlap("long rows");
      if (DH.on) {
        strip_transpose(DH, &DH, n, at_offsets, T.host_idx());
        hT_off.swap(DH.st_off), hT_idx.swap(DH.st_idx), hT_perm.swap(DH.st_perm);
      }
      if (!hT_off.empty()) T.off = hT_off.data(), T.idx = hT_idx.data();
      rbt = build_row_blocks(n, T.off);
      wlap("row blocks");
      if (walk) at_rc = layout_walk(ctx, P, T);
    };
    struct Join {
      std::thread t;
      ~Join() { if (t.joinable()) t.join(); }
    } worker;  // (an early return waits for the A^T side too)
    if (at_thread) worker.t = std::thread(at_side, true);
    {
      LayoutSide A;  // (its host constructions go back to the pool at the end of this block)
      init_side(A, &ctx->A, 0);
      A.off = A_off, A.idx = A_idx, A.d_off = ctx->A.hot.off, A.d_idx = ctx->A.hot.idx, A.d_val = ctx->A.hot.val, A.lap = lap;
      A.first_seg = DH.on ? &DH.first_seg : nullptr;
      TRY(layout_walk(ctx, P, A));
      TRY(upload_side(ctx, P, A));
      if (ctx->A.pan.on && DH.on) TRY(own_segments(ctx, DH, A.ph));
      lap("upload layouts A");
    }
    if (at_thread) worker.t.join();
    else at_side(false);
    lap("wait for the A^T side");
    if ((int64_t)at_offsets[n] != ctx->nnz) return fail(-1, "pdlpdev_create: A and A^T disagree on nnz");
    if (!an) {
      TRY(upload_i32(ctx, &ctx->At.full.off, at_offsets, (size_t)n + 1));
      TRY(upload_i32(ctx, &ctx->At.full.idx, at_indices, nnz, 8));
      TRY(upload_f64(ctx, &ctx->At.full.val, at_values, nnz, 8));
    }
    ctx->At.nlong = (int)lat.size();
    if (ctx->At.nlong) TRY(upload_i32(ctx, &ctx->At.longs, lat.data(), lat.size()));
    const bool hot_t = !hT_off.empty();
    ctx->At.hot = ctx->At.full;
    ctx->At.hot_nnz = (int64_t)T.off[n];
    if (hot_t) {
      TRY(upload_i32(ctx, &ctx->At.hot.off, T.off, (size_t)n + 1));
      TRY(upload_i32(ctx, &ctx->At.hot.idx, T.idx, (size_t)ctx->At.hot_nnz, 8));
      TRY(dev_alloc(ctx, &ctx->At.hot.val, (size_t)ctx->At.hot_nnz + 8));
      TRY(upload_i32(ctx, &ctx->dense.s_perm_at, hT_perm.data(), hT_perm.size()));
    }
    if (DH.on) TRY(dev_alloc(ctx, &ctx->At.dense_add, (size_t)n));
    ctx->At.nb = (int)rbt.size() / 2 - 1;
    TRY(upload_i32(ctx, &ctx->At.rb, rbt.data(), rbt.size()));
    lap("upload A^T");
    T.d_off = ctx->At.hot.off, T.d_idx = ctx->At.hot.idx, T.d_val = ctx->At.hot.val;
    TRY(at_thread ? at_rc : layout_walk(ctx, P, T));
    TRY(upload_side(ctx, P, T));
    if (ctx->At.pan.on && DH.on) TRY(column_segments(ctx, DH, T.ph));
    lap("upload layouts A^T");
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the staged copies have left the host arrays
  }
  {
    // small LPs: a whole batch of attempts inside one workgroup (CUOPT_AMD_SMALL=0 switches it off)
    const char* small_env = getenv("CUOPT_AMD_SMALL");
    const int tier        = resident_tier(m, n, ctx->nnz);
    ctx->eval_reuse_aty   = cuopt_amd::tune_int("eval_reuse_aty", 1) != 0;
    const long long decides_key = cuopt_amd::tune_int("primal_decides", -1);
    ctx->primal_decides   = decides_key < 0 ? n >= pdlpdev_ctx::kPrimalDecidesMinCols : decides_key != 0;
    ctx->primal_decide_grid_cap = (int)std::max<long long>(1, std::min<long long>(cuopt_amd::tune_int("primal_decide_grid", 512), 512));
    ctx->small_resident   = tier >= 0 && !(small_env && atoi(small_env) == 0) && !ctx->A.dense_add && !ctx->At.dense_add && !g_create_no_resident;
    g_create_no_resident  = 0;
    if (small_env && atoi(small_env) != 0 && tier < 0)
      return fail(-1, "CUOPT_AMD_SMALL=1: the LP does not fit the resident kernel (m, n <= 2048, nnz <= 4096 ...)");
  }
  ctx->slab_cap += slab_rest;
  for (pdlpdev_ctx::MatrixSide* s : {&ctx->A, &ctx->At}) {
    // every layout adds what the dense segments contribute ahead of its epilogue (null: nothing to add) -- except the panels whose
    // kernels add the segments themselves (own-row workgroups / the column epilogue): no launch in front
    s->pan.v.dense_add = s->jag.v.dense_add = s->pb.v.dense_add = s->dense_add;
    if (s->pan.v.dn_own_seg || s->pan.v.dn_pan_ptr) s->pan.v.dense_add = nullptr;
  }
  TRY(lp_alloc_partials(ctx));
  lap("partial buffers");
  k_fill<<<grid_for(m), kBlock, 0, ctx->stream>>>(m, ctx->dr, 1.0);
  k_fill<<<grid_for(n), kBlock, 0, ctx->stream>>>(n, ctx->dc, 1.0);
  HIP_TRY(hipGetLastError());
  lap("fill D");
  TRY(sync_panel_values(ctx));
  lap("panel values (permute)");
  if (P.mode == LayoutPolicy::kTimed) {
    TRY(pick_layout(ctx, &ctx->A, ctx->tmp_n, ctx->tmp_m));
    lap("layout autotune A");
    TRY(pick_layout(ctx, &ctx->At, ctx->tmp_m, ctx->tmp_n));
    lap("layout autotune");
  }
  // Zero skip: the bitmap of xbar's non-zeros (whole 16-byte quads) and the counts -- only for a context whose A product can ever read
  // them (attempt_xmask, pdlp_device.hip: one GPU, A in the row-sum panels), and as the LAST allocation of the set-up, so that no
  // other buffer of any context lies anywhere else than it would without them.
  if (one_gpu && !ctx->small_resident && ctx->A.layout() == pdlpdev_ctx::MatrixSide::kPanel && !ctx->A.pan.v.seg && cuopt_amd::tune_int("zero_skip", 1) != 0) {
    const size_t words = 2 * (((size_t)n + 127) / 128);
    ctx->zs_mode = cuopt_amd::tune_int("zero_skip", 1) == 2 ? 2 : 1;
    TRY(dev_alloc(ctx, &ctx->zcount, (size_t)grid_for(n)));
    TRY(dev_alloc(ctx, &ctx->xmask, words + 2));  // (+ the quad of the masked launches' counter)
    HIP_TRY(hipMemsetAsync(ctx->xmask, 0, (words + 2) * sizeof(unsigned long long), ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  scratch_free(ctx);  // (the layout constructions' temporaries: both sides are built)
  return 0;
}

extern "C" {

void pdlpdev_destroy(pdlpdev_ctx* ctx)
{
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  scratch_free(ctx);
  for (auto& kv : ctx->graphs) (void)hipGraphExecDestroy(kv.second);
  if (ctx->shared_with_parent && ctx->parent) ctx->parent->clones_alive -= 1;
  if (ctx->batches_alive > 0)  // (a batch holds plain pointers to its members: destroy it first)
    fprintf(stderr, "[cuopt_amd] pdlpdev_destroy: %d batch(es) still hold this context -- destroy the batch before its members\n", ctx->batches_alive);
  if (ctx->clones_alive > 0)  // (a contract of pdlpdev_clone_shared; said aloud, since what follows frees the clones' matrices)
    fprintf(stderr, "[cuopt_amd] pdlpdev_destroy: %d clone(s) of this context are still alive -- they alias its matrices and must be destroyed first\n", ctx->clones_alive);
  for (void* mapped : ctx->p2p.opened) (void)hipIpcCloseMemHandle(mapped);
  if (ctx->p2p.base) (void)hipFree(ctx->p2p.base);
  if (ctx->comm && !ctx->soft) comm_cache::release(ctx->comm_key);
  for (void* p : ctx->allocs) (void)hipFree(p);
  if (ctx->hal_h) (void)hipHostFree(ctx->hal_h);
  if (ctx->hmaj_ring) (void)hipHostFree(ctx->hmaj_ring);
  const bool whole = ctx->stream && ctx->scal_h && ctx->first_chunk && !ctx->shared_with_parent && !ctx->stream_borrowed;
  if (!(whole && give_recycled(Recycled{ctx->device, ctx->stream, ctx->scal_h, ctx->first_chunk}))) {
    if (ctx->first_chunk) (void)hipFree(ctx->first_chunk);
    if (ctx->scal_h) (void)hipHostFree(ctx->scal_h);  // ctl_h lives in the same block
    if (ctx->stream && !ctx->shared_with_parent && !ctx->stream_borrowed) (void)hipStreamDestroy(ctx->stream);
  }
  delete ctx;
}

}  // extern "C"
