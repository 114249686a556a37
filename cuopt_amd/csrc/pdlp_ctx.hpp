#pragma once
// HIP/gfx950 device layer of the MI355X-native PDLP solver: kernels + the `pdlpdev_*` C-ABI
// declared in include/cuopt_amd/pdlp_device.h (which lists the reference code each entry point
// replaces).  Hand-written for CDNA4: wave64, LDS-staged CSR stream SpMV with fused PDHG epilogues,
// device-resident step acceptance (no host round trip per PDHG step), hipGraph replay.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <tuple>
#include <utility>

#include <dlfcn.h>
#include <unistd.h>
#include <mutex>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "host_parallel.hpp"
#include "pdlp_kernels.hpp"
#include "pdlp_epilogues.hpp"
#include "pdlp_kernel_decls.hpp"

using namespace pdlp;

// ================================================================================================
// error plumbing
// ================================================================================================
inline thread_local std::string g_err;
inline int fail(int code, const char* fmt, ...)
{
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(-2, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// ================================================================================================
// RCCL, bound lazily so that the library loads (and the single-GPU path runs) without it
// ================================================================================================
namespace rccl {
typedef struct ncclComm* comm_t;
typedef struct { char internal[128]; } unique_id;
enum { kFloat64 = 8 };           // ncclDouble
enum { kSum = 0, kMax = 2 };     // ncclSum / ncclMax
inline void* lib;
inline int (*GetUniqueId)(unique_id*);
inline int (*CommInitRank)(comm_t*, int, unique_id, int);
inline int (*CommDestroy)(comm_t);
inline int (*CommAbort)(comm_t);
inline int (*AllReduce)(const void*, void*, size_t, int, int, comm_t, hipStream_t);
inline int (*ReduceScatter)(const void*, void*, size_t, int, int, comm_t, hipStream_t);
inline int (*AllGather)(const void*, void*, size_t, int, comm_t, hipStream_t);
inline int (*Send)(const void*, size_t, int, int, comm_t, hipStream_t);  // halo exchange of a sharded structured LP
inline int (*Recv)(void*, size_t, int, int, comm_t, hipStream_t);
inline int (*GroupStart)();
inline int (*GroupEnd)();
inline const char* (*GetErrorString)(int);
inline std::mutex load_mutex;
inline int load()
{
  std::lock_guard<std::mutex> guard(load_mutex);
  if (lib) return 0;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (const char* nm : names) {
    lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
    if (lib) break;
  }
  if (!lib) return fail(-3, "RCCL not found (dlopen librccl.so.1): %s", dlerror());
  *(void**)&GetUniqueId    = dlsym(lib, "ncclGetUniqueId");
  *(void**)&CommInitRank   = dlsym(lib, "ncclCommInitRank");
  *(void**)&CommDestroy    = dlsym(lib, "ncclCommDestroy");
  *(void**)&CommAbort      = dlsym(lib, "ncclCommAbort");
  *(void**)&AllReduce      = dlsym(lib, "ncclAllReduce");
  *(void**)&ReduceScatter  = dlsym(lib, "ncclReduceScatter");
  *(void**)&AllGather      = dlsym(lib, "ncclAllGather");
  *(void**)&Send           = dlsym(lib, "ncclSend");
  *(void**)&Recv           = dlsym(lib, "ncclRecv");
  *(void**)&GroupStart     = dlsym(lib, "ncclGroupStart");
  *(void**)&GroupEnd       = dlsym(lib, "ncclGroupEnd");
  *(void**)&GetErrorString = dlsym(lib, "ncclGetErrorString");
  if (!GetUniqueId || !CommInitRank || !CommDestroy || !AllReduce)
    return fail(-3, "RCCL symbols missing");
  return 0;
}
}  // namespace rccl
#define RCCL_TRY(expr)                                                                     \
  do {                                                                                     \
    int r_ = (expr);                                                                       \
    if (r_ != 0)                                                                           \
      return fail(-4, "%s failed: %s", #expr,                                              \
                  rccl::GetErrorString ? rccl::GetErrorString(r_) : "rccl error");         \
  } while (0)


// RCCL communicators of this process: one per (unique id, rank), shared by the solvers created with the same pair while
// any of them is alive (reference count); the last solver to go destroys it -- a unique id bootstraps exactly one communicator
// per rank, so a caller that creates a second solver after the first one is gone draws a new id.
namespace comm_cache {
struct Entry {
  rccl::comm_t comm;
  int refs;
  bool aborted = false;
};
inline std::mutex mu;
inline std::map<std::string, Entry> map;
inline void release(const std::string& key)
{
  rccl::comm_t dead = nullptr;
  bool aborted      = false;
  {
    std::lock_guard<std::mutex> lock(mu);
    auto it = map.find(key);
    if (it == map.end() || --it->second.refs > 0) return;
    dead = it->second.comm, aborted = it->second.aborted;
    map.erase(it);
  }
  if (dead && !aborted && rccl::CommDestroy) (void)rccl::CommDestroy(dead);  // (ncclCommAbort already freed an aborted one)
}
}  // namespace comm_cache

// ================================================================================================
// in-process "soft" communicator (verification of the sharded path at world > 1 on one GPU)
// ================================================================================================
#include <condition_variable>
#include <mutex>
namespace softcomm {
constexpr char kMagic[8] = {'C', 'U', 'O', 'P', 'T', 'S', 'F', 'T'};
struct Comm {
  int world = 0;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0, generation = 0;
  int refs = 0;                  // solvers attached (the last one to leave frees the communicator)
  bool aborted = false;          // a rank failed: every barrier returns false from now on, nobody waits for the missing rank
  std::vector<double*> bufs;     // this round's buffer of every rank
  std::vector<double*> scratch;  // per-rank result staging
  std::vector<size_t> scratch_size;
  std::vector<void*> p2p_base;   // direct-peer transport: every rank's landing block (same device, same process)
  bool barrier()
  {
    std::unique_lock<std::mutex> lk(mu);
    if (aborted) return false;
    const int gen = generation;
    if (++arrived == world) {
      arrived = 0;
      ++generation;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return gen != generation || aborted; });
    }
    return !aborted;
  }
  void abort()
  {
    std::lock_guard<std::mutex> lk(mu);
    aborted = true;
    cv.notify_all();
  }
};
#define SOFT_BARRIER(c)                                                                                   \
  do {                                                                                                    \
    if (!(c)->barrier()) return fail(-6, "in-process communicator: another rank failed, solve abandoned"); \
  } while (0)
struct Peers {
  const double* p[16];
};
static __global__ void __launch_bounds__(256) k_combine(Peers peers, int world, size_t count, int op, double* __restrict__ out)
{
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
    double acc = peers.p[0][i];
    for (int r = 1; r < world; ++r) {  // fixed rank order -> every rank computes the same bits
      const double v = peers.p[r][i];
      acc            = op == 0 ? acc + v : (v > acc ? v : acc);
    }
    out[i] = acc;
  }
}
}  // namespace softcomm

// ---- roctx ranges (the reference marks every phase with NVTX: LP/pdhg.cu:75,168,241, LP/pdlp.cu:541,1227) --------------
// bound lazily like RCCL: without the library (or with CUOPT_AMD_ROCTX=0) the calls are no-ops
namespace roctx {
inline int (*Push)(const char*) = nullptr;
inline int (*Pop)()             = nullptr;
inline std::once_flag once;
inline void load()
{
  std::call_once(once, [] {
    if (cuopt_amd::tune_int("roctx", 1) == 0) return;
    for (const char* name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
      if (void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {
        Push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        Pop  = (int (*)())dlsym(h, "roctxRangePop");
        if (Push && Pop) return;
        Push = nullptr, Pop = nullptr;
      }
    }
  });
}
struct Range {
  explicit Range(const char* name)
  {
    load();
    if (Push) Push(name);
  }
  ~Range()
  {
    if (Pop) Pop();
  }
};
}  // namespace roctx

// ================================================================================================
// direct peer transport (owner-computes dataflow): push / pull kernels
// ================================================================================================
namespace p2pdev {
// wait until every rank's flag of exchange `kind` shows this rank's epoch, then landing -> dst (`count` doubles) EXCEPT this rank's
// own share [own0, own0 + own_count), which its producing kernel stored straight into dst.  Every workgroup polls for itself (local
// memory, one load per rank per poll); patience is bounded: a peer that never arrives sets the step error and the fault flag instead
// of hanging the device.  Four 16-byte requests per thread in flight (the landing block is fine-grained: every read is a trip to
// memory, and one request at a time ran at 0.75 TB/s).
static __global__ void __launch_bounds__(256) k_pull(pdlpdev_ctl* __restrict__ ctl, double* __restrict__ dst, const double* __restrict__ land, int count,
                                              int own0, int own_count, const unsigned long long* __restrict__ flags, int world, int kind,
                                              const unsigned long long* __restrict__ epoch, int* __restrict__ fault, const Push* __restrict__ push)
{
  if (!active(ctl)) return;
  raise(push);  // the producing kernel before this one in the stream is complete: its exchange is published here
  if (!wait_flags(flags, world, kind, epoch)) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *fault = 1, ctl->error = 1;
    return;
  }
  // (count, own0 and own_count are multiples of 16 entries and both buffers are 256-byte aligned: 16-byte requests)
  typedef double v2 __attribute__((ext_vector_type(2)));
  const v2* __restrict__ src2 = reinterpret_cast<const v2*>(land);
  v2* __restrict__ dst2       = reinterpret_cast<v2*>(dst);
  const int n2 = (count - own_count) >> 1, o2 = own0 >> 1, skip2 = own_count >> 1;  // pairs to copy; the own share is stepped over
  constexpr int U = 4;
  for (int i = blockIdx.x * 256 * U + threadIdx.x; i < n2; i += gridDim.x * 256 * U) {
    v2 v[U];
    int at[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = i + u * 256;
      at[u]       = k < n2 ? (k < o2 ? k : k + skip2) : -1;
      if (at[u] >= 0) v[u] = __builtin_nontemporal_load(src2 + at[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (at[u] >= 0) dst2[at[u]] = v[u];
  }
}
// the halo exchange's consumer: per peer ONE range [off, off + cnt) of the landed vector (buffer coordinates) instead of everything
struct PullRanges {
  int off[16], cnt[16];
};
static __global__ void __launch_bounds__(256) k_pull_ranges(pdlpdev_ctl* __restrict__ ctl, double* __restrict__ dst, const double* __restrict__ land, PullRanges R,
                                                     const unsigned long long* __restrict__ flags, int world, int kind, const unsigned long long* __restrict__ epoch,
                                                     int* __restrict__ fault, const Push* __restrict__ push)
{
  if (!active(ctl)) return;
  raise(push);
  if (!wait_flags(flags, world, kind, epoch)) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *fault = 1, ctl->error = 1;
    return;
  }
  for (int q = 0; q < world; ++q)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < R.cnt[q]; i += gridDim.x * 256) dst[R.off[q] + i] = __builtin_nontemporal_load(land + R.off[q] + i);
}
}  // namespace p2pdev

// ================================================================================================
// context
// ================================================================================================
constexpr size_t kSlicePad = 512;  // spare entries of the vectors that are exchanged in equal slices (sliced-primal dataflow)
struct pdlpdev_ctx;
// The context is three plain structs side by side (pdlpdev_ctx below inherits all of them: ctx->x reaches every field).
//
// CtxProblem: the problem as the device holds it, immutable once pdlpdev_scale_problem has run -- device, stream, dimensions, both
// matrices with their layouts, the objective, the scaling vectors, the tuning switches, the sharded dataflow.  Written by the set-up
// (pdlp_create.hip, pdlpdev_scale_problem, pdlpdev_owner_setup) only; pdlpdev_clone_shared copies this part, and nothing else, into a
// clone, which then ALIASES every array in it.  One exception: MatrixSide::part is per LP (each side's epilogue partials); it lives in
// the side because every launch site reads it from there, and lp_alloc_partials re-points it at the clone's own buffer.
struct CtxProblem {
  int device = 0;
  hipStream_t stream = nullptr;
  int32_t m = 0, n = 0;
  int64_t nnz = 0;
  int cus = 256;  // compute units of the device (hipDeviceProp_t::multiProcessorCount)
  // slab-major row panels (optional second layout of the same nonzeros, see pdlp_kernels.hpp)
  struct Panels {
    bool on = false;
    PanelView v{};
    int32_t* perm = nullptr;  // position in CSR order of each panel-order nonzero
    double* val   = nullptr;
    int64_t nent  = 0;        // nonzeros inside the panels (rows with a workgroup of their own are read from the CSR)
  };
  // sorted jagged rows with LDS column sets (third layout, structured matrices; pdlp_kernels.hpp)
  struct Jag {
    bool on = false;
    JagView v{};
    int32_t* perm = nullptr;  // position in CSR order of each jagged-order entry
    double* val   = nullptr;
    int64_t nent  = 0;
    double saving = 0.0;      // share of the global gathers the LDS column sets save (build_jag)
  };
  // gather-free layout (fourth layout: huge unstructured matrices; pdlp_kernels.hpp "pb")
  struct Pb {
    bool on = false;
    PbView v{};
    int32_t* perm = nullptr;  // position in CSR order of each padded P-order entry (-1: padding)
    double* val   = nullptr;
    int64_t np    = 0;        // padded entries
    int p_threads = 512;      // phase P workgroup: 512 (8192-column panels) or 1024 (16384)
    double pad    = 1.0;      // padded entries / nonzeros
  };
  struct Csr {
    int32_t *off = nullptr, *idx = nullptr;
    double* val = nullptr;
  };
  // What one matrix owns for the hot loop.  The context holds three: A (m x n), A^T (n x m) and, under the owner-computes dataflow, the
  // rank's column block.  At most one of the three layout slots is on; the CSR stream is the layout of a side with none.  The product
  // launches go through launch_product (pdlp_launch.hpp), the only other place that knows the four-way choice.
  struct MatrixSide {
    const char* name = "";
    int32_t rows = 0, cols = 0;
    Csr full;  // as uploaded (values are scaled in place by pdlpdev_scale_problem): the set-up kernels (norms, scaling) run on it
    Csr hot;   // what the hot loop multiplies: `full` unless dense segments left the matrix (Dense below)
    int64_t hot_nnz = 0;
    int32_t* rb = nullptr;  // row-block boundaries of the stream kernels
    int nb = 0;
    int32_t* longs = nullptr;  // rows with more than kLongRow nonzeros (set-up kernels give each a workgroup instead of a lane)
    int nlong = 0;
    Panels pan;
    Jag jag;
    Pb pb;
    double* part = nullptr;       // per-workgroup partials of the side's fused epilogue (8 quantities each)
    double* dense_add = nullptr;  // what the dense segments contribute to the product, per row of this side (null: no segments)
    enum Layout { kStream = 0, kPanel = 1, kJag = 3, kPb = 4 };  // (the numbers pdlpdev_layout_info reports)
    Layout layout() const { return pb.on ? kPb : jag.on ? kJag : pan.on ? kPanel : kStream; }
    // partial sums the side's epilogue leaves / the most any layout the side may still run leaves (the buffer's size)
    int partials() const
    {
      switch (layout()) {
        case kPb: return pb.v.B;
        case kJag: return jag.v.nblk + jag.v.nlong;
        case kPanel: return pan.v.W;
        default: return nb;
      }
    }
    int max_partials() const { return std::max({nb, pb.on ? pb.v.B : 0, pan.on ? pan.v.W : 0, jag.on ? jag.v.nblk + jag.v.nlong : 0, 1}); }
    // pdlpdev_layout_info's triple: the layout, its workgroups (bins / row blocks / panels), and a figure of merit of its own
    void info(int32_t out[3]) const
    {
      out[0] = layout();
      switch (layout()) {
        case kPb: out[1] = pb.v.B, out[2] = (int)(100.0 * (pb.pad - 1.0) + 0.5); break;
        case kJag: out[1] = jag.v.nblk, out[2] = (int)(100.0 * jag.saving + 0.5); break;
        case kPanel: out[1] = pan.v.W, out[2] = pan.v.S; break;
        default: out[1] = nb, out[2] = 1;
      }
    }
    // the panel kernels add the dense segments themselves (own-row workgroups of A, the column epilogue of A^T): no launches in front
    bool fuses_dense() const { return pan.on && (pan.v.dn_own_seg != nullptr || pan.v.dn_pan_ptr != nullptr); }
  };
  MatrixSide A, At;
  // Dense row segments (runs of >= kDenseMin consecutive columns inside a row: budget / convexity / linking constraints that
  // run through a block of variables) are stored INDEX-FREE, 8 bytes per entry instead of 12, and multiplied by two streaming
  // kernels of their own (k_dense_rows: lane <-> entry, the vector read coalesced; k_dense_cols: lane <-> column, the rows that
  // cover it in ascending order); the four layouts then work on the sparse remainder (each side's "hot" CSR, the matrices
  // without the segments' entries) and add what the segments contribute ahead of their fused epilogues (dense_plus).  The
  // set-up kernels (norms, scaling) keep running on the full CSR.  Rows / columns a segment touches are compared with the
  // oracle at the long-row tolerance (their sums are split in two).
  struct Dense {
    bool on = false;
    int nrows = 0, nseg = 0, ntiles = 0;
    int64_t nent = 0;
    int32_t *row = nullptr, *row_seg = nullptr;  // rows that own segments, their segment ranges
    int32_t *seg_row = nullptr, *seg_c0 = nullptr, *seg_len = nullptr, *seg_ptr = nullptr;  // nseg (+1)
    int32_t *ch_seg = nullptr, *ch_k0 = nullptr, *row_ch = nullptr;  // chunks of the segments (k_dense_rows), per owning row
    double* ch_part = nullptr;
    int nchunks = 0;
    int32_t *tile_ptr = nullptr, *tile_seg = nullptr, *tile_id = nullptr;  // per 256-column tile some segment overlaps: those segments, ascending rows
    int32_t *perm = nullptr, *s_perm_a = nullptr, *s_perm_at = nullptr;  // positions in the FULL CSR of A / A / A^T
    double* val = nullptr;                   // nent: the segments' values, row after row
    int32_t* tile_slot = nullptr;               // per 256-column tile: its index in tile_ptr, -1 where no segment overlaps it
  } dense;
  double *c = nullptr, *c_u = nullptr;  // the objective: scaled working copy and the unscaled original
  double *dr = nullptr, *dc = nullptr;
  bool scaled = false;
  int eval_reuse_aty = 1;   // CUOPT_AMD_TUNE=eval_reuse_aty
  // CUOPT_AMD_TUNE=primal_decides=0|1 (default: by n, below): on one GPU in the averaging modes a chunk of N attempts -- one graph, or the plain
  // launches of a round -- decides the step of attempts 1 .. N - 1 at the head of the NEXT attempt's primal kernel, under its operand
  // loads, and launches the decision kernel once, behind the last attempt (enqueue_single_chunk, pdlp_device.hip: 3 N + 1 launches).
  // 0: the decision kernel behind every attempt, 4 N launches (A/B runs, tests).  The same bits either way.
  // Without the key: on from kPrimalDecidesMinCols columns.  Measured against the parent's sequence (three alternating runs each,
  // profiles/primal_decides_other_workloads.jsonl): n = 1e5 (C2, stream layout: 25 workgroups of the fused kernel, nothing to hide the
  // chain under) 32.5 k against 33.5 k it/s, 2.9 % SLOWER at a spread of 0.7 %; n = 1e6: C3 + 1.7 %, banded + 3.1 %.  The break-even lies
  // between the two and was not located: the constant stays near the measured gain -- 192 workgroups of 4096 columns, three quarters of
  // the 256 CUs.
  static constexpr int kPrimalDecidesMinCols = 786432;
  int primal_decides = 1;
  int primal_decide_grid_cap = 512;  // most workgroups of k_primal_decide (kPrimalDecideMaxGrid; CUOPT_AMD_TUNE=primal_decide_grid=1 .. 512: tests)
  int batch_lanes = 0;  // jagged layouts built for lockstep batches of up to this many LPs (cuoptamd_settings::batch_lanes)
  bool small_resident = false;  // whole attempt batches inside one workgroup (k_pdhg_small)
  // multi-GPU (a sharded context is never cloned: the dataflow's own buffers stay with what describes it)
  rccl::comm_t comm = nullptr;  // non-null also marks "sharded mode" when the soft communicator is used
  softcomm::Comm* soft = nullptr;
  std::string comm_key;  // RCCL: this solver's entry of the communicator cache
  int rank = 0, world = 1;
  // "sliced primal" dataflow of a sharded solve (CUOPT_AMD_SHARD_DATAFLOW=rsag): inside the attempt loop a rank updates only
  // its slice [rank * slice, rank * slice + slice) of the primal-side vectors; reduce-scatter(A^T y' partials) -> slice of
  // A^T y', all-gather(xbar slices) -> the gathered vector of the next A xbar.  Outside the loop everything is replicated.
  bool rsag = false;
  int slice = 0;               // entries per rank, a multiple of 16; slice * world >= n
  double* rs_buf = nullptr;    // slice + 8: this rank's part of the reduced A^T y'
  double* rs_scal = nullptr;   // ||dy||^2, interaction, ||dx||^2 partial sums of this rank -> all-reduced
  // "owner computes" dataflow (CUOPT_AMD_SHARD_DATAFLOW=owner): on top of the sliced primal update a rank also holds ITS
  // COLUMNS of A (rows [rank * slice, ...) of A^T over ALL rows of A), so that A^T y' of its slice is complete on the rank:
  // all-gather(xbar slices) -> local rows of A -> y' -> all-gather(y' row blocks) -> local columns of A -> slice of A^T y'
  // and of the step-size sums.  No partial products travel, nothing is reduced but three scalars, and every column is summed
  // over all rows in row order exactly as on one GPU.
  bool owner = false;
  int ypad = 0;               // entries per rank in the gathered dual vector: the largest row block, a multiple of 16
  double* ygather = nullptr;  // world * ypad: rank q's y' at [q * ypad, ...); also the gather vector of the column block
  MatrixSide Oc;              // the column block: rows = the columns of A this rank owns, cols = the gathered dual's length
  // HALO exchange of the owner-computes dataflow (round 5).  A rank's rows touch only the columns of its own slice plus, on a
  // structured LP (a band, a staircase -- as given or as the set-up's reordering found it), a few thousand columns at the edges of
  // its neighbours' slices; its columns likewise touch its own rows plus the edges of the neighbours' row blocks.  Then the two
  // all-gathers of an attempt (7/8 of n + m doubles received per rank at 8 ranks) shrink to neighbour messages of the ranges
  // actually referenced: per peer ONE contiguous range of xbar (global column numbers) and one of the gathered y' -- kilobytes.
  // Decided at pdlpdev_owner_setup from the matrices themselves (every rank learns every rank's needs through one all-gather of
  // the range table); used when the ranges sum to at most a quarter of the all-gathers' volume (CUOPT_AMD_TUNE=shard_halo=0|1
  // forces it off / on).  Values are the same doubles either way: iterates are bit-identical to the all-gather's.
  struct Halo {
    bool on = false;
    std::vector<int32_t> recv_off[2], recv_cnt[2], send_off[2], send_cnt[2];  // [kind 0 xbar | kind 1 y'][peer]: offsets into the buffer
    int64_t bytes = 0, bytes_allgather = 0;  // received per attempt by this rank: the halo's ranges / the two all-gathers
  } halo;
  // direct peer transport of the owner-computes dataflow (CUOPT_AMD_SHARD_TRANSPORT=p2p): every rank owns one fine-grained
  // LANDING block [xbar of all ranks | y' of all ranks | 4 step-size scalars per rank | 3 * world epoch flags]; a producer
  // stores its slice into every rank's block (peer-mapped: same process -> the pointer itself after
  // hipDeviceEnablePeerAccess, other process -> hipIpcOpenMemHandle) and then raises its flag there; a consumer waits for the
  // world flags of the exchange, then copies the landed data into its ordinary vectors.  No collective call, no host between
  // the kernels of an attempt -> the attempt graph replays as on one GPU.
  struct P2P {
    bool on = false;
    char* base = nullptr;            // this rank's landing block
    size_t bytes = 0;
    size_t off_x = 0, off_y = 0, off_s = 0, off_f = 0;  // byte offsets inside every rank's block
    p2pdev::Peers peers{};           // base of every rank's block as THIS process addresses it
    std::vector<void*> opened;       // hipIpcOpenMemHandle mappings to close
    unsigned long long* epoch = nullptr;  // device: epochs of the three exchanges (xbar, y', scalars) as this rank counts them
    int* fault = nullptr;            // device: set when a wait ran out of patience (peer died)
    p2pdev::Push* push_dev = nullptr;  // device: the three exchanges' descriptors (xbar, y', scalars) for the producing kernels
    p2pdev::Push push_host[p2pdev::kKinds];  // their host copies (the halo set-up narrows the ranges afterwards)
  } p2p;
};

// bursts of device-decided major iterations, the periods they enqueued, the records written, the periods behind a stop (halpern_major.hpp)
struct HalpernBurstStats { int64_t bursts = 0, periods = 0, records = 0, empty = 0; };

// CtxLp: ONE LP over that problem -- its bounds, iterate, sums, averages, anchor, control block with the pinned mirror, partial buffers,
// zero-skip bitmap and best-point snapshot on the device, and what the host knows about them without asking (validity flags, counters,
// profiling events).  Written by everything that moves the LP (pdlpdev_reset, the loop, the evaluations).  A clone starts from the
// member initialisers below; pdlpdev_clone_shared carries over, by name, the few values it takes from its parent, and
// lp_alloc_iterate / lp_alloc_partials give it its buffers.
struct CtxLp {
  // bounds: scaled working copies and the unscaled originals
  double *lb = nullptr, *ub = nullptr, *lo = nullptr, *hi = nullptr;  // (what is known about lb / ub: pdlpdev_ctx::ubd)
  double *lb_u = nullptr, *ub_u = nullptr, *lo_u = nullptr, *hi_u = nullptr;
  // iterate state
  double *x[2] = {nullptr, nullptr}, *y[2] = {nullptr, nullptr}, *aty[2] = {nullptr, nullptr};
  double *xbar = nullptr, *sumx = nullptr, *sumy = nullptr, *avgx = nullptr, *avgy = nullptr;
  // Zero skip: one bit per column, set where xbar is not 0.0 (k_primal's ballots; ceil(n / 128) 16-byte quads, the unit the panels of A
  // fetch).  CUOPT_AMD_TUNE=zero_skip=0, or an A that is not in the row-sum panels: not allocated, every entry of xbar is gathered as before; 1 (default), 2: in use wherever
  // attempt_xmask (pdlp_device.hip) says it applies.  A clone has none (like every CtxLp field it starts from the initialiser: the parent's bitmap is of ITS xbar), and gathers every entry.  One more
  // word behind the quads counts the launches of the A product that took the masked path (PDLPDEV_BUF_ZS_LAUNCHES: tests).
  unsigned long long* xmask = nullptr;
  int* zcount = nullptr;  // k_primal's per-workgroup counts of the set bits (grid_for(n) of them): the density guard's input
  int zs_mode = 0;        // 1: the product skips when the control block's flag is up (pdlpdev_ctl::zskip); 2: always
  // A chunk of attempts that decides in the primal kernel (CtxProblem::primal_decides): the two scratch control blocks its decided blocks
  // alternate between and the second buffer of counts (zcount is the first).  Allocated at the first such chunk (chunk_blocks_ready).
  pdlpdev_ctl* chunk_ctl[2] = {nullptr, nullptr};
  int* zcount_alt = nullptr;
  double *lrx = nullptr, *lry = nullptr, *rc[2] = {nullptr, nullptr};
  double *tmp_n = nullptr, *tmp_m = nullptr;
  double *ax_u[3] = {nullptr, nullptr, nullptr}, *aty_u[3] = {nullptr, nullptr, nullptr};  // unscaled A x / A^T y of pdlpdev_eval(which)
  double* rc_scratch = nullptr;  // reduced costs of eval(LAST_RESTART): never returned
  double *bestx = nullptr, *besty = nullptr, *bestrc = nullptr;  // save_best_primal_so_far snapshot (scaled x, y)
  // reductions (each side's own partials: MatrixSide::part)
  double *part_g = nullptr;                      // generic grid-stride partials
  double *scal = nullptr;                        // device scalars (outputs of finalize kernels)
  double *scal_h = nullptr;                      // pinned mirror
  pdlpdev_ctl *ctl = nullptr, *ctl_h = nullptr;  // device control block + pinned mirror
  pdlpdev_step_params sp = {0.3, 0.6, 0.5, 0.5};
  // restarted reflected-Halpern mode (pdlpdev_set_halpern): z^k lives in the iterate buffers, T(z^k) of a run's last step in avgx / avgy
  // (avgy is also the vector the A^T product gathers), the anchor in lrx / lry / lraty; the mode's scalars in a block of their own
  bool halpern = false;
  double* lraty = nullptr;                                  // A^T y of the anchor
  pdlpdev_halpern *hal = nullptr, *hal_h = nullptr;         // device block + pinned mirror (read back with the control block)
  bool halpern_rays = false;  // pdlpdev_set_halpern_rays: every evaluation of T(z^k) is followed by the ray pass on T(z^k) - z^k
  // pdlpdev_set_halpern_device_major (cuoptamd_settings::halpern_device_major): the burst's own device block (halpern_major.hpp) and its
  // ring of 16 records in pinned host memory -- allocated only when the option is set; a clone starts without them like every CtxLp field
  struct pdlpdev_halpern_major_state* hmaj = nullptr;
  pdlpdev_halpern_major_record* hmaj_ring = nullptr;
  HalpernBurstStats burst_stats;  // pdlpdev_halpern_burst_stats
  // n + pad doubles: A^T y partial + packed scalars between attempts (pdlpdev_compute_aty, the evaluation, pdlpdev_spectral_norm).  A
  // sharded context in Halpern mode (owner-computes dataflow) ALSO keeps x' of a run's last step there, on the rank's slice, from the
  // column block's product of that step until run_epilogue has all-gathered it and copied it into avgx (which has no spare entries for
  // equal slices): nothing else may write ar_buf between enqueue_attempts and run_epilogue of one pdlpdev_run.
  double* ar_buf = nullptr;
  // pdlpdev_time_kernel: the next launch through launch_k carries these events (kernel start / stop timestamps of the
  // dispatch itself, what rocprofv3 --kernel-trace reports)
  // (a call site may consist of several launches -- dense segments, phase P, phase R: each gets its own pair, the durations add up)
  bool prof_armed = false;
  static constexpr int kProfPairs = 8;
  hipEvent_t prof_ev[2 * kProfPairs] = {};
  int prof_used = 0;
  int rejected_in_a_row = 0;  // attempts enqueued since the last accepted step (pdlpdev_run's guard against endless rejections)
  // What the host knows about the loop's state without asking the device (pdlpdev_run, pdlpdev_run_period, enqueue_eval):
  //   aty_valid      aty[cur] holds A^T y[cur] as this side's product kernels form it: after an accepted attempt (k_*_at_step stored
  //                  A^T y' and the decision flipped to it), until anything else writes y[cur] or flips cur (loop_state_touched
  //                  below) or the step error comes up.  pdlpdev_compute_aty restores the buffer too, but attempts always follow it
  //                  before the next evaluation, so it is not counted.  The evaluation of the CURRENT iterate then reads its dual
  //                  side from there instead of running the product again (CUOPT_AMD_TUNE=eval_reuse_aty=0: never).
  //   ctl_h_current  the pinned copy of the control block is what the device holds: the read-back behind k_set_target is skipped.
  bool aty_valid = false, ctl_h_current = false;
  // A member of a lockstep batch (kernels_batch.hip); loop_state_touched drops both:
  //   batch_ctl_fresh   pdlpdev_batch_run's last read-back of the control block is what the device holds
  //   batch_ray_steps   >= 0: the K-wide ray pass (pdlpdev_batch_halpern_rays) served this context at that accepted-step count, with the
  //                     reduced-cost rule batch_ray_rule: the evaluation of T(z^k) at that count leaves the single pass out
  bool batch_ctl_fresh = false;
  int batch_ray_steps = -1, batch_ray_rule = -1;
  int64_t stat_single_rays = 0;  // single ray passes enqueued (enqueue_halpern_ray)
  int spare_attempts = 0;   // pdlpdev_run_period: empty-unless-needed attempts behind a period's, from the rejections the period before saw
  // pdlpdev_loop_stats: evaluations of the current iterate that reused A^T y / ran the product, synchronisations inside
  // pdlpdev_run and pdlpdev_run_period (pdlpdev_major_eval's own included), attempts enqueued that found the target reached
  int64_t stat_eval_reused = 0, stat_eval_product = 0, stat_loop_syncs = 0, stat_empty_attempts = 0;
  // pdlpdev_scaling_stats: launches per site of the scaling, [side][norms of a max pass x 3 shapes, of a sum pass x 3, value scaling x 3]
  int64_t stat_scaling[2][9] = {};
  int use_graph = 1;  // attempts are replayed from captured graphs (CtxOwned::graphs)
  bool comm_warm = false;          // one attempt went out eagerly over this communicator (before the first capture)
  bool graph_comm_failed = false;  // capturing the RCCL collectives into an attempt graph failed once: plain launches from then on
};

// CtxOwned: what this context has to give back -- allocations, slab, arena, graphs, the set-up's scratch -- and its links to the
// contexts that alias its arrays (parent, clones, batches).  Written by dev_alloc, the graph cache, clone / batch creation and
// pdlpdev_destroy; never copied from one context to another.
struct CtxOwned {
  // one allocation for the ~40 problem / iterate vectors of a large LP (each hipMalloc + memset pair costs ~0.1 ms: 3 ms of a 25 ms
  // set-up at 1e6 x 1e6); dev_alloc draws from it while it lasts
  char* slab = nullptr;
  size_t slab_cap = 0, slab_used = 0;
  char* arena = nullptr;  // current small-buffer chunk (dev_alloc)
  char* first_chunk = nullptr;  // recycled with the stream, not in `allocs`
  bool stream_borrowed = false; // pdlpdev_create_share_stream: the stream is another context's
  size_t arena_used = 0;
  bool shared_with_parent = false;  // pdlpdev_clone_shared: matrices, layouts, scaling vectors, c and the stream are another context's
  pdlpdev_ctx* parent = nullptr;    // ... that one
  bool rows_aliased = false;        // ... and so are the row bounds (lo, hi and their unscaled twins) until a reset brings other ones:
                                    // K clones that differ in their VARIABLE bounds read one copy (the batched dual step then fetches
                                    // lo / hi once for all LPs -- the caches see the same addresses)
  int clones_alive = 0;             // contexts that alias this one's arrays
  bool rows_private = false;        // a parent whose lo / hi were re-allocated by a reset AFTER its last clone was made: no clone aliases them
  int batches_alive = 0;            // pdlpdev_batch / pdlpdev_small_batch objects that hold this context's pointer
  int lockstep_batches_alive = 0;   // ... the pdlpdev_batch objects among them: their kb_* kernels read ONE objective for all members
  std::map<int, hipGraphExec_t> graphs;  // attempts-per-replay -> executable graph
  std::vector<void*> allocs;
  int64_t bytes = 0;
  // Scratch of the layouts' device constructions (kernels_layout_build.hip): the A side's temporaries serve the A^T side again -- a
  // hipMalloc of a few GB right after a hipFree of the same size took 1.9 s at 1e9 nonzeros (the first one of the process: 2 ms) --
  // and go back to the runtime when the context has been created (scratch_free, pdlp_create.hip).
  struct Scratch {
    void* p = nullptr;
    size_t bytes = 0;
    bool busy = false;
  };
  std::vector<Scratch> scratch;
};

struct pdlpdev_ctx : CtxProblem, CtxLp, CtxOwned {
  // all lower (upper) bounds are the same 0 or infinity: k_primal takes the constant instead of streaming the array.  Per LP like
  // CtxLp's fields (a clone carries its parent's over with the bounds); declared here because the type is a kernel argument: as a
  // member of this struct it keeps the name the kernels' symbols are mangled with.
  struct UniformBounds {
    int lb_same = 0, ub_same = 0;
    double lb = 0.0, ub = 0.0;
  } ubd;
  void note_uniform_bounds(const double* lb_host, const double* ub_host)  // (null: that side is unchanged)
  {
    auto same = [&](const double* v, int* flag, double* value) {
      if (!v) return;
      *flag = 0;
      if (n <= 0) return;
      const double v0 = v[0];
      if (!(v0 == 0.0 || std::isinf(v0))) return;
      // (16 MB of bounds at n = 1e6: the scan runs on the host pool's threads)
      constexpr int kParts = 16;
      bool differs[kParts] = {false};
      cuopt_amd::parallel_tasks(kParts, [&](int t) {
        const int32_t a = (int32_t)((int64_t)n * t / kParts), b = (int32_t)((int64_t)n * (t + 1) / kParts);
        for (int32_t j = a; j < b; ++j)
          if (v[j] != v0) {
            differs[t] = true;
            return;
          }
      }, (int64_t)n * 4);
      for (bool d : differs)
        if (d) return;
      *flag = 1, *value = v0;
    };
    same(lb_host, &ubd.lb_same, &ubd.lb);
    same(ub_host, &ubd.ub_same, &ubd.ub);
  }
};
inline int scratch_take(pdlpdev_ctx* c, void** p, size_t bytes)
{
  bytes = std::max<size_t>(bytes, 256);
  for (auto& b : c->scratch)
    if (!b.busy && b.bytes >= bytes && b.bytes <= 2 * bytes + 4096) {
      b.busy = true;
      *p     = b.p;
      return 0;
    }
  HIP_TRY(hipMalloc(p, bytes));
  c->scratch.push_back(pdlpdev_ctx::Scratch{*p, bytes, true});
  return 0;
}
inline void scratch_release(pdlpdev_ctx* c, void* p)
{
  for (auto& b : c->scratch)
    if (b.p == p) b.busy = false;
}
inline void scratch_free(pdlpdev_ctx* c)
{
  for (auto& b : c->scratch) (void)hipFree(b.p);
  c->scratch.clear();
}

// one LP's arguments of k_step_decision_batch (pdlp_device.hip; launched by kernels_batch.hip)
struct pdlpdev_decision_args {
  pdlpdev_ctl* ctl;
  const double* part_dy;
  int nb_dy;
  const double* part_t;
  int nb_t;
  pdlpdev_step_params sp;
};

constexpr int kGenericBlocks = 1024;
constexpr int kScalars       = 64;
constexpr int kCtlSlot       = 48;  // scal[kCtlSlot ..): the control block as pdlpdev_run_period's last kernel copied it (one read-back for both)
static_assert(kCtlSlot * sizeof(double) + sizeof(pdlpdev_ctl) <= kScalars * sizeof(double), "the control block fits behind the scalars");
// Halpern mode, the ray pass on T(z^k) - z^k (pdlpdev_halpern_eval_infeasibility): the slots of pdlpdev_eval_infeasibility, which the mode
// leaves free, on the device (multi-launch path) and in the pinned block the one-workgroup evaluation writes (resident path) alike
constexpr int kRayRows = 16;  // max homogeneous primal residual, ||dy||_inf, sum B(dy, lo, hi)
constexpr int kRayCols = 24;  // max homogeneous dual residual, ||rc||_inf, ||dx||_inf, max bound violation, sum B(rc, lb, ub), c . dx
constexpr int kRayMark = 30;  // the accepted-step count the pass ran at, and its reduced-cost rule (0 / 1)
// the iterate or the control block changed behind the loop's back
inline void loop_state_touched(pdlpdev_ctx* c) { c->aty_valid = false, c->ctl_h_current = false, c->batch_ctl_fresh = false, c->batch_ray_steps = -1; }
// Shared by the single loop (pdlp_device.hip) and the lockstep batch (kernels_batch.hip).  The attempts of a round go out in chunks, one
// graph per chunk size: the largest power of two <= min(remaining, 64)
inline int attempt_chunk(int remaining)
{
  int chunk = 1;
  while (chunk * 2 <= remaining && chunk < 64) chunk *= 2;
  return chunk;
}
// The rejection rule, on the fresh ctl_h behind a round that started at `before` accepted steps and made `counted` attempts that count.
// Every rejection shrinks the step size; 64 in a row leave nothing of it: the caller raises the step error (true: k_set_error on its own
// stream), like the reference's invalid step size, instead of re-enqueueing forever.  Counted across rounds AND calls.
inline bool too_many_rejections(pdlpdev_ctx* c, int before, int counted)
{
  c->rejected_in_a_row = c->ctl_h->steps_taken == before ? c->rejected_in_a_row + counted : 0;
  if (c->ctl_h->error != 0 || c->rejected_in_a_row < 64) return false;
  c->rejected_in_a_row = 0;
  return true;
}
// guarded evaluation kernels exist for this context: only the panel kernels know the guard flag, an unfused dense segment's do not
inline bool has_guarded_eval(const pdlpdev_ctx* c)
{
  const bool both_panels   = c->A.layout() == pdlpdev_ctx::MatrixSide::kPanel && c->At.layout() == pdlpdev_ctx::MatrixSide::kPanel;
  const bool dense_unfused = c->dense.on && !(c->At.fuses_dense() && c->A.fuses_dense());
  return !c->small_resident && both_panels && !dense_unfused;
}
// the l-infinity residuals are wanted: the host driver passes negative relative tolerances otherwise
inline bool wants_linf(double eps_rel_primal, double eps_rel_dual) { return eps_rel_primal >= 0.0 && eps_rel_dual >= 0.0; }

// A kernel that takes more dynamic LDS than the default limit allows: the attribute is per kernel and device, and set ONCE, under the
// lock (batch solves create contexts from many threads), the first time the triple (kernel, device, size) comes by.  A kernel's
// launches all ask for the same size today (jag by WAVES, pb by WIDE, phase P always 160 KiB, the resident loops by tier); the size is
// part of the key so that one which ever asks for a second size gets it set.  The list is per translation unit: setting a kernel's
// attribute twice is harmless.
static int allow_dynamic_lds(const void* kernel, int device, size_t bytes)
{
  static std::mutex mu;
  static std::vector<std::tuple<const void*, int, size_t>> done;
  std::lock_guard<std::mutex> lock(mu);
  const std::tuple<const void*, int, size_t> key(kernel, device, bytes);
  if (std::find(done.begin(), done.end(), key) == done.end()) {
    HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done.push_back(key);
  }
  return 0;
}

// Streams (an HSA queue each: ~2 ms to create), the pinned read-back block and the first arena chunk are handed from
// a destroyed context to the next one created on the same device: back-to-back small solves (cuOptSolve in a loop,
// MIP-style re-solves) otherwise spend more time in these three calls than in PDHG.  Never freed (a few per device).
struct Recycled {
  int device;
  hipStream_t stream;
  double* pinned;
  char* chunk;
};
inline std::mutex g_recycle_mutex;
inline std::vector<Recycled> g_recycled;
inline bool take_recycled(int device, Recycled* out)
{
  std::lock_guard<std::mutex> lock(g_recycle_mutex);
  for (size_t i = 0; i < g_recycled.size(); ++i)
    if (g_recycled[i].device == device) {
      *out = g_recycled[i];
      g_recycled.erase(g_recycled.begin() + i);
      return true;
    }
  return false;
}
inline bool give_recycled(const Recycled& r)
{
  std::lock_guard<std::mutex> lock(g_recycle_mutex);
  if (g_recycled.size() >= 16) return false;
  g_recycled.push_back(r);
  return true;
}

// Zero-filled device memory.  Buffers under 256 KiB are carved out of 1 MiB chunks: a small LP (the MIP-style
// re-solve case) needs ~60 buffers, and 60 hipMalloc + hipFree calls cost more than its whole solve.
constexpr size_t kArenaChunk = (size_t)1 << 20, kArenaMaxItem = (size_t)256 << 10;
template <class T>
inline int dev_alloc(pdlpdev_ctx* c, T** p, size_t count)
{
  size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  c->bytes += (int64_t)bytes;
  if (bytes <= kArenaMaxItem) {
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (c->arena == nullptr || c->arena_used + need > kArenaChunk) {
      HIP_TRY(hipMalloc((void**)&c->arena, kArenaChunk));
      HIP_TRY(hipMemsetAsync(c->arena, 0, kArenaChunk, c->stream));
      c->allocs.push_back(c->arena);
      c->arena_used = 0;
    }
    *p = (T*)(c->arena + c->arena_used);
    c->arena_used += need;
    return 0;
  }
  {
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (c->slab && c->slab_used + need <= c->slab_cap) {
      *p = (T*)(c->slab + c->slab_used);
      c->slab_used += need;
      return 0;
    }
  }
  static const bool timing = getenv("CUOPT_AMD_TIMING") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  HIP_TRY(hipMalloc((void**)p, bytes));
  const auto t1 = std::chrono::steady_clock::now();
  HIP_TRY(hipMemsetAsync(*p, 0, bytes, c->stream));
  if (timing && std::chrono::duration<double>(t1 - t0).count() > 1e-3)  // only the surprising ones
    fprintf(stderr, "[cuopt_amd setup]     hipMalloc %10zu B: %.2f ms\n", bytes, 1e3 * std::chrono::duration<double>(t1 - t0).count());
  c->allocs.push_back(*p);
  return 0;
}
#define TRY(expr)          \
  do {                     \
    int rc_ = (expr);      \
    if (rc_ != 0) return rc_; \
  } while (0)

// ---- the device vectors of ONE LP (CtxLp), for pdlpdev_create and pdlpdev_clone_shared alike.  The order of the dev_alloc calls is part of
// the contract: buffer addresses are what the attempt kernels' speed depends on, and the zero-skip buffers come last of all (pdlp_create.hip).
// the slab that the problem / iterate vectors of a large LP are carved from (24 of n (+ pad), 15 of m entries), zero-filled
inline int lp_alloc_slab(pdlpdev_ctx* c)
{
  if ((int64_t)c->m + c->n < 262144) return 0;
  const size_t bytes = (24 * ((size_t)c->n + kSlicePad + 32) + 15 * ((size_t)c->m + 32)) * sizeof(double);
  if (hipMalloc((void**)&c->slab, bytes) == hipSuccess) {
    c->allocs.push_back(c->slab);
    c->slab_cap = bytes, c->slab_used = 0;
    HIP_TRY(hipMemsetAsync(c->slab, 0, bytes, c->stream));
  } else {
    c->slab = nullptr;
    (void)hipGetLastError();
  }
  return 0;
}
// the iterate and its companions.  x, A^T y, xbar, sum_x carry kSlicePad spare entries: the sliced-primal dataflow of a sharded solve
// all-gathers them in equal slices of a multiple of 16 entries per rank (slice * world may exceed n by up to 16 * 16 - 1)
inline int lp_alloc_iterate(pdlpdev_ctx* c)
{
  const size_t m = (size_t)c->m, n = (size_t)c->n;
  for (int i = 0; i < 2; ++i) {
    TRY(dev_alloc(c, &c->x[i], n + kSlicePad)); TRY(dev_alloc(c, &c->y[i], m));
    TRY(dev_alloc(c, &c->aty[i], n + kSlicePad)); TRY(dev_alloc(c, &c->rc[i], n));
  }
  TRY(dev_alloc(c, &c->xbar, n + kSlicePad)); TRY(dev_alloc(c, &c->sumx, n + kSlicePad)); TRY(dev_alloc(c, &c->sumy, m));
  TRY(dev_alloc(c, &c->avgx, n)); TRY(dev_alloc(c, &c->avgy, m));
  TRY(dev_alloc(c, &c->lrx, n)); TRY(dev_alloc(c, &c->lry, m));
  TRY(dev_alloc(c, &c->tmp_n, n)); TRY(dev_alloc(c, &c->tmp_m, m));
  for (int i = 0; i < 3; ++i) {
    TRY(dev_alloc(c, &c->ax_u[i], m));
    TRY(dev_alloc(c, &c->aty_u[i], n));
  }
  TRY(dev_alloc(c, &c->rc_scratch, n));
  return 0;
}
// what needs the layouts in place: each side's epilogue partials (MatrixSide::part, the one per-LP field of CtxProblem: pointed at
// this LP's own buffer here), the generic partials, the scalars and the control block
inline int lp_alloc_partials(pdlpdev_ctx* c)
{
  TRY(dev_alloc(c, &c->A.part, (size_t)8 * c->A.max_partials()));
  TRY(dev_alloc(c, &c->At.part, (size_t)8 * c->At.max_partials()));
  TRY(dev_alloc(c, &c->part_g, (size_t)8 * 2048));
  TRY(dev_alloc(c, &c->scal, kScalars));
  TRY(dev_alloc(c, &c->ctl, 1));
  TRY(dev_alloc(c, &c->ar_buf, (size_t)c->n + kSlicePad));
  return 0;
}

// the stream kernels remap blockIdx so that each XCD owns a contiguous range of row blocks
// (xcd_remap); the grid is padded to a multiple of 8 so the remap is a bijection.
static inline int stream_grid(int nb) { return std::max(8, ((nb + 7) / 8) * 8); }
static inline int grid_for(int64_t n, int per_thread = 1)
{
  int64_t g = (n + (int64_t)kBlock * per_thread - 1) / ((int64_t)kBlock * per_thread);
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, 2048));
}

// ---- defined in pdlp_comm.hip (communicators, collectives, the peer transport's set-up) ------------------------------------------
int setup_dataflow(pdlpdev_ctx* ctx);
int reduce_scatter(pdlpdev_ctx* ctx, const double* send, double* recv, size_t count);
int all_gather(pdlpdev_ctx* ctx, double* buf, size_t count);
int allreduce(pdlpdev_ctx* ctx, double* buf, size_t count, int op);
int p2p_setup(pdlpdev_ctx* ctx);
int p2p_push_ranges(pdlpdev_ctx* ctx);
int halo_setup(pdlpdev_ctx* ctx, const int32_t* need /* [world][4]: xbar lo, hi (columns), y' lo, hi (positions in ygather) */);
int halo_exchange(pdlpdev_ctx* ctx, int kind, double* buf);
