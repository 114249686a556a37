// What the lockstep batch kernels of kernels_batch.hip (the averaging iteration) and kernels_batch_halpern.hip (the restarted
// reflected-Halpern iteration) share: the per-LP table, the wave <-> LP assignment, the K-wide product geometry and its LDS, the row
// sums of a block, their cross-over and the per-LP partial sums.  The products are described in kernels_batch.hip ("(2), (3) the two
// products for K LPs").  Everything is internal to the unit that includes it.
#pragma once
#include <hip/hip_runtime.h>

#include "pdlp_ctx.hpp"

namespace {

constexpr int kBT = kPanelThreads;  // threads per workgroup = the panel kernels' (the partial sums reproduce their tree)
static_assert(kBT == 512, "8 waves of 64 lanes: the reduction below mirrors block_reduce<.., kPanelWaves>");
constexpr int kBatchMax = 16;       // LPs per batch

struct BatchLp {  // what the batched kernels need of one LP, in device memory
  pdlpdev_ctl* ctl;
  double *y0, *y1, *sumy;
  const double *lo, *hi;
  double *x0, *x1, *aty0, *aty1, *sumx;
  const double *c, *lb, *ub;
  pdlpdev_ctx::UniformBounds ubd;
  double *part_a, *part_at;
};
static_assert(sizeof(BatchLp) == 16 * sizeof(void*) + 2 * sizeof(int) + 2 * sizeof(double), "no padding: batch_refresh_table compares entries with memcmp");

// wave <-> LP in the element-wise phases: K <= 8: 8 / K waves share an LP (wave w: LP w % K, every (8 / K)-th piece of 64 rows from
// piece w / K on); K = 16: a wave serves two LPs one after the other (w and w + 8)
template <int K>
struct WaveLps {
  static constexpr int PASSES = K > 8 ? K / 8 : 1;  // LPs per wave
  static constexpr int NSUB   = K > 8 ? 1 : 8 / K;  // waves per LP
  static __device__ __forceinline__ int lp(int wave, int pass) { return K > 8 ? wave + 8 * pass : wave % K; }
  static __device__ __forceinline__ int sub(int wave) { return K > 8 ? 0 : wave / K; }
};

template <int K>
struct BatchGeometry {
  static constexpr int KL    = K / 2;              // lanes per entry
  static constexpr int G     = kBT / KL;           // groups per workgroup
  static constexpr int CHUNK = K > 8 ? 256 : 512;  // matrix entries staged per pass (64 KB of products in two buffers)
  static constexpr int PER   = CHUNK / G;          // entries per lane and chunk
  static constexpr int RU    = kBT / G;            // rows per lane and block of 512 rows
};
template <int K>
struct alignas(16) BatchShared {
  using Geo = BatchGeometry<K>;
  union {
    struct {
      double prod[2][Geo::CHUNK][K];
      int scol[2][Geo::CHUNK];
      double sval[2][Geo::CHUNK];
    } p;
    double sums[kBT][K + 1];  // the epilogue's view of a block: row sums / new iterates, one padded row per matrix row
  } u;
  double red[2][K][8];
};
static_assert(sizeof(BatchShared<8>) <= 80 * 1024 && sizeof(BatchShared<16>) <= 80 * 1024, "two workgroups per CU");

// row sums of the block [b0, b0 + 512) of panel rows [r0, r0 + nr): lane (g, h) -- group g of K / 2 lanes, lane h of it = the LPs 2h and
// 2h + 1 -- ends with s[u][0..1] = the sums of row b0 + g + G * u for its two LPs
// LDS hazards of batch_block_sums (round-6 audit; the stage round 5's contention run had caught one barrier short):
//   prod[2][], scol[2][], sval[2][]  double-buffered by chunk parity.  Trip c (ends in barrier E(c)): reads scol / sval[(c + 1) & 1]
//   (chunk c + 1's entries, written in trip c - 1), reads prod[(c - 1) & 1] (chunk c - 1's products, written in trip c - 1), writes
//   prod[c & 1] (last read by the row sums of chunk c - 2 in trip c - 1, before E(c - 1)) and scol / sval[c & 1] with chunk c + 2's
//   entries (last read by trip c - 1's requests for chunk c, before E(c - 1)).  Every write is separated from the last read of its slot
//   by E(c - 1), every read from the write it depends on by E(c - 1) as well; the barrier in front of trip 0 covers the two staged chunks.
template <int K>
__device__ __forceinline__ void batch_block_sums(BatchShared<K>& S, int r0, int nr, int b0, const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                                 const double* __restrict__ val, const double* __restrict__ vK, double (&s)[BatchGeometry<K>::RU][2])
{
  using Geo = BatchGeometry<K>;
  constexpr int KL = Geo::KL, G = Geo::G, PER = Geo::PER, RU = Geo::RU, CH = Geo::CHUNK;
  const int tid = threadIdx.x, h = tid % KL, g = tid / KL;
  int k0[RU], k1[RU];
#pragma unroll
  for (int u = 0; u < RU; ++u) {
    const int r = b0 + g + G * u;
    const int i = r0 + (r < nr ? r : 0);
    k0[u] = off[i];
    k1[u] = r < nr ? off[i + 1] : k0[u];
    s[u][0] = 0.0, s[u][1] = 0.0;
  }
  const int eb0 = off[r0 + b0], eb1 = off[r0 + (b0 + kBT < nr ? b0 + kBT : nr)];
  const int nch = (eb1 - eb0 + CH - 1) / CH;
  const bool stager = CH == kBT || tid < CH;  // (chunks of 256: the first four waves fetch and stage)
  // chunks 0 and 1 staged (past the block's last entry: column 0 with value 0 -- gathered, multiplied, never added);
  // chunk 0's gathers on their way
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int e   = eb0 + c * CH + tid;
    const bool in = stager && e < eb1;
    const int cl  = idx[in ? e : eb0];
    const double vl = val[in ? e : eb0];
    if (stager) S.u.p.scol[c][tid] = in ? cl : 0, S.u.p.sval[c][tid] = in ? vl : 0.0;
  }
  __syncthreads();
  auto rowsum = [&](int cc) {
    const int c0 = eb0 + cc * CH, c1 = c0 + CH < eb1 ? c0 + CH : eb1, pb = cc & 1;
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int a = k0[u] > c0 ? k0[u] : c0, e = k1[u] < c1 ? k1[u] : c1;
      for (int k = a; k < e; ++k) {
        const double2 p = *(const double2*)&S.u.p.prod[pb][k - c0][2 * h];
        s[u][0] = s[u][0] + p.x, s[u][1] = s[u][1] + p.y;
      }
    }
  };
  double2 pv[PER], pvn[PER];
  double sv[PER], svn[PER];
  auto request = [&](int cc, double2 (&p)[PER], double (&v)[PER]) {  // chunk cc: its entries' values, its gathers
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      v[i] = S.u.p.sval[cc & 1][g + G * i];
      p[i] = *(const double2*)(vK + ((unsigned)S.u.p.scol[cc & 1][g + G * i] * (unsigned)K + 2u * h));
    }
  };
  // the entries of chunk c + 2 wait in registers for one trip before they go to LDS: every wait below is for loads issued a whole
  // trip earlier (the vector memory counter completes in order: a load consumed in the trip that issued it would drag the trip's
  // gathers along)
  auto fetch = [&](int cc, int& col, double& v) {
    const int e   = eb0 + cc * CH + tid;
    const bool in = stager && e < eb1;
    const int cl  = idx[in ? e : eb0];
    const double vl = val[in ? e : eb0];
    col = in ? cl : 0, v = in ? vl : 0.0;
  };
  int colA = 0, colB = 0;
  double valA = 0.0, valB = 0.0;
  // one trip: chunk c's products (its gathers were issued a trip ago into `cur`), chunk c + 1's gathers into `nxt`, chunk c + 2's
  // entries from their registers to LDS, chunk c + 3's entries requested.  (Two register sets that swap roles, the loop unrolled by
  // two: a copy "cur = nxt" at the end of a trip would wait for the gathers it has just issued.)
  auto trip = [&](int c, double2 (&cur)[PER], double (&curv)[PER], double2 (&nxt)[PER], double (&nxtv)[PER], int& col_st, double& val_st, int& col_ld,
                  double& val_ld) {
    request(c + 1, nxt, nxtv);  // (past the last chunk: staged zeros -- column 0, value 0; no branch around the loads: the counter
    fetch(c + 3, col_ld, val_ld);  //  bookkeeping of the compiler stays exact only in straight-line code)
    rowsum(c - 1);                // (c = 0: an empty range)
#pragma unroll
    for (int i = 0; i < PER; ++i) *(double2*)&S.u.p.prod[c & 1][g + G * i][2 * h] = double2{curv[i] * cur[i].x, curv[i] * cur[i].y};
    if (stager) S.u.p.scol[c & 1][tid] = col_st, S.u.p.sval[c & 1][tid] = val_st;  // (chunk c + 2 takes chunk c's place: read one barrier ago)
    __syncthreads();
  };
  request(0, pv, sv);
  fetch(2, colA, valA);
  __syncthreads();  // (trip 0 puts chunk 2 where chunk 0's entries are: every lane has read them first)
  for (int c = 0; c < nch; c += 2) {
    trip(c, pv, sv, pvn, svn, colA, valA, colB, valB);
    if (c + 1 < nch) trip(c + 1, pvn, svn, pv, sv, colB, valB, colA, valA);
  }
  if (nch > 0) rowsum(nch - 1);
}

// the row sums of a block cross over: lane (g, h) -> sums[row][LP] (padded rows), for the epilogue's wave <-> LP, lane <-> row
template <int K>
__device__ __forceinline__ void batch_cross_over(BatchShared<K>& S, const double (&s)[BatchGeometry<K>::RU][2])
{
  using Geo = BatchGeometry<K>;
  const int h = threadIdx.x % Geo::KL, g = threadIdx.x / Geo::KL;
  __syncthreads();  // (the last chunk's products are read)
#pragma unroll
  for (int u = 0; u < Geo::RU; ++u) S.u.sums[g + Geo::G * u][2 * h] = s[u][0], S.u.sums[g + Geo::G * u][2 * h + 1] = s[u][1];
  __syncthreads();
}

// block_reduce<SumOp, NQ, VW> of the single-LP kernels for every LP: acc[pass][q][v] = the sums of virtual threads lane + 64 v of LP
// (wave, pass).  VW = 8: the panel kernels' 512 threads; VW = 4: the CSR stream kernels' 256 (row t of a block belongs to thread t mod 256).
template <int K, int NQ, int VW>
__device__ __forceinline__ void batch_block_partials(BatchShared<K>& S, const double (&acc)[WaveLps<K>::PASSES][NQ][8], const BatchLp* __restrict__ lp, bool a_side,
                                                     int W, int w)
{
  using WL = WaveLps<K>;
  static_assert(WL::NSUB <= VW, "a wave owns whole virtual waves");
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, sub = WL::sub(wave);
#pragma unroll
  for (int pass = 0; pass < WL::PASSES; ++pass)
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int v = 0; v < VW; ++v)
        if (v % WL::NSUB == sub) {  // (rows lane + 64 j, j = sub mod NSUB, are this wave's: virtual waves j mod VW)
          const double r = wave_reduce<SumOp>(acc[pass][q][v]);
          if (lane == 0) S.red[q][WL::lp(wave, pass)][v] = r;
        }
  __syncthreads();
  if (threadIdx.x < K * NQ) {
    const int q = threadIdx.x / K, ll = threadIdx.x % K;
    if (loop_active(lp[ll].ctl)) {
      double total = S.red[q][ll][0];
      for (int vw = 1; vw < VW; ++vw) total = total + S.red[q][ll][vw];
      (a_side ? lp[ll].part_a : lp[ll].part_at)[(size_t)q * W + w] = total;
    }
  }
}

// A batch in reflected Halpern mode: the anchor and T(z^k) pointers of one LP, a second table next to BatchLp (which keeps its layout)
struct BatchHalpernLp {
  pdlpdev_halpern* hal;
  double *avgx, *avgy;              // T(z^k): x' (the last step of a run only) and y' (every step)
  const double *lrx, *lry, *lraty;  // the anchor z^0 and A^T y^0
};
static_assert(sizeof(BatchHalpernLp) == 6 * sizeof(void*), "no padding: batch_refresh_table compares entries with memcmp");

}  // namespace

// one matrix side as the CSR-walking batched products take it (the row blocks whose partial sums they reproduce, the hot CSR arrays)
struct BatchProductSide {
  int W;
  const int32_t* row0;
  bool panel;
  const int32_t *off, *idx;
  const double* val;
};
// kernels_batch_halpern.hip: the three launches of a Halpern attempt behind kb_primal -- kb_a_halpern, kb_at_halpern, the K decisions.
// lp_table / halpern_table: the device tables of K BatchLp / BatchHalpernLp (untyped here: the two structs are internal to each unit)
int batch_halpern_enqueue_tail(int K, hipStream_t s, const BatchProductSide& A, const BatchProductSide& T, const void* lp_table, const void* halpern_table,
                               double* xK, double* yK);

// kernels_batch_halpern_ray.hip: the K-wide ray pass of a batch in reflected Halpern mode and the K-wide plain product it is made of.
// What the pass needs of one LP, in device memory, kept current as the two tables above are (every vector is the member's own: a
// clone shares none of them with its parent).  Which LPs a pass serves and their reduced-cost rules travel by value in the launch
// arguments (bit l of on_mask / rule_mask): the table changes with a reset only, and a pass uploads nothing.
struct BatchRayLp {
  const pdlpdev_ctl* ctl;
  const double *avgx, *avgy;             // T(z^k)
  const double *x0, *x1, *y0, *y1;       // z^k: the side `cur` does NOT select
  double *tmp_n, *tmp_m;                 // the scaled displacement (k_halpern_ray_diff's slots)
  double *ax, *aty;                      // ax_u / aty_u[PDLPDEV_CURRENT]: the two products formed from it
  const double *lo_u, *hi_u, *lb_u, *ub_u;
  double *part_g, *scal;
};
static_assert(sizeof(BatchRayLp) == 17 * sizeof(void*), "no padding: batch_refresh_table compares entries with memcmp");
// what the K LPs share (the parent's): dimensions, the scaling vectors, the unscaled objective
struct BatchRayShared {
  int n, m;
  const double *dr, *dc, *c_u;
};
// the pass for the LPs of on_mask behind whatever runs on s: kb_ray_diff, kb_plain on either side, the two statistics kernels
// (grid y <-> LP), one finalize (workgroup <-> LP) -- six launches, two streams of the matrix
int batch_halpern_enqueue_rays(int K, hipStream_t s, const BatchProductSide& A, const BatchProductSide& T, const void* ray_table, const BatchRayShared& sh,
                               unsigned on_mask, unsigned rule_mask, double* xK, double* yK);
// vK[i * K + l] = (transpose ? tmp_m : tmp_n of LP l)[i] (0 for an LP outside on_mask), then ONE kb_plain<K> on that side: row sums to
// the LP's aty / ax for the LPs of on_mask, nobody else's output is touched (pdlpdev_batch_spmv)
int batch_enqueue_plain(int K, hipStream_t s, const BatchProductSide& side, int transpose, int len, const void* ray_table, unsigned on_mask, double* vK);
