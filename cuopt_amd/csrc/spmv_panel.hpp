// The panel layout's SpMV skeleton (device code).  Included by kernels_panel.hip only; the layout's view struct and constants, which the
// host side needs too, stay in pdlp_kernels.hpp.
#pragma once
#include <type_traits>

#include "pdlp_kernels.hpp"

namespace pdlp {

// ---- the chunks of a panel, one stage ahead ------------------------------------------------------------------------
// A chunk is <= kPanelChunk consecutive nonzeros of one tile, handled in R = ceil(len / 512) rounds (lane <-> nonzero;
// only the last round has idle lanes: they re-read the chunk's last nonzero and never store).  The value / column
// loads and the packed 16-bit row extents of chunk i+1 are requested before the row sums of chunk i, so one of the two
// dependent memory round trips of a chunk (matrix stream -> gather) always overlaps LDS work of the same workgroup.
// Stages are straight-line code selected by a switch on R (exact load accounting, no wasted gathers); the request of the next chunk
// is, by default, a chain of rounds behind its extent loads instead (panel_load_rounds, PanelView::req_order).
struct PanelChunk {
  int s, c0, c1, t0;  // tile (slab) index, nonzero range of the chunk, start of its tile
  bool valid;
};
template <int R>
__device__ __forceinline__ void panel_load(const PanelView& P, double (&va)[kPanelPer], int (&ja)[kPanelPer], int c0, int c1)
{
#pragma unroll
  for (int u = 0; u < R; ++u) {
    int k = c0 + threadIdx.x + u * kPanelThreads;
    if (u == R - 1) k = k < c1 ? k : c1 - 1;
    va[u] = __builtin_nontemporal_load(P.val + k);
    ja[u] = __builtin_nontemporal_load(P.col + k);
  }
}
// The same loads for the request that goes out behind the extent loads (PanelView::req_order), without the switch on the number of
// rounds.  The compiler lays the cases of that switch one behind the other, and a case that computes anything -- an address, the
// clamped index, a move out of the spare registers it loaded into -- waits for whatever a case in front of it MIGHT have loaded into
// the registers it computes in: a wait three loads into a request and, where the cases meet, a wait for half the request in front of
// the extent loads.  Here every lane's byte offsets (clamped to the chunk's last entry, so only the last round re-reads it) are final
// before the first load, and round u is loaded where the chunk has a round u: a chain of uniform branches around nothing but loads
// from the chunk's base (scalar registers) plus one offset register each.  A round the chunk does not have is SET (to an entry nothing
// reads): carried through instead, the registers of the request and of the chunk in front of it become two sets with moves between.
__device__ __forceinline__ void panel_load_rounds(const PanelView& P, double (&va)[kPanelPer], int (&ja)[kPanelPer], int c0, int c1, int rounds)
{
  unsigned ov[kPanelPer], oc[kPanelPer];
  const int last = c1 - c0 - 1;
#pragma unroll
  for (int u = 0; u < kPanelPer; ++u) {
    int i = (int)threadIdx.x + u * kPanelThreads;
    i     = i < last ? i : last;
    ov[u] = (unsigned)i * 8u, oc[u] = (unsigned)i * 4u;
    asm volatile("" : "+v"(ov[u]), "+v"(oc[u]));  // (final here: nothing of an address is computed between the loads)
  }
  const char* vb = reinterpret_cast<const char*>(P.val + c0);
  const char* cb = reinterpret_cast<const char*>(P.col + c0);
#pragma unroll
  for (int u = 0; u < kPanelPer; ++u)
    if (u == 0 || u < rounds) {  // (a chunk has a round 0)
      va[u] = __builtin_nontemporal_load(reinterpret_cast<const double*>(vb + ov[u]));
      ja[u] = __builtin_nontemporal_load(reinterpret_cast<const int*>(cb + oc[u]));
    } else {
      va[u] = 0.0, ja[u] = 0;
    }
}
// Column-sorted chunks (P.sorted, uniform): the stored word is slot << kSegColBits | (column - slab_base); the entry at position i of the
// chunk is gathered by lane i % 512 as ever, and its product goes to prod[slot], where the (row, CSR) order would have put it.
__device__ __forceinline__ void panel_decode(int word, int i, bool sorted, int slab_base, int& col, int& slot)
{
  col  = sorted ? slab_base + (int)((unsigned)word & kSegColMask) : word;
  slot = sorted ? (int)((unsigned)word >> kSegColBits) : i;
}
template <int R>
__device__ __forceinline__ void panel_products(const double* __restrict__ vec, double* prod, const double (&va)[kPanelPer],
                                               const int (&ja)[kPanelPer], int len, bool sorted, int slab_base)
{
  double x[R];
  int slot[R];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    int c;
    panel_decode(ja[u], threadIdx.x + u * kPanelThreads, sorted, slab_base, c, slot[u]);
    x[u] = vec[c];
  }
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int i = threadIdx.x + u * kPanelThreads;
    if (u < R - 1 || i < len) prod[slot[u]] = va[u] * x[u];
  }
}
// Zero skip: the gathered vector's entry is fetched only where its bit of the slab's bitmap (LDS, 32-bit words from word `zbase`) is
// set; a clear bit stands for an entry that is exactly 0.0, whose product is stored as +0.0 -- a row sum that starts at +0.0 holds the
// same bits with that addend as with a * (+-0.0).  The bits are read first, then the R gathers go out in one batch as above.
// The LDS window holds kZsQuads * 128 columns from the slab's first quad; a slab wider than that (the default 174 762 columns) has its
// last columns outside the window, and those are gathered whatever they hold -- so the slabs keep the width they had.
template <int R>
__device__ __forceinline__ void panel_products_zs(const double* __restrict__ vec, double* prod, const double (&va)[kPanelPer],
                                                  const int (&ja)[kPanelPer], int len, const unsigned* zbits, int zbase, bool sorted,
                                                  int slab_base)
{
  unsigned w[R];
  int c[R], slot[R];  // (the bitmap is indexed by the absolute column, whichever way it is stored)
#pragma unroll
  for (int u = 0; u < R; ++u) {
    panel_decode(ja[u], threadIdx.x + u * kPanelThreads, sorted, slab_base, c[u], slot[u]);
    const int wi = (c[u] >> 5) - zbase;
    w[u]         = wi < kZsQuads * 4 ? zbits[wi] : ~0u;
  }
  double x[R];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    x[u] = 0.0;
    if ((w[u] >> (c[u] & 31)) & 1u) x[u] = vec[c[u]];
  }
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int i = threadIdx.x + u * kPanelThreads;
    if (u < R - 1 || i < len) prod[slot[u]] = va[u] * x[u];
  }
}
// the bitmap of slab s: the 16-byte quads (128 columns each) from the one that holds the slab's first column to the one that holds its
// last, kZsPer per lane through registers (requested behind one barrier, stored in front of the next: see the hazard comment)
constexpr int kZsPer = (kZsQuads + kPanelThreads - 1) / kPanelThreads;
__device__ __forceinline__ int panel_zs_first_quad(const PanelView& P, int s) { return (int)(((long long)s * P.slab_w) >> 7); }  // (s < S: at most the vector's length)
__device__ __forceinline__ void panel_zs_load(const PanelView& P, int s, uint4 (&st)[kZsPer])
{
  const long long c1 = (long long)(s + 1) * P.slab_w;
  const int last     = (int)(c1 < P.zcols ? c1 : P.zcols) - 1;  // the slab's last column
  const int q0       = panel_zs_first_quad(P, s);
  int nq             = (last >> 7) - q0 + 1;
  nq                 = nq < kZsQuads ? nq : kZsQuads;
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(P.zmask) + q0;
#pragma unroll
  for (int k = 0; k < kZsPer; ++k) {
    const int q = threadIdx.x + k * kPanelThreads;
    st[k]       = uint4{0u, 0u, 0u, 0u};
    if (q < nq) st[k] = src[q];
  }
}
__device__ __forceinline__ void panel_zs_store(uint4* zq, const uint4 (&st)[kZsPer])
{
#pragma unroll
  for (int k = 0; k < kZsPer; ++k) {
    const int q = threadIdx.x + k * kPanelThreads;
    if (q < kZsQuads) zq[q] = st[k];
  }
}
#define PANEL_DISPATCH(rounds, CALL) \
  switch (rounds) {                   \
    case 1: CALL(1); break;           \
    case 2: CALL(2); break;           \
    case 3: CALL(3); break;           \
    case 4: CALL(4); break;           \
    case 5: CALL(5); break;           \
    case 6: CALL(6); break;           \
    case 7: CALL(7); break;           \
    default: CALL(8); break;          \
  }

// ---- a row of its own (more than kPanelOwnRow nonzeros): the whole workgroup strides over it, 16 entries per thread in flight
// (fixed tree, compared with a tolerance like every long row)
template <class Epi>
__device__ __forceinline__ void panel_own_row(const PanelView& P, const double* __restrict__ vec, Epi& epi, double* __restrict__ partials,
                                              int w, int NP, double* scratch /* >= kPanelWaves doubles of LDS */)
{
  const int r  = P.own_row[w - NP];
  const int k0 = P.csr_off[r], k1 = P.csr_off[r + 1];
  double part[1] = {0.0};
  constexpr int kLongU = 16;
  for (int k = k0 + (int)threadIdx.x; k < k1; k += kLongU * kPanelThreads) {
    double a[kLongU];
    int j[kLongU];
#pragma unroll
    for (int u = 0; u < kLongU; ++u) {
      a[u] = 0.0, j[u] = 0;
      if (k + u * kPanelThreads < k1) {
        a[u] = __builtin_nontemporal_load(P.csr_val + k + u * kPanelThreads);
        j[u] = __builtin_nontemporal_load(P.csr_idx + k + u * kPanelThreads);
      }
    }
    double xv[kLongU];
#pragma unroll
    for (int u = 0; u < kLongU; ++u) xv[u] = k + u * kPanelThreads < k1 ? vec[j[u]] : 0.0;
#pragma unroll
    for (int u = 0; u < kLongU; ++u) part[0] = part[0] + a[u] * xv[u];
  }
  if (P.dn_own_seg) {  // the row's dense segments: values and vector are coalesced streams, 8 entries per thread in flight
    for (int sg = P.dn_own_seg[w - NP]; sg < P.dn_own_seg[w - NP + 1]; ++sg) {
      const int len = P.dn_seg_len[sg];
      const double* __restrict__ a = P.dn_val + P.dn_seg_ptr[sg];
      const double* __restrict__ x = vec + P.dn_seg_c0[sg];
      constexpr int kSegU = 8;
      for (int k = (int)threadIdx.x; k < len; k += kSegU * kPanelThreads) {
        double av[kSegU], xv[kSegU];
#pragma unroll
        for (int u = 0; u < kSegU; ++u) {
          const int i = k + u * kPanelThreads;
          av[u] = i < len ? __builtin_nontemporal_load(a + i) : 0.0;
          xv[u] = i < len ? x[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kSegU; ++u) part[0] = part[0] + av[u] * xv[u];
      }
    }
  }
  block_reduce<SumOp, 1, kPanelWaves>(part, scratch);
  double acc[Epi::NQ > 0 ? Epi::NQ : 1];
#pragma unroll
  for (int q = 0; q < (Epi::NQ > 0 ? Epi::NQ : 1); ++q) acc[q] = Epi::Op::identity();
  if (threadIdx.x == 0) {
    epi.row(r, dense_plus(P.dense_add, r, part[0]), acc);
    if constexpr (Epi::NQ > 0) {
#pragma unroll
      for (int q = 0; q < Epi::NQ; ++q) partials[(size_t)q * P.W + w] = acc[q];
    }
  }
}
// the dense segments that reach into a panel of the column side, in LDS: first column, length, where the values start, and the
// gathered vector's entry of the segment's row
struct PanelDenseSegs {
  int n;
  int c0[kPanelDenseSegs], len[kPanelDenseSegs], ptr[kPanelDenseSegs];
  double y[kPanelDenseSegs];
};
__device__ __forceinline__ void panel_dense_prepare(const PanelView& P, int w, const double* __restrict__ vec, PanelDenseSegs* D)
{
  if (!P.dn_pan_ptr) return;  // (uniform)
  const int q0 = P.dn_pan_ptr[w], n = P.dn_pan_ptr[w + 1] - q0;
  if (threadIdx.x == 0) D->n = n;
  if ((int)threadIdx.x < n) {
    const int sg = P.dn_pan_seg[q0 + threadIdx.x];
    D->c0[threadIdx.x] = P.dn_seg_c0[sg], D->len[threadIdx.x] = P.dn_seg_len[sg], D->ptr[threadIdx.x] = P.dn_seg_ptr[sg];
    D->y[threadIdx.x]  = vec[P.dn_seg_row[sg]];
  }
}
// what the dense segments contribute to column j of the panel, ascending rows: the sum k_dense_cols formed.  Added in the epilogue
// (as cheap as the kernel it replaces, one launch less; starting the rows' LDS sums from it at the head of the kernel instead was
// measured 5 us SLOWER: one more barrier in front of the first chunk)
__device__ __forceinline__ double panel_dense_col(const PanelView& P, const PanelDenseSegs* D, int j)
{
  double add   = 0.0;
  const int ns = D->n;
  for (int q = 0; q < ns; ++q) {
    const int k = j - D->c0[q];
    if (k >= 0 && k < D->len[q]) add += __builtin_nontemporal_load(P.dn_val + D->ptr[q] + k) * D->y[q];
  }
  return add;
}
// the fused epilogue over a panel's rows, natural order, from the row sums in LDS: a lane's rows first, first + 512, ... through row(),
// then the workgroup's partials
template <class Epi>
__device__ __forceinline__ void panel_epilogue_rows(const PanelView& P, Epi& epi, double (&acc)[Epi::NQ > 0 ? Epi::NQ : 1], const double* psum,
                                                    int first, int r0, int nr, const PanelDenseSegs* D, const double* psum2)
{
  for (int r = first; r < nr; r += kPanelThreads)
    if (__double_as_longlong(psum[r]) != kPanelNotMine) {
      double v = psum2 ? psum[r] + psum2[r] : psum[r];
      if (P.dn_pan_ptr) v = v + panel_dense_col(P, D, r0 + r);
      epi.row(r0 + r, dense_plus(P.dense_add, r0 + r, v), acc);
    }
}
template <class Epi>
__device__ __forceinline__ void panel_epilogue_partials(const PanelView& P, double* __restrict__ partials, double (&acc)[Epi::NQ > 0 ? Epi::NQ : 1],
                                                        double* red, int w)
{
  if constexpr (Epi::NQ > 0) {
    block_reduce<typename Epi::Op, Epi::NQ, kPanelWaves>(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int q = 0; q < Epi::NQ; ++q) partials[(size_t)q * P.W + w] = acc[q];
    }
  }
}
template <class Epi>
__device__ __forceinline__ void panel_epilogue(const PanelView& P, Epi& epi, double* __restrict__ partials, const double* psum, double* red,
                                               int w, int r0, int nr, const PanelDenseSegs* D,
                                               const double* psum2 = nullptr /* long-tail variant: the edge runs' share */)
{
  double acc[Epi::NQ > 0 ? Epi::NQ : 1];
#pragma unroll
  for (int q = 0; q < (Epi::NQ > 0 ? Epi::NQ : 1); ++q) acc[q] = Epi::Op::identity();
  panel_epilogue_rows(P, epi, acc, psum, threadIdx.x, r0, nr, D, psum2);
  panel_epilogue_partials<Epi>(P, partials, acc, red, w);
}

// ---- the epilogue's operands, requested before the last row sums ------------------------------------------------------------------
// An epilogue with an `Ops` type (pdlp_epilogues.hpp: the two products of an attempt and their Halpern twins) splits row() into
// load() and apply().  The walkers below request the operands of a lane's first kPanelEpiDepth rows in ONE batch where their final
// chunk would have requested a following chunk: the round trip to HBM runs under the final chunk's row sums instead of once per
// row, one after the other, at the tail of the kernel.  Register budget: the final chunk is peeled off the chunk loop, so the
// batch is never live across the loop and takes the registers the stream no longer needs (va / ja / gathered x / ext_next, about
// 45 VGPRs in the row kernel; the largest batch, HalpernStepEpilogue's, is 4 x 5 doubles = 40) -- every panel kernel stays within the
// 128 VGPRs that two workgroups per CU allow.  Epilogues without `Ops` (Store, Eval) keep row() and their loop as it was.
constexpr int kPanelEpiDepth = 4;  // rows per lane requested early (C3: ~1 960 rows per panel = 4 per lane); later rows: row()
template <class Epi, class = void>
struct PanelEarlyOps {
  static constexpr bool on = false;
  struct type {};
};
template <class Epi>
struct PanelEarlyOps<Epi, std::void_t<typename Epi::Ops>> {
  static constexpr bool on = true;
  using type = typename Epi::Ops;
};
// (lanes without a row at a slot clamp the index like PANEL_REQUEST; a slot on a "not mine" row is loaded and never used)
template <class Epi>
__device__ __forceinline__ void panel_epilogue_request(const Epi& epi, typename Epi::Ops (&pre)[kPanelEpiDepth], int r0, int nr)
{
#pragma unroll
  for (int q = 0; q < kPanelEpiDepth; ++q) {
    int r  = threadIdx.x + q * kPanelThreads;
    r      = r < nr ? r : 0;
    pre[q] = epi.load(r0 + r);
  }
}
// panel_epilogue with the operands of the first kPanelEpiDepth slots already requested: the same rows per lane in the same ascending
// order into `acc`, the same skip, addends, reduction and partials slot
template <class Epi>
__device__ __forceinline__ void panel_epilogue_early(const PanelView& P, Epi& epi, double* __restrict__ partials, const double* psum, double* red,
                                                     int w, int r0, int nr, const PanelDenseSegs* D,
                                                     const typename Epi::Ops (&pre)[kPanelEpiDepth], const double* psum2 = nullptr)
{
  double acc[Epi::NQ > 0 ? Epi::NQ : 1];
#pragma unroll
  for (int q = 0; q < (Epi::NQ > 0 ? Epi::NQ : 1); ++q) acc[q] = Epi::Op::identity();
  // ONE wait for the whole batch, in front of the first store: left to the compiler, slot q + 1 waits for its operands behind the
  // branches around slot q's stores, where it no longer knows how many stores are in flight and waits for all of them -- a store's
  // round trip per slot.  (gfx9 encoding of s_waitcnt: vmcnt(0), expcnt and lgkmcnt untouched)
  __builtin_amdgcn_s_waitcnt(0x0F70);
#pragma unroll
  for (int q = 0; q < kPanelEpiDepth; ++q) {
    const int r = threadIdx.x + q * kPanelThreads;
    if (r < nr && __double_as_longlong(psum[r]) != kPanelNotMine) {
      double v = psum2 ? psum[r] + psum2[r] : psum[r];
      if (P.dn_pan_ptr) v = v + panel_dense_col(P, D, r0 + r);
      epi.apply(r0 + r, dense_plus(P.dense_add, r0 + r, v), pre[q], acc);
    }
  }
  panel_epilogue_rows(P, epi, acc, psum, threadIdx.x + kPanelEpiDepth * kPanelThreads, r0, nr, D, psum2);
  panel_epilogue_partials<Epi>(P, partials, acc, red, w);
}

// the row sums of one staged chunk [lo, hi) of its tile: lane r % 512 adds row r's segment of prod[] to psum[r]
// (`slots`, uniform: the slots that hold a row of the panel, ceil(nr / 512), or kPanelRowsPer where the bound is not in use)
// A TUNING CONSTANT, not the exact bound: the first kPanelRowsLow slots are requested and walked in every panel (a panel of 300 rows
// still issues four extent loads, three of them of row 0), the others only in a panel of more rows than those slots hold -- ONE
// uniform branch instead of one per slot, which cost scalar-register spills in the chunk loop.  4 = what C3's ~1 960-row panels need.
constexpr int kPanelRowsLow = 4;
static_assert(kPanelRowsLow < kPanelRowsPer, "");
__device__ __forceinline__ void panel_row_sums(const PanelView& P, const unsigned (&ext)[kPanelRowsPer], const double* prod, double* psum,
                                               int nr, int lo, int hi, int slots)
{
  if (!P.any_long) {  // (uniform) the common case: no extra instruction in the loop
#pragma unroll
    for (int q = 0; q < kPanelRowsPer; ++q) {
      if (q == kPanelRowsLow && slots <= kPanelRowsLow) break;  // (one uniform branch)
      const int r = threadIdx.x + q * kPanelThreads;
      if (r < nr) {
        int a = (int)(ext[q] & 0xFFFFu), b = (int)(ext[q] >> 16);
        a = a > lo ? a : lo;
        b = b < hi ? b : hi;
        if (a < b) {
          double sum = psum[r];
          for (int k = a; k < b; ++k) sum = sum + prod[k - lo];
          psum[r] = sum;
        }
      }
    }
    return;
  }
  bool any_long = false;
#pragma unroll
  for (int q = 0; q < kPanelRowsPer; ++q) {
    const int r = threadIdx.x + q * kPanelThreads;
    if (r < nr) {
      int a = (int)(ext[q] & 0xFFFFu), b = (int)(ext[q] >> 16);
      a = a > lo ? a : lo;
      b = b < hi ? b : hi;
      if (b - a > kLongRow) {
        any_long = true;  // handled below, by the whole wave
      } else if (a < b) {  // left to right by the row's lane: bit-identical to a sequential CSR sum
        double sum = psum[r];
        for (int k = a; k < b; ++k) sum = sum + prod[k - lo];
        psum[r] = sum;
      }
    }
  }
  // A segment longer than kLongRow would keep ONE lane busy for thousands of dependent LDS reads: its wave sums it
  // together instead (64 strided chains + the fixed butterfly; compared with a tolerance like every long row).
  // One ballot per chunk on the common path.
  if (__ballot(any_long)) {
#pragma unroll
    for (int q = 0; q < kPanelRowsPer; ++q) {
      const int r = threadIdx.x + q * kPanelThreads;
      int a = 0, b = 0;
      if (r < nr) {
        a = (int)(ext[q] & 0xFFFFu), b = (int)(ext[q] >> 16);
        a = a > lo ? a : lo;
        b = b < hi ? b : hi;
      }
      unsigned long long todo = __ballot(b - a > kLongRow);
      while (todo) {
        const int l  = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int la = __builtin_amdgcn_readlane(a, l), lb = __builtin_amdgcn_readlane(b, l);
        double part  = 0.0;
        for (int k = la + (int)(threadIdx.x & 63); k < lb; k += 64) part = part + prod[k - lo];
        part = wave_reduce<SumOp>(part);
        if ((int)(threadIdx.x & 63) == l) psum[r] = psum[r] + part;
      }
    }
  }
}

// LDS hazards of panel_spmv_block (round-6 audit; "reader -> next writer: the barrier between them"):
//   prod[]  (ONE buffer; the chunk "one stage ahead" lives in REGISTERS: va / ja / ext_next)
//            written by panel_products of chunk i between barrier T(i) [loop top] and barrier M(i) [after the next chunk's requests];
//            read by the row sums of chunk i after M(i); next written by chunk i + 1 after T(i + 1) -- every row sum of chunk i ends
//            before its thread arrives at T(i + 1).  With column-sorted chunks (P.sorted) a lane writes prod[slot] for the slot its entry
//            carries instead of prod[its own position]: the slots of a chunk are a permutation of 0 .. len - 1, so no two lanes meet
//            at an element, every element below len is written, and the barriers are the same.
//   psum[]  zeroed before the first barrier; row r is read and written by lane r % 512 ONLY (also in the long-segment path: the lane
//            that owns the row adds the wave's partial), the "not mine" marks are written after the first barrier to rows that have no
//            segment in any tile; the epilogue reads behind the barrier after the loop.
//   tile_s / base_s  written once before the first barrier, read-only afterwards.
//   zq[]    (ZS only) the bitmap of the CURRENT chunk's slab.  Read by panel_products_zs of chunk i between T(i) and M(i).  When chunk
//            i + 1 opens another slab, that slab's bits are requested from global memory behind M(i) -- every read of the old bits
//            ends before its thread arrives at M(i) -- held in registers over the row sums of chunk i and stored in front of T(i + 1),
//            the barrier that makes them visible to the first panel_products_zs of the new slab.  The first slab's bits are stored in
//            front of T(0).  The bits themselves were written by k_primal of the same attempt, a kernel boundary away.
// Global memory, the epilogue operands requested early (panel_epilogue_request): nothing is read before its writer.  A row's operands
// are written by that row's own lane only, and only in apply(), behind the request in program order (sumy[i], the Halpern x'[j]: read,
// then written by the same lane); y / lo / hi / x / xn / aty and the anchors are read-only in these kernels; the next-iterate buffers
// are only stored to.  A row with a workgroup of its own is written by that workgroup: its slot here is requested and never used.
// ZS: the instantiation can skip the gathers of zero entries (panel_products_zs); it does so when `zmask` is not null (uniform).
// Without ZS nothing of it is compiled.
template <class Epi, bool ZS = false>
__device__ __forceinline__ void panel_spmv_block(const PanelView& P, const double* __restrict__ vec,
                                                 Epi& epi, double* __restrict__ partials, const unsigned long long* zmask = nullptr)
{
  static_assert(kPanelPer == 8, "PANEL_DISPATCH enumerates 1..8 rounds");
  [[maybe_unused]] uint4* zq = nullptr;
  if constexpr (ZS) {
    __shared__ uint4 zq_s[kZsQuads];
    zq = zq_s;
  }
  const bool zon = ZS && zmask != nullptr;
  __shared__ double prod[kPanelChunk];
  __shared__ double psum[kPanelMaxRows];
  __shared__ double red[kPanelWaves * (Epi::NQ > 0 ? Epi::NQ : 1)];
  __shared__ int tile_s[17];        // this panel's tile boundaries (S <= 16) and row-pointer bases, fetched once
  __shared__ long long base_s[16];
  const int w  = blockIdx.x;
  const int NP = P.NP ? P.NP : P.W;
  if (w >= NP) {
    panel_own_row(P, vec, epi, partials, w, NP, prod);
    return;
  }
  __shared__ PanelDenseSegs dseg;
  const int r0 = P.row0[w], nr = P.row0[w + 1] - r0;
  panel_dense_prepare(P, w, vec, &dseg);  // (visible after the barriers of the chunk loop / before the epilogue)
  if (threadIdx.x <= P.S) tile_s[threadIdx.x] = P.tile_ptr[w * P.S + threadIdx.x];
  if (threadIdx.x < P.S) base_s[threadIdx.x] = P.rp_base[w * P.S + threadIdx.x];
  for (int r = threadIdx.x; r < nr; r += kPanelThreads) psum[r] = 0.0;
  __syncthreads();
  if (P.own_ptr)  // rows that have a workgroup of their own: no segment of theirs is in the tiles, the epilogue below skips them
    for (int q = P.own_ptr[w] + (int)threadIdx.x; q < P.own_ptr[w + 1]; q += kPanelThreads) psum[P.own_row[q] - r0] = __longlong_as_double(kPanelNotMine);
  // (the tile boundaries are the same in every lane; read through the first lane the compiler knows it too: the chunk's bookkeeping
  // stays in scalar registers, the chunk loop and the switches on the number of rounds are scalar branches -- left as LDS values
  // they count as different from lane to lane, and the cases of a switch are then laid one behind the other under execution masks,
  // each waiting for the loads a case in front of it MIGHT have issued)
  auto tile = [&](int i) -> int { return __builtin_amdgcn_readfirstlane(tile_s[i]); };
  auto advance = [&](PanelChunk c) -> PanelChunk {
    if (c.valid && c.c1 < tile(c.s + 1)) {  // next chunk of the same tile
      c.c0 = c.c1;
      c.c1 = c.c0 + kPanelChunk < tile(c.s + 1) ? c.c0 + kPanelChunk : tile(c.s + 1);
      return c;
    }
    int s = c.s + 1;
    while (s < P.S && tile(s + 1) == tile(s)) ++s;  // empty tiles contribute nothing
    c.valid = s < P.S;
    c.s     = s;
    if (c.valid) {
      c.t0 = c.c0 = tile(s);
      c.c1 = c.c0 + kPanelChunk < tile(s + 1) ? c.c0 + kPanelChunk : tile(s + 1);
    }
    return c;
  };
  double va[kPanelPer];
  int ja[kPanelPer];
  // (begin | end << 16) of the lane's rows in the chunk's tile.  The extent-first request leaves the slots a panel does not have
  // unwritten; they are neither copied to `ext` (the copy below has the request's bound) nor read by a row sum (r < nr fails there).
  // Setting them once instead keeps three more values alive round the chunk loop: measured 0.8 % of the headline rate.
  unsigned ext_next[kPanelRowsPer], ext[kPanelRowsPer];
  // (macros for what touches the register arrays lane by lane: they must stay visible to scalar replacement)
#define PANEL_ROUNDS(c) (((c).c1 - (c).c0 + kPanelThreads - 1) / kPanelThreads)
#define PANEL_CALL_LOAD(R) panel_load<R>(P, va, ja, nxt.c0, nxt.c1)
#define PANEL_CALL_PRODUCTS(R) panel_products<R>(vec, prod, va, ja, cur.c1 - cur.c0, P.sorted != 0, cur.s * P.slab_w)
#define PANEL_CALL_PRODUCTS_ZS(R) panel_products_zs<R>(vec, prod, va, ja, cur.c1 - cur.c0, reinterpret_cast<const unsigned*>(zq), panel_zs_first_quad(P, cur.s) << 2, P.sorted != 0, cur.s * P.slab_w)
#define PANEL_REQUEST(c)                                                         \
  if ((c).valid) {                                                               \
    PANEL_DISPATCH(PANEL_ROUNDS(c), PANEL_CALL_LOAD)                             \
    const uint16_t* __restrict__ rp_ = P.rowptr + base_s[(c).s];                 \
    _Pragma("unroll") for (int q = 0; q < kPanelRowsPer; ++q) {                  \
      int r_      = threadIdx.x + q * kPanelThreads;                             \
      r_          = r_ < nr ? r_ : 0;                                            \
      ext_next[q] = (unsigned)rp_[r_] | ((unsigned)rp_[r_ + 1] << 16);           \
    }                                                                            \
  }
  // The same request in the other order (PanelView::req_order): the extents first -- of the first kPanelRowsLow slots always, of the
  // others only where the panel has more rows than those hold (C3: ~1 960 rows, 4 slots of 7) -- then the stream.
#define PANEL_EXTENT(q)                                                          \
  {                                                                              \
    int r_      = threadIdx.x + (q) * kPanelThreads;                             \
    r_          = r_ < nr ? r_ : 0;                                              \
    ext_next[q] = (unsigned)rp_[r_] | ((unsigned)rp_[r_ + 1] << 16);             \
  }
#define PANEL_REQUEST_EXT_FIRST(c)                                                                         \
  if ((c).valid) {                                                                                         \
    const uint16_t* __restrict__ rp_ = P.rowptr + base_s[(c).s];                                           \
    _Pragma("unroll") for (int q = 0; q < kPanelRowsLow; ++q) PANEL_EXTENT(q)                              \
    if (slots > kPanelRowsLow) {                                                                           \
      _Pragma("unroll") for (int q = kPanelRowsLow; q < kPanelRowsPer; ++q) PANEL_EXTENT(q)                \
    }                                                                                                      \
    panel_load_rounds(P, va, ja, (c).c0, (c).c1, PANEL_ROUNDS(c));                                         \
  }
  const bool ext_first = P.req_order != 0;                                                     // (uniform)
  const int slots      = ext_first ? (nr + kPanelThreads - 1) / kPanelThreads : kPanelRowsPer;  // (nr <= kPanelMaxRows)
  PanelChunk none{-1, 0, 0, 0, false};
  PanelChunk nxt = advance(none);
  PanelChunk cur = nxt;
  constexpr bool kEarly = PanelEarlyOps<Epi>::on;
  [[maybe_unused]] typename PanelEarlyOps<Epi>::type pre[kPanelEpiDepth];
  [[maybe_unused]] int lo_last = 0, hi_last = 0;
  // The first request and the chunk loop stand ONCE PER ORDER of the request (a generic lambda, inlined twice, the order a constant in
  // each copy).  Where two orders meet inside a loop, the compiler counts what EITHER may have in flight into whichever registers:
  // row sums shared behind such a meeting point wait for the request in the registers the other order loads into, and the two
  // orders' register sets are moved into each other once per chunk.  Once the order has settled, the other copy can go.
  auto walk = [&](auto first) __attribute__((always_inline)) {
    constexpr bool kFirst = decltype(first)::value;
    if constexpr (kFirst) { PANEL_REQUEST_EXT_FIRST(nxt) }
    else { PANEL_REQUEST(nxt) }
    if (zon && cur.valid) {  // the first slab's bits (zon is a constant false without ZS: nothing of the bitmap is compiled there)
      uint4 st[kZsPer];
      panel_zs_load(P, cur.s, st);
      panel_zs_store(zq, st);
    }
    while (cur.valid) {
      __syncthreads();  // the previous chunk's row sums are done with prod
      if (zon) { PANEL_DISPATCH(PANEL_ROUNDS(cur), PANEL_CALL_PRODUCTS_ZS) }
      else { PANEL_DISPATCH(PANEL_ROUNDS(cur), PANEL_CALL_PRODUCTS) }
#pragma unroll
      for (int q = 0; q < kPanelRowsLow; ++q) ext[q] = ext_next[q];
      if (!kFirst || slots > kPanelRowsLow) {  // (the slots the request wrote: all of them in the other order)
#pragma unroll
        for (int q = kPanelRowsLow; q < kPanelRowsPer; ++q) ext[q] = ext_next[q];
      }
      const int lo = cur.c0 - cur.t0, hi = cur.c1 - cur.t0;
      nxt = advance(cur);
      if constexpr (kEarly)
        if (!nxt.valid) {  // the final chunk leaves the loop here: what it requests instead of a chunk is live only below the loop
          lo_last = lo, hi_last = hi;
          break;
        }
      if constexpr (kFirst) { PANEL_REQUEST_EXT_FIRST(nxt) }  // in flight during the row sums below
      else { PANEL_REQUEST(nxt) }
      __syncthreads();
      if (zon && nxt.valid && nxt.s != cur.s) {  // (uniform) the next chunk opens another slab: its bits travel under the row sums
        uint4 st[kZsPer];
        panel_zs_load(P, nxt.s, st);
        panel_row_sums(P, ext, prod, psum, nr, lo, hi, slots);
        panel_zs_store(zq, st);
      } else {
        panel_row_sums(P, ext, prod, psum, nr, lo, hi, slots);
      }
      cur = nxt;
    }
  };
  if (ext_first) walk(std::true_type{});
  else walk(std::false_type{});
#undef PANEL_REQUEST_EXT_FIRST
#undef PANEL_EXTENT
#undef PANEL_REQUEST
#undef PANEL_CALL_PRODUCTS_ZS
#undef PANEL_CALL_PRODUCTS
#undef PANEL_CALL_LOAD
#undef PANEL_ROUNDS
  if constexpr (kEarly) {
    panel_epilogue_request(epi, pre, r0, nr);  // (a panel without a chunk requests here as well)
    if (cur.valid) {  // the final chunk's row sums, the request in flight
      __syncthreads();
      panel_row_sums(P, ext, prod, psum, nr, lo_last, hi_last, slots);
    }
    __syncthreads();
    panel_epilogue_early(P, epi, partials, psum, red, w, r0, nr, &dseg, pre);
  } else {
    __syncthreads();
    panel_epilogue(P, epi, partials, psum, red, w, r0, nr, &dseg);
  }
}
// ------------------------------------------------------------------------------------------------
// Long-tail variant of the panels: row sums dealt by NONZERO, not by row.
// The panel kernel above gives every ROW of the panel a lane, which walks the row's segment of the staged chunk while its wave
// waits for the longest one: on a matrix whose row lengths have a heavy tail (power law: 0.26 of the HBM roofline in round 3,
// 21.6 M issue cycles against 14.0 M on the uniform matrix of the same size) that walk is what the kernel waits for.  Here
//   * the storage is the panels' (chunk entry i <-> lane i % 512, round i / 512: neighbouring lanes hold neighbouring nonzeros, which
//     is what lets the texture path merge the gathers of neighbouring columns -- a first version that gave each lane CONSECUTIVE
//     entries lost 8 % on matrices with a diagonal for exactly that reason); each entry carries its row within the panel (12 bits)
//     next to its column relative to the slab (20 bits): 12 bytes per nonzero and no row pointers at all; products stay in registers;
//   * per round, a wave holds 64 consecutive entries: a segmented scan over the wave (DPP, fixed tree) sums the runs of equal rows;
//     a run that lies inside the wave-round is added to its row's LDS sum by the lane that ends it (LDS atomic as a fire-and-forget
//     add: one emission per run and chunk, so never two lanes at one row between two barriers);
//   * the runs that touch the edges of a wave-round (at most two per wave and round) go to a table of 64 records per chunk; after the
//     chunk's ONE barrier wave 0 joins neighbouring records of equal rows -- a second, 64-lane segmented scan in logical order --
//     and adds the joined sums to a second LDS strip that only it writes (so no emission of the next chunk can race with it).
// The work of a chunk is the same whatever the row lengths are; rows of any length need no special path.  The additions of a row are
// no longer left to right: this layout is compared with the oracle at rtol 1e-12 for EVERY row (the contract of rows > kLongRow in
// the other layouts), which is why `auto` takes it only for long-tailed matrices (build_panels) and the uniform ones keep their
// bit-exact kernels.
// ------------------------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double seg_dpp(double v)
{
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, false);
  return __hiloint2double(hi, lo);
}
// inclusive sums over the wave's lanes, restarting at every lane >= seg0 (seg0: the first lane of this lane's segment): four row_shr
// steps inside the 16-lane DPP rows, then the row totals through row_bcast:15 / row_bcast:31 -- VALU only, a fixed tree
__device__ __forceinline__ double seg_scan(double S, int lane, int seg0)
{
  double u;
  u = seg_dpp<0x111, 0xf>(S); if ((lane & 15) >= 1 && lane - 1 >= seg0) S = S + u;
  u = seg_dpp<0x112, 0xf>(S); if ((lane & 15) >= 2 && lane - 2 >= seg0) S = S + u;
  u = seg_dpp<0x114, 0xf>(S); if ((lane & 15) >= 4 && lane - 4 >= seg0) S = S + u;
  u = seg_dpp<0x118, 0xf>(S); if ((lane & 15) >= 8 && lane - 8 >= seg0) S = S + u;
  u = seg_dpp<0x142, 0xa>(S); if ((lane & 16) && (lane | 15) - 16 >= seg0) S = S + u;  // rows 1, 3 <- the last lane of rows 0, 2
  u = seg_dpp<0x143, 0xc>(S); if (lane >= 32 && 31 >= seg0) S = S + u;                 // rows 2, 3 <- lane 31
  return S;
}
__device__ __forceinline__ void seg_emit(double* strip, int row, double v)
{
  __hip_atomic_fetch_add(strip + row, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// the edge runs of one wave-round: the run that starts at lane 0 and -- unless that run fills the whole wave-round -- the run that
// ends at lane 63
struct SegRecord {
  double lsum, rsum;
  int lkey, rkey;  // rkey < 0: one run from edge to edge (lsum is its sum)
};
template <int R>
__device__ __forceinline__ void seg_load(const PanelView& P, double (&va)[kPanelPer], int (&pk)[kPanelPer], int c0, int c1)
{
#pragma unroll
  for (int u = 0; u < R; ++u) {
    int k = c0 + threadIdx.x + u * kPanelThreads;
    if (u == R - 1) k = k < c1 ? k : c1 - 1;
    va[u] = __builtin_nontemporal_load(P.val + k);
    pk[u] = __builtin_nontemporal_load(P.col + k);
  }
}
template <int R>
__device__ __forceinline__ void seg_rounds(const double* __restrict__ vec, int slab_base, const double (&va)[kPanelPer], const int (&pk)[kPanelPer], int len,
                                           double* psum, SegRecord* rec /* this wave's records of the chunk, one per round */, int lane)
{
  double x[R];
#pragma unroll
  for (int u = 0; u < R; ++u) x[u] = vec[slab_base + (int)((unsigned)pk[u] & kSegColMask)];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int i   = threadIdx.x + u * kPanelThreads;
    const int key = (int)((unsigned)pk[u] >> kSegColBits);
    const double v = (u < R - 1 || i < len) ? va[u] * x[u] : 0.0;  // lanes behind the chunk's end repeat its last entry's row with nothing to add
    const int prev = __builtin_amdgcn_update_dpp(-1, key, 0x138, 0xf, 0xf, false);  // wave_shr:1 (lane 0: -1, no row)
    const unsigned long long starts = __ballot(key != prev);                       // bit t: a run starts at lane t (bit 0 always)
    const unsigned long long below  = starts & ((2ull << lane) - 1ull);
    const int seg0                  = 63 - __builtin_clzll(below);
    const double S                  = seg_scan(v, lane, seg0);
    const bool ends                 = lane == 63 || ((starts >> (lane + 1)) & 1ull);
    if (ends) {
      if (seg0 == 0) {  // the run that started at the wave-round's left edge
        rec[u].lsum = S, rec[u].lkey = key;
        if (lane == 63) rec[u].rkey = -1;
      } else if (lane == 63) {
        rec[u].rsum = S, rec[u].rkey = key;
      } else {
        seg_emit(psum, key, S);
      }
    }
  }
}
// wave 0, behind a chunk's barrier: joins the chunk's edge-run records (R rounds) and emits the joined sums to psum2
__device__ __forceinline__ void panel_seg_join(const SegRecord* rec /* the chunk's parity */, double* psum2, int R, int lane)
{
  // join the edge runs in logical order: lane l <-> wave-round (round l / 8, wave l % 8), two pieces each (the run from the
  // left edge, the run to the right edge; one piece when a single run fills the wave-round)
  const int u = lane >> 3, q = lane & 7;
  const bool on = u < R;
  SegRecord g{0.0, 0.0, 0, -1};
  if (on) g = rec[q * kPanelPer + u];
  const bool single = g.rkey < 0;
  const int my_first = g.lkey, my_last = single ? g.lkey : g.rkey;
  const double open  = on ? (single ? g.lsum : g.rsum) : 0.0;  // the run still open at this lane's right edge
  int prev_last      = __builtin_amdgcn_update_dpp(0, my_last, 0x138, 0xf, 0xf, false);
  if (lane == 0) prev_last = my_first;
  const bool flag = on && (!single || my_first != prev_last);  // a run ends inside this lane's pieces or at its left edge
  const unsigned long long fm = __ballot(flag);
  const unsigned long long at_or_below = fm & ((2ull << lane) - 1ull);
  const int seg0  = at_or_below ? 63 - __builtin_clzll(at_or_below) : 0;
  const double S  = seg_scan(open, lane, seg0);
  double carry_in = seg_dpp<0x138, 0xf>(S);
  if (lane == 0) carry_in = 0.0;
  if (on) {
    int key    = prev_last;
    double sum = carry_in;
    if (my_first != key) {
      seg_emit(psum2, key, sum);
      key = my_first, sum = 0.0;
    }
    sum = sum + g.lsum;
    if (!single) {
      seg_emit(psum2, key, sum);
      key = g.rkey, sum = g.rsum;
    }
    if (lane == R * kPanelWaves - 1) seg_emit(psum2, key, sum);  // the chunk's last wave-round closes what is still open
  }
}
// LDS hazards of panel_seg_block (round-6 audit):
//   rec[2][]  the edge-run records, double-buffered by chunk parity.  rec[p] is written by every wave during the rounds of chunk i
//             (parity p), read by wave 0's join after the chunk's barrier B(i), and next written during the rounds of chunk i + 2,
//             i.e. after B(i + 1) -- wave 0 finishes its join of chunk i, in program order, before it arrives at B(i + 1).
//   psum[]    LDS atomics (ds_add_f64) from every wave, at most ONE emission per row and chunk (a row's interior run lies inside one
//             wave-round; its edge runs go through the records), so two chunks' emissions to one row are separated by a barrier and
//             the order of a row's additions is fixed.
//   psum2[]   emitted to by wave 0 alone (the joined edge runs), in program order.
//   the epilogue reads psum + psum2 behind the barrier after the loop.
// Global memory, the epilogue operands requested early: as in panel_spmv_block (nothing is read before its writer).
template <class Epi>
__device__ __forceinline__ void panel_seg_block(const PanelView& P, const double* __restrict__ vec, Epi& epi, double* __restrict__ partials)
{
  static_assert(kPanelPer == 8 && kPanelWaves == 8, "64 wave-rounds per chunk: one lane of wave 0 each");
  static_assert(kPanelMaxRows <= (1 << (32 - kSegColBits)), "row within the panel must fit beside the column");
  __shared__ double psum[kPanelMaxRows];   // runs inside a wave-round (every wave emits)
  __shared__ double psum2[kPanelMaxRows];  // runs that touch a wave-round's edge, joined (wave 0 alone emits)
  __shared__ double red[kPanelWaves * (Epi::NQ > 0 ? Epi::NQ : 1)];
  __shared__ SegRecord rec[2][kPanelWaves * kPanelPer];  // [chunk parity][wave * 8 + round]
  __shared__ int tile_s[17];
  const int w  = blockIdx.x;
  const int NP = P.NP ? P.NP : P.W;
  if (w >= NP) {
    panel_own_row(P, vec, epi, partials, w, NP, psum);
    return;
  }
  __shared__ PanelDenseSegs dseg;
  const int r0 = P.row0[w], nr = P.row0[w + 1] - r0;
  panel_dense_prepare(P, w, vec, &dseg);
  if (threadIdx.x <= P.S) tile_s[threadIdx.x] = P.tile_ptr[w * P.S + threadIdx.x];
  for (int r = threadIdx.x; r < nr; r += kPanelThreads) psum[r] = 0.0, psum2[r] = 0.0;
  __syncthreads();
  if (P.own_ptr)
    for (int q = P.own_ptr[w] + (int)threadIdx.x; q < P.own_ptr[w + 1]; q += kPanelThreads) psum[P.own_row[q] - r0] = __longlong_as_double(kPanelNotMine);
  auto advance = [&](PanelChunk c) -> PanelChunk {
    if (c.valid && c.c1 < tile_s[c.s + 1]) {
      c.c0 = c.c1;
      c.c1 = c.c0 + kPanelChunk < tile_s[c.s + 1] ? c.c0 + kPanelChunk : tile_s[c.s + 1];
      return c;
    }
    int s = c.s + 1;
    while (s < P.S && tile_s[s + 1] == tile_s[s]) ++s;
    c.valid = s < P.S;
    c.s     = s;
    if (c.valid) {
      c.t0 = c.c0 = tile_s[s];
      c.c1 = c.c0 + kPanelChunk < tile_s[s + 1] ? c.c0 + kPanelChunk : tile_s[s + 1];
    }
    return c;
  };
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double va[kPanelPer];
  int pk[kPanelPer];
#define SEG_ROUNDS(c) (((c).c1 - (c).c0 + kPanelThreads - 1) / kPanelThreads)
#define SEG_CALL_LOAD(R) seg_load<R>(P, va, pk, nxt.c0, nxt.c1)
#define SEG_CALL_ROUNDS(R) seg_rounds<R>(vec, cur.s * P.slab_w, va, pk, cur.c1 - cur.c0, psum, &rec[parity][wave * kPanelPer], lane)
  PanelChunk none{-1, 0, 0, 0, false};
  PanelChunk nxt = advance(none);
  if (nxt.valid) { PANEL_DISPATCH(SEG_ROUNDS(nxt), SEG_CALL_LOAD) }
  PanelChunk cur = nxt;
  int parity = 0;
  constexpr bool kEarly = PanelEarlyOps<Epi>::on;
  [[maybe_unused]] typename PanelEarlyOps<Epi>::type pre[kPanelEpiDepth];
  [[maybe_unused]] int R_last = 0;
  while (cur.valid) {
    const int R = SEG_ROUNDS(cur);
    PANEL_DISPATCH(R, SEG_CALL_ROUNDS)   // gathers, products, the runs inside the wave-rounds, the edge records
    nxt = advance(cur);
    if constexpr (kEarly)
      if (!nxt.valid) {  // the final chunk leaves the loop here (see panel_spmv_block)
        R_last = R;
        break;
      }
    if (nxt.valid) { PANEL_DISPATCH(SEG_ROUNDS(nxt), SEG_CALL_LOAD) }  // the next chunk's stream, in flight over the barrier and the join
    __syncthreads();  // the chunk's records are complete; every emission of the chunk before is done
    if (wave == 0) panel_seg_join(rec[parity], psum2, R, lane);
    parity ^= 1;
    cur = nxt;
  }
#undef SEG_CALL_ROUNDS
#undef SEG_CALL_LOAD
#undef SEG_ROUNDS
  if constexpr (kEarly) {
    panel_epilogue_request(epi, pre, r0, nr);
    if (cur.valid) {  // the final chunk's barrier and join, the request in flight
      __syncthreads();
      if (wave == 0) panel_seg_join(rec[parity], psum2, R_last, lane);
    }
    __syncthreads();
    panel_epilogue_early(P, epi, partials, psum, red, w, r0, nr, &dseg, pre, psum2);
  } else {
    __syncthreads();
    panel_epilogue(P, epi, partials, psum, red, w, r0, nr, &dseg, psum2);
  }
}
#undef PANEL_DISPATCH
template <bool SEG, class Epi>
__device__ __forceinline__ void panel_block(const PanelView& P, const double* __restrict__ vec, Epi& epi, double* __restrict__ partials)
{
  if constexpr (SEG) panel_seg_block(P, vec, epi, partials);
  else panel_spmv_block(P, vec, epi, partials);
}
// the product whose gathered vector comes with a bitmap of its non-zeros (P.zmask, null: none): the row-sum variant can skip the zeros
template <bool SEG, class Epi>
__device__ __forceinline__ void panel_block_zs(const PanelView& P, const double* __restrict__ vec, Epi& epi, double* __restrict__ partials, bool on)
{
  if constexpr (SEG) panel_seg_block(P, vec, epi, partials);
  else panel_spmv_block<Epi, true>(P, vec, epi, partials, on ? P.zmask : nullptr);
}

}  // namespace pdlp
