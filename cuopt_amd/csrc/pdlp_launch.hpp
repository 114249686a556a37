// Launch helpers shared by the translation units of the core (pdlp_device.hip: set-up, the attempt, results; pdlp_eval.hip: the major
// iteration): argument packing for hipExtLaunchKernel-style launches with the context's timing hooks, the per-layout launch wrappers
// (the two geometries of the jagged kernels, the two launches of a gather-free product), and launch_product, which takes one product
// of one matrix side to the kernels of the side's layout.  (allow_dynamic_lds, the once-per-kernel LDS attribute: pdlp_ctx.hpp.)
#pragma once
#include <algorithm>
#include <mutex>
#include <tuple>
#include <utility>
#include <vector>

#include "pdlp_ctx.hpp"
#include "pdlp_layouts.hpp"

template <size_t... I, typename Tuple>
static void arg_pointers(Tuple& t, void** out, std::index_sequence<I...>)
{
  ((out[I] = (void*)&std::get<I>(t)), ...);
}
template <typename... KArgs, typename... Args>
static void launch_k(pdlpdev_ctx* c, void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, Args... args)
{
  static_assert(sizeof...(KArgs) == sizeof...(Args), "argument count");
  if (c->prof_armed && c->prof_used < pdlpdev_ctx::kProfPairs) {
    hipEvent_t e0_ = c->prof_ev[2 * c->prof_used], e1_ = c->prof_ev[2 * c->prof_used + 1];
    c->prof_used += 1;
    std::tuple<std::remove_cv_t<KArgs>...> vals{static_cast<KArgs>(args)...};
    void* ptrs[sizeof...(KArgs)];
    arg_pointers(vals, ptrs, std::index_sequence_for<KArgs...>{});
    (void)hipExtLaunchKernel((const void*)kernel, grid, block, ptrs, lds, c->stream, e0_, e1_, 0);
    return;
  }
  kernel<<<grid, block, lds, c->stream>>>(static_cast<KArgs>(args)...);
}
// Launch of a jagged-layout kernel: 80 or 160 KiB of dynamic LDS
template <typename... KArgs, typename... Args>
static int jag_launch(pdlpdev_ctx* c, void (*kernel)(JagView, KArgs...), const JagView& v, Args... args)
{
  const size_t lds = jag_lds_bytes(v.waves);
  TRY(allow_dynamic_lds((const void*)kernel, c->device, lds));
  launch_k(c, kernel, ((v.nblk + 7) & ~7) + v.nlong, v.waves * 64, lds, v, args...);
  return 0;
}
// the two launches of a gather-free SpMV: phase P with the gathered vector picked on the device (mode: GatherMode), ...
static int pb_products(pdlpdev_ctx* c, const pdlpdev_ctx::Pb& L, const double* v0, const double* v1, int mode, int in_loop)
{
  const auto kernel = L.p_threads == 1024 ? k_pb_products<1024> : k_pb_products<512>;
  TRY(allow_dynamic_lds((const void*)kernel, c->device, 160 * 1024));
  launch_k(c, kernel, (L.v.nwg + 7) & ~7, L.p_threads == 1024 ? 1024 : 512, sizeof(double) << L.v.panel_shift, L.v, c->ctl, v0, v1, mode, in_loop);
  return 0;
}
// ... and phase R with the epilogue of the call site (two skeletons: the image in LDS, or -- wide bins -- the accumulators in LDS)
template <typename... KArgs, typename... Args>
static int pb_rows_launch(pdlpdev_ctx* c, void (*kernel)(PbView, KArgs...), const pdlpdev_ctx::Pb& L, Args... args)
{
  const size_t lds = L.v.wide ? kPbwLdsBytes : kPbLdsBytes;
  TRY(allow_dynamic_lds((const void*)kernel, c->device, lds));
  launch_k(c, kernel, (L.v.B + 7) & ~7, L.v.wide ? kPbwThreads : kPbThreads, lds, L.v, args...);
  return 0;
}

// ---- one product of one matrix side, in the side's layout ---------------------------------------------------------------------------
// The kernels of one product: the CSR stream's, the panels' (by SEG), the jagged rows' (WAVES = 8, 16), the gather-free rows' (by WIDE)
template <class S, class P, class J, class B>
struct ProductKernels {
  S* stream;
  P* panel[2];
  J* jag[2];
  B* pb[2];
};
template <class S, class P, class J, class B>
static ProductKernels<S, P, J, B> product_kernels(S* s, P* p0, P* p1, J* j8, J* j16, B* b0, B* b1)
{
  return ProductKernels<S, P, J, B>{s, {p0, p1}, {j8, j16}, {b0, b1}};
}
#define PRODUCT_KERNELS(STREAM, PRODUCT)                                                                                                  \
  product_kernels(STREAM, k_panel_##PRODUCT<false>, k_panel_##PRODUCT<true>, k_jag_##PRODUCT<8>, k_jag_##PRODUCT<16>, k_pb_##PRODUCT<false>, \
                  k_pb_##PRODUCT<true>)
namespace products {
inline const auto a_dual      = PRODUCT_KERNELS(k_spmv_a_dual, a_dual);
inline const auto at_step     = PRODUCT_KERNELS(k_spmv_at_step, at_step);
inline const auto at_cur      = PRODUCT_KERNELS(k_spmv_at_cur, at_cur);
inline const auto plain       = PRODUCT_KERNELS(k_spmv_plain, plain);
inline const auto eval_primal = PRODUCT_KERNELS(k_eval_primal, eval_primal);
inline const auto eval_dual   = PRODUCT_KERNELS(k_eval_dual, eval_dual);
inline const auto a_halpern   = PRODUCT_KERNELS(k_spmv_a_halpern, a_halpern);
inline const auto at_halpern  = PRODUCT_KERNELS(k_spmv_at_halpern, at_halpern);
inline const auto a_halpern_sharded = PRODUCT_KERNELS(k_spmv_a_halpern_sharded, a_halpern_sharded);
}  // namespace products

// the vector a product gathers, as the device picks it (GatherMode, pdlp_epilogues.hpp): one vector as it is, or the trial / the
// current side of a ping-pong pair by the control block; in_loop: the product belongs to an attempt (its kernels ask loop_active)
struct Gathered {
  const double *v0, *v1;
  int mode, in_loop;
  static Gathered fixed(const double* v, bool in_loop = false) { return {v, nullptr, kGatherFixed, in_loop ? 1 : 0}; }
  static Gathered trial(const double* v0, const double* v1, bool in_loop = false) { return {v0, v1, kGatherTrial, in_loop ? 1 : 0}; }
  static Gathered current(const double* v0, const double* v1, bool in_loop = false) { return {v0, v1, kGatherCurrent, in_loop ? 1 : 0}; }
};
// dense row segments: their share of the product lands in the side's dense_add right before the layout's kernel adds it -- unless the
// side's panels add the segments themselves; the owner-computes column block has none
static void dense_prologue(pdlpdev_ctx* c, const pdlpdev_ctx::MatrixSide& s, const Gathered& g)
{
  const pdlpdev_ctx::Dense& D = c->dense;
  if (!D.on || s.fuses_dense() || &s == &c->Oc) return;
  DenseView V{D.row, D.row_seg, D.seg_row, D.seg_c0, D.seg_len, D.seg_ptr, D.tile_ptr, D.tile_seg, D.tile_id, D.val, D.ch_seg, D.ch_k0, D.row_ch, D.ch_part};
  if (&s == &c->At) {
    launch_k(c, k_dense_cols, D.ntiles, kBlock, 0, V, c->n, c->ctl, g.v0, g.v1, g.mode, g.in_loop, s.dense_add);
  } else {
    launch_k(c, k_dense_rows, D.nchunks, kBlock, 0, V, c->ctl, g.v0, g.v1, g.mode, g.in_loop);
    launch_k(c, k_dense_rows_finish, (D.nrows + kBlock - 1) / kBlock, kBlock, 0, V, D.nrows, c->ctl, g.in_loop, s.dense_add);
  }
}
// The launches of one product: the dense prologue, then the layout's kernel (the gather-free layout: phase P, then its row kernel).
// The kernel's arguments come in three groups behind the layout's own leading ones: `pre`, `vecs` (the gathered vectors' pointers:
// the gather-free row kernel goes without them, phase P consumed `g`) and `post`; the stream kernel ends with the side's dense_add.
// Together they are the product's list in pdlp_kernel_decls.hpp: <PRODUCT>_KERNELS' ROW line is pre + vecs + post, its PB line
// pre + post.  `g` names the same vector for the kernels that pick it on the device (Gathered's makers above).
// Returns the code of an attribute call that failed (launch errors are left to the caller's hipGetLastError, as ever).
template <class K, class... Pre, class... Vecs, class... Post>
static int launch_product(pdlpdev_ctx* c, const pdlpdev_ctx::MatrixSide& s, const K& k, const Gathered& g, const std::tuple<Pre...>& pre,
                          const std::tuple<Vecs...>& vecs, const std::tuple<Post...>& post)
{
  dense_prologue(c, s, g);
  switch (s.layout()) {
    case pdlpdev_ctx::MatrixSide::kPb:
      TRY(pb_products(c, s.pb, g.v0, g.v1, g.mode, g.in_loop));
      return std::apply([&](auto... a) { return pb_rows_launch(c, k.pb[s.pb.v.wide ? 1 : 0], s.pb, a...); }, std::tuple_cat(pre, post));
    case pdlpdev_ctx::MatrixSide::kJag:
      return std::apply([&](auto... a) { return jag_launch(c, k.jag[s.jag.v.waves == 16 ? 1 : 0], s.jag.v, a...); }, std::tuple_cat(pre, vecs, post));
    case pdlpdev_ctx::MatrixSide::kPanel:
      std::apply([&](auto... a) { launch_k(c, k.panel[s.pan.v.seg ? 1 : 0], s.pan.v.W, kPanelThreads, 0, s.pan.v, a...); }, std::tuple_cat(pre, vecs, post));
      return 0;
    default:
      std::apply([&](auto... a) { launch_k(c, k.stream, stream_grid(s.nb), kBlock, 0, s.nb, s.rb, s.hot.off, s.hot.idx, s.hot.val, a..., s.dense_add); },
                 std::tuple_cat(pre, vecs, post));
      return 0;
  }
}
