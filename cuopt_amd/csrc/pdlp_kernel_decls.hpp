// Prototypes of the SpMV kernels, which are DEFINED one layout per translation unit (kernels_<layout>.hip) and launched from the
// core through launch_product (pdlp_launch.hpp); the templated ones are instantiated explicitly where they are defined.  A product's
// panel, jagged and gather-free kernels have their parameter lists in ONE place, the product's <PRODUCT>_KERNELS list below: this
// header turns it into the templates' declarations and the explicit-instantiation declarations of their two variants
// (DECLARE_KERNELS), the layout's unit into the explicit instantiations (INSTANTIATE_PANEL / _JAG / _PB, one line per product).  Only
// the kernel's definition repeats the list, with the names its body uses: a list that does not match leaves the instantiation without
// its template, which does not compile.  The panel and the jagged kernel of a product take the same arguments behind their view; the
// gather-free row kernel takes them without the gathered vectors, which phase P (k_pb_products) consumed.
#pragma once
#include "pdlp_epilogues.hpp"

// what a list is expanded with: the template's declaration + both variants declared extern, or both variants instantiated
#define KERNEL_PAIR_DECLARE(TPARAM, BOUNDS, NAME, V0, V1, ...)                    \
  template <TPARAM>                                                               \
  __global__ void __launch_bounds__(BOUNDS) NAME(__VA_ARGS__);                    \
  extern template __global__ void NAME<V0>(__VA_ARGS__);                          \
  extern template __global__ void NAME<V1>(__VA_ARGS__);
#define KERNEL_PAIR_INSTANTIATE(TPARAM, BOUNDS, NAME, V0, V1, ...)                \
  template __global__ void NAME<V0>(__VA_ARGS__);                                 \
  template __global__ void NAME<V1>(__VA_ARGS__);
// k_panel_<product><SEG> (SEG: the long-tail variant), k_jag_<product><WAVES> (the two geometries) and k_pb_<product><WIDE> (phase R:
// WIDE = the wide-bin skeleton, 1024 threads; otherwise the image-in-LDS skeleton, 512)
#define PANEL_KERNEL(EMIT, PRODUCT, ...) EMIT(bool SEG, kPanelThreads, k_panel_##PRODUCT, true, false, PanelView P, __VA_ARGS__)
#define JAG_KERNEL(EMIT, PRODUCT, ...) EMIT(int WAVES, WAVES * 64, k_jag_##PRODUCT, 8, 16, JagView J, __VA_ARGS__)
#define PB_KERNEL(EMIT, PRODUCT, ...) EMIT(bool WIDE, WIDE ? kPbwThreads : kPbThreads, k_pb_##PRODUCT, false, true, PbView V, __VA_ARGS__)
// A list is <PRODUCT>_KERNELS(ROW, PB) = ROW(product, the panel / jagged kernels' parameters) PB(product, the gather-free row kernel's)
#define NO_KERNELS(...)
#define DECLARE_ROW_KERNELS(PRODUCT, ...) PANEL_KERNEL(KERNEL_PAIR_DECLARE, PRODUCT, __VA_ARGS__) JAG_KERNEL(KERNEL_PAIR_DECLARE, PRODUCT, __VA_ARGS__)
#define DECLARE_PB_KERNEL(PRODUCT, ...) PB_KERNEL(KERNEL_PAIR_DECLARE, PRODUCT, __VA_ARGS__)
#define INSTANTIATE_PANEL_KERNEL(PRODUCT, ...) PANEL_KERNEL(KERNEL_PAIR_INSTANTIATE, PRODUCT, __VA_ARGS__)
#define INSTANTIATE_JAG_KERNEL(PRODUCT, ...) JAG_KERNEL(KERNEL_PAIR_INSTANTIATE, PRODUCT, __VA_ARGS__)
#define INSTANTIATE_PB_KERNEL(PRODUCT, ...) PB_KERNEL(KERNEL_PAIR_INSTANTIATE, PRODUCT, __VA_ARGS__)
#define DECLARE_KERNELS(LIST) LIST(DECLARE_ROW_KERNELS, DECLARE_PB_KERNEL)
#define INSTANTIATE_PANEL(LIST) LIST(INSTANTIATE_PANEL_KERNEL, NO_KERNELS)
#define INSTANTIATE_JAG(LIST) LIST(INSTANTIATE_JAG_KERNEL, NO_KERNELS)
#define INSTANTIATE_PB(LIST) LIST(NO_KERNELS, INSTANTIATE_PB_KERNEL)

__global__ void __launch_bounds__(kBlock)
k_spmv_a_dual(int nb, const int32_t* __restrict__ rb, const int32_t* __restrict__ off,
              const int32_t* __restrict__ idx, const double* __restrict__ val,
              const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ xbar,
              double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo,
              const double* __restrict__ hi, double* __restrict__ sumy, double* __restrict__ part, double* __restrict__ ycopy,
              const p2pdev::Push* __restrict__ push, const double* __restrict__ dadd);
__global__ void __launch_bounds__(kBlock)
k_spmv_at_step(int nb, const int32_t* __restrict__ rb, const int32_t* __restrict__ off,
               const int32_t* __restrict__ idx, const double* __restrict__ val,
               const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ y0,
               const double* __restrict__ y1, const double* __restrict__ x0,
               const double* __restrict__ x1, double* __restrict__ aty0, double* __restrict__ aty1,
               double* __restrict__ part, const double* __restrict__ dadd);
__global__ void __launch_bounds__(kBlock)
k_spmv_plain(int nb, const int32_t* __restrict__ rb, const int32_t* __restrict__ off,
             const int32_t* __restrict__ idx, const double* __restrict__ val,
             const double* __restrict__ vec, double* __restrict__ out, const double* __restrict__ dadd);
__global__ void __launch_bounds__(kBlock)
k_spmv_at_cur(int nb, const int32_t* __restrict__ rb, const int32_t* __restrict__ off,
              const int32_t* __restrict__ idx, const double* __restrict__ val,
              const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ y0,
              const double* __restrict__ y1, double* __restrict__ aty0, double* __restrict__ aty1,
              double* __restrict__ out_override, int use_next, const double* __restrict__ dadd);
__global__ void __launch_bounds__(kBlock)
k_eval_primal(int nb, const int32_t* __restrict__ rb, const int32_t* __restrict__ off,
              const int32_t* __restrict__ idx, const double* __restrict__ val,
              const pdlpdev_ctl* __restrict__ ctl, int which, const double* __restrict__ x0,
              const double* __restrict__ x1, const double* __restrict__ avgx,
              const double* __restrict__ y0, const double* __restrict__ y1,
              const double* __restrict__ avgy, const double* __restrict__ dr,
              const double* __restrict__ lo_u, const double* __restrict__ hi_u, double eps_rel,
              double* __restrict__ linf_rows, double* __restrict__ ax_out, double* __restrict__ part, const double* __restrict__ dadd);
__global__ void __launch_bounds__(kBlock)
k_eval_dual(int nb, const int32_t* __restrict__ rb, const int32_t* __restrict__ off,
            const int32_t* __restrict__ idx, const double* __restrict__ val,
            const pdlpdev_ctl* __restrict__ ctl, int which, const double* __restrict__ x0,
            const double* __restrict__ x1, const double* __restrict__ avgx,
            const double* __restrict__ y0, const double* __restrict__ y1,
            const double* __restrict__ avgy, EvalDualCore core, double* __restrict__ part, const double* __restrict__ dadd);
#define A_DUAL_KERNELS(ROW, PB) \
  ROW(a_dual, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ xbar, double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo, const double* __restrict__ hi, double* __restrict__ sumy, double* __restrict__ part, double* __restrict__ ycopy, const p2pdev::Push* __restrict__ push) \
  PB(a_dual, const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo, const double* __restrict__ hi, double* __restrict__ sumy, double* __restrict__ part, double* __restrict__ ycopy, const p2pdev::Push* __restrict__ push)
DECLARE_KERNELS(A_DUAL_KERNELS)
#define AT_STEP_KERNELS(ROW, PB) \
  ROW(at_step, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ y0, const double* __restrict__ y1, const double* __restrict__ x0, const double* __restrict__ x1, double* __restrict__ aty0, double* __restrict__ aty1, double* __restrict__ part) \
  PB(at_step, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ x0, const double* __restrict__ x1, double* __restrict__ aty0, double* __restrict__ aty1, double* __restrict__ part)
DECLARE_KERNELS(AT_STEP_KERNELS)
#define AT_CUR_KERNELS(ROW, PB) \
  ROW(at_cur, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ y0, const double* __restrict__ y1, double* __restrict__ aty0, double* __restrict__ aty1, double* __restrict__ out_override, int use_next) \
  PB(at_cur, const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ aty0, double* __restrict__ aty1, double* __restrict__ out_override, int use_next)
DECLARE_KERNELS(AT_CUR_KERNELS)
#define PLAIN_KERNELS(ROW, PB) \
  ROW(plain, const double* __restrict__ vec, double* __restrict__ out) \
  PB(plain, double* __restrict__ out)
DECLARE_KERNELS(PLAIN_KERNELS)
#define EVAL_PRIMAL_KERNELS(ROW, PB) \
  ROW(eval_primal, const pdlpdev_ctl* __restrict__ ctl, int which, const double* __restrict__ x0, const double* __restrict__ x1, const double* __restrict__ avgx, const double* __restrict__ y0, const double* __restrict__ y1, const double* __restrict__ avgy, const double* __restrict__ dr, const double* __restrict__ lo_u, const double* __restrict__ hi_u, double eps_rel, double* __restrict__ linf_rows, double* __restrict__ ax_out, double* __restrict__ part) \
  PB(eval_primal, const pdlpdev_ctl* __restrict__ ctl, int which, const double* __restrict__ y0, const double* __restrict__ y1, const double* __restrict__ avgy, const double* __restrict__ dr, const double* __restrict__ lo_u, const double* __restrict__ hi_u, double eps_rel, double* __restrict__ linf_rows, double* __restrict__ ax_out, double* __restrict__ part)
DECLARE_KERNELS(EVAL_PRIMAL_KERNELS)
#define EVAL_DUAL_KERNELS(ROW, PB) \
  ROW(eval_dual, const pdlpdev_ctl* __restrict__ ctl, int which, const double* __restrict__ x0, const double* __restrict__ x1, const double* __restrict__ avgx, const double* __restrict__ y0, const double* __restrict__ y1, const double* __restrict__ avgy, EvalDualCore core, double* __restrict__ part) \
  PB(eval_dual, const pdlpdev_ctl* __restrict__ ctl, int which, const double* __restrict__ x0, const double* __restrict__ x1, const double* __restrict__ avgx, EvalDualCore core, double* __restrict__ part)
DECLARE_KERNELS(EVAL_DUAL_KERNELS)
__global__ void __launch_bounds__(kPanelThreads)
k_panel_eval_dual_from_aty(PanelView P, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ x0, const double* __restrict__ x1,
                           const double* __restrict__ aty0, const double* __restrict__ aty1, EvalDualCore core,
                           double* __restrict__ part, int guard);
// phase P of every gather-free product; mode: which vector it gathers (GatherMode, pdlp_epilogues.hpp)
#define PB_PRODUCTS_KERNEL(EMIT) EMIT(int THREADS, THREADS, k_pb_products, 512, 1024, PbView V, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ v0, const double* __restrict__ v1, int mode, int in_loop)
PB_PRODUCTS_KERNEL(KERNEL_PAIR_DECLARE)
__global__ void __launch_bounds__(kBlock)
k_dense_rows(DenseView D, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ v0, const double* __restrict__ v1, int mode, int in_loop);
__global__ void __launch_bounds__(kBlock)
k_dense_rows_finish(DenseView D, int nrows, const pdlpdev_ctl* __restrict__ ctl, int in_loop, double* __restrict__ add);
__global__ void __launch_bounds__(kBlock)
k_dense_cols(DenseView D, int n, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ v0, const double* __restrict__ v1, int mode,
             int in_loop, double* __restrict__ add);

// ---- restarted reflected-Halpern mode: the twins of k_*_a_dual / k_*_at_step with the Halpern epilogues (pdlp_epilogues.hpp) ----
__global__ void __launch_bounds__(kBlock)
k_spmv_a_halpern(int nb, const int32_t* __restrict__ rb, const int32_t* __restrict__ off,
                 const int32_t* __restrict__ idx, const double* __restrict__ val,
                 const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ xbar,
                 double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo,
                 const double* __restrict__ hi, HalpernArgs h, double* __restrict__ part, const double* __restrict__ dadd);
__global__ void __launch_bounds__(kBlock)
k_spmv_at_halpern(int nb, const int32_t* __restrict__ rb, const int32_t* __restrict__ off,
                  const int32_t* __restrict__ idx, const double* __restrict__ val,
                  const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ x0, double* __restrict__ x1,
                  double* __restrict__ aty0, double* __restrict__ aty1, HalpernArgs h,
                  double* __restrict__ part, const double* __restrict__ dadd);
#define A_HALPERN_KERNELS(ROW, PB) \
  ROW(a_halpern, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ xbar, double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo, const double* __restrict__ hi, HalpernArgs h, double* __restrict__ part) \
  PB(a_halpern, const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo, const double* __restrict__ hi, HalpernArgs h, double* __restrict__ part)
DECLARE_KERNELS(A_HALPERN_KERNELS)
#define AT_HALPERN_KERNELS(ROW, PB) \
  ROW(at_halpern, const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ x0, double* __restrict__ x1, double* __restrict__ aty0, double* __restrict__ aty1, HalpernArgs h, double* __restrict__ part) \
  PB(at_halpern, const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ x0, double* __restrict__ x1, double* __restrict__ aty0, double* __restrict__ aty1, HalpernArgs h, double* __restrict__ part)
DECLARE_KERNELS(AT_HALPERN_KERNELS)
// ... and the A product of a sharded Halpern step (HalpernShardedDualEpilogue: y' also into the gathered dual / the peers' blocks)
__global__ void __launch_bounds__(kBlock)
k_spmv_a_halpern_sharded(int nb, const int32_t* __restrict__ rb, const int32_t* __restrict__ off,
                         const int32_t* __restrict__ idx, const double* __restrict__ val,
                         const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ xbar,
                         double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo,
                         const double* __restrict__ hi, HalpernArgs h, double* __restrict__ part, double* __restrict__ ycopy,
                         const p2pdev::Push* __restrict__ push, const double* __restrict__ dadd);
#define A_HALPERN_SHARDED_KERNELS(ROW, PB) \
  ROW(a_halpern_sharded, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ xbar, double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo, const double* __restrict__ hi, HalpernArgs h, double* __restrict__ part, double* __restrict__ ycopy, const p2pdev::Push* __restrict__ push) \
  PB(a_halpern_sharded, const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo, const double* __restrict__ hi, HalpernArgs h, double* __restrict__ part, double* __restrict__ ycopy, const p2pdev::Push* __restrict__ push)
DECLARE_KERNELS(A_HALPERN_SHARDED_KERNELS)
