// Prototypes of the SpMV kernels, which are DEFINED one layout per translation unit (kernels_<layout>.hip) and launched from the
// core through launch_product (pdlp_launch.hpp); the templated ones are instantiated explicitly where they are defined.  A templated
// kernel's parameter list is written ONCE here: the macros below turn it into the template's declaration and the explicit-instantiation
// declarations of its two variants.  The panel and the jagged kernel of a product take the same arguments behind their view; the
// gather-free row kernel takes them without the gathered vectors, which phase P (k_pb_products) consumed.
#pragma once
#include "pdlp_epilogues.hpp"

#define KERNEL_PAIR(TPARAM, BOUNDS, NAME, V0, V1, ...)                            \
  template <TPARAM>                                                               \
  __global__ void __launch_bounds__(BOUNDS) NAME(__VA_ARGS__);                    \
  extern template __global__ void NAME<V0>(__VA_ARGS__);                          \
  extern template __global__ void NAME<V1>(__VA_ARGS__);
// k_panel_<product><SEG> (SEG: the long-tail variant) and k_jag_<product><WAVES> (the two geometries)
#define ROW_KERNELS(PRODUCT, ...)                                                              \
  KERNEL_PAIR(bool SEG, kPanelThreads, k_panel_##PRODUCT, true, false, PanelView P, __VA_ARGS__) \
  KERNEL_PAIR(int WAVES, WAVES * 64, k_jag_##PRODUCT, 8, 16, JagView J, __VA_ARGS__)
// k_pb_<product><WIDE> (phase R: WIDE = the wide-bin skeleton, 1024 threads; otherwise the image-in-LDS skeleton, 512)
#define PB_KERNEL(PRODUCT, ...) KERNEL_PAIR(bool WIDE, WIDE ? kPbwThreads : kPbThreads, k_pb_##PRODUCT, false, true, PbView V, __VA_ARGS__)

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
ROW_KERNELS(a_dual, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ xbar, double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo, const double* __restrict__ hi, double* __restrict__ sumy, double* __restrict__ part, double* __restrict__ ycopy, const p2pdev::Push* __restrict__ push)
PB_KERNEL(a_dual, const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo, const double* __restrict__ hi, double* __restrict__ sumy, double* __restrict__ part, double* __restrict__ ycopy, const p2pdev::Push* __restrict__ push)
ROW_KERNELS(at_step, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ y0, const double* __restrict__ y1, const double* __restrict__ x0, const double* __restrict__ x1, double* __restrict__ aty0, double* __restrict__ aty1, double* __restrict__ part)
PB_KERNEL(at_step, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ x0, const double* __restrict__ x1, double* __restrict__ aty0, double* __restrict__ aty1, double* __restrict__ part)
ROW_KERNELS(at_cur, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ y0, const double* __restrict__ y1, double* __restrict__ aty0, double* __restrict__ aty1, double* __restrict__ out_override, int use_next)
PB_KERNEL(at_cur, const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ aty0, double* __restrict__ aty1, double* __restrict__ out_override, int use_next)
ROW_KERNELS(plain, const double* __restrict__ vec, double* __restrict__ out)
PB_KERNEL(plain, double* __restrict__ out)
ROW_KERNELS(eval_primal, const pdlpdev_ctl* __restrict__ ctl, int which, const double* __restrict__ x0, const double* __restrict__ x1, const double* __restrict__ avgx, const double* __restrict__ y0, const double* __restrict__ y1, const double* __restrict__ avgy, const double* __restrict__ dr, const double* __restrict__ lo_u, const double* __restrict__ hi_u, double eps_rel, double* __restrict__ linf_rows, double* __restrict__ ax_out, double* __restrict__ part)
PB_KERNEL(eval_primal, const pdlpdev_ctl* __restrict__ ctl, int which, const double* __restrict__ y0, const double* __restrict__ y1, const double* __restrict__ avgy, const double* __restrict__ dr, const double* __restrict__ lo_u, const double* __restrict__ hi_u, double eps_rel, double* __restrict__ linf_rows, double* __restrict__ ax_out, double* __restrict__ part)
ROW_KERNELS(eval_dual, const pdlpdev_ctl* __restrict__ ctl, int which, const double* __restrict__ x0, const double* __restrict__ x1, const double* __restrict__ avgx, const double* __restrict__ y0, const double* __restrict__ y1, const double* __restrict__ avgy, EvalDualCore core, double* __restrict__ part)
PB_KERNEL(eval_dual, const pdlpdev_ctl* __restrict__ ctl, int which, const double* __restrict__ x0, const double* __restrict__ x1, const double* __restrict__ avgx, EvalDualCore core, double* __restrict__ part)
__global__ void __launch_bounds__(kPanelThreads)
k_panel_eval_dual_from_aty(PanelView P, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ x0, const double* __restrict__ x1,
                           const double* __restrict__ aty0, const double* __restrict__ aty1, EvalDualCore core,
                           double* __restrict__ part, int guard);
KERNEL_PAIR(int THREADS, THREADS, k_pb_products, 512, 1024, PbView V, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ v0, const double* __restrict__ v1, int mode, int in_loop)
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
ROW_KERNELS(a_halpern, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ xbar, double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo, const double* __restrict__ hi, HalpernArgs h, double* __restrict__ part)
PB_KERNEL(a_halpern, const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo, const double* __restrict__ hi, HalpernArgs h, double* __restrict__ part)
ROW_KERNELS(at_halpern, const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ x0, double* __restrict__ x1, double* __restrict__ aty0, double* __restrict__ aty1, HalpernArgs h, double* __restrict__ part)
PB_KERNEL(at_halpern, const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ x0, double* __restrict__ x1, double* __restrict__ aty0, double* __restrict__ aty1, HalpernArgs h, double* __restrict__ part)
