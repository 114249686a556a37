// gfx950 kernels of the restarted reflected-Halpern mode on the stream layout.  A translation unit of their own: next to
// k_spmv_a_dual / k_spmv_at_step in kernels_stream.hip they changed how the compiler laid out that unit's existing kernels, and
// those are to stay, instruction for instruction, what they were.  (The twins of the other three layouts are templates next to
// their skeletons in kernels_panel / _jag / _pb .hip, where they leave the existing instantiations as they are.)
// Launched from pdlp_device.hip through the prototypes of pdlp_kernel_decls.hpp.
#include <hip/hip_runtime.h>

#include "pdlp_kernel_decls.hpp"
#include "pdlp_layouts.hpp"
#include "spmv_stream.hpp"

// Halpern twins of k_spmv_a_dual / k_spmv_at_step (pdlp_epilogues.hpp): same skeleton, the epilogues carry the combination
__global__ void __launch_bounds__(kBlock)
k_spmv_a_halpern(int nb, const int32_t* __restrict__ rb, const int32_t* __restrict__ off,
                 const int32_t* __restrict__ idx, const double* __restrict__ val,
                 const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ xbar,
                 double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo,
                 const double* __restrict__ hi, HalpernArgs h, double* __restrict__ part, const double* __restrict__ dadd)
{
  if (!loop_active(ctl)) return;
  HalpernDualEpilogue e = HalpernDualEpilogue::make(ctl, y0, y1, lo, hi, h);
  csr_stream_block(nb, rb, off, idx, val, xbar, e, part, dadd);
}

__global__ void __launch_bounds__(kBlock)
k_spmv_at_halpern(int nb, const int32_t* __restrict__ rb, const int32_t* __restrict__ off,
                  const int32_t* __restrict__ idx, const double* __restrict__ val,
                  const pdlpdev_ctl* __restrict__ ctl, double* __restrict__ x0, double* __restrict__ x1,
                  double* __restrict__ aty0, double* __restrict__ aty1, HalpernArgs h,
                  double* __restrict__ part, const double* __restrict__ dadd)
{
  if (!loop_active(ctl)) return;
  HalpernStepEpilogue e = HalpernStepEpilogue::make(ctl, x0, x1, aty0, aty1, h);
  csr_stream_block(nb, rb, off, idx, val, h.ty /* y' */, e, part, dadd);
}
