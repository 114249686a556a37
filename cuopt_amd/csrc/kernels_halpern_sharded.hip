// gfx950 kernel of the sharded reflected-Halpern step on the stream layout (cuoptamd_settings::halpern_sharded).  A translation unit of
// its own, for the reason kernels_halpern.hip is one: next to k_spmv_a_halpern / k_spmv_at_halpern it changed how the compiler laid
// out that unit's existing kernels (k_spmv_at_halpern lost 256 instructions), and those are to stay, instruction for instruction, what
// they were.  Launched from pdlp_device.hip through the prototypes of pdlp_kernel_decls.hpp.
#include <hip/hip_runtime.h>

#include "pdlp_kernel_decls.hpp"
#include "pdlp_layouts.hpp"
#include "spmv_stream.hpp"

// the A product of a sharded Halpern step, owner-computes dataflow: y' also into this rank's slot of the gathered dual and, over the
// direct peer transport, into the other ranks' landing blocks (HalpernShardedDualEpilogue)
__global__ void __launch_bounds__(kBlock)
k_spmv_a_halpern_sharded(int nb, const int32_t* __restrict__ rb, const int32_t* __restrict__ off,
                         const int32_t* __restrict__ idx, const double* __restrict__ val,
                         const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ xbar,
                         double* __restrict__ y0, double* __restrict__ y1, const double* __restrict__ lo,
                         const double* __restrict__ hi, HalpernArgs h, double* __restrict__ part, double* __restrict__ ycopy,
                         const p2pdev::Push* __restrict__ push, const double* __restrict__ dadd)
{
  if (!loop_active(ctl)) return;
  HalpernShardedDualEpilogue e = HalpernShardedDualEpilogue::make(ctl, y0, y1, lo, hi, h, ycopy, push);
  csr_stream_block(nb, rb, off, idx, val, xbar, e, part, dadd);
  if (push) p2pdev::count_exchange(push);
}
