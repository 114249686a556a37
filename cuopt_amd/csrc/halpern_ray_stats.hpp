// The statistics of the Halpern ray pass for ONE LP by one workgroup of kBlock threads of a grid over its rows / columns: the bodies of
// k_halpern_ray_rows / k_halpern_ray_cols (pdlp_eval.hip) and of k_halpern_ray_rows_batch / k_halpern_ray_cols_batch
// (kernels_batch_halpern_ray.hip, grid y <-> LP), so that the two cannot drift apart -- the same expressions, the same grid-stride
// order, the same trees (halpern_decision.hpp does this for the decisions).  blockIdx.x / gridDim.x are the LP's own grid in both.
#pragma once
#include "pdlp_kernels.hpp"

// k_infeas_rows' statistics with the unscaled ray: (A dx_u)_i = (A^ dx^)_i / D_r,i and dy_u,i = dy^_i D_r,i
__device__ __forceinline__ void halpern_ray_rows_block(int m, int nbg, const double* __restrict__ a_dx, const double* __restrict__ dy, const double* __restrict__ dr,
                                                       const double* __restrict__ lo_u, const double* __restrict__ hi_u, double* __restrict__ part)
{
  using namespace pdlp;
  __shared__ double red[12];
  double mx[2] = {0.0, 0.0}, sm[1] = {0.0};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < m; i += gridDim.x * kBlock) {
    const double d  = dr[i];
    const double lo = lo_u[i], hi = hi_u[i];
    const double hl = dfinite(lo) ? 0.0 : lo, hu = dfinite(hi) ? 0.0 : hi;  // zero_if_is_finite
    const double r  = fabs(violation(a_dx[i] / d, hl, hu));
    const double yi = dy[i] * d;
    mx[0] = r > mx[0] ? r : mx[0];
    mx[1] = fabs(yi) > mx[1] ? fabs(yi) : mx[1];
    sm[0] += bound_value_product(yi, lo, hi);
  }
  block_reduce<MaxOp, 2>(mx, red);
  __syncthreads();
  block_reduce<SumOp, 1>(sm, red + 8);
  if (threadIdx.x == 0) {
    part[blockIdx.x]           = mx[0];
    part[nbg + blockIdx.x]     = mx[1];
    part[2 * nbg + blockIdx.x] = sm[0];
  }
}

// k_infeas_cols' statistics likewise: (A^T dy_u)_j = (A^T^ dy^)_j / D_c,j and dx_u,j = dx^_j D_c,j; both reduced-cost rules look at the
// ray's own x.  mark (two doubles): the accepted-step count the pass belongs to and its rule, for the host to recognise the figures by.
__device__ __forceinline__ void halpern_ray_cols_block(int n, int nbg, const pdlpdev_ctl* __restrict__ ctl, const double* __restrict__ at_dy,
                                                       const double* __restrict__ dx, const double* __restrict__ dc, const double* __restrict__ c_u,
                                                       const double* __restrict__ lb_u, const double* __restrict__ ub_u, int rule_finite,
                                                       double* __restrict__ part, double* __restrict__ mark)
{
  using namespace pdlp;
  __shared__ double red[28];
  if (blockIdx.x == 0 && threadIdx.x == 0) mark[0] = (double)ctl->steps_taken, mark[1] = (double)rule_finite;
  double mx[4] = {0.0, 0.0, 0.0, 0.0}, sm[2] = {0.0, 0.0};
  for (int j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
    const double d  = dc[j];
    const double g  = -1.0 * (at_dy[j] / d);
    const double xj = dx[j] * d;
    const double lb = lb_u[j], ub = ub_u[j];
    const double bv = g > 0.0 ? lb : ub;
    double rc;
    if (g == 0.0)
      rc = g;
    else if (rule_finite)
      rc = dfinite(bv) ? g : 0.0;
    else
      rc = fabs(xj - bv) <= fabs(xj) ? g : 0.0;
    const double rd = fabs(g - rc);
    double viol     = 0.0;  // max_violation, utils.cuh:181-193
    if (dfinite(lb)) viol = dmax(viol, -xj);
    if (dfinite(ub)) viol = dmax(viol, xj);
    mx[0] = rd > mx[0] ? rd : mx[0];
    mx[1] = fabs(rc) > mx[1] ? fabs(rc) : mx[1];
    mx[2] = fabs(xj) > mx[2] ? fabs(xj) : mx[2];
    mx[3] = viol > mx[3] ? viol : mx[3];
    sm[0] += bound_value_product(rc, lb, ub);
    sm[1] += c_u[j] * xj;
  }
  block_reduce<MaxOp, 4>(mx, red);
  __syncthreads();
  block_reduce<SumOp, 2>(sm, red + 16);
  if (threadIdx.x == 0) {
    for (int q = 0; q < 4; ++q) part[(size_t)q * nbg + blockIdx.x] = mx[q];
    part[(size_t)4 * nbg + blockIdx.x] = sm[0];
    part[(size_t)5 * nbg + blockIdx.x] = sm[1];
  }
}
