// The ray pass of a shared-matrix lockstep batch in reflected Halpern mode (docs/design/04d_halpern_mode.md, "The K-wide ray pass"):
// what enqueue_halpern_ray (pdlp_eval.hip) does for one LP -- the scaled displacement T(z^k) - z^k, the two plain products formed
// from it, the nine raw statistics, the mark -- for every LP of a pass at once.  A translation unit of its own: the kernels of
// kernels_batch.hip and kernels_batch_halpern.hip are to stay, instruction for instruction, what they were.
//   * kb_ray_diff<K>: k_halpern_ray_diff's expression per LP, to the LP's own tmp_n / tmp_m and interleaved into xK / yK (free
//     between runs: kb_primal and kb_a_halpern rewrite them before anything gathers them);
//   * kb_plain<K>: the K-wide PLAIN product -- batch_block_sums, batch_cross_over (batch_common.hpp), then the row sums as they are
//     to each LP's output vector.  A row is added left to right in CSR order from 0.0, as the layouts' own plain products add it
//     (panel_block with StoreEpilogue, k_spmv_plain): bit-equal to pdlpdev_spmv.  No partial sums, no epilogue operands;
//   * the statistics: halpern_ray_stats.hpp's bodies (those of k_halpern_ray_rows / k_halpern_ray_cols) on each LP's own vectors
//     and part_g, grid y <-> LP, grid x the single pass's own blocks; the finalize is finalize_rows (k_finalize's body) twice per
//     LP, workgroup <-> LP: the same trees, the same bits.
// Which LPs a pass serves (on_mask) and their reduced-cost rules (rule_mask) are launch arguments: wave-uniform scalars.
#include <hip/hip_runtime.h>

#include "batch_common.hpp"
#include "halpern_ray_stats.hpp"
#include "pdlp_ctx.hpp"

#define LAUNCH_CHECK() HIP_TRY(hipGetLastError())

namespace {

// dx = T(x) - x^k, dy = T(y) - y^k of every LP in the pass: one thread per index, the K LPs one after the other (each LP's loads and
// its own store coalesce across the wave; the interleaved store is K consecutive doubles per lane).  An LP outside the pass: zeros
// in its interleaved lane (gathered and multiplied, never stored), its own vectors untouched.
template <int K>
__global__ void __launch_bounds__(kBlock) kb_ray_diff(int n, int m, const BatchRayLp* __restrict__ lp, unsigned on_mask, double* __restrict__ xK,
                                                      double* __restrict__ yK)
{
  const int tot = n > m ? n : m;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < tot; i += gridDim.x * kBlock) {
    double vx[K], vy[K];
#pragma unroll
    for (int l = 0; l < K; ++l) {
      vx[l] = 0.0, vy[l] = 0.0;
      if (!((on_mask >> l) & 1u)) continue;
      const BatchRayLp L = lp[l];
      const int cur      = L.ctl->cur;
      const double* __restrict__ xk = cur ? L.x0 : L.x1;
      const double* __restrict__ yk = cur ? L.y0 : L.y1;
      if (i < n) vx[l] = L.avgx[i] - xk[i], L.tmp_n[i] = vx[l];
      if (i < m) vy[l] = L.avgy[i] - yk[i], L.tmp_m[i] = vy[l];
    }
    if (i < n) {
#pragma unroll
      for (int l = 0; l < K; l += 2) *(double2*)&xK[(size_t)i * K + l] = double2{vx[l], vx[l + 1]};
    }
    if (i < m) {
#pragma unroll
      for (int l = 0; l < K; l += 2) *(double2*)&yK[(size_t)i * K + l] = double2{vy[l], vy[l + 1]};
    }
  }
}

// the parity hook's interleave: vK[i][l] = the LP's input vector (tmp_m / tmp_n, where pdlpdev_spmv puts it), 0 outside the pass
template <int K>
__global__ void __launch_bounds__(kBlock) kb_interleave(int len, int transpose, const BatchRayLp* __restrict__ lp, unsigned on_mask, double* __restrict__ vK)
{
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < len; i += gridDim.x * kBlock) {
    double v[K];
#pragma unroll
    for (int l = 0; l < K; ++l) {
      v[l] = 0.0;
      if ((on_mask >> l) & 1u) v[l] = (transpose ? lp[l].tmp_m : lp[l].tmp_n)[i];
    }
#pragma unroll
    for (int l = 0; l < K; l += 2) *(double2*)&vK[(size_t)i * K + l] = double2{v[l], v[l + 1]};
  }
}

// rows of one side for K LPs, no epilogue: out_l[row] = the row sum of LP l, for the LPs of on_mask (transpose: the LP's aty, else
// its ax).  Wave <-> LP, lane <-> row as in the Halpern epilogues.
// LDS: the store phase only READS S.u.sums, between batch_cross_over's second barrier and the barrier that ends the block's trip
// (below); the next block's batch_block_sums writes scol / sval -- the union's other view -- behind it (docs/design/10_lds_hazard_audit.md)
template <int K>
__global__ void __launch_bounds__(kBT) kb_plain(const int32_t* __restrict__ row0, const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
                                                const double* __restrict__ val, const BatchRayLp* __restrict__ lp, int transpose, unsigned on_mask,
                                                const double* __restrict__ vK)
{
  __shared__ BatchShared<K> S;
  using WL = WaveLps<K>;
  const int w = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, sub = WL::sub(wave);
  const int r0 = row0[w], nr = row0[w + 1] - r0;
  for (int b0 = 0; b0 < nr; b0 += kBT) {
    double s[BatchGeometry<K>::RU][2];
    batch_block_sums<K>(S, r0, nr, b0, off, idx, val, vK, s);
    batch_cross_over<K>(S, s);
#pragma unroll
    for (int pass = 0; pass < WL::PASSES; ++pass) {
      const int l = WL::lp(wave, pass);
      if (!((on_mask >> l) & 1u)) continue;
      double* __restrict__ out = transpose ? lp[l].aty : lp[l].ax;
#pragma unroll
      for (int j = sub; j < 8; j += WL::NSUB) {
        const int r = b0 + lane + 64 * j;
        if (r < nr) out[r0 + r] = S.u.sums[lane + 64 * j][l];
      }
    }
    __syncthreads();  // (the end of the trip: every read of S.u.sums is done before the next block stages its entries over them)
  }
}

// the statistics of the LPs of the pass: grid y <-> LP, grid x the single pass's own blocks, the single kernels' bodies
__global__ void __launch_bounds__(kBlock) k_halpern_ray_rows_batch(int m, int nbg, const BatchRayLp* __restrict__ lp, unsigned on_mask, const double* __restrict__ dr)
{
  const int l = blockIdx.y;
  if (!((on_mask >> l) & 1u)) return;
  const BatchRayLp L = lp[l];
  halpern_ray_rows_block(m, nbg, L.ax, L.tmp_m, dr, L.lo_u, L.hi_u, L.part_g);
}
__global__ void __launch_bounds__(kBlock) k_halpern_ray_cols_batch(int n, int nbg, const BatchRayLp* __restrict__ lp, unsigned on_mask, unsigned rule_mask,
                                                                   const double* __restrict__ dc, const double* __restrict__ c_u)
{
  const int l = blockIdx.y;
  if (!((on_mask >> l) & 1u)) return;
  const BatchRayLp L = lp[l];
  halpern_ray_cols_block(n, nbg, L.ctl, L.aty, L.tmp_n, dc, c_u, L.lb_u, L.ub_u, (int)((rule_mask >> l) & 1u), L.part_g + 3 * 2048, L.scal + kRayMark);
}
// workgroup <-> LP: k_finalize(part_rows, gr, 3, 0x3) and k_finalize(part_cols, gc, 6, 0xF) of enqueue_halpern_ray, one after the other
__global__ void __launch_bounds__(kBlock) k_halpern_ray_finalize_batch(const BatchRayLp* __restrict__ lp, unsigned on_mask, int gr, int gc)
{
  __shared__ double red[8];
  const int l = blockIdx.x;
  if (!((on_mask >> l) & 1u)) return;
  const BatchRayLp L = lp[l];
  finalize_rows(L.part_g, gr, 3, 0x3u, L.scal + kRayRows, red);
  finalize_rows(L.part_g + 3 * 2048, gc, 6, 0xFu, L.scal + kRayCols, red);
}

template <int K>
void launch_plain_k(hipStream_t s, const BatchProductSide& side, const BatchRayLp* lp, int transpose, unsigned on_mask, const double* vK)
{
  kb_plain<K><<<side.W, kBT, 0, s>>>(side.row0, side.off, side.idx, side.val, lp, transpose, on_mask, vK);
}

template <int K>
int enqueue_rays(hipStream_t s, const BatchProductSide& A, const BatchProductSide& T, const BatchRayLp* lp, const BatchRayShared& sh, unsigned on_mask,
                 unsigned rule_mask, double* xK, double* yK)
{
  const int n = sh.n, m = sh.m;
  kb_ray_diff<K><<<grid_for(std::max(n, m)), kBlock, 0, s>>>(n, m, lp, on_mask, xK, yK);
  launch_plain_k<K>(s, A, lp, 0, on_mask, xK);
  launch_plain_k<K>(s, T, lp, 1, on_mask, yK);
  const int gr = std::min(grid_for(m), kGenericBlocks), gc = std::min(grid_for(n), kGenericBlocks);  // (enqueue_halpern_ray's grids)
  k_halpern_ray_rows_batch<<<dim3(gr, K), kBlock, 0, s>>>(m, gr, lp, on_mask, sh.dr);
  k_halpern_ray_cols_batch<<<dim3(gc, K), kBlock, 0, s>>>(n, gc, lp, on_mask, rule_mask, sh.dc, sh.c_u);
  k_halpern_ray_finalize_batch<<<K, kBlock, 0, s>>>(lp, on_mask, gr, gc);
  LAUNCH_CHECK();
  return 0;
}

template <int K>
int enqueue_plain(hipStream_t s, const BatchProductSide& side, int transpose, int len, const BatchRayLp* lp, unsigned on_mask, double* vK)
{
  kb_interleave<K><<<grid_for(len), kBlock, 0, s>>>(len, transpose, lp, on_mask, vK);
  launch_plain_k<K>(s, side, lp, transpose, on_mask, vK);
  LAUNCH_CHECK();
  return 0;
}

}  // namespace

int batch_halpern_enqueue_rays(int K, hipStream_t s, const BatchProductSide& A, const BatchProductSide& T, const void* ray_table, const BatchRayShared& sh,
                               unsigned on_mask, unsigned rule_mask, double* xK, double* yK)
{
  const BatchRayLp* lp = static_cast<const BatchRayLp*>(ray_table);
  return K == 16  ? enqueue_rays<16>(s, A, T, lp, sh, on_mask, rule_mask, xK, yK)
         : K == 8 ? enqueue_rays<8>(s, A, T, lp, sh, on_mask, rule_mask, xK, yK)
         : K == 4 ? enqueue_rays<4>(s, A, T, lp, sh, on_mask, rule_mask, xK, yK)
                  : enqueue_rays<2>(s, A, T, lp, sh, on_mask, rule_mask, xK, yK);
}

int batch_enqueue_plain(int K, hipStream_t s, const BatchProductSide& side, int transpose, int len, const void* ray_table, unsigned on_mask, double* vK)
{
  const BatchRayLp* lp = static_cast<const BatchRayLp*>(ray_table);
  return K == 16  ? enqueue_plain<16>(s, side, transpose, len, lp, on_mask, vK)
         : K == 8 ? enqueue_plain<8>(s, side, transpose, len, lp, on_mask, vK)
         : K == 4 ? enqueue_plain<4>(s, side, transpose, len, lp, on_mask, vK)
                  : enqueue_plain<2>(s, side, transpose, len, lp, on_mask, vK);
}
