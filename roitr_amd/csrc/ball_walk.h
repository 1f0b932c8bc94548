// The float64 fixed-radius walk over the per-cloud grid of knn_grid.h, for the sources that decide in float64 on fp32 inputs
// (pairgt.hip, icp_common.h, outlier.hip; fpfh.hip takes the rounded operations alone): the three rounded operations and the cell range
// of a ball with the proof that it cannot miss a point.  The walk itself -- three ball_cells calls, the rows of the box, four candidates
// in flight -- stands in each of the three kernels: shared forms of it compiled to slower kernels (profiles/cloud_ops_refactor.txt).
// Include it AFTER `#pragma clang fp contract(off)`: the rule "every product and sum rounded on its own" is written with pg_mul /
// pg_add / pg_sub, which are plain operators that contraction would fuse again.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ double pg_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double pg_add(double a, double b) { return a + b; }
__device__ __forceinline__ double pg_sub(double a, double b) { return a - b; }

// Cells [lo, hi] of one axis that can hold a searched point q (fp32) with a within-radius distance to the query coordinate x.
//   * Accepted means d2 < r^2 with d2 >= fl((x - q)^2) (1 - 2^-52) (the two other squares are >= 0 and a sum rounds by 2^-53 twice),
//     and fl((x - q)^2) >= (x - q)^2 (1 - 2^-52) (one rounded difference, one rounded square): |x - q| < r (1 + 2^-51).
//   * wlo = fl(x - rb), whi = fl(x + rb) are off by at most 2^-53 (|x| + rb) each.  With rb = r (1 + 1e-9) + 1e-15 |x| (itself good to
//     three roundings of 2^-53) the slack 1e-9 r + 1e-15 |x| exceeds 2^-51 r + 2^-53 (|x| + rb) + 3 * 2^-53 rb by orders of
//     magnitude, so wlo <= x - |x - q| <= q <= whi for every accepted q.
//   * __double2float_rd / _ru round OUTWARDS, so flo <= q <= fhi in fp32.  The grid's cell of a coordinate,
//     min(max((int)floorf((v - o) * inv_h), 0), dim - 1), is a composition of non-decreasing fp32 functions of v (a rounded difference
//     with a constant, a rounded product with a positive constant, floor, clamp), and the expression below is the same one in the same
//     precision (the clamp is done in float first, so nothing far outside overflows an int): cell(flo) <= cell(q) <= cell(fhi).
// Hence no margin in cell units is needed and the range can never exclude a pair the float64 test accepts.
__device__ __forceinline__ int cell_of_axis(float v, float o, float inv_h, int dim)
{
    return (int)fminf(fmaxf(floorf((v - o) * inv_h), 0.f), (float)(dim - 1));
}
__device__ __forceinline__ void ball_cells(double x, double r, float o, float inv_h, int dim, int& lo, int& hi, float& fhi)
{
    const double rb = r * (1.0 + 1e-9) + 1e-15 * fabs(x);
    const float flo = __double2float_rd(x - rb);
    fhi = __double2float_ru(x + rb);
    lo = cell_of_axis(flo, o, inv_h, dim);
    hi = cell_of_axis(fhi, o, inv_h, dim);
}
