// Device pieces of the weighted solve `Solve` that include/roitr_engine.h states above roitr_lgr_batch, shared by the two estimators
// that are built on it (lgr.hip, compat.hip): float64 moments as strided per-lane sums over a local row index, the fixed butterflies
// that fold them over a lane group or a block of 256, and the centroids with the reference's eps.  Every sum has one order, so a
// result depends on the rows it is given and on nothing else.
#pragma once
#include "common.h"

namespace {

constexpr int LG_THREADS = 256;
constexpr int LG_ROWS = 512;     // rows per verification block: its LDS tile and its row chunk (2 x 8 KB)
constexpr int LG_GROUP = 16;     // lanes that share one hypothesis's moment sums
constexpr double LG_EPS = 1e-5;  // lib/utils.py:159 weighted_procrustes eps

// butterfly sum over W consecutive lanes (W <= 64, a power of two): every lane of the group gets the same bits
template <int W>
__device__ __forceinline__ double lanes_sum_d(double v)
{
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, W);
    return v;
}

// block sum of NV doubles per thread, every thread gets the totals: wave butterfly, then (w0 + w1) + (w2 + w3); red: 4 * NV doubles
template <int NV>
__device__ __forceinline__ void block_sum_d(double (&v)[NV], double* red)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = lanes_sum_d<64>(v[k]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) red[wave * NV + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = (red[k] + red[NV + k]) + (red[2 * NV + k] + red[3 * NV + k]);
}

__device__ __forceinline__ int block_sum_i(int v, int* red)   // red: 4 ints
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// The two moment passes of one weighted solve over rows j = lane, lane + stride, ... < n (row(j, p, q, w): source, target, weight):
// a = {sum w, sum w p, sum w q}, then H = sum w (p - cs)(q - ct)^T with cs, ct = sum w p / (sum w + eps).  `sum` reduces an array
// over the lanes that share the solve.
template <class Row>
__device__ __forceinline__ void moments_first(int n, int lane, int stride, Row row, double (&a)[7])
{
#pragma unroll
    for (int k = 0; k < 7; ++k) a[k] = 0.0;
    for (int j = lane; j < n; j += stride) {
        float p[3], q[3], w;
        row(j, p, q, w);
        a[0] += w;
        a[1] += (double)w * p[0]; a[2] += (double)w * p[1]; a[3] += (double)w * p[2];
        a[4] += (double)w * q[0]; a[5] += (double)w * q[1]; a[6] += (double)w * q[2];
    }
}
template <class Row>
__device__ __forceinline__ void moments_second(int n, int lane, int stride, Row row, const double (&cs)[3], const double (&ct)[3],
                                               double (&H)[9])
{
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = 0.0;
    for (int j = lane; j < n; j += stride) {
        float p[3], q[3], w;
        row(j, p, q, w);
        if (w == 0.f) continue;
        const double ps[3] = {p[0] - cs[0], p[1] - cs[1], p[2] - cs[2]}, qs[3] = {q[0] - ct[0], q[1] - ct[1], q[2] - ct[2]};
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) H[3 * x + y] += (double)w * ps[x] * qs[y];
    }
}
__device__ __forceinline__ void centroids(const double (&a)[7], double (&cs)[3], double (&ct)[3])
{
    const double den = a[0] + LG_EPS;
#pragma unroll
    for (int k = 0; k < 3; ++k) { cs[k] = a[1 + k] / den; ct[k] = a[4 + k] / den; }
}

}  // namespace
