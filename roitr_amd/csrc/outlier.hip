// Outlier removal: Open3D's remove_statistical_outlier and remove_radius_outlier restated.
// The operators are defined in include/roitr_pointops.h above roitr_remove_statistical_outlier; this file follows that text.
//
// Both: the prepare pass of cloud_status.h (the cloud of every point, the status bit, a copy with non-finite coordinates zeroed for the
// grid), the decision into a flag per point, then the flags to `index` and `new_offset` (flag_compact.h, which voxel.hip's cap shares:
// tile sums, one-block scan, compaction with the inclusive counts kept; then one thread per cloud for the offsets).
// Statistical: the grid and the exact kNN(nb_neighbors) of pointops_knn.hip, its idx rows (n, k) in the workspace, then
//   outlier_mean_kernel    one LANE per point: the definition is k dependent float64 sqrt + add steps per point, so a wave per point
//                          (fpfh.hip's shape) idles 44 lanes at k = 20 (measured on the same rows: 0.66 against 0.17 ms for 64 x 30 000
//                          points at k = 20, 1.34 against 0.93 ms at k = 100).  A wave's 64 rows (64 k ints, contiguous) are
//                          staged through LDS in one coalesced read, at an odd row stride so that the lanes' reads of one column spread
//                          over the banks.
//   outlier_stats_kernel   one workgroup per cloud: thread t sums the cloud's 256-point segments t, t + 256, ... one term after the other,
//                          thread 0 adds the segment sums in segment order; S1, then S2 on cloud_mean, then the keep flags.
// Radius: the grid alone (cell size chosen for the radius), one lane per query walking the cells under the ball (ball_cells of
// ball_walk.h: the walk cannot miss an accepted point) with the float64 test on every candidate; without `count` a lane stops at
// nb_points + 1.
#include "cloud_status.h"
#include "common.h"
#include "flag_compact.h"
#include "knn_grid.h"
#include "roitr_pointops.h"
#include "workspace.h"
#include <cmath>

#define OL_THREADS 256
#define OL_SEG 256          // points per segment of a per-cloud sum: part of the definition
#define OL_MAX_NN 100
#define OL_MAX_CLOUDS 65535

#pragma clang fp contract(off)
#include "ball_walk.h"   // pg_mul / pg_add / pg_sub, ball_cells

namespace {

struct OlWs {
    void* knn;              // grid (+ kNN) workspace of the clouds against themselves
    float* clean;           // (n, 3) points with non-finite coordinates zeroed: what the grid is built on
    int* cloud;             // (n) the cloud of every point (-1: a row behind the last offset)
    int* idx;               // (n, k) kNN rows (statistical)
    double* mean;           // (n) mean_i (statistical)
    double* seg;            // (n / 256 + b + 1) segment sums; cloud c owns the slots from start(c) / 256 + c
    int* incl;              // (n) inclusive count of kept rows
    int* tilesum;           // (flag_tiles(n) + 1) tile sums -> exclusive bases, the total behind them
    size_t bytes;
};

OlWs carve(void* ws, int b, int n, int k)
{
    Carve c(Carve::aligned(ws));
    OlWs w;
    w.knn = c.take<char>(roitr_knn_workspace_bytes(b, n, k > 0 ? n : 0));
    w.clean = c.take<float>((size_t)n * 3);
    w.cloud = c.take<int>(n);
    w.idx = c.take<int>((size_t)n * k);
    w.mean = c.take<double>(k > 0 ? n : 0);
    w.seg = c.take<double>(k > 0 ? (size_t)n / OL_SEG + b + 1 : 0);
    w.incl = c.take<int>(n);
    w.tilesum = c.take<int>((size_t)flag_tiles(n) + 1);
    w.bytes = c.bytes + 256;   // room to align the caller's pointer
    return w;
}

// One thread per point (cloud_status.h): its cloud, the cloud's status bit and the copy the grid is built on.
__global__ __launch_bounds__(OL_THREADS) void outlier_prepare_kernel(int b, int n, const float* __restrict__ xyz, const int* __restrict__ offset,
                                                                     float* __restrict__ clean, int* __restrict__ cloud,
                                                                     int* __restrict__ status)
{
    const int t = blockIdx.x * OL_THREADS + threadIdx.x;
    if (t < n) cloud_prepare(t, b, xyz, nullptr, offset, clean, cloud, status, ROITR_OUTLIER_NONFINITE);
}

// One lane per point, one wave per workgroup.  rows: 64 rows of k ints at stride k | 1 (dynamic LDS).
__global__ __launch_bounds__(64) void outlier_mean_kernel(int n, int k, const float* __restrict__ xyz, const int* __restrict__ offset,
                                                          const int* __restrict__ cloud, const int* __restrict__ status,
                                                          const int* __restrict__ idx, double* __restrict__ mean,
                                                          double* __restrict__ mean_out)
{
    extern __shared__ int rows[];
    const int lane = threadIdx.x, kp = k | 1;
    const long base = (long)blockIdx.x * 64;
    const int nrow = (int)min((long)64, (long)n - base);
    const int* __restrict__ src = idx + (size_t)base * k;
    for (int e = lane; e < nrow * k; e += 64) {
        const int r = e / k;
        rows[r * kp + (e - r * k)] = src[e];
    }
    __syncthreads();
    if (lane >= nrow) return;
    const int i = (int)base + lane;
    const int c = cloud[i];
    double m = 0.0;
    if (c >= 0 && !(status[c] & ROITR_OUTLIER_NONFINITE)) {
        const int2 se = cloud_range(offset, c, n);
        const int v = min(k, se.y - se.x);     // slots behind the cloud's size are the kNN's padding; v >= 1: the cloud holds i
        const double px = xyz[(size_t)i * 3], py = xyz[(size_t)i * 3 + 1], pz = xyz[(size_t)i * 3 + 2];
        const int* __restrict__ row = rows + lane * kp;
        double s = 0.0;
        constexpr int NF = 4;
        for (int t = 0; t < v; t += NF) {
            double d2[NF];
#pragma unroll
            for (int u = 0; u < NF; ++u) {
                // the clamp changes no row of the kNN; it keeps the gather inside the cloud whatever the workspace holds
                const size_t j = (size_t)min(max(row[min(t + u, v - 1)], se.x), se.y - 1);
                const double dx = pg_sub((double)xyz[j * 3], px), dy = pg_sub((double)xyz[j * 3 + 1], py), dz = pg_sub((double)xyz[j * 3 + 2], pz);
                d2[u] = pg_add(pg_add(pg_mul(dx, dx), pg_mul(dy, dy)), pg_mul(dz, dz));
            }
#pragma unroll
            for (int u = 0; u < NF; ++u)
                if (t + u < v) s = pg_add(s, sqrt(d2[u]));
        }
        m = s / (double)v;
    }
    mean[i] = m;
    if (mean_out) mean_out[i] = m;
}

// One workgroup per cloud.  A per-cloud sum in the definition's order: thread t takes the segments t, t + 256, ... of 256 points each, one
// term after the other from +0; thread 0 then adds the segment sums in segment order from +0.  SQ: the terms are squared deviations.
template <bool SQ>
__device__ __forceinline__ double cloud_sum(const double* __restrict__ mean, int start, int size, double centre, double* __restrict__ seg,
                                            double* bcast)
{
    const int nseg = (size + OL_SEG - 1) / OL_SEG;
    for (int g = threadIdx.x; g < nseg; g += OL_THREADS) {
        const int p0 = start + g * OL_SEG, p1 = min(p0 + OL_SEG, start + size);
        double s = 0.0;
        for (int p = p0; p < p1; ++p) {
            const double m = mean[p];
            double term = 0.0;
            if (m > 0.0) {
                if (SQ) { const double d = pg_sub(m, centre); term = pg_mul(d, d); }
                else term = m;
            }
            s = pg_add(s, term);
        }
        seg[g] = s;
    }
    __syncthreads();   // the segment sums were written by this workgroup: visible to its thread 0 after the barrier
    if (threadIdx.x == 0) {
        double s = 0.0;
        constexpr int NF = 16;   // sixteen loads in flight, the adds in segment order: a large cloud has a thousand segments
        for (int g = 0; g < nseg; g += NF) {
            double v[NF];
#pragma unroll
            for (int u = 0; u < NF; ++u) v[u] = seg[min(g + u, nseg - 1)];
#pragma unroll
            for (int u = 0; u < NF; ++u)
                if (g + u < nseg) s = pg_add(s, v[u]);
        }
        *bcast = s;
    }
    __syncthreads();
    const double total = *bcast;
    __syncthreads();   // everyone has read it before the next sum overwrites it
    return total;
}

__global__ __launch_bounds__(OL_THREADS) void outlier_stats_kernel(int n, double std_ratio, const int* __restrict__ offset,
                                                                   const int* __restrict__ status, const double* __restrict__ mean,
                                                                   double* __restrict__ seg_all, unsigned char* __restrict__ keep,
                                                                   double* __restrict__ stats)
{
    __shared__ double bcast;
    const int c = blockIdx.x;
    const int2 se = cloud_range(offset, c, n);
    const int start = se.x, size = se.y - se.x;
    if (size == 0 || (status[c] & ROITR_OUTLIER_NONFINITE)) {   // uniform over the workgroup
        for (int p = threadIdx.x; p < size; p += OL_THREADS) keep[start + p] = 0;
        if (stats && threadIdx.x < 3) stats[(size_t)c * 3 + threadIdx.x] = 0.0;
        return;
    }
    double* __restrict__ seg = seg_all + (size_t)start / OL_SEG + c;   // the clouds before c own at most start / 256 + c slots
    const double V = (double)size;
    const double s1 = cloud_sum<false>(mean, start, size, 0.0, seg, &bcast);
    const double cloud_mean = s1 / V;
    const double s2 = cloud_sum<true>(mean, start, size, cloud_mean, seg, &bcast);
    const double sd = sqrt(s2 / pg_sub(V, 1.0));
    const double thr = pg_add(cloud_mean, pg_mul(std_ratio, sd));
    for (int p = threadIdx.x; p < size; p += OL_THREADS) {
        const double m = mean[start + p];
        keep[start + p] = (m > 0.0 && m < thr) ? 1 : 0;
    }
    if (stats && threadIdx.x == 0) {
        stats[(size_t)c * 3] = cloud_mean; stats[(size_t)c * 3 + 1] = sd; stats[(size_t)c * 3 + 2] = thr;
    }
}

// One lane per query: the cells under the ball of the query's own cloud, the float64 test on every candidate (pairgt.hip's walk).
template <bool COUNT>
__global__ __launch_bounds__(OL_THREADS) void outlier_radius_kernel(int n, double r, int nb_points, const float* __restrict__ xyz,
                                                                    const int* __restrict__ cloud, const int* __restrict__ status,
                                                                    const RoitrGrid* __restrict__ grids, const int* __restrict__ cell_start,
                                                                    const float4* __restrict__ sorted, unsigned char* __restrict__ keep,
                                                                    int* __restrict__ count)
{
    const int i = blockIdx.x * OL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int c = cloud[i];
    int have = 0;
    if (c >= 0 && !(status[c] & ROITR_OUTLIER_NONFINITE)) {
        const RoitrGrid g = grids[c];
        const int* __restrict__ cs = cell_start + (size_t)c * (GRID_MAX_CELLS + 1);
        const double q[3] = {xyz[(size_t)i * 3], xyz[(size_t)i * 3 + 1], xyz[(size_t)i * 3 + 2]};
        const double r2 = pg_mul(r, r);
        int x0, x1, y0, y1, z0, z1;
        float hx, hy, hz;
        ball_cells(q[0], r, g.ox, g.inv_h, g.nx, x0, x1, hx);
        ball_cells(q[1], r, g.oy, g.inv_h, g.ny, y0, y1, hy);
        ball_cells(q[2], r, g.oz, g.inv_h, g.nz, z0, z1, hz);
        bool done = false;
        for (int cz = z0; cz <= z1 && !done; ++cz)
            for (int cy = y0; cy <= y1 && !done; ++cy) {
                const int rowbase = (cz * g.ny + cy) * g.nx;
                const int s = cs[rowbase + x0], e = cs[rowbase + x1 + 1];
                constexpr int NF = 4;
                for (int p = s; p < e; p += NF) {
                    float4 f[NF];
#pragma unroll
                    for (int u = 0; u < NF; ++u) f[u] = sorted[min(p + u, e - 1)];
#pragma unroll
                    for (int u = 0; u < NF; ++u) {
                        const double dx = pg_sub((double)f[u].x, q[0]), dy = pg_sub((double)f[u].y, q[1]), dz = pg_sub((double)f[u].z, q[2]);
                        const double d2 = pg_add(pg_add(pg_mul(dx, dx), pg_mul(dy, dy)), pg_mul(dz, dz));
                        have += (p + u < e && d2 < r2) ? 1 : 0;
                    }
                    if (!COUNT && have > nb_points) { done = true; break; }   // keep is decided
                }
            }
    }
    keep[i] = have > nb_points ? 1 : 0;   // a cloud with a status bit: have == 0 and nb_points >= 0
    if (COUNT) count[i] = have;
}

// ------------------------------------------------------------------ flags -> index, new_offset (flag_compact.h), one thread per cloud
__global__ __launch_bounds__(OL_THREADS) void outlier_offset_kernel(int b, int n, const int* __restrict__ offset, const int* __restrict__ incl,
                                                                    int* __restrict__ new_offset)
{
    const int c = blockIdx.x * OL_THREADS + threadIdx.x;
    if (c >= b) return;
    const int e = min(max(offset[c], 0), n);
    new_offset[c] = e > 0 ? incl[e - 1] : 0;
}

int compact(const OlWs& w, int b, int n, const int* offset, const unsigned char* keep, int* index, int* new_offset, hipStream_t stream)
{
    flag_compact(n, keep, w.tilesum, index, w.incl, stream);
    outlier_offset_kernel<<<div_up(b, OL_THREADS), OL_THREADS, 0, stream>>>(b, n, offset, w.incl, new_offset);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}

// The refusals both entry points share; `who` is the message.
int check_args(const char* who, int b, int n, const float* xyz, const int* offset, const unsigned char* keep, const int* index,
               const int* new_offset, const int* status, const void* workspace, size_t workspace_bytes, int k)
{
    if (b < 0 || n < 0 || b > OL_MAX_CLOUDS || (b == 0 && n > 0) || n > 0x7fffffff - FLAG_TILE) return refuse(ROITR_ERR_ARG, who);
    if (b > 0 && (!offset || !new_offset || !status || (n > 0 && (!xyz || !keep || !index || !workspace)))) return refuse(ROITR_ERR_ARG, who);
    if (n > 0 && workspace_bytes < carve(nullptr, b, n, k).bytes) return refuse(ROITR_ERR_ARG, who);
    return ROITR_OK;
}

// b > 0: the status words, and what a call without points returns (stats: nullable)
int zero_outputs(int b, int n, int* new_offset, int* status, double* stats, hipStream_t stream)
{
    ROITR_HIP(hipMemsetAsync(status, 0, (size_t)b * 4, stream));
    if (n == 0) ROITR_HIP(hipMemsetAsync(new_offset, 0, (size_t)b * 4, stream));
    if (n == 0 && stats) ROITR_HIP(hipMemsetAsync(stats, 0, (size_t)b * 24, stream));
    return ROITR_OK;
}

}  // namespace

extern "C" size_t roitr_outlier_workspace_bytes(int b, int n, int nb_neighbors)
{
    if (b <= 0 || n < 0 || nb_neighbors < 0 || nb_neighbors == 1 || nb_neighbors > OL_MAX_NN) return 0;
    return carve(nullptr, b, n, nb_neighbors).bytes;
}

extern "C" int roitr_remove_statistical_outlier(int b, int n, const float* xyz, const int* offset, int nb_neighbors, double std_ratio,
                                                unsigned char* keep, int* index, int* new_offset, int* status, double* mean_dist,
                                                double* stats, void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    if (nb_neighbors < 2 || nb_neighbors > OL_MAX_NN)
        return refuse(ROITR_ERR_ARG, "remove_statistical_outlier: nb_neighbors must lie in [2, 100]");
    if (!std::isfinite(std_ratio)) return refuse(ROITR_ERR_ARG, "remove_statistical_outlier: std_ratio must be finite");
    int rc = check_args("remove_statistical_outlier: 0 <= b <= 65535 clouds, n >= 0, no null pointer, workspace of "
                        "roitr_outlier_workspace_bytes(b, n, nb_neighbors)", b, n, xyz, offset, keep, index, new_offset, status, workspace,
                        workspace_bytes, nb_neighbors);
    if (rc != ROITR_OK || b == 0) return rc;
    rc = zero_outputs(b, n, new_offset, status, stats, stream);
    if (rc != ROITR_OK || n == 0) return rc;
    const OlWs w = carve(workspace, b, n, nb_neighbors);
    ROITR_HIP(hipMemsetAsync(keep, 0, (size_t)n, stream));   // rows behind offset[b - 1] belong to no cloud's workgroup
    outlier_prepare_kernel<<<div_up(n, OL_THREADS), OL_THREADS, 0, stream>>>(b, n, xyz, offset, w.clean, w.cloud, status);
    ROITR_LAUNCH_CHECK();
    rc = roitr_knn_build_grid_ex(b, n, n, w.clean, offset, w.knn, (float)(nb_neighbors + 1) / 3.0f, stream);
    if (rc != ROITR_OK) return rc;
    rc = roitr_knnquery_ex(b, n, n, nb_neighbors, w.clean, w.clean, offset, offset, w.idx, nullptr, nullptr, nullptr, nullptr, nullptr, 1,
                           n, w.knn, stream);
    if (rc != ROITR_OK) return rc;
    const size_t lds = (size_t)64 * (nb_neighbors | 1) * sizeof(int);   // at most 25 856 bytes
    outlier_mean_kernel<<<div_up(n, 64), 64, lds, stream>>>(n, nb_neighbors, xyz, offset, w.cloud, status, w.idx, w.mean, mean_dist);
    outlier_stats_kernel<<<b, OL_THREADS, 0, stream>>>(n, std_ratio, offset, status, w.mean, w.seg, keep, stats);
    ROITR_LAUNCH_CHECK();
    return compact(w, b, n, offset, keep, index, new_offset, stream);
}

extern "C" int roitr_remove_radius_outlier(int b, int n, const float* xyz, const int* offset, double radius, int nb_points,
                                           unsigned char* keep, int* index, int* new_offset, int* status, int* count, void* workspace,
                                           size_t workspace_bytes, hipStream_t stream)
{
    if (!(radius > 0.0) || !std::isfinite(radius)) return refuse(ROITR_ERR_ARG, "remove_radius_outlier: radius must be finite and positive");
    if (nb_points < 0) return refuse(ROITR_ERR_ARG, "remove_radius_outlier: nb_points must not be negative");
    int rc = check_args("remove_radius_outlier: 0 <= b <= 65535 clouds, n >= 0, no null pointer, workspace of "
                        "roitr_outlier_workspace_bytes(b, n, 0)", b, n, xyz, offset, keep, index, new_offset, status, workspace,
                        workspace_bytes, 0);
    if (rc != ROITR_OK || b == 0) return rc;
    rc = zero_outputs(b, n, new_offset, status, nullptr, stream);
    if (rc != ROITR_OK || n == 0) return rc;
    const OlWs w = carve(workspace, b, n, 0);
    outlier_prepare_kernel<<<div_up(n, OL_THREADS), OL_THREADS, 0, stream>>>(b, n, xyz, offset, w.clean, w.cloud, status);
    ROITR_LAUNCH_CHECK();
    // Cell size for the radius: a point at the keep threshold has nb_points + 1 points in its ball; on a surface a cell of edge `radius`
    // covers 1 / pi of the ball's disc, so about (nb_points + 1) / 3 points per occupied cell put the ball under 3 x 3 x 3 cells.
    const float occupancy = fmaxf((float)(nb_points + 1) / 3.0f, 2.0f);
    rc = roitr_knn_build_grid_ex(b, n, 0, w.clean, offset, w.knn, occupancy, stream);
    if (rc != ROITR_OK) return rc;
    const RoitrGridView gv = roitr_knn_grid_view(b, n, 0, w.knn);
    if (count)
        outlier_radius_kernel<true><<<div_up(n, OL_THREADS), OL_THREADS, 0, stream>>>(n, radius, nb_points, xyz, w.cloud, status, gv.grids,
                                                                                     gv.cell_start, gv.sorted, keep, count);
    else
        outlier_radius_kernel<false><<<div_up(n, OL_THREADS), OL_THREADS, 0, stream>>>(n, radius, nb_points, xyz, w.cloud, status, gv.grids,
                                                                                      gv.cell_start, gv.sorted, keep, count);
    ROITR_LAUNCH_CHECK();
    return compact(w, b, n, offset, keep, index, new_offset, stream);
}
