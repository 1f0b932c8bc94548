// FPFH descriptors: Open3D's compute_fpfh_feature(KDTreeSearchParamHybrid(radius, max_nn)) restated.
// The operator is defined in include/roitr_pointops.h above roitr_fpfh_batch; this file follows that text.
//
// Once per call: the status pass of cloud_status.h (non-finite coordinates or normals; the cloud of every point; a copy of the points with
// non-finite coordinates zeroed, which is what the grid is built on), the grid and the exact kNN(max_nn) of pointops_knn.hip of every cloud
// against itself, its idx rows (n, max_nn) in the workspace.  Then two launches, one wave per point each:
//   fpfh_spfh_kernel   lanes own the slots of the point's kNN row (two per lane: max_nn <= 100).  Ballots give every slot its rank
//                      among the non-self entries and, after the float64 radius test, its place in K(i); the kept indices are
//                      written back over the front of the row, in row order.  Every kept lane computes its pair feature in
//                      float64 and adds 1 to three of the wave's 33 integer LDS counters.  The point's row leaves as 36 bytes:
//                      33 counts (<= 99 each) and m_i.
//   fpfh_blend_kernel  lanes stage K(i) in LDS (d2, 100 / m_j and the neighbour's 36-byte row: two neighbours per lane), then lane
//                      b < 33 walks the list in row order on byte b of every staged row; the sum of a group of 11 bins is taken
//                      over the lanes of the group in bin order after every neighbour, as the definition has it.
// Counts are integers, every float64 sum runs in row order inside one wave: a point's outputs depend on its own row alone.
#include "cloud_status.h"
#include "common.h"
#include "roitr_pointops.h"
#include "workspace.h"
#include <cmath>

#define FPFH_THREADS 256
#define FPFH_WAVES 4
#define FPFH_BINS 33
#define FPFH_ROW_WORDS 9   // 36 bytes: 33 counts, m_i, two bytes of padding
#define FPFH_MAX_NN 100
#define FPFH_MAX_CLOUDS 65535
#define FPFH_NONFINITE 1

#pragma clang fp contract(off)
#include "ball_walk.h"

namespace {

struct FpfhWs {
    void* knn;            // grid + kNN workspace of the clouds against themselves
    float* clean;         // (n, 3) points with non-finite coordinates zeroed: what the kNN runs on
    int* cloud;           // (n) the cloud of every point (-1: a row behind the last offset)
    int* idx;             // (n, max_nn) kNN rows; after the SPFH kernel the first m_i entries of row i are K(i)
    unsigned int* rows;   // (n, 9) the 36-byte SPFH rows
    size_t bytes;
};

FpfhWs carve(void* ws, int b, int n, int max_nn)
{
    Carve c(Carve::aligned(ws));
    FpfhWs w;
    w.knn = c.take<char>(roitr_knn_workspace_bytes(b, n, n));
    w.clean = c.take<float>((size_t)n * 3);
    w.cloud = c.take<int>(n);
    w.idx = c.take<int>((size_t)n * max_nn);
    w.rows = c.take<unsigned int>((size_t)n * FPFH_ROW_WORDS);
    w.bytes = c.bytes + 256;   // room to align the caller's pointer
    return w;
}

// One thread per point (cloud_status.h): its cloud (the binary search over the offsets is done here, 64 points per wave, and not by
// every wave of the SPFH kernel: there it was ten dependent loads in front of everything else), the cloud's status bit for a non-finite
// coordinate or normal, and the copy the kNN runs on.
__global__ __launch_bounds__(FPFH_THREADS) void fpfh_prepare_kernel(int b, int n, const float* __restrict__ xyz,
                                                                    const float* __restrict__ normals, const int* __restrict__ offset,
                                                                    float* __restrict__ clean, int* __restrict__ cloud,
                                                                    int* __restrict__ status)
{
    const int t = blockIdx.x * FPFH_THREADS + threadIdx.x;
    if (t < n) cloud_prepare(t, b, xyz, normals, offset, clean, cloud, status, FPFH_NONFINITE);
}

__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3])
{
    return pg_add(pg_add(pg_mul(a[0], b[0]), pg_mul(a[1], b[1])), pg_mul(a[2], b[2]));
}
__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3])
{
    c[0] = pg_sub(pg_mul(a[1], b[2]), pg_mul(a[2], b[1]));
    c[1] = pg_sub(pg_mul(a[2], b[0]), pg_mul(a[0], b[2]));
    c[2] = pg_sub(pg_mul(a[0], b[1]), pg_mul(a[1], b[0]));
}
// clamp(floor(x), 0, 10); fmax / fmin drop a NaN, so the bin is in range whatever x is
__device__ __forceinline__ int bin11(double x) { return (int)fmin(fmax(floor(x), 0.0), 10.0); }

// The three bins of the pair (i, j): dp = p_j - p_i, d2 = |dp|^2 as the radius test computed it.
__device__ __forceinline__ void pair_bins(const double (&ni)[3], const double (&nj)[3], const double (&dp_)[3], double d2, int (&h)[3])
{
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    const double d = sqrt(d2);
    if (d != 0.0) {
        const double a1 = dot3(ni, dp_) / d, a2 = dot3(nj, dp_) / d;
        const bool swap = fabs(a1) < fabs(a2);
        double n1[3], n2[3], dp[3], v[3], w[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { n1[a] = swap ? nj[a] : ni[a]; n2[a] = swap ? ni[a] : nj[a]; dp[a] = swap ? -dp_[a] : dp_[a]; }
        cross3(dp, n1, v);
        const double vn = sqrt(dot3(v, v));
        if (vn != 0.0) {
            v[0] /= vn; v[1] /= vn; v[2] /= vn;
            cross3(n1, v, w);
            f2 = swap ? -a2 : a1;
            f1 = dot3(v, n2);
            f0 = atan2(dot3(w, n2), dot3(n1, n2));
        }
    }
    h[0] = bin11(11.0 * (f0 + M_PI) / (2.0 * M_PI));
    h[1] = bin11(11.0 * (f1 + 1.0) / 2.0);
    h[2] = bin11(11.0 * (f2 + 1.0) / 2.0);
}

// One wave per point.  idx is read (the kNN row) and written (K(i) over its front) by the point's own wave only.
__global__ __launch_bounds__(FPFH_THREADS) void fpfh_spfh_kernel(int n, int max_nn, double r2, const float* __restrict__ xyz,
                                                                 const float* __restrict__ normals, const int* __restrict__ offset,
                                                                 const int* __restrict__ cloud, const int* __restrict__ status, int* idx,
                                                                 unsigned int* __restrict__ rows, int* __restrict__ spfh_counts,
                                                                 int* __restrict__ nbr_count)
{
    __shared__ unsigned int cnt[FPFH_WAVES][36];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long i_ = (long)blockIdx.x * FPFH_WAVES + wave;
    const bool valid = i_ < n;
    const int i = valid ? (int)i_ : 0;
    if (lane < 36) cnt[wave][lane] = 0;
    __syncthreads();
    int m = 0;
    bool in_cloud = false;
    const int c = valid ? cloud[i] : -1;
    if (c >= 0) {
        const int2 se = cloud_range(offset, c, n);
        const int start = se.x, end = se.y;
        in_cloud = i < end && !(status[c] & FPFH_NONFINITE);
        const int nv = in_cloud ? min(max_nn, end - start) : 0;     // slots behind the cloud's size are the kNN's padding
        const size_t row = (size_t)i * max_nn;
        const unsigned long long lt = (1ull << lane) - 1ull;
        int j[2];
        bool ns[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int k = lane + 64 * r;
            j[r] = k < nv ? idx[row + k] : -1;
            ns[r] = j[r] >= start && j[r] < end && j[r] != i;
        }
        const unsigned long long n0 = __ballot(ns[0]), n1 = __ballot(ns[1]);
        const int rank[2] = {(int)__popcll(n0 & lt), (int)(__popcll(n0) + __popcll(n1 & lt))};
        const double pi[3] = {xyz[(size_t)i * 3], xyz[(size_t)i * 3 + 1], xyz[(size_t)i * 3 + 2]};
        double dp[2][3], d2[2];
        bool keep[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            keep[r] = false;
            d2[r] = 0.0;
            if (ns[r] && rank[r] < max_nn - 1) {
#pragma unroll
                for (int a = 0; a < 3; ++a) dp[r][a] = pg_sub((double)xyz[(size_t)j[r] * 3 + a], pi[a]);
                d2[r] = dot3(dp[r], dp[r]);
                keep[r] = d2[r] < r2;
            }
        }
        const unsigned long long k0 = __ballot(keep[0]), k1 = __ballot(keep[1]);
        const int pos[2] = {(int)__popcll(k0 & lt), (int)(__popcll(k0) + __popcll(k1 & lt))};
        m = __popcll(k0) + __popcll(k1);
        if (keep[0] || keep[1]) {
            const double ni[3] = {normals[(size_t)i * 3], normals[(size_t)i * 3 + 1], normals[(size_t)i * 3 + 2]};
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (!keep[r]) continue;
                idx[row + pos[r]] = j[r];
                const double nj[3] = {normals[(size_t)j[r] * 3], normals[(size_t)j[r] * 3 + 1], normals[(size_t)j[r] * 3 + 2]};
                int h[3];
                pair_bins(ni, nj, dp[r], d2[r], h);
                atomicAdd(&cnt[wave][h[0]], 1u);
                atomicAdd(&cnt[wave][11 + h[1]], 1u);
                atomicAdd(&cnt[wave][22 + h[2]], 1u);
            }
        }
    }
    __syncthreads();
    if (!valid) return;   // the last barrier is behind every wave
    if (lane < FPFH_ROW_WORDS) {
        const unsigned int* q = &cnt[wave][4 * lane];
        unsigned int word = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
        if (lane == 8) word = q[0] | ((unsigned int)m << 8);   // bytes 32 .. 35: the last count, m_i, padding
        rows[(size_t)i * FPFH_ROW_WORDS + lane] = word;
    }
    if (spfh_counts && lane < FPFH_BINS) spfh_counts[(size_t)i * FPFH_BINS + lane] = (int)cnt[wave][lane];
    if (nbr_count && lane == 0) nbr_count[i] = m;
}

// One wave per point; lane bin < 33 owns a bin.  rows / idx are the SPFH kernel's outputs.  Staging: lane k takes neighbour k (two per
// lane) -- its index, d2, 100 / m_j and its whole 36-byte row go to LDS, so every global load of the point is in flight at once and
// the walk below reads LDS only.  Walk, in row order: val = SPFH_j[bin] / d2 per lane; the group sum S takes the 11 values of the
// lane's group in bin order through an LDS line of the wave (a wave's LDS operations execute in order; the waitcnt is the compiler's
// fence as much as the hardware's).
__global__ __launch_bounds__(FPFH_THREADS) void fpfh_blend_kernel(int n, int max_nn, int out_stride, const float* __restrict__ xyz,
                                                                  const int* __restrict__ idx, const unsigned int* __restrict__ rows,
                                                                  float* __restrict__ fpfh)
{
    __shared__ double s_d2[FPFH_WAVES][FPFH_MAX_NN];
    __shared__ double s_scale[FPFH_WAVES][FPFH_MAX_NN];
    __shared__ double s_val[FPFH_WAVES][64];
    __shared__ unsigned int s_row[FPFH_WAVES][FPFH_MAX_NN][FPFH_ROW_WORDS];   // 9-word stride: odd, so the lanes' writes spread over the banks
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long i_ = (long)blockIdx.x * FPFH_WAVES + wave;
    const bool valid = i_ < n;
    const int i = valid ? (int)i_ : 0;
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(rows);
    const int m = valid ? (int)bytes[(size_t)i * 36 + 33] : 0;
    if (valid) {
        const double pi[3] = {xyz[(size_t)i * 3], xyz[(size_t)i * 3 + 1], xyz[(size_t)i * 3 + 2]};
        for (int k = lane; k < m; k += 64) {
            const int j = idx[(size_t)i * max_nn + k];
            unsigned int word[FPFH_ROW_WORDS];
#pragma unroll
            for (int w = 0; w < FPFH_ROW_WORDS; ++w) word[w] = rows[(size_t)j * FPFH_ROW_WORDS + w];
            double dp[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) dp[a] = pg_sub((double)xyz[(size_t)j * 3 + a], pi[a]);
#pragma unroll
            for (int w = 0; w < FPFH_ROW_WORDS; ++w) s_row[wave][k][w] = word[w];
            const int mj = (int)((word[8] >> 8) & 0xffu);
            s_d2[wave][k] = dot3(dp, dp);
            s_scale[wave][k] = mj > 0 ? 100.0 / (double)mj : 0.0;
        }
    }
    __syncthreads();
    if (!valid) return;   // the last barrier is behind every wave
    const int bin = lane < FPFH_BINS ? lane : FPFH_BINS - 1, g0 = bin / 11 * 11;
    const unsigned char* nb = reinterpret_cast<const unsigned char*>(&s_row[wave][0][0]);
    double F = 0.0, S = 0.0;
    for (int k = 0; k < m; ++k) {
        const double d2 = s_d2[wave][k];
        if (!(d2 > 0.0)) continue;   // wave-uniform
        const double val = ((double)nb[k * 36 + bin] * s_scale[wave][k]) / d2;
        F += val;
        s_val[wave][lane] = val;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int t = 0; t < 11; ++t) S += s_val[wave][g0 + t];
        asm volatile("" ::: "memory");   // the reads stay in front of the next neighbour's write
    }
    const double own = m > 0 ? (double)bytes[(size_t)i * 36 + bin] * (100.0 / (double)m) : 0.0;
    const double out = (S != 0.0 ? F * 100.0 / S : F) + own;
    for (int col = lane; col < out_stride; col += 64) fpfh[(size_t)i * out_stride + col] = col < FPFH_BINS ? (float)out : 0.f;
}

}  // namespace

extern "C" size_t roitr_fpfh_workspace_bytes(int b, int n, int max_nn)
{
    if (b <= 0 || n < 0 || max_nn < 2 || max_nn > FPFH_MAX_NN) return 0;
    return carve(nullptr, b, n, max_nn).bytes;
}

extern "C" int roitr_fpfh_batch(int b, int n, const float* xyz, const float* normals, const int* offset, double radius, int max_nn,
                                int out_stride, float* fpfh, int* spfh_counts, int* nbr_count, int* status, void* workspace,
                                size_t workspace_bytes, hipStream_t stream)
{
    if (max_nn < 2 || max_nn > FPFH_MAX_NN) return refuse(ROITR_ERR_ARG, "fpfh_batch: max_nn must lie in [2, 100]");
    if (out_stride < FPFH_BINS) return refuse(ROITR_ERR_ARG, "fpfh_batch: out_stride must be at least 33");
    if (!(radius > 0.0) || !std::isfinite(radius)) return refuse(ROITR_ERR_ARG, "fpfh_batch: radius must be finite and positive");
    if (b < 0 || n < 0 || b > FPFH_MAX_CLOUDS || (b == 0 && n > 0)) return refuse(ROITR_ERR_ARG, "fpfh_batch: 0 <= b <= 65535 clouds, n >= 0");
    if (n > 0x7fffffff - FPFH_THREADS) return refuse(ROITR_ERR_ARG, "fpfh_batch: point count out of range");
    if (b == 0) return ROITR_OK;
    if (!offset || !status || (n > 0 && (!xyz || !normals || !fpfh || !workspace))) return refuse(ROITR_ERR_ARG, "fpfh_batch: null pointer");
    ROITR_HIP(hipMemsetAsync(status, 0, (size_t)b * 4, stream));
    if (n == 0) return ROITR_OK;
    if (workspace_bytes < carve(nullptr, b, n, max_nn).bytes) return refuse(ROITR_ERR_ARG, "fpfh_batch: workspace too small");
    const FpfhWs w = carve(workspace, b, n, max_nn);
    fpfh_prepare_kernel<<<div_up(n, FPFH_THREADS), FPFH_THREADS, 0, stream>>>(b, n, xyz, normals, offset, w.clean, w.cloud, status);
    ROITR_LAUNCH_CHECK();
    int rc = roitr_knn_build_grid_ex(b, n, n, w.clean, offset, w.knn, (float)(max_nn + 1) / 3.0f, stream);
    if (rc != ROITR_OK) return rc;
    rc = roitr_knnquery_ex(b, n, n, max_nn, w.clean, w.clean, offset, offset, w.idx, nullptr, nullptr, nullptr, nullptr, nullptr, 1, n,
                           w.knn, stream);
    if (rc != ROITR_OK) return rc;
    const int blocks = div_up(n, FPFH_WAVES);
    fpfh_spfh_kernel<<<blocks, FPFH_THREADS, 0, stream>>>(n, max_nn, radius * radius, xyz, normals, offset, w.cloud, status, w.idx, w.rows,
                                                         spfh_counts, nbr_count);
    ROITR_LAUNCH_CHECK();
    fpfh_blend_kernel<<<blocks, FPFH_THREADS, 0, stream>>>(n, max_nn, out_stride, xyz, w.idx, w.rows, fpfh);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}
