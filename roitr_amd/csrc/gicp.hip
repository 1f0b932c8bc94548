// Generalized ICP on the dense clouds: plane-to-plane refinement from the normals of both clouds,
// B ragged pairs per call.  The operator is defined in include/roitr_pointops.h above roitr_gicp_batch; this file follows that text.
//
// The covariance of a point is fixed by its unit normal, C = I - (1 - eps) n n^T, so nothing is estimated here: the call is
// roitr_icp_batch's (icp_common.h: icp_run with its checks, status pass, grid, start, exact match and loop; icp_stats, icp_stop_early and
// icp_commit around the solve) with another update step.  Per evaluation, two launches:
//   icp_match_kernel     the match of icp.hip, unchanged.
//   gicp_update_kernel   one workgroup per pair: per matched point, in registers, the unit normals, the rotated source normal, the
//                        symmetric M = 2I - (1 - eps)(a a^T + b b^T), its inverse W by cofactors, W J through the structure of
//                        J = [-[p']x | I]; 30 ordered float64 sums (count, sum d2, sum d^T W d, the 21 + 6 of the system) in the
//                        order of icp_update_kernel, then wave 0 tests convergence, solves and writes as that kernel does.
#include "common.h"
#include "knn_grid.h"
#include "roitr_pointops.h"
#include "workspace.h"
#include <cmath>

#pragma clang fp contract(off)
#include "icp_common.h"

namespace {

constexpr int GICP_NV = 30;   // 0 count, 1 sum d2, 2 sum d^T W d, 3..23 A (upper triangle, row-major), 24..29 g

__global__ __launch_bounds__(ICP_THREADS) void gicp_prepare_kernel(int b, int n, int m, const float* __restrict__ src,
                                                                   const int* __restrict__ src_offset, const float* __restrict__ tgt,
                                                                   const int* __restrict__ tgt_offset,
                                                                   const float* __restrict__ src_normals,
                                                                   const float* __restrict__ tgt_normals,
                                                                   const float* __restrict__ init_T, float* __restrict__ clean,
                                                                   int* __restrict__ status)
{
    icp_prepare(b, n, m, src, src_offset, tgt, tgt_offset, src_normals, tgt_normals, init_T, clean, status);
}

// n / sqrt((nx^2 + ny^2) + nz^2) in float64 on the fp32 values; a squared length of exactly 0 gives 0 (an isotropic point)
__device__ __forceinline__ void gicp_unit(const float* __restrict__ v, double (&u)[3])
{
    const double x = v[0], y = v[1], z = v[2];
    const double l2 = pg_add(pg_add(pg_mul(x, x), pg_mul(y, y)), pg_mul(z, z));
    const double l = sqrt(l2);
    const bool zero = l2 == 0.0;
    u[0] = zero ? 0.0 : x / l; u[1] = zero ? 0.0 : y / l; u[2] = zero ? 0.0 : z / l;
}

__global__ __launch_bounds__(ICP_THREADS) void gicp_update_kernel(int b, int s, int iterations, double rel_fitness, double rel_rmse,
                                                                  double c, const float* __restrict__ src,
                                                                  const int* __restrict__ src_offset, const float* __restrict__ tgt,
                                                                  const int* __restrict__ tgt_offset,
                                                                  const float* __restrict__ src_normals,
                                                                  const float* __restrict__ tgt_normals, const int* __restrict__ match,
                                                                  const double* __restrict__ d2, float* __restrict__ state,
                                                                  int* __restrict__ active, double* __restrict__ prev, IcpOut o,
                                                                  double* __restrict__ objective)
{
    constexpr int NV = GICP_NV;
    __shared__ double red[2][NV][64];
    const int pr = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!active[pr]) return;
    const int s0 = pr ? src_offset[pr - 1] : 0, ns = src_offset[pr] - s0, t0 = pr ? tgt_offset[pr - 1] : 0;
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = state[(size_t)pr * 12 + k];
    double a[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) a[k] = 0.0;
    for (int k = tid; k < ns; k += ICP_THREADS) {
        const int j = match[s0 + k];
        if (j < 0) continue;
        const size_t pi = (size_t)(s0 + k) * 3, qi = (size_t)(t0 + j) * 3;
        double p[3], us[3], bn[3];
        icp_move(T, (double)src[pi], (double)src[pi + 1], (double)src[pi + 2], p);
        const double d[3] = {pg_sub(p[0], (double)tgt[qi]), pg_sub(p[1], (double)tgt[qi + 1]), pg_sub(p[2], (double)tgt[qi + 2])};
        gicp_unit(src_normals + pi, us);
        gicp_unit(tgt_normals + qi, bn);
        double an[3];   // a = R n_s
#pragma unroll
        for (int r = 0; r < 3; ++r)
            an[r] = pg_add(pg_add(pg_mul((double)T[4 * r], us[0]), pg_mul((double)T[4 * r + 1], us[1])), pg_mul((double)T[4 * r + 2], us[2]));
        // M = 2I - c (a a^T + b b^T), upper triangle
#define GICP_M(x, y, diag) pg_sub(diag, pg_mul(c, pg_add(pg_mul(an[x], an[y]), pg_mul(bn[x], bn[y]))))
        const double m00 = GICP_M(0, 0, 2.0), m01 = GICP_M(0, 1, 0.0), m02 = GICP_M(0, 2, 0.0), m11 = GICP_M(1, 1, 2.0),
                     m12 = GICP_M(1, 2, 0.0), m22 = GICP_M(2, 2, 2.0);
#undef GICP_M
        // W = M^-1: the six cofactors over the determinant
        const double c00 = pg_sub(pg_mul(m11, m22), pg_mul(m12, m12)), c01 = pg_sub(pg_mul(m12, m02), pg_mul(m01, m22)),
                     c02 = pg_sub(pg_mul(m01, m12), pg_mul(m11, m02)), c11 = pg_sub(pg_mul(m00, m22), pg_mul(m02, m02)),
                     c12 = pg_sub(pg_mul(m01, m02), pg_mul(m00, m12)), c22 = pg_sub(pg_mul(m00, m11), pg_mul(m01, m01));
        const double det = pg_add(pg_add(pg_mul(m00, c00), pg_mul(m01, c01)), pg_mul(m02, c02));
        const double W[3][3] = {{c00 / det, c01 / det, c02 / det}, {c01 / det, c11 / det, c12 / det}, {c02 / det, c12 / det, c22 / det}};
        // e = W d, K = W (-[p]x): row x is p x W[x]; G = [p]x K: column y is p x K[:, y]
        double e[3], K[3][3];
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            e[x] = pg_add(pg_add(pg_mul(W[x][0], d[0]), pg_mul(W[x][1], d[1])), pg_mul(W[x][2], d[2]));
            K[x][0] = pg_sub(pg_mul(p[1], W[x][2]), pg_mul(p[2], W[x][1]));
            K[x][1] = pg_sub(pg_mul(p[2], W[x][0]), pg_mul(p[0], W[x][2]));
            K[x][2] = pg_sub(pg_mul(p[0], W[x][1]), pg_mul(p[1], W[x][0]));
        }
        a[0] = pg_add(a[0], 1.0);
        a[1] = pg_add(a[1], d2[s0 + k]);
        a[2] = pg_add(a[2], pg_add(pg_add(pg_mul(d[0], e[0]), pg_mul(d[1], e[1])), pg_mul(d[2], e[2])));
        // rows 0..2 of A: G (from the diagonal on), then K^T
        a[3] = pg_add(a[3], pg_sub(pg_mul(p[1], K[2][0]), pg_mul(p[2], K[1][0])));     // G00
        a[4] = pg_add(a[4], pg_sub(pg_mul(p[1], K[2][1]), pg_mul(p[2], K[1][1])));     // G01
        a[5] = pg_add(a[5], pg_sub(pg_mul(p[1], K[2][2]), pg_mul(p[2], K[1][2])));     // G02
        a[6] = pg_add(a[6], K[0][0]); a[7] = pg_add(a[7], K[1][0]); a[8] = pg_add(a[8], K[2][0]);
        a[9] = pg_add(a[9], pg_sub(pg_mul(p[2], K[0][1]), pg_mul(p[0], K[2][1])));     // G11
        a[10] = pg_add(a[10], pg_sub(pg_mul(p[2], K[0][2]), pg_mul(p[0], K[2][2])));   // G12
        a[11] = pg_add(a[11], K[0][1]); a[12] = pg_add(a[12], K[1][1]); a[13] = pg_add(a[13], K[2][1]);
        a[14] = pg_add(a[14], pg_sub(pg_mul(p[0], K[1][2]), pg_mul(p[1], K[0][2])));   // G22
        a[15] = pg_add(a[15], K[0][2]); a[16] = pg_add(a[16], K[1][2]); a[17] = pg_add(a[17], K[2][2]);
        // rows 3..5: W
        a[18] = pg_add(a[18], W[0][0]); a[19] = pg_add(a[19], W[0][1]); a[20] = pg_add(a[20], W[0][2]);
        a[21] = pg_add(a[21], W[1][1]); a[22] = pg_add(a[22], W[1][2]); a[23] = pg_add(a[23], W[2][2]);
        // g = J^T W d = (p x e, e)
        a[24] = pg_add(a[24], pg_sub(pg_mul(p[1], e[2]), pg_mul(p[2], e[1])));
        a[25] = pg_add(a[25], pg_sub(pg_mul(p[2], e[0]), pg_mul(p[0], e[2])));
        a[26] = pg_add(a[26], pg_sub(pg_mul(p[0], e[1]), pg_mul(p[1], e[0])));
        a[27] = pg_add(a[27], e[0]); a[28] = pg_add(a[28], e[1]); a[29] = pg_add(a[29], e[2]);
    }
    ICP_REDUCE_TREE(a, red, NV, wave, lane)
    // every lane of wave 0 holds the same sums and takes the same decisions; lane 0 writes (icp_common.h)
    const IcpStats st = icp_stats(a, ns);
    const double obj = st.nc > 0 ? a[2] / st.cn : 0.0;
    int bits = 0;
    float Tn[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Tn[k] = T[k];
    bool stop = icp_stop_early(s, iterations, st, prev + 2 * (size_t)pr, rel_fitness, rel_rmse, 6, bits);
    if (!stop) {
        double rhs[6], x[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) rhs[k] = -a[24 + k];
        if (ldl_solve6(a + 3, rhs, x)) {
            compose_step(x, T, Tn);
        } else {
            stop = true; bits = ROITR_ICP_SINGULAR;
        }
    }
    icp_commit<3>(b, pr, s, iterations, lane, T, Tn, stop, bits, st, obj, state, active, prev, o, objective);
}

}  // namespace

extern "C" size_t roitr_gicp_workspace_bytes(int b, int n, int m, int iterations)
{
    if (b <= 0 || n < 0 || m < 0 || iterations < 0) return 0;
    return carve(nullptr, b, n, m, iterations).bytes;
}

extern "C" int roitr_gicp_batch(int b, int n, int m, const float* src, const int* src_offset, const float* tgt, const int* tgt_offset,
                                const float* src_normals, const float* tgt_normals, const float* init_T, float max_dist, double epsilon,
                                int iterations, double rel_fitness, double rel_rmse, float* T, double* fitness, double* rmse,
                                double* objective, int* n_corr, int* steps, int* status, int* nn_idx, float* trace_T,
                                double* trace_stat, void* ws, hipStream_t stream)
{
    if (!(epsilon >= 1e-6 && epsilon <= 1.0)) return refuse(ROITR_ERR_ARG, "gicp_batch: epsilon must lie in [1e-6, 1]");
    if (!src_normals || !tgt_normals) return refuse(ROITR_ERR_ARG, "gicp_batch: null normals pointer (both clouds need normals)");
    const IcpOut o{T, fitness, rmse, n_corr, steps, status, trace_T, trace_stat};
    auto prepare = [&](const IcpWs& w, int most) {
        // all-ones bytes are a NaN: what the objective of a pair that never runs (NONFINITE, EMPTY) stays; every other pair writes its
        // own.  Set here, behind the driver's checks: a refused call leaves the outputs untouched.
        if (objective) ROITR_HIP(hipMemsetAsync(objective, 0xff, (size_t)b * 8, stream));
        gicp_prepare_kernel<<<div_up(most, ICP_THREADS), ICP_THREADS, 0, stream>>>(b, n, m, src, src_offset, tgt, tgt_offset, src_normals,
                                                                               tgt_normals, init_T, w.clean, status);
        return ROITR_OK;
    };
    const double c = 1.0 - epsilon;
    auto update = [&](const IcpWs& w, const int* match, int s) {
        gicp_update_kernel<<<b, ICP_THREADS, 0, stream>>>(b, s, iterations, rel_fitness, rel_rmse, c, src, src_offset, tgt, tgt_offset,
                                                         src_normals, tgt_normals, match, w.d2, w.state, w.active, w.prev, o, objective);
    };
    return icp_run<3>("gicp_batch", b, n, m, src, src_offset, tgt, tgt_offset, init_T, max_dist, iterations, rel_fitness, rel_rmse, o,
                      nn_idx, ws, stream, prepare, update);
}
