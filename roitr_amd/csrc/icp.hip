// ICP pose refinement on the dense clouds: point-to-point and point-to-plane, B ragged pairs per call.
// The operator is defined in include/roitr_pointops.h above roitr_icp_batch; this file follows that text.
//
// Once per call: the status pass (non-finite values, empty clouds), the grid of pointops_knn.hip over the target clouds (built on a
// copy with non-finite coordinates zeroed, as pairgt.hip does) and the per-pair start (state = init_T, active word, the outputs of the
// pairs that never run).  Per evaluation s = 0 .. iterations, two launches:
//   icp_match_kernel    one lane per source point: the point moved by the pair's state in float64, then the nearest target point under
//                       (d2, j) with d2 < max_dist^2 among the cells of the ball.  The cells are taken from the lane's own cell outwards
//                       and the ball shrinks to the best distance found so far, by the same proven cell range (ball_walk.h) with
//                       r' = sqrt(best) (1 + 1e-9): r'^2 > best, so a cell outside r' holds only points with d2 > best, which can
//                       neither win nor tie.  The result is the exact decision whatever the order of the walk.
//                       The lane's match of the evaluation before is taken as the first candidate, so the ball starts small.
//   icp_update_kernel   one workgroup per pair: the ordered float64 sums (thread t takes points t, t + 256, ..., then the binary tree of
//                       pairgt_reduce_kernel: t + 128, t + 64 through LDS, t + 32 .. t + 1 inside wave 0), then wave 0 tests
//                       convergence, solves, and writes the next state, the trace row and -- at a stop -- the outputs.
// Lanes and workgroups of a stopped pair leave at once: the launch count depends on `iterations` alone, nothing is read back.
// What is left here is the mode's own part: the per-point sums and the solve of icp_update_kernel, and the two launches handed to icp_run.
// The host sequence (icp_run), the match kernel, the tree and what wave 0 does around the solve (icp_stats, icp_stop_early, icp_commit)
// live in icp_common.h, which gicp.hip shares.
#include "common.h"
#include "knn_grid.h"
#include "registration_math.h"
#include "roitr_pointops.h"
#include "workspace.h"
#include <cmath>

#pragma clang fp contract(off)
#include "icp_common.h"

namespace {

__global__ __launch_bounds__(ICP_THREADS) void icp_prepare_kernel(int b, int n, int m, const float* __restrict__ src,
                                                                  const int* __restrict__ src_offset, const float* __restrict__ tgt,
                                                                  const int* __restrict__ tgt_offset, const float* __restrict__ normals,
                                                                  const float* __restrict__ init_T, float* __restrict__ clean,
                                                                  int* __restrict__ status)
{
    icp_prepare(b, n, m, src, src_offset, tgt, tgt_offset, nullptr, normals, init_T, clean, status);
}

template <bool PLANE>
__global__ __launch_bounds__(ICP_THREADS) void icp_update_kernel(int b, int s, int iterations, double rel_fitness, double rel_rmse,
                                                                 const float* __restrict__ src, const int* __restrict__ src_offset,
                                                                 const float* __restrict__ tgt, const int* __restrict__ tgt_offset,
                                                                 const float* __restrict__ normals, const int* __restrict__ match,
                                                                 const double* __restrict__ d2, float* __restrict__ state,
                                                                 int* __restrict__ active, double* __restrict__ prev, IcpOut o)
{
    constexpr int NV = PLANE ? 29 : 17;
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
        const double p[3] = {src[pi], src[pi + 1], src[pi + 2]}, q[3] = {tgt[qi], tgt[qi + 1], tgt[qi + 2]};
        a[0] = pg_add(a[0], 1.0);
        a[1] = pg_add(a[1], d2[s0 + k]);
        if (!PLANE) {   // sum p, sum q, sum p q^T
#pragma unroll
            for (int c = 0; c < 3; ++c) { a[2 + c] = pg_add(a[2 + c], p[c]); a[5 + c] = pg_add(a[5 + c], q[c]); }
#pragma unroll
            for (int x = 0; x < 3; ++x)
#pragma unroll
                for (int y = 0; y < 3; ++y) a[8 + 3 * x + y] = pg_add(a[8 + 3 * x + y], pg_mul(p[x], q[y]));
        } else {        // sum J J^T (upper triangle), sum J r with J = [p' x n, n], r = (p' - q) . n
            double m[3];
            icp_move(T, p[0], p[1], p[2], m);
            const double nn[3] = {normals[qi], normals[qi + 1], normals[qi + 2]};
            const double res = pg_add(pg_add(pg_mul(pg_sub(m[0], q[0]), nn[0]), pg_mul(pg_sub(m[1], q[1]), nn[1])),
                                      pg_mul(pg_sub(m[2], q[2]), nn[2]));
            const double J[6] = {pg_sub(pg_mul(m[1], nn[2]), pg_mul(m[2], nn[1])), pg_sub(pg_mul(m[2], nn[0]), pg_mul(m[0], nn[2])),
                                 pg_sub(pg_mul(m[0], nn[1]), pg_mul(m[1], nn[0])), nn[0], nn[1], nn[2]};
            int at = 2;
#pragma unroll
            for (int x = 0; x < 6; ++x)
#pragma unroll
                for (int y = x; y < 6; ++y) { a[at] = pg_add(a[at], pg_mul(J[x], J[y])); ++at; }
#pragma unroll
            for (int x = 0; x < 6; ++x) a[23 + x] = pg_add(a[23 + x], pg_mul(J[x], res));
        }
    }
    ICP_REDUCE_TREE(a, red, NV, wave, lane)
    // every lane of wave 0 holds the same sums and takes the same decisions; lane 0 writes (icp_common.h)
    const IcpStats st = icp_stats(a, ns);
    int bits = 0;
    float Tn[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Tn[k] = T[k];
    bool stop = icp_stop_early(s, iterations, st, prev + 2 * (size_t)pr, rel_fitness, rel_rmse, PLANE ? 6 : 3, bits);
    if (!stop && !PLANE) {
        double cs_[3], ct_[3], H[9];
#pragma unroll
        for (int c = 0; c < 3; ++c) { cs_[c] = a[2 + c] / st.cn; ct_[c] = a[5 + c] / st.cn; }
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) H[3 * x + y] = a[8 + 3 * x + y] - a[2 + x] * ct_[y];   // sum (p - cs)(q - ct)^T
        rg_solve_rigid(H, cs_, ct_, Tn);
    } else if (!stop) {
        double rhs[6], x[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) rhs[k] = -a[23 + k];
        if (ldl_solve6(a + 2, rhs, x)) {
            compose_step(x, T, Tn);
        } else {
            stop = true; bits = ROITR_ICP_SINGULAR;
        }
    }
    icp_commit<2>(b, pr, s, iterations, lane, T, Tn, stop, bits, st, 0.0, state, active, prev, o, nullptr);
}

}  // namespace

extern "C" size_t roitr_icp_workspace_bytes(int b, int n, int m, int iterations)
{
    if (b <= 0 || n < 0 || m < 0 || iterations < 0) return 0;
    return carve(nullptr, b, n, m, iterations).bytes;
}

extern "C" int roitr_icp_batch(int b, int n, int m, const float* src, const int* src_offset, const float* tgt, const int* tgt_offset,
                               const float* tgt_normals, const float* init_T, float max_dist, int iterations, double rel_fitness,
                               double rel_rmse, float* T, double* fitness, double* rmse, int* n_corr, int* steps, int* status,
                               int* nn_idx, float* trace_T, double* trace_stat, void* ws, hipStream_t stream)
{
    const IcpOut o{T, fitness, rmse, n_corr, steps, status, trace_T, trace_stat};
    auto prepare = [&](const IcpWs& w, int most) {
        icp_prepare_kernel<<<div_up(most, ICP_THREADS), ICP_THREADS, 0, stream>>>(b, n, m, src, src_offset, tgt, tgt_offset, tgt_normals,
                                                                              init_T, w.clean, status);
        return ROITR_OK;
    };
    auto update = [&](const IcpWs& w, const int* match, int s) {
        if (tgt_normals)
            icp_update_kernel<true><<<b, ICP_THREADS, 0, stream>>>(b, s, iterations, rel_fitness, rel_rmse, src, src_offset, tgt, tgt_offset,
                                                                   tgt_normals, match, w.d2, w.state, w.active, w.prev, o);
        else
            icp_update_kernel<false><<<b, ICP_THREADS, 0, stream>>>(b, s, iterations, rel_fitness, rel_rmse, src, src_offset, tgt, tgt_offset,
                                                                    nullptr, match, w.d2, w.state, w.active, w.prev, o);
    };
    return icp_run<2>("icp_batch", b, n, m, src, src_offset, tgt, tgt_offset, init_T, max_dist, iterations, rel_fitness, rel_rmse, o, nn_idx,
                      ws, stream, prepare, update);
}
