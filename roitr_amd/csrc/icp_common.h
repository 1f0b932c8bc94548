// What the ICP family shares on the device (icp.hip: point-to-point / point-to-plane, gicp.hip: plane-to-plane): the workspace, the
// status pass, the per-pair start, the float64 move, the exact nearest-neighbour match, the 6x6 L D L^T solve, the composition of a
// step with the state, the ordered reduction tree, what wave 0 of an update kernel does around its solve (icp_stats, icp_stop_early,
// icp_commit) and the host side of a call (icp_run).  Carved out of icp.hip, the way ball_walk.h was carved out of pairgt.hip; every
// translation unit that includes it gets its own copy of the kernels (anonymous namespace).  The device functions round every product
// and sum on its own: pg_add / pg_mul / pg_sub, or plain operators under the includer's contract(off).
// Include it AFTER `#pragma clang fp contract(off)`, like ball_walk.h: the operator's rule is "every product and sum rounded on its own";
// and include common.h, knn_grid.h and workspace.h BEFORE that pragma, as icp.hip always has, so that their inline fp32 code keeps
// the contraction it is compiled with everywhere else (the includes below are then no-ops).
#pragma once
#include "cloud_status.h"
#include "common.h"
#include "knn_grid.h"
#include "roitr_pointops.h"
#include "workspace.h"
#include <cmath>
#include <cstdio>

#define ICP_THREADS 256
#define ICP_MAX_PAIRS 65536
#define ICP_SKIP (ROITR_ICP_NONFINITE | ROITR_ICP_EMPTY)

#include "ball_walk.h"
#include "gauss_newton6.h"

namespace {

struct IcpWs {
    void* knn;       // grid workspace of the target clouds
    float* clean;    // (m, 3) target points with non-finite coordinates zeroed: what the grid is built on
    int* match;      // (n) pair-local match of every source point under the last evaluated state (-1: none)
    double* d2;      // (n) its squared distance
    float* state;    // (B, 12) T_s, rows of [R | t]
    int* active;     // (B) 1 while the pair iterates
    double* prev;    // (B, 2) fitness and rmse of the evaluation before
    size_t bytes;
};

IcpWs carve(void* ws, int b, int n, int m, int iterations)
{
    (void)iterations;   // the trace is the caller's: no buffer here grows with the iteration count
    Carve c(Carve::aligned(ws));
    IcpWs w;
    w.knn = c.take<char>(roitr_knn_workspace_bytes(b, m, 0));
    w.clean = c.take<float>((size_t)m * 3);
    w.match = c.take<int>(n);
    w.d2 = c.take<double>(n);
    w.state = c.take<float>((size_t)b * 12);
    w.active = c.take<int>(b);
    w.prev = c.take<double>((size_t)b * 2);
    w.bytes = c.bytes + 256;   // room to align the caller's pointer
    return w;
}

struct IcpOut {   // the caller's arrays; any but T and status may be null
    float* T; double* fitness; double* rmse; int* n_corr; int* steps; int* status; float* trace_T; double* trace_stat;
};

// One thread per pair, per source point and per target point: the status bits (integer atomicOr on a word the host zeroed) and the
// copy of the target points the grid is built on.  src_normals: null unless the mode reads them (gicp.hip).
__device__ __forceinline__ void icp_prepare(int b, int n, int m, const float* __restrict__ src, const int* __restrict__ src_offset,
                                            const float* __restrict__ tgt, const int* __restrict__ tgt_offset,
                                            const float* __restrict__ src_normals, const float* __restrict__ normals,
                                            const float* __restrict__ init_T, float* __restrict__ clean, int* __restrict__ status)
{
    const int t = blockIdx.x * ICP_THREADS + threadIdx.x;
    if (t < b) {
        bool ok = true;
        for (int k = 0; k < 12; ++k) ok &= isfinite(init_T[(size_t)t * 16 + k]);
        const int ns = src_offset[t] - (t ? src_offset[t - 1] : 0), nt = tgt_offset[t] - (t ? tgt_offset[t - 1] : 0);
        const int bits = (ok ? 0 : ROITR_ICP_NONFINITE) | ((ns <= 0 || nt <= 0) ? ROITR_ICP_EMPTY : 0);
        if (bits) atomicOr(&status[t], bits);
    }
    if (t < n) {
        bool ok = finite3(src[(size_t)t * 3], src[(size_t)t * 3 + 1], src[(size_t)t * 3 + 2]);
        if (src_normals) ok = ok && finite3(src_normals[(size_t)t * 3], src_normals[(size_t)t * 3 + 1], src_normals[(size_t)t * 3 + 2]);
        if (!ok) atomicOr(&status[segment_of(t, src_offset, b)], ROITR_ICP_NONFINITE);
    }
    if (t < m) {
        const float x = tgt[(size_t)t * 3], y = tgt[(size_t)t * 3 + 1], z = tgt[(size_t)t * 3 + 2];
        bool ok = finite3(x, y, z);
        store_clean(clean, t, x, y, z, ok);
        if (normals) ok = ok && finite3(normals[(size_t)t * 3], normals[(size_t)t * 3 + 1], normals[(size_t)t * 3 + 2]);
        if (!ok) atomicOr(&status[segment_of(t, tgt_offset, b)], ROITR_ICP_NONFINITE);
    }
}

// T (4,4) of one pair from the 12 state values
__device__ __forceinline__ void write_T16(float* __restrict__ o, const float* T)
{
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = T[k];
    o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
}

// One thread per pair: T_0 = init_T, the active word, and everything a pair that never runs (NONFINITE, EMPTY) returns.  NSTAT: the
// columns of trace_stat (2: fitness, rmse; 3: a third one of the mode's own).
template <int NSTAT>
__global__ __launch_bounds__(ICP_THREADS) void icp_start_kernel(int b, int iterations, const float* __restrict__ init_T,
                                                                float* __restrict__ state, int* __restrict__ active,
                                                                double* __restrict__ prev, IcpOut o)
{
    const int pr = blockIdx.x * ICP_THREADS + threadIdx.x;
    if (pr >= b) return;
    float T[12];
    for (int k = 0; k < 12; ++k) { T[k] = init_T[(size_t)pr * 16 + k]; state[(size_t)pr * 12 + k] = T[k]; }
    prev[2 * (size_t)pr] = 0.0; prev[2 * (size_t)pr + 1] = 0.0;
    const bool skip = o.status[pr] & ICP_SKIP;
    active[pr] = skip ? 0 : 1;
    if (!skip) return;
    if (o.T) write_T16(o.T + 16 * (size_t)pr, T);
    if (o.fitness) o.fitness[pr] = (double)NAN;
    if (o.rmse) o.rmse[pr] = (double)NAN;
    if (o.n_corr) o.n_corr[pr] = 0;
    if (o.steps) o.steps[pr] = 0;
    for (int r = 0; r <= iterations; ++r) {
        const size_t row = (size_t)r * b + pr;
        if (o.trace_T) for (int k = 0; k < 12; ++k) o.trace_T[row * 12 + k] = T[k];
        if (o.trace_stat) {
            o.trace_stat[row * NSTAT] = (double)NAN; o.trace_stat[row * NSTAT + 1] = (double)NAN;
            if (NSTAT == 3) o.trace_stat[row * NSTAT + 2] = (double)NAN;
        }
    }
}

// p' = ((R[c][0] px + R[c][1] py) + R[c][2] pz) + t[c] with T the rows [R | t]: the forward move of pairgt.hip
__device__ __forceinline__ void icp_move(const float (&T)[12], double px, double py, double pz, double (&o)[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c)
        o[c] = pg_add(pg_add(pg_add(pg_mul((double)T[4 * c], px), pg_mul((double)T[4 * c + 1], py)), pg_mul((double)T[4 * c + 2], pz)),
                      (double)T[4 * c + 3]);
}

// k-th cell of [lo, hi] counted from c outwards: c, c + 1, c - 1, c + 2, ... (lo <= c <= hi); out of range: -1
__device__ __forceinline__ int outward(int c, int k, int lo, int hi)
{
    const int v = c + ((k & 1) ? (k + 1) >> 1 : -(k >> 1));
    return (v < lo || v > hi) ? -1 : v;
}

__global__ __launch_bounds__(ICP_THREADS) void icp_match_kernel(int b, int n, const float* __restrict__ src,
                                                                const int* __restrict__ src_offset, const float* __restrict__ tgt,
                                                                const int* __restrict__ tgt_offset, const float* __restrict__ state,
                                                                const int* __restrict__ active, double r,
                                                                const RoitrGrid* __restrict__ grids, const int* __restrict__ cell_start,
                                                                const float4* __restrict__ sorted, int* __restrict__ match,
                                                                double* __restrict__ out_d2)
{
    const int i = blockIdx.x * ICP_THREADS + threadIdx.x;
    if (i >= n) return;
    const int seg = segment_of(i, src_offset, b);
    if (!active[seg]) return;
    const int t0 = seg ? tgt_offset[seg - 1] : 0;
    const RoitrGrid g = grids[seg];
    const int* cs = cell_start + (size_t)seg * (GRID_MAX_CELLS + 1);
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = state[(size_t)seg * 12 + k];
    double q[3];
    icp_move(T, (double)src[(size_t)i * 3], (double)src[(size_t)i * 3 + 1], (double)src[(size_t)i * 3 + 2], q);
    const double r2 = pg_mul(r, r);
    int best_j = -1;
    double best = INFINITY;
    int x0, x1, y0, y1, z0, z1;
    float hx, hy, hz;
    ball_cells(q[0], r, g.ox, g.inv_h, g.nx, x0, x1, hx);
    ball_cells(q[1], r, g.oy, g.inv_h, g.ny, y0, y1, hy);
    ball_cells(q[2], r, g.oz, g.inv_h, g.nz, z0, z1, hz);
    // g.ox is the cloud's exact minimum: with fhi < g.ox (ball_walk.h: q <= fhi for every accepted q) nothing can be accepted
    if (!(hx < g.ox || hy < g.oy || hz < g.oz)) {
        // the lane's own cell, clamped into the ball's range (cell_of_axis is monotone, so it lies inside already for a finite q)
        const int ccy = min(max(cell_of_axis((float)q[1], g.oy, g.inv_h, g.ny), y0), y1);
        const int ccz = min(max(cell_of_axis((float)q[2], g.oz, g.inv_h, g.nz), z0), z1);
        const int kz = 2 * max(ccz - z0, z1 - ccz), ky = 2 * max(ccy - y0, y1 - ccy);
        bool shrink = false;   // best has improved since the ranges were last computed
        // The match of the evaluation before (-1 at s = 0) is a candidate like any other, taken first: after the first steps it is the
        // new match or close to it, so the ball starts at that distance.  The walk meets it again (same coordinates, same d2) and
        // still takes a lower j at an equal d2, so the result does not depend on it.
        const int jp = match[i];
        if (jp >= 0) {
            const size_t qi = (size_t)(t0 + jp) * 3;
            const double dx = pg_sub(q[0], (double)tgt[qi]), dy = pg_sub(q[1], (double)tgt[qi + 1]), dz = pg_sub(q[2], (double)tgt[qi + 2]);
            const double d2 = pg_add(pg_add(pg_mul(dx, dx), pg_mul(dy, dy)), pg_mul(dz, dz));
            if (d2 < r2) { best = d2; best_j = jp; shrink = true; }
        }
        for (int a = 0; a <= kz; ++a) {
            const int cz = outward(ccz, a, z0, z1);
            if (cz < 0) continue;
            for (int c = 0; c <= ky; ++c) {
                if (shrink) {
                    // every point that can still win or tie has d2 <= best < rr^2: the ranges of radius rr hold them all
                    const double rr = fmin(r, sqrt(best) * (1.0 + 1e-9));
                    int lo, hi;
                    float f;
                    ball_cells(q[0], rr, g.ox, g.inv_h, g.nx, lo, hi, f); x0 = max(x0, lo); x1 = min(x1, hi);
                    ball_cells(q[1], rr, g.oy, g.inv_h, g.ny, lo, hi, f); y0 = max(y0, lo); y1 = min(y1, hi);
                    ball_cells(q[2], rr, g.oz, g.inv_h, g.nz, lo, hi, f); z0 = max(z0, lo); z1 = min(z1, hi);
                    shrink = false;
                }
                if (cz < z0 || cz > z1) break;
                const int cy = outward(ccy, c, y0, y1);
                if (cy < 0 || x0 > x1) continue;
                const int rowbase = (cz * g.ny + cy) * g.nx;
                const int s = cs[rowbase + x0], e = cs[rowbase + x1 + 1];
                constexpr int NF = 4;
                for (int p = s; p < e; p += NF) {
                    float4 cd[NF];
#pragma unroll
                    for (int u = 0; u < NF; ++u) cd[u] = sorted[min(p + u, e - 1)];
#pragma unroll
                    for (int u = 0; u < NF; ++u) {
                        const double dx = pg_sub(q[0], (double)cd[u].x), dy = pg_sub(q[1], (double)cd[u].y),
                                     dz = pg_sub(q[2], (double)cd[u].z);
                        const double d2 = pg_add(pg_add(pg_mul(dx, dx), pg_mul(dy, dy)), pg_mul(dz, dz));
                        const int j = __float_as_int(cd[u].w) - t0;
                        if (p + u < e && d2 < r2 && (d2 < best || (d2 == best && j < best_j))) {
                            shrink = shrink || d2 < best;
                            best = d2; best_j = j;
                        }
                    }
                }
            }
        }
    }
    match[i] = best_j;
    out_d2[i] = best;
}

// ldl_solve6 (the 6x6 L D L^T solve) and compose_step (the composition of a step with the state) live in gauss_newton6.h, which
// fgr.hip includes too.

// The tree of pairgt_reduce_kernel over the NV per-thread sums a[NV] of a workgroup of 256, with red the kernel's __shared__ double
// [2][NV][64]: t += t + 128, t += t + 64 (LDS), then t += t + 32 .. t + 1 inside wave 0, every lane of which ends up holding the
// totals; the other waves return from the kernel after the last barrier.  A macro, not a function: the text is expanded in place, so the
// ICP kernels compile to the instructions they had when this tree stood in icp_update_kernel (a function of the same text changed the
// instruction schedule of the point-to-point kernel).
#define ICP_REDUCE_TREE(a, red, NV, wave, lane)                                                  \
    if (wave >= 2)                                                                               \
        _Pragma("unroll") for (int k = 0; k < NV; ++k) red[wave - 2][k][lane] = a[k];            \
    __syncthreads();                                                                             \
    if (wave < 2)                                                                                \
        _Pragma("unroll") for (int k = 0; k < NV; ++k) a[k] = pg_add(a[k], red[wave][k][lane]);  \
    __syncthreads();                                                                             \
    if (wave == 1)                                                                               \
        _Pragma("unroll") for (int k = 0; k < NV; ++k) red[0][k][lane] = a[k];                   \
    __syncthreads();                                                                             \
    if (wave != 0) return; /* no barrier below */                                                \
    _Pragma("unroll") for (int k = 0; k < NV; ++k) {                                             \
        double v = pg_add(a[k], red[0][k][lane]);                                                \
        _Pragma("unroll") for (int w = 32; w > 0; w >>= 1) v = pg_add(v, __shfl_down(v, w, 64)); \
        a[k] = __shfl(v, 0, 64);                                                                 \
    }

// What wave 0 of an update kernel does after the tree, every lane holding the same sums and taking the same decisions: icp_stats,
// icp_stop_early, the mode's own solve (Tn, or SINGULAR and a stop), icp_commit.
struct IcpStats { double cn; int nc; double fitness, rmse; };

// a[0]: the match count (below 2^53: exact), a[1]: sum d2; ns: the pair's source points
__device__ __forceinline__ IcpStats icp_stats(const double* a, int ns)
{
    IcpStats st;
    st.cn = a[0];
    st.nc = (int)st.cn;
    st.fitness = st.cn / (double)ns;
    st.rmse = st.nc > 0 ? sqrt(a[1] / st.cn) : 0.0;
    return st;
}

// The stops that come before a solve, in their order: converged against the pair's prev (fitness, rmse), the last evaluation, fewer than
// min_corr matches.  true: the pair stops at this evaluation with `bits`.
__device__ __forceinline__ bool icp_stop_early(int s, int iterations, const IcpStats& st, const double* prev, double rel_fitness,
                                               double rel_rmse, int min_corr, int& bits)
{
    if (s > 0 && fabs(st.fitness - prev[0]) < rel_fitness && fabs(st.rmse - prev[1]) < rel_rmse) { bits = ROITR_ICP_CONVERGED; return true; }
    if (s == iterations) return true;
    if (st.nc < min_corr) { bits = ROITR_ICP_TOO_FEW; return true; }
    return false;
}

// The trace row of evaluation s, then either the next state Tn and the pair's prev, or -- at a stop -- the rest of the trace (it repeats
// this row), the active word, the outputs and the status bits.  NSTAT 3: `third` is the last trace_stat column and goes to objective[pr].
template <int NSTAT>
__device__ __forceinline__ void icp_commit(int b, int pr, int s, int iterations, int lane, const float (&T)[12], const float (&Tn)[12],
                                           bool stop, int bits, const IcpStats& st, double third, float* __restrict__ state,
                                           int* __restrict__ active, double* __restrict__ prev, const IcpOut& o,
                                           double* __restrict__ objective)
{
    auto trace = [&](size_t row) {   // constant indices only: a lane-indexed T[] would live in scratch
        if (o.trace_T)
#pragma unroll
            for (int k = 0; k < 12; ++k) o.trace_T[row * 12 + k] = T[k];
        if (o.trace_stat) {
            o.trace_stat[row * NSTAT] = st.fitness; o.trace_stat[row * NSTAT + 1] = st.rmse;
            if (NSTAT == 3) o.trace_stat[row * NSTAT + 2] = third;
        }
    };
    if (lane == 0) trace((size_t)s * b + pr);
    if (!stop) {
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k) state[(size_t)pr * 12 + k] = Tn[k];
            prev[2 * (size_t)pr] = st.fitness; prev[2 * (size_t)pr + 1] = st.rmse;
        }
        return;
    }
    for (int e = lane; e < iterations - s; e += 64) trace((size_t)(s + 1 + e) * b + pr);
    if (lane == 0) {
        active[pr] = 0;
        if (o.T) write_T16(o.T + 16 * (size_t)pr, T);
        if (o.fitness) o.fitness[pr] = st.fitness;
        if (o.rmse) o.rmse[pr] = st.rmse;
        if (NSTAT == 3 && objective) objective[pr] = third;
        if (o.n_corr) o.n_corr[pr] = st.nc;
        if (o.steps) o.steps[pr] = s;
        o.status[pr] |= bits;
    }
}

// The host side of a call: the argument checks (error texts begin with `who`), the two memsets, prepare(w, most) -- the mode's status
// pass over `most` threads --, the target grid, the start and the evaluation loop of icp_match_kernel and update(w, match, s).  NSTAT:
// the columns of trace_stat.
template <int NSTAT, class Prepare, class Update>
int icp_run(const char* who, int b, int n, int m, const float* src, const int* src_offset, const float* tgt, const int* tgt_offset,
            const float* init_T, float max_dist, int iterations, double rel_fitness, double rel_rmse, const IcpOut& o, int* nn_idx, void* ws,
            hipStream_t stream, Prepare prepare, Update update)
{
    auto bad = [&](const char* what) {
        char text[160];
        snprintf(text, sizeof(text), "%s: %s", who, what);
        return refuse(ROITR_ERR_ARG, text);
    };
    if (!(max_dist > 0.f) || !std::isfinite(max_dist)) return bad("max_dist must be finite and positive");
    if (iterations < 0 || !(rel_fitness >= 0.0) || !(rel_rmse >= 0.0)) return bad("iterations, rel_fitness and rel_rmse must not be negative");
    if (b <= 0 || b > ICP_MAX_PAIRS) return bad("1 <= B <= 65536 pairs");
    if (n < 0 || m < 0 || n > 0x7fffffff - ICP_THREADS || m > 0x7fffffff - ICP_THREADS) return bad("point counts out of range");
    if (!src_offset || !tgt_offset || !init_T || !o.T || !o.status || !ws || (n > 0 && !src) || (m > 0 && !tgt)) return bad("null pointer");
    const IcpWs w = carve(ws, b, n, m, iterations);
    int* match = nn_idx ? nn_idx : w.match;   // stopped pairs are not matched again: the buffer ends up holding every pair's final matches
    ROITR_HIP(hipMemsetAsync(o.status, 0, (size_t)b * 4, stream));
    if (n > 0) ROITR_HIP(hipMemsetAsync(match, 0xff, (size_t)n * 4, stream));
    const int rcp = prepare(w, n > m ? (n > b ? n : b) : (m > b ? m : b));
    if (rcp != ROITR_OK) return rcp;
    ROITR_LAUNCH_CHECK();
    const RoitrGridView gv = roitr_knn_grid_view(b, m, 0, w.knn);
    if (m > 0) {
        const int rc = roitr_knn_build_grid_ex(b, m, 0, w.clean, tgt_offset, w.knn, 0.f, stream);
        if (rc != ROITR_OK) return rc;
    }
    icp_start_kernel<NSTAT><<<div_up(b, ICP_THREADS), ICP_THREADS, 0, stream>>>(b, iterations, init_T, w.state, w.active, w.prev, o);
    ROITR_LAUNCH_CHECK();
    // n == 0 or m == 0: every pair carries EMPTY, nothing is active and no lane reads the (unbuilt) grid
    for (int s = 0; s <= iterations && n > 0 && m > 0; ++s) {
        icp_match_kernel<<<div_up(n, ICP_THREADS), ICP_THREADS, 0, stream>>>(b, n, src, src_offset, tgt, tgt_offset, w.state, w.active,
                                                                            (double)max_dist, gv.grids, gv.cell_start, gv.sorted, match, w.d2);
        update(w, match, s);
        ROITR_LAUNCH_CHECK();
    }
    return ROITR_OK;
}

}  // namespace
