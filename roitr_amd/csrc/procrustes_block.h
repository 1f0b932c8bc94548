// Device pieces shared by the two hypothesis estimators (lgr.hip, compat.hip).  The weighted solve `Solve` that include/roitr_engine.h
// states above roitr_lgr_batch: float64 moments as strided per-lane sums over a local row index, the fixed butterflies that fold them
// over a lane group or a block of 256, and the centroids with the reference's eps.  Every sum has one order, so a result depends on
// the rows it is given and on nothing else.  And the stages both estimators end with, whose __global__ kernels are shells around them:
// verify_tile (every hypothesis against a 512-row tile), block_winner, global_refit (start, `steps` reweighted solves, final count)
// and write_T44.
#pragma once
#include "common.h"
#include "registration_math.h"
#include "roitr_engine.h"

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
// (registration.hip has a block_sum_d of its own, an LDS tree that folds in another order: unifying the two would change result bits)
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

// sum over the 64 lanes of a wave, in every lane
__device__ __forceinline__ int wave_sum_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int block_sum_i(int v, int* red)   // red: 4 ints
{
    v = wave_sum_i(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// block maximum of one double per thread, every thread gets it (fgr.hip, posegraph.hip)
__device__ __forceinline__ double block_max_d(double v, double* red)   // red: 4 doubles; a maximum has no order
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
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

// ------------------------------------------------------------------------------------------------------------------ shared stages
// The whole verification kernel: the block's LG_ROWS rows of the concatenated array staged in LDS once, then every hypothesis of the
// pair(s) that own some of them scored against them, one hypothesis per lane with its transform in registers, the rows read as
// broadcasts; integer counts are added into hyp_count.  slots(p, first_row) says where pair p's hypotheses live: {H, base}, slots
// [base, base + H) of hyp_T / hyp_count.  SKIP_NEGATIVE: a slot whose count is negative is invalid and stays as it is.
template <class Base>
struct HypSlots { int H; Base base; };

template <bool SKIP_NEGATIVE, class Slots>
__device__ __forceinline__ void verify_tile(int pairs, const int* __restrict__ starts, int total_rows, const float* __restrict__ src,
                                            const float* __restrict__ tgt, Slots slots, const float* hyp_T, int* hyp_count, float thr2)
{
    __shared__ float4 ts[LG_ROWS], tt[LG_ROWS];
    const int row0 = blockIdx.x * LG_ROWS, m = min(LG_ROWS, total_rows - row0);
    if (row0 >= starts[pairs]) return;   // capacity rows behind the last pair (the engine's buffers are sized for the worst case)
    for (int j = threadIdx.x; j < m; j += LG_THREADS) {
        const size_t r = (size_t)(row0 + j);
        ts[j] = make_float4(src[3 * r], src[3 * r + 1], src[3 * r + 2], 0.f);
        tt[j] = make_float4(tgt[3 * r], tgt[3 * r + 1], tgt[3 * r + 2], 0.f);
    }
    __syncthreads();
    // the last pair that starts at or before row0 (pair 0 if none does), then every pair that starts inside the block's rows
    int lo = 0, hi = pairs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= row0) lo = mid; else hi = mid - 1;
    }
    for (int p = lo; p < pairs; ++p) {
        const int2 rg = starts_range(starts, p, total_rows);
        if (rg.x >= row0 + m) break;
        const int j0 = max(rg.x, row0) - row0, j1 = min(rg.y, row0 + m) - row0;
        if (j1 <= j0) continue;
        const auto sl = slots(p, rg.x);
        for (int h = threadIdx.x; h < sl.H; h += LG_THREADS) {
            if (SKIP_NEGATIVE && hyp_count[sl.base + h] < 0) continue;   // a valid count only grows from 0
            float T[12];
            const float* Th = hyp_T + 12 * (size_t)(sl.base + h);
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = Th[k];
            int cnt = 0;
#pragma unroll 4
            for (int j = j0; j < j1; ++j) {
                const float4 a = ts[j], q = tt[j];
                cnt += rg_dist2(T, a.x, a.y, a.z, q.x, q.y, q.z) < thr2;
            }
            if (cnt) atomicAdd(hyp_count + sl.base + h, cnt);
        }
    }
}

// block maximum of one 64-bit key per thread (the winner: the largest (count, ~number)); redk: 4 words
__device__ __forceinline__ unsigned long long block_winner(unsigned long long key, unsigned long long* redk)
{
    key = wave_max_u64(key);
    if ((threadIdx.x & 63) == 0) redk[threadIdx.x >> 6] = key;
    __syncthreads();
    return max(max(redk[0], redk[1]), max(redk[2], redk[3]));
}

// The status bits global_refit returns: the values both operators give them (ROITR_COMPAT_TRUNCATED, 8, is compat's own).
constexpr int REFIT_NO_ROWS = 1, REFIT_NO_START = 2, REFIT_EMPTY = 4;
static_assert(ROITR_LGR_NO_ROWS == REFIT_NO_ROWS && ROITR_LGR_NO_LOCAL == REFIT_NO_START && ROITR_LGR_EMPTY_REFIT == REFIT_EMPTY, "");
static_assert(ROITR_COMPAT_NO_ROWS == REFIT_NO_ROWS && ROITR_COMPAT_NO_HYPOTHESIS == REFIT_NO_START &&
              ROITR_COMPAT_EMPTY_REFIT == REFIT_EMPTY, "");

// The global stage of a pair of rows [s, s + n), by its whole block: from the winner's transform T0 and count *local0 (both null: no
// hypothesis, GeoTransformer's degenerate branch: start from all rows under their scores), `steps` solves over all rows with the
// weights score x [inlier under T], then the count under the last T.  A solve whose weights sum to 0 keeps T and ends the loop.
// T comes in as the identity, which a pair without rows keeps.  Returns the status bits.  red: 4 * 9 doubles, red4: 4 ints, Ts: 12
// floats (LDS).
__device__ __forceinline__ int global_refit(int s, int n, const float* __restrict__ src, const float* __restrict__ tgt,
                                            const float* __restrict__ scores, int steps, float thr2, const float* T0, const int* local0,
                                            float (&T)[12], int& local, int& final_count, double* red, int* red4, float* Ts)
{
    const int tid = threadIdx.x;
    local = 0; final_count = 0;
    auto count_under = [&](const float (&Tc)[12]) {
        int c = 0;
        for (int j = tid; j < n; j += LG_THREADS) {
            const size_t r = (size_t)(s + j);
            c += rg_dist2(Tc, src[3 * r], src[3 * r + 1], src[3 * r + 2], tgt[3 * r], tgt[3 * r + 1], tgt[3 * r + 2]) < thr2;
        }
        return block_sum_i(c, red4);
    };
    // one solve over all rows of the pair, weights score x [inlier under Tc] (gate) or the score alone; false: the weights sum to 0
    auto solve = [&](const float (&Tc)[12], bool gate, float (&Tn)[12]) {
        auto row = [&](int j, float (&p)[3], float (&q)[3], float& w) {
            const size_t r = (size_t)(s + j);
            p[0] = src[3 * r]; p[1] = src[3 * r + 1]; p[2] = src[3 * r + 2];
            q[0] = tgt[3 * r]; q[1] = tgt[3 * r + 1]; q[2] = tgt[3 * r + 2];
            const bool in = !gate || rg_dist2(Tc, p[0], p[1], p[2], q[0], q[1], q[2]) < thr2;
            w = in ? (scores ? scores[r] : 1.0f) : 0.f;
        };
        double a[7], cs[3], ct[3], Hm[9];
        moments_first(n, tid, LG_THREADS, row, a);
        block_sum_d<7>(a, red);
        if (a[0] == 0.0) return false;
        centroids(a, cs, ct);
        moments_second(n, tid, LG_THREADS, row, cs, ct, Hm);
        block_sum_d<9>(Hm, red);
        // every lane holds the same moments: one wave solves, the others leave the float64 pipe to the block next door
        if (tid < 64) {
            rg_solve_rigid(Hm, cs, ct, Tn);
            if (tid == 0)
#pragma unroll
                for (int k = 0; k < 12; ++k) Ts[k] = Tn[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 12; ++k) Tn[k] = Ts[k];
        return true;
    };
    if (n == 0) return REFIT_NO_ROWS;
    int st = 0;
    bool alive = true;
    if (T0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = T0[k];
        local = *local0;
    } else {
        st |= REFIT_NO_START;
        float Tn[12];
        alive = solve(T, false, Tn);
        if (alive) {
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = Tn[k];
            local = count_under(T);
        }
    }
    for (int k = 0; k < steps && alive; ++k) {
        const float Tc[12] = {T[0], T[1], T[2], T[3], T[4], T[5], T[6], T[7], T[8], T[9], T[10], T[11]};
        float Tn[12];
        alive = solve(Tc, true, Tn);
        if (alive) {
#pragma unroll
            for (int i = 0; i < 12; ++i) T[i] = Tn[i];
        }
    }
    if (!alive) st |= REFIT_EMPTY;
    final_count = count_under(T);
    return st;
}

// T (4,4) of one pair from the 12 values of [R | t], by 16 lanes
__device__ __forceinline__ void write_T44(float* __restrict__ out, const float (&T)[12])
{
    const int tid = threadIdx.x;
    if (tid < 16) {
        const int r = tid >> 2, c = tid & 3;
        float v = r == 3 ? (c == 3 ? 1.f : 0.f) : 0.f;
#pragma unroll
        for (int k = 0; k < 12; ++k) v = (r < 3 && k == 4 * r + c) ? T[k] : v;
        out[tid] = v;
    }
}

}  // namespace
