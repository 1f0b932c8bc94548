// RANSAC-free registration: GeoTransformer's local-to-global registration (LGR) on the patch
// structure of the coarse-to-fine matcher.  The rules are stated in include/roitr_engine.h above roitr_lgr_batch.
//
// Pair b owns rows [starts[b], starts[b + 1]) of src / tgt / scores / row_patch.  Its hypotheses live in the workspace at slots
// [starts[b] / min_rows, starts[b] / min_rows + hypotheses[b]): a pair of n rows has at most n / min_rows of them, so the slot
// ranges of different pairs never meet and nobody has to scan over the pairs.  Three launches on the caller's stream:
//   lgr_local_kernel    one block per pair: run heads compacted in row order, the runs of at least min_rows rows compacted into
//                       hypotheses, their float64 moments by groups of 16 lanes (16 hypotheses per block pass), then one lane per
//                       hypothesis for the Jacobi solve (every lane live, where one lane per group would leave 15 of 16 idle);
//   lgr_verify_kernel   one block per LG_ROWS rows of the concatenated row array: the rows are staged in LDS once and every
//                       hypothesis of the pair(s) they belong to is scored against them, one hypothesis per lane with its transform
//                       in registers, the rows read as broadcasts; integer counts are added into the workspace;
//   lgr_global_kernel   one block per pair: arg-max of the counts (ties: lower number), then `steps` reweighted solves over the
//                       pair's rows and the final count.
// The verification grid is rows-only because the host does not know a pair's hypothesis count without a round trip: a grid of
// (hypothesis chunks x row chunks x pairs) would have to be sized for the worst pair in both dimensions.  Counts are integers, so
// the chunk borders (global row positions) cannot change a result.  Every float64 sum is a strided per-lane sum over the local
// row index followed by a fixed butterfly, so it depends on the pair's (the run's) own rows only.
// The bodies of the last two kernels are verify_tile, block_winner, global_refit and write_T44 of procrustes_block.h, which compat.hip
// calls too: the kernels here say where a pair's hypothesis slots are, form the winner key and write this operator's outputs.
#include "common.h"
#include "procrustes_block.h"
#include "registration_math.h"
#include "roitr_engine.h"
#include "workspace.h"

namespace {

struct LgWorkspace {
    int* run_first;    // (total_rows) local first row of every run, pair b's at [starts[b], ...)
    int* hyp_first;    // (cap) local first row of the hypothesis's run
    int* hyp_len;      // (cap) rows of that run
    int* hyp_count;    // (cap) inliers over the pair's rows
    float* hyp_T;      // (cap, 12)
    double* moments;   // (cap, 15) cs, ct, H of the local solve
    size_t bytes;
};

LgWorkspace carve(void* ws, int total_rows)
{
    const size_t cap = (size_t)total_rows / 3;   // min_rows >= 3
    Carve c(ws);
    LgWorkspace w;
    w.run_first = c.take<int>(total_rows);
    w.hyp_first = c.take<int>(cap);
    w.hyp_len = c.take<int>(cap);
    w.hyp_count = c.take<int>(cap);
    w.hyp_T = c.take<float>(12 * cap);
    w.moments = c.take<double>(15 * cap);
    w.bytes = c.bytes;
    return w;
}

__global__ __launch_bounds__(LG_THREADS) void lgr_local_kernel(const int* __restrict__ starts, int total_rows,
                                                               const float* __restrict__ src, const float* __restrict__ tgt,
                                                               const float* __restrict__ scores, const int* __restrict__ row_patch,
                                                               int min_rows, LgWorkspace ws, int* __restrict__ hypotheses)
{
    __shared__ int wsum[LG_THREADS / 64];
    __shared__ int carry;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int2 rg = starts_range(starts, b, total_rows);
    const int s = rg.x, n = rg.y - rg.x;
    const int hb = s / min_rows;
    int* rf = ws.run_first + s;
    // run heads, in row order
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int j0 = 0; j0 < n; j0 += LG_THREADS) {
        const int j = j0 + tid;
        const bool head = j < n && (j == 0 || row_patch[s + j] != row_patch[s + j - 1]);
        const int end = block_running_scan<LG_THREADS>(head ? 1 : 0, wsum, &carry);
        if (head) rf[end - 1] = j;
    }
    const int nruns = carry;
    __syncthreads();   // everybody has read the run count, and the heads (global memory, same block) are visible
    if (tid == 0) carry = 0;
    __syncthreads();
    // runs of at least min_rows rows, in row order
    for (int j0 = 0; j0 < nruns; j0 += LG_THREADS) {
        const int j = j0 + tid;
        int first = 0, len = 0;
        if (j < nruns) { first = rf[j]; len = (j + 1 < nruns ? rf[j + 1] : n) - first; }
        const bool hyp = len >= min_rows;
        const int end = block_running_scan<LG_THREADS>(hyp ? 1 : 0, wsum, &carry);
        if (hyp) { ws.hyp_first[hb + end - 1] = first; ws.hyp_len[hb + end - 1] = len; ws.hyp_count[hb + end - 1] = 0; }
    }
    const int H = carry;
    __syncthreads();
    // moments: one group of LG_GROUP lanes per hypothesis.  A group without one runs on an empty run, so that no shuffle is divergent.
    const int g = tid / LG_GROUP, l = tid % LG_GROUP;
    for (int h0 = 0; h0 < H; h0 += LG_THREADS / LG_GROUP) {
        const int h = h0 + g;
        const bool live = h < H;
        const int first = live ? ws.hyp_first[hb + h] : 0, len = live ? ws.hyp_len[hb + h] : 0;
        auto row = [&](int j, float (&p)[3], float (&q)[3], float& w) {
            const size_t r = (size_t)(s + first + j);
            p[0] = src[3 * r]; p[1] = src[3 * r + 1]; p[2] = src[3 * r + 2];
            q[0] = tgt[3 * r]; q[1] = tgt[3 * r + 1]; q[2] = tgt[3 * r + 2];
            w = scores ? scores[r] : 1.0f;
        };
        double a[7], cs[3], ct[3], Hm[9];
        moments_first(len, l, LG_GROUP, row, a);
#pragma unroll
        for (int k = 0; k < 7; ++k) a[k] = lanes_sum_d<LG_GROUP>(a[k]);
        centroids(a, cs, ct);
        moments_second(len, l, LG_GROUP, row, cs, ct, Hm);
#pragma unroll
        for (int k = 0; k < 9; ++k) Hm[k] = lanes_sum_d<LG_GROUP>(Hm[k]);
        if (live && l == 0) {
            double* m = ws.moments + 15 * (size_t)(hb + h);
#pragma unroll
            for (int k = 0; k < 3; ++k) { m[k] = cs[k]; m[3 + k] = ct[k]; }
#pragma unroll
            for (int k = 0; k < 9; ++k) m[6 + k] = Hm[k];
        }
    }
    __syncthreads();
    // solves: one hypothesis per lane
    for (int h = tid; h < H; h += LG_THREADS) {
        const double* m = ws.moments + 15 * (size_t)(hb + h);
        const double cs[3] = {m[0], m[1], m[2]}, ct[3] = {m[3], m[4], m[5]};
        const double Hm[9] = {m[6], m[7], m[8], m[9], m[10], m[11], m[12], m[13], m[14]};
        float T[12];
        rg_solve_rigid(Hm, cs, ct, T);
        float* o = ws.hyp_T + 12 * (size_t)(hb + h);
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = T[k];
    }
    if (tid == 0) hypotheses[b] = H;
}

__global__ __launch_bounds__(LG_THREADS) void lgr_verify_kernel(int pairs, const int* __restrict__ starts, int total_rows,
                                                                const float* __restrict__ src, const float* __restrict__ tgt,
                                                                int min_rows, LgWorkspace ws, const int* __restrict__ hypotheses,
                                                                float thr2)
{
    auto slots = [&](int p, int first_row) { return HypSlots<int>{hypotheses[p], first_row / min_rows}; };
    verify_tile<false>(pairs, starts, total_rows, src, tgt, slots, ws.hyp_T, ws.hyp_count, thr2);
}

__global__ __launch_bounds__(LG_THREADS) void lgr_global_kernel(const int* __restrict__ starts, int total_rows,
                                                                const float* __restrict__ src, const float* __restrict__ tgt,
                                                                const float* __restrict__ scores, int min_rows, int steps, float thr2,
                                                                LgWorkspace ws, const int* __restrict__ hypotheses,
                                                                float* __restrict__ T_out, int* __restrict__ inliers,
                                                                int* __restrict__ best_hypothesis, int* __restrict__ best_first_row,
                                                                int* __restrict__ local_inliers, int* __restrict__ status,
                                                                int* __restrict__ hyp_starts, int* __restrict__ hyp_first_row,
                                                                float* __restrict__ hyp_transforms, int* __restrict__ hyp_counts)
{
    __shared__ double red[4 * 9];
    __shared__ unsigned long long redk[LG_THREADS / 64];
    __shared__ int red4[4];
    __shared__ float Ts[12];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int2 rg = starts_range(starts, b, total_rows);
    const int s = rg.x, n = rg.y - rg.x;
    const int H = hypotheses[b], hb = s / min_rows;
    // winner: most inliers, the lower number at equal counts = the largest (count, ~number) key
    unsigned long long key = 0;
    for (int h = tid; h < H; h += LG_THREADS) {
        const unsigned long long k = ((unsigned long long)(unsigned)ws.hyp_count[hb + h] << 32) | (unsigned)(0x7fffffff - h);
        key = k > key ? k : key;
    }
    key = block_winner(key, redk);
    const int best = H > 0 ? 0x7fffffff - (int)(unsigned)(key & 0xffffffffu) : -1;
    if (hyp_starts) {
        if (tid == 0) hyp_starts[b] = hb;
        if (tid == 0 && b == (int)gridDim.x - 1) hyp_starts[b + 1] = rg.y / min_rows;
    }
    for (int h = tid; h < H; h += LG_THREADS) {
        if (hyp_first_row) hyp_first_row[hb + h] = ws.hyp_first[hb + h];
        if (hyp_counts) hyp_counts[hb + h] = ws.hyp_count[hb + h];
        if (hyp_transforms)
            for (int k = 0; k < 12; ++k) hyp_transforms[12 * (size_t)(hb + h) + k] = ws.hyp_T[12 * (size_t)(hb + h) + k];
    }

    float T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    int local, final_count;
    const bool won = best >= 0;
    const int st = global_refit(s, n, src, tgt, scores, steps, thr2, won ? ws.hyp_T + 12 * (size_t)(hb + best) : nullptr,
                                won ? ws.hyp_count + hb + best : nullptr, T, local, final_count, red, red4, Ts);
    write_T44(T_out + 16 * (size_t)b, T);
    if (tid == 0) {
        inliers[b] = final_count;
        best_hypothesis[b] = best;
        best_first_row[b] = best >= 0 ? ws.hyp_first[hb + best] : -1;
        local_inliers[b] = local;
        status[b] = st;
    }
}

}  // namespace

extern "C" size_t roitr_lgr_workspace_bytes(int pairs, int total_rows)
{
    if (pairs <= 0 || total_rows < 0) return 0;
    return carve(nullptr, total_rows).bytes;
}

extern "C" int roitr_lgr_batch(int pairs, const int* starts, int total_rows, const float* src_pts, const float* tgt_pts,
                               const float* scores, const int* row_patch, float radius, int min_rows, int steps, void* workspace,
                               size_t workspace_bytes_given, float* transforms, int* inliers, int* best_hypothesis,
                               int* best_first_row, int* hypotheses, int* local_inliers, int* status, int* hyp_starts,
                               int* hyp_first_row, float* hyp_transforms, int* hyp_counts, hipStream_t stream)
{
    if (!(radius > 0.f) || !(radius <= 3.402823466e38f)) return refuse(ROITR_ERR_ARG, "roitr_lgr_batch: radius must be finite and positive");
    if (min_rows < 3) return refuse(ROITR_ERR_ARG, "roitr_lgr_batch: min_rows < 3");
    if (steps < 1) return refuse(ROITR_ERR_ARG, "roitr_lgr_batch: steps < 1");
    if (pairs <= 0) return ROITR_OK;
    if (total_rows < 0 || pairs > 65535) return refuse(ROITR_ERR_ARG, "roitr_lgr_batch: total_rows < 0 or pairs > 65535");
    if (!starts || !transforms || !inliers || !best_hypothesis || !best_first_row || !hypotheses || !local_inliers || !status ||
        (total_rows > 0 && (!src_pts || !tgt_pts || !row_patch)))
        return refuse(ROITR_ERR_ARG, "roitr_lgr_batch: null pointer");
    const LgWorkspace ws = carve(workspace, total_rows);
    if (workspace_bytes_given < ws.bytes || (ws.bytes > 0 && !workspace))
        return refuse(ROITR_ERR_ARG, "roitr_lgr_batch: workspace smaller than roitr_lgr_workspace_bytes()");
    const float thr2 = radius * radius;
    lgr_local_kernel<<<pairs, LG_THREADS, 0, stream>>>(starts, total_rows, src_pts, tgt_pts, scores, row_patch, min_rows, ws, hypotheses);
    ROITR_LAUNCH_CHECK();
    if (total_rows > 0) {
        lgr_verify_kernel<<<div_up(total_rows, LG_ROWS), LG_THREADS, 0, stream>>>(pairs, starts, total_rows, src_pts, tgt_pts, min_rows,
                                                                                 ws, hypotheses, thr2);
        ROITR_LAUNCH_CHECK();
    }
    lgr_global_kernel<<<pairs, LG_THREADS, 0, stream>>>(starts, total_rows, src_pts, tgt_pts, scores, min_rows, steps, thr2, ws,
                                                        hypotheses, transforms, inliers, best_hypothesis, best_first_row, local_inliers,
                                                        status, hyp_starts, hyp_first_row, hyp_transforms, hyp_counts);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}
