// Validation losses: the forward values of lib/loss.py:8-166 (weighted_circle_loss,
// CoarseMatchingLoss, FineMatchingLoss), batched over the pairs of one engine call, on the engine's output buffers in place.
//
// Fine loss, lib/loss.py:119-143 per patch: src' = src R^T + t, gt[i][j] = (|tgt_i - src'_j|^2 < r^2) & tgt_mask[i] & src_mask[j],
// a slack-row label where a valid tgt row has no gt, a slack-column label likewise, loss = -mean of the labelled matching_scores.
//   fine_patch_kernel    one wave per patch slot, laid flat over the slots; the pair of a slot is found by binary search over the
//                        first-slot array (dead slots leave at once).  Lane i keeps target point i in registers and stages the
//                        transformed source point i in LDS (1 KB; with the label rows 1.8 KB at any L); it builds its 64-bit row of
//                        the gt map from fp32 DIFFERENCE-form distances (common.h sqdist3, as nfmr_anchor_kernel: the reference's
//                        |a|^2 + |b|^2 - 2ab only exists to feed a matmul and cancels at metre-scale coordinates against
//                        r^2 = 0.0025); the column "any" is an OR butterfly.  The (L+1)^2 scores are then read ONCE with coalesced
//                        dword loads along the rows (rows of L+1 floats are not 16-byte aligned, and the order of the sum must not
//                        depend on the slot's address) and summed where labelled: per lane in element order, then the fixed DPP
//                        tree.  One (sum, count) partial per slot.
//   fine_reduce_kernel   one block per pair adds the pair's partials: thread k takes partials k, k + 256, ... of the PAIR (not of the
//                        call) in float64, then a fixed LDS tree.  No float atomics anywhere: every output is bitwise independent of
//                        the batch, of the slot a patch sits in and of repeats.  The search needs the ranges in increasing order:
//                        every block checks the whole list, and one range out of order or overlapping empties and flags ALL pairs.
//
// Coarse loss, lib/loss.py:8-49, 88-111 per pair (n_t x n_s node pairs, D-wide descriptors):
//   coarse_dist_kernel     feat_dists = sqrt(max((-2 t.s + |t|^2) + |s|^2, 1e-12)) (square_distance's order), 64 x 64 tiles, fp32 FMA
//                          in k order from LDS, 4 x 4 per thread;
//   coarse_scatter_kernel  overlaps[gt_t, gt_s] = gt_overlap as the LIST INDEX of the entry (atomicMax on an int matrix preset to -1:
//                          the last entry of a repeated node pair wins, as a sequential index_put does; deterministic);
//   coarse_row_kernel      one wave per target row: pos = overlap > positive_overlap, neg = overlap == 0, the two weights, and the
//                          log-sum-exp of both terms with a running maximum (a non-positive entry contributes exp(0) to the positive
//                          sum and likewise for negatives: the reference's -1e5 masking), lanes merged by a symmetric butterfly;
//   coarse_col_kernel      one lane per source column, the rows in four contiguous quarters merged in order;
//   coarse_final_kernel    softplus was applied per row / column; the masked means over rows and columns in float64, fixed tree.
// Ranges and indices are checked before anything is read through them; a bad range empties the pair and sets a status bit.
#include "common.h"
#include "roitr_engine.h"
#include "workspace.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------ fine loss

// pair b's slots [first[b], first[b] + count[b]) must lie in [0, slots) (common.h count_bad) and behind pair b - 1's: what the
// binary search of fine_patch_kernel stands on
__device__ __forceinline__ bool fl_unordered(const int* __restrict__ first, const int* __restrict__ count, int b)
{
    return b > 0 && first[b] < (long long)first[b - 1] + max(count[b - 1], 0);
}

__global__ __launch_bounds__(64) void fine_patch_kernel(int pairs, int slots, const int* __restrict__ first, const int* __restrict__ count,
                                                        const float* __restrict__ tgt_pts, const float* __restrict__ src_pts,
                                                        const int* __restrict__ tgt_masks, const int* __restrict__ src_masks,
                                                        const float* __restrict__ scores, const float* __restrict__ rot,
                                                        const float* __restrict__ trans, float r2, int L, float* __restrict__ part_sum,
                                                        int* __restrict__ part_cnt)
{
    __shared__ float4 s_src[64];
    __shared__ unsigned long long s_row[65];   // row i < L: bit j = label (i, j); row L: bit j = slack-column label of column j
    __shared__ int s_slack[65];                // label (i, L); 0 for row L
    const int s = blockIdx.x, lane = threadIdx.x;
    int lo = 0, hi = pairs - 1;   // the last pair whose first slot is not beyond s (empty pairs share their successor's first slot)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= s) lo = mid; else hi = mid - 1;
    }
    const int b = lo;
    const int f = first[b];
    if (s < f || s - f >= count[b] || count_bad(first, count, b, slots)) return;   // block-uniform: a dead slot, never summed
    const float* R = rot + (size_t)b * 9;
    const float* t = trans + (size_t)b * 3;
    bool sm = false, tm = false;
    float sx = 0.f, sy = 0.f, sz = 0.f, tx = 0.f, ty = 0.f, tz = 0.f;
    if (lane < L) {
        const size_t row = (size_t)s * L + lane;
        const float x = src_pts[row * 3], y = src_pts[row * 3 + 1], z = src_pts[row * 3 + 2];
        // src @ rot.T + trans.T: row i of rot dotted with the point, fp32 FMA chain in k order (as eval.hip)
        sx = fmaf(z, R[2], fmaf(y, R[1], x * R[0])) + t[0];
        sy = fmaf(z, R[5], fmaf(y, R[4], x * R[3])) + t[1];
        sz = fmaf(z, R[8], fmaf(y, R[7], x * R[6])) + t[2];
        sm = src_masks[row] != 0;
        tx = tgt_pts[row * 3]; ty = tgt_pts[row * 3 + 1]; tz = tgt_pts[row * 3 + 2];
        tm = tgt_masks[row] != 0;
    }
    s_src[lane] = make_float4(sx, sy, sz, 0.f);
    const unsigned long long smask = __ballot(sm);
    __syncthreads();
    unsigned long long row = 0;
    for (int j = 0; j < L; ++j) {
        const float4 v = s_src[j];   // every lane reads the same address: a broadcast
        row |= (unsigned long long)(sqdist3(tx, ty, tz, v.x, v.y, v.z) < r2 ? 1 : 0) << j;
    }
    row = tm ? row & smask : 0ull;
    unsigned long long any = row;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) any |= __shfl_xor(any, o, 64);
    const bool slack_row = tm && row == 0ull;
    const unsigned long long slack_col = smask & ~any;
    if (lane < L) { s_row[lane] = row; s_slack[lane] = slack_row ? 1 : 0; }
    if (lane == 0) { s_row[L] = slack_col; s_slack[L] = 0; }
    int cnt = (int)wave_sum((float)(__popcll(row) + (slack_row ? 1 : 0)));   // exact: at most 65 * 64
    cnt += __popcll(slack_col);
    __syncthreads();
    const int W = L + 1, n = W * W;
    const float* sc = scores + (size_t)s * n;
    const int q = 64 / W, r = 64 % W;
    int ri = lane / W, ci = lane % W;
    float acc = 0.f;
#pragma unroll 4
    for (int e = lane; e < n; e += 64) {
        const float v = sc[e];
        const bool lab = ci < L ? ((s_row[ri] >> ci) & 1ull) != 0ull : s_slack[ri] != 0;
        acc += lab ? v : 0.f;
        ci += r; ri += q;
        if (ci >= W) { ci -= W; ++ri; }
    }
    acc = wave_sum(acc);
    if (lane == 0) { part_sum[s] = acc; part_cnt[s] = cnt; }
}

__global__ __launch_bounds__(256) void fine_reduce_kernel(int pairs, int slots, const int* __restrict__ first, const int* __restrict__ count,
                                                          const float* __restrict__ part_sum, const int* __restrict__ part_cnt,
                                                          float* __restrict__ f_sum, int* __restrict__ f_count, float* __restrict__ f_loss,
                                                          int* __restrict__ status)
{
    __shared__ double s_sum[256];
    __shared__ int s_cnt[256];
    const int b = blockIdx.x;
    int unordered = 0;   // anywhere in the call: a slot may then have been resolved to another pair and its partial left unwritten
    for (int p = threadIdx.x; p < pairs; p += 256) unordered |= fl_unordered(first, count, p) ? 1 : 0;
    const bool bad = __syncthreads_or(unordered) != 0 || count_bad(first, count, b, slots);
    const int f = bad ? 0 : first[b], c = bad ? 0 : count[b];
    double acc = 0.0;
    int cnt = 0;
    for (int k = threadIdx.x; k < c; k += 256) { acc += (double)part_sum[f + k]; cnt += part_cnt[f + k]; }
    s_sum[threadIdx.x] = acc; s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { s_sum[threadIdx.x] += s_sum[threadIdx.x + o]; s_cnt[threadIdx.x] += s_cnt[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double tot = s_sum[0];
        const int n = s_cnt[0];
        f_sum[b] = (float)tot;
        f_count[b] = n;
        f_loss[b] = n > 0 ? (float)(-tot / (double)n) : NAN;   // the reference's mean of an empty selection
        status[b] = (bad ? ROITR_LOSS_BAD_OFFSETS : 0) | (n > 0 ? 0 : ROITR_LOSS_FINE_EMPTY);
    }
}

// ------------------------------------------------------------------------------------------------ coarse loss

constexpr int CT = 64;   // tile edge of the distance kernel
constexpr int CK = 16;   // k per LDS chunk

struct CircleConst { float pos_margin, neg_margin, pos_optimal, neg_optimal, log_scale, pos_overlap; };

__global__ __launch_bounds__(256) void coarse_dist_kernel(int D, const float* __restrict__ tgt_feats, int total_t, const int* __restrict__ t_first,
                                                          const int* __restrict__ t_count, const float* __restrict__ src_feats, int total_s,
                                                          const int* __restrict__ s_first, const int* __restrict__ s_count, int max_t, int max_s,
                                                          float* __restrict__ dist)
{
    __shared__ __align__(16) float At[CK][CT + 4];
    __shared__ __align__(16) float Bt[CK][CT + 4];
    __shared__ float s_nt[CT], s_ns[CT];
    const int b = blockIdx.z;
    const int2 tr = count_range(t_first, t_count, b, total_t, max_t), sr = count_range(s_first, s_count, b, total_s, max_s);
    const int i0 = blockIdx.y * CT, j0 = blockIdx.x * CT;
    if (i0 >= tr.y || j0 >= sr.y) return;   // block-uniform
    const int tid = threadIdx.x, lr = tid >> 2, kq = tid & 3, ty = tid >> 4, tx = tid & 15;
    float acc[4][4] = {};
    float nrm = 0.f;   // threads 0..63: |t_row|^2, threads 64..127: |s_row|^2, k in order
    for (int k0 = 0; k0 < D; k0 += CK) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
        if (k0 + kq * 4 < D) {   // D % 4 == 0: a whole float4 or nothing
            if (i0 + lr < tr.y) a = *(const float4*)(tgt_feats + (size_t)(tr.x + i0 + lr) * D + k0 + kq * 4);
            if (j0 + lr < sr.y) c = *(const float4*)(src_feats + (size_t)(sr.x + j0 + lr) * D + k0 + kq * 4);
        }
        __syncthreads();   // the previous chunk has been read
        At[kq * 4][lr] = a.x; At[kq * 4 + 1][lr] = a.y; At[kq * 4 + 2][lr] = a.z; At[kq * 4 + 3][lr] = a.w;
        Bt[kq * 4][lr] = c.x; Bt[kq * 4 + 1][lr] = c.y; Bt[kq * 4 + 2][lr] = c.z; Bt[kq * 4 + 3][lr] = c.w;
        __syncthreads();
        if (tid < 2 * CT) {
            const float (*M)[CT + 4] = tid < CT ? At : Bt;
#pragma unroll
            for (int k = 0; k < CK; ++k) { const float x = M[k][tid & (CT - 1)]; nrm = fmaf(x, x, nrm); }
        }
#pragma unroll
        for (int k = 0; k < CK; ++k) {
            const float4 av = *(const float4*)&At[k][ty * 4];
            const float4 bv = *(const float4*)&Bt[k][tx * 4];
            const float ar[4] = {av.x, av.y, av.z, av.w}, br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(ar[u], br[v], acc[u][v]);
        }
    }
    if (tid < CT) s_nt[tid] = nrm;
    else if (tid < 2 * CT) s_ns[tid - CT] = nrm;
    __syncthreads();
    float* out = dist + (size_t)b * max_t * max_s;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = i0 + ty * 4 + u;
        if (i >= tr.y) continue;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = j0 + tx * 4 + v;
            if (j >= sr.y) continue;
            const float d2 = (-2.0f * acc[u][v] + s_nt[ty * 4 + u]) + s_ns[tx * 4 + v];   // square_distance's order
            out[(size_t)i * max_s + j] = sqrtf(fmaxf(d2, 1e-12f));
        }
    }
}

// one thread per pair: the status word the later kernels OR into
__global__ __launch_bounds__(256) void coarse_status_kernel(int pairs, int total_t, const int* __restrict__ t_first, const int* __restrict__ t_count,
                                                            int total_s, const int* __restrict__ s_first, const int* __restrict__ s_count,
                                                            int max_t, int max_s, int* __restrict__ status)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= pairs) return;
    status[b] = count_bad(t_first, t_count, b, total_t, max_t) || count_bad(s_first, s_count, b, total_s, max_s) ? ROITR_LOSS_BAD_OFFSETS : 0;
}

__global__ __launch_bounds__(256) void coarse_scatter_kernel(int gt_cap, const int* __restrict__ gt_idx, const int* __restrict__ gt_count,
                                                             int total_t, const int* __restrict__ t_first, const int* __restrict__ t_count,
                                                             int total_s, const int* __restrict__ s_first, const int* __restrict__ s_count,
                                                             int max_t, int max_s, int* __restrict__ slot, int* __restrict__ status)
{
    const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= min(gt_count[b], gt_cap)) return;
    const int nt = count_range(t_first, t_count, b, total_t, max_t).y, ns = count_range(s_first, s_count, b, total_s, max_s).y;
    const int i = gt_idx[((size_t)b * gt_cap + e) * 2], j = gt_idx[((size_t)b * gt_cap + e) * 2 + 1];
    if (i < 0 || i >= nt || j < 0 || j >= ns) { atomicOr(status + b, ROITR_LOSS_BAD_INDEX); return; }   // never dereferenced
    atomicMax(slot + (size_t)b * max_t * max_s + (size_t)i * max_s + j, e);
}

// log-sum-exp with a running maximum: (m, s) stands for m + log(s)
struct Lse {
    float m, s;
    __device__ __forceinline__ void add(float x)
    {
        if (x > m) { s = s * expf(m - x) + 1.0f; m = x; }
        else s += expf(x - m);
    }
    // symmetric in its two sides bit for bit: both products are rounded before the (commutative) addition, no FMA contraction
    __device__ __forceinline__ void merge(float om, float os)
    {
        const float mm = fmaxf(m, om);
        if (mm == -INFINITY) return;   // both empty
        s = __fadd_rn(__fmul_rn(s, expf(m - mm)), __fmul_rn(os, expf(om - mm)));
        m = mm;
    }
};

struct CircleAcc {
    Lse pos, neg;
    bool any_pos, any_neg;
    __device__ __forceinline__ void init() { pos.m = neg.m = -INFINITY; pos.s = neg.s = 0.f; any_pos = any_neg = false; }
    // lib/loss.py:25-43 for one entry: the weights of a masked-out entry are max(0, -1e5) = 0, its term is 0 and it adds exp(0)
    __device__ __forceinline__ void add(float d, float ov, const CircleConst& k)
    {
        const bool p = ov > k.pos_overlap, n = ov == 0.f;
        const float pw = p ? fmaxf(0.f, d - k.pos_optimal) * sqrtf(ov) : 0.f;
        const float nw = n ? fmaxf(0.f, k.neg_optimal - d) : 0.f;
        pos.add(k.log_scale * (d - k.pos_margin) * pw);
        neg.add(k.log_scale * (k.neg_margin - d) * nw);
        any_pos |= p; any_neg |= n;
    }
    // softplus(lse_pos + lse_neg) / log_scale, F.softplus's threshold of 20 included
    __device__ __forceinline__ float loss(const CircleConst& k) const
    {
        const float x = (pos.m + logf(pos.s)) + (neg.m + logf(neg.s));
        return (x > 20.f ? x : log1pf(expf(x))) / k.log_scale;
    }
};

__device__ __forceinline__ float cl_overlap(const int* __restrict__ slot, const float* __restrict__ gt_ov, size_t at)
{
    const int e = slot[at];
    return e >= 0 ? gt_ov[e] : 0.f;
}

__global__ __launch_bounds__(256) void coarse_row_kernel(int total_t, const int* __restrict__ t_first, const int* __restrict__ t_count, int total_s,
                                                         const int* __restrict__ s_first, const int* __restrict__ s_count, int max_t, int max_s,
                                                         const float* __restrict__ dist, const int* __restrict__ slot, int gt_cap,
                                                         const float* __restrict__ gt_overlaps, CircleConst k, float* __restrict__ row_loss,
                                                         int* __restrict__ row_valid)
{
    const int b = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int nt = count_range(t_first, t_count, b, total_t, max_t).y, ns = count_range(s_first, s_count, b, total_s, max_s).y;
    if (i >= nt || ns == 0) return;   // wave-uniform; no barrier below
    const size_t base = (size_t)b * max_t * max_s + (size_t)i * max_s;
    const float* gt_ov = gt_overlaps + (size_t)b * gt_cap;
    CircleAcc a;
    a.init();
    for (int j = lane; j < ns; j += 64) a.add(dist[base + j], cl_overlap(slot, gt_ov, base + j), k);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float pm = __shfl_xor(a.pos.m, o, 64), ps = __shfl_xor(a.pos.s, o, 64);
        const float nm = __shfl_xor(a.neg.m, o, 64), nsum = __shfl_xor(a.neg.s, o, 64);
        a.pos.merge(pm, ps);
        a.neg.merge(nm, nsum);
    }
    const bool valid = __ballot(a.any_pos) != 0ull && __ballot(a.any_neg) != 0ull;
    if (lane == 0) { row_loss[(size_t)b * max_t + i] = a.loss(k); row_valid[(size_t)b * max_t + i] = valid ? 1 : 0; }
}

__global__ __launch_bounds__(256) void coarse_col_kernel(int total_t, const int* __restrict__ t_first, const int* __restrict__ t_count, int total_s,
                                                         const int* __restrict__ s_first, const int* __restrict__ s_count, int max_t, int max_s,
                                                         const float* __restrict__ dist, const int* __restrict__ slot, int gt_cap,
                                                         const float* __restrict__ gt_overlaps, CircleConst k, float* __restrict__ col_loss,
                                                         int* __restrict__ col_valid)
{
    __shared__ float s_m[2][4][64], s_s[2][4][64];
    __shared__ int s_any[4][64];
    const int b = blockIdx.y, cx = threadIdx.x & 63, seg = threadIdx.x >> 6, j = blockIdx.x * 64 + cx;
    const int nt = count_range(t_first, t_count, b, total_t, max_t).y, ns = count_range(s_first, s_count, b, total_s, max_s).y;
    if (blockIdx.x * 64 >= ns || nt == 0) return;   // block-uniform
    const int chunk = (nt + 3) >> 2, r0 = seg * chunk, r1 = min(nt, r0 + chunk);   // the quarters depend on the pair alone
    const size_t base = (size_t)b * max_t * max_s;
    const float* gt_ov = gt_overlaps + (size_t)b * gt_cap;
    CircleAcc a;
    a.init();
    if (j < ns)
        for (int i = r0; i < r1; ++i) a.add(dist[base + (size_t)i * max_s + j], cl_overlap(slot, gt_ov, base + (size_t)i * max_s + j), k);
    s_m[0][seg][cx] = a.pos.m; s_s[0][seg][cx] = a.pos.s; s_m[1][seg][cx] = a.neg.m; s_s[1][seg][cx] = a.neg.s;
    s_any[seg][cx] = (a.any_pos ? 1 : 0) | (a.any_neg ? 2 : 0);
    __syncthreads();
    if (seg != 0 || j >= ns) return;
    int any = s_any[0][cx];
    for (int q = 1; q < 4; ++q) {   // quarters in order
        a.pos.merge(s_m[0][q][cx], s_s[0][q][cx]);
        a.neg.merge(s_m[1][q][cx], s_s[1][q][cx]);
        any |= s_any[q][cx];
    }
    col_loss[(size_t)b * max_s + j] = a.loss(k);
    col_valid[(size_t)b * max_s + j] = any == 3 ? 1 : 0;
}

// sum and count of the valid entries of v[0..n), thread-strided in float64, then a fixed tree; the result in every thread
__device__ __forceinline__ double cl_masked_mean(const float* __restrict__ v, const int* __restrict__ valid, int n, double* s_sum, int* s_cnt,
                                                 int* n_valid)
{
    double acc = 0.0;
    int cnt = 0;
    for (int i = threadIdx.x; i < n; i += 256)
        if (valid[i]) { acc += (double)v[i]; ++cnt; }
    __syncthreads();   // the arrays are free again
    s_sum[threadIdx.x] = acc; s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { s_sum[threadIdx.x] += s_sum[threadIdx.x + o]; s_cnt[threadIdx.x] += s_cnt[threadIdx.x + o]; }
        __syncthreads();
    }
    *n_valid = s_cnt[0];
    return s_sum[0] / (double)s_cnt[0];   // 0 / 0: the reference's mean of an empty selection
}

__global__ __launch_bounds__(256) void coarse_final_kernel(int total_t, const int* __restrict__ t_first, const int* __restrict__ t_count, int total_s,
                                                           const int* __restrict__ s_first, const int* __restrict__ s_count, int max_t, int max_s,
                                                           const float* __restrict__ row_loss, const int* __restrict__ row_valid,
                                                           const float* __restrict__ col_loss, const int* __restrict__ col_valid,
                                                           float* __restrict__ c_loss, int* __restrict__ status)
{
    __shared__ double s_sum[256];
    __shared__ int s_cnt[256];
    const int b = blockIdx.x;
    int nt = count_range(t_first, t_count, b, total_t, max_t).y, ns = count_range(s_first, s_count, b, total_s, max_s).y;
    if (nt == 0 || ns == 0) nt = ns = 0;   // the row / column kernels wrote nothing
    int nr = 0, nc = 0;
    const double mr = cl_masked_mean(row_loss + (size_t)b * max_t, row_valid + (size_t)b * max_t, nt, s_sum, s_cnt, &nr);
    const double mc = cl_masked_mean(col_loss + (size_t)b * max_s, col_valid + (size_t)b * max_s, ns, s_sum, s_cnt, &nc);
    if (threadIdx.x == 0) {
        c_loss[b] = nr > 0 && nc > 0 ? (float)((mr + mc) / 2.0) : NAN;
        if (nr == 0 || nc == 0) status[b] |= ROITR_LOSS_COARSE_EMPTY;   // this block is the only writer of status[b] by now
    }
}

struct FineWs { float* part_sum; int* part_cnt; size_t bytes; };   // (sum, count) per slot
FineWs fine_ws(void* base, int slots)
{
    Carve c(base);
    FineWs w;
    w.part_sum = c.take<float>(slots);
    w.part_cnt = c.take<int>(slots);
    w.bytes = c.bytes;
    return w;
}

struct CoarseWs { float* dist; int* slot; float* row_loss; int* row_valid; float* col_loss; int* col_valid; size_t bytes; };
CoarseWs coarse_ws(void* base, int pairs, int max_t, int max_s)
{
    const size_t mat = (size_t)pairs * max_t * max_s, rows = (size_t)pairs * max_t, cols = (size_t)pairs * max_s;
    Carve c(base);
    CoarseWs w;
    w.dist = c.take<float>(mat); w.slot = c.take<int>(mat);
    w.row_loss = c.take<float>(rows); w.row_valid = c.take<int>(rows);
    w.col_loss = c.take<float>(cols); w.col_valid = c.take<int>(cols);
    w.bytes = c.bytes;
    return w;
}

}  // namespace

extern "C" size_t roitr_fine_loss_workspace_bytes(int slots)
{
    if (slots < 0) return 0;
    return fine_ws(nullptr, slots).bytes;
}

extern "C" int roitr_fine_loss_batch(int pairs, int slots, const int* first_slot, const int* patch_count, int L, const float* tgt_knn_pts,
                                     const float* src_knn_pts, const int* tgt_knn_masks, const int* src_knn_masks,
                                     const float* matching_scores, const float* rot, const float* trans, float positive_radius, float* f_sum,
                                     int* f_count, float* f_loss, int* status, void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    if (pairs < 0 || slots < 0) return refuse(ROITR_ERR_ARG, "roitr_fine_loss_batch: negative count");
    if (L < 1 || L > 64) return refuse(ROITR_ERR_UNSUPPORTED, "roitr_fine_loss_batch: point_limit L must lie in [1, 64]");
    if (pairs == 0) return ROITR_OK;
    if (!(positive_radius > 0.f) || !isfinite(positive_radius))
        return refuse(ROITR_ERR_ARG, "roitr_fine_loss_batch: positive_radius must be finite and positive");
    if (!first_slot || !patch_count || !rot || !trans || !f_sum || !f_count || !f_loss || !status ||
        (slots > 0 && (!tgt_knn_pts || !src_knn_pts || !tgt_knn_masks || !src_knn_masks || !matching_scores)))
        return refuse(ROITR_ERR_ARG, "roitr_fine_loss_batch: null pointer");
    const FineWs w = fine_ws(workspace, slots);
    if (workspace_bytes < w.bytes || (slots > 0 && !workspace))
        return refuse(ROITR_ERR_ARG, "roitr_fine_loss_batch: workspace smaller than roitr_fine_loss_workspace_bytes()");
    const float r2 = (float)((double)positive_radius * (double)positive_radius);
    if (slots > 0) {
        fine_patch_kernel<<<slots, 64, 0, stream>>>(pairs, slots, first_slot, patch_count, tgt_knn_pts, src_knn_pts, tgt_knn_masks, src_knn_masks,
                                                    matching_scores, rot, trans, r2, L, w.part_sum, w.part_cnt);
        ROITR_LAUNCH_CHECK();
    }
    fine_reduce_kernel<<<pairs, 256, 0, stream>>>(pairs, slots, first_slot, patch_count, w.part_sum, w.part_cnt, f_sum, f_count, f_loss, status);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}

extern "C" size_t roitr_coarse_loss_workspace_bytes(int pairs, int max_t, int max_s)
{
    if (pairs < 0 || max_t < 0 || max_s < 0) return 0;
    return coarse_ws(nullptr, pairs, max_t, max_s).bytes;
}

extern "C" int roitr_coarse_loss_batch(int pairs, int D, const float* tgt_feats, int total_tgt, const int* tgt_first, const int* tgt_count,
                                       const float* src_feats, int total_src, const int* src_first, const int* src_count, int max_t, int max_s,
                                       int gt_cap, const int* gt_idx, const float* gt_overlaps, const int* gt_count, float pos_margin,
                                       float neg_margin, float pos_optimal, float neg_optimal, float log_scale, float pos_overlap, float* c_loss,
                                       int* status, void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    if (pairs < 0 || total_tgt < 0 || total_src < 0 || max_t < 0 || max_s < 0 || gt_cap < 0)
        return refuse(ROITR_ERR_ARG, "roitr_coarse_loss_batch: negative count");
    if (D < 4 || D % 4 != 0) return refuse(ROITR_ERR_UNSUPPORTED, "roitr_coarse_loss_batch: the descriptor width must be a positive multiple of 4");
    if (pairs > 65535) return refuse(ROITR_ERR_UNSUPPORTED, "roitr_coarse_loss_batch: at most 65535 pairs per call");
    if (pairs == 0) return ROITR_OK;
    if (!(log_scale > 0.f) || !isfinite(log_scale)) return refuse(ROITR_ERR_ARG, "roitr_coarse_loss_batch: log_scale must be finite and positive");
    if (!tgt_first || !tgt_count || !src_first || !src_count || !gt_count || !c_loss || !status || (total_tgt > 0 && !tgt_feats) ||
        (total_src > 0 && !src_feats) || (gt_cap > 0 && (!gt_idx || !gt_overlaps)))
        return refuse(ROITR_ERR_ARG, "roitr_coarse_loss_batch: null pointer");
    if (((uintptr_t)tgt_feats | (uintptr_t)src_feats) & 15) return refuse(ROITR_ERR_ARG, "roitr_coarse_loss_batch: descriptors must be 16-byte aligned");
    const CoarseWs w = coarse_ws(workspace, pairs, max_t, max_s);
    if (workspace_bytes < w.bytes || (w.bytes > 0 && !workspace))
        return refuse(ROITR_ERR_ARG, "roitr_coarse_loss_batch: workspace smaller than roitr_coarse_loss_workspace_bytes()");
    const CircleConst k = {pos_margin, neg_margin, pos_optimal, neg_optimal, log_scale, pos_overlap};
    coarse_status_kernel<<<div_up(pairs, 256), 256, 0, stream>>>(pairs, total_tgt, tgt_first, tgt_count, total_src, src_first, src_count, max_t,
                                                                 max_s, status);
    ROITR_LAUNCH_CHECK();
    if (max_t > 0 && max_s > 0) {
        const int tiles_t = div_up(max_t, CT), tiles_s = div_up(max_s, CT);
        ROITR_HIP(hipMemsetAsync(w.slot, 0xFF, (size_t)pairs * max_t * max_s * sizeof(int), stream));   // -1: no ground-truth entry
        if (gt_cap > 0) {
            coarse_scatter_kernel<<<dim3(div_up(gt_cap, 256), pairs), 256, 0, stream>>>(gt_cap, gt_idx, gt_count, total_tgt, tgt_first, tgt_count,
                                                                                         total_src, src_first, src_count, max_t, max_s, w.slot,
                                                                                         status);
            ROITR_LAUNCH_CHECK();
        }
        coarse_dist_kernel<<<dim3(tiles_s, tiles_t, pairs), 256, 0, stream>>>(D, tgt_feats, total_tgt, tgt_first, tgt_count, src_feats, total_src,
                                                                               src_first, src_count, max_t, max_s, w.dist);
        ROITR_LAUNCH_CHECK();
        coarse_row_kernel<<<dim3(div_up(max_t, 4), pairs), 256, 0, stream>>>(total_tgt, tgt_first, tgt_count, total_src, src_first, src_count, max_t,
                                                                             max_s, w.dist, w.slot, gt_cap, gt_overlaps, k, w.row_loss,
                                                                             w.row_valid);
        ROITR_LAUNCH_CHECK();
        coarse_col_kernel<<<dim3(tiles_s, pairs), 256, 0, stream>>>(total_tgt, tgt_first, tgt_count, total_src, src_first, src_count, max_t, max_s,
                                                                    w.dist, w.slot, gt_cap, gt_overlaps, k, w.col_loss, w.col_valid);
        ROITR_LAUNCH_CHECK();
    }
    coarse_final_kernel<<<pairs, 256, 0, stream>>>(total_tgt, tgt_first, tgt_count, total_src, src_first, src_count, max_t, max_s, w.row_loss,
                                                   w.row_valid, w.col_loss, w.col_valid, c_loss, status);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}
