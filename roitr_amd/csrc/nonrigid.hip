// 4DMatch non-rigid evaluation: NFMR, the non-rigid feature matching recall, batched over pairs.
//
// Reference: registration/evaluate_fdmatch.py:50-115 (compute_nrfmr, blend_anchor_motion, knn_point_np).  Per pair:
//   anchors   every correspondence's source point is looked up in the DEFORMED source cloud (nearest point), the anchor is the
//             point of the RAW cloud at that index and carries the motion  tgt_corr - anchor;
//   blend     every metric point p = raw[metric_index[m]] takes its 3 nearest anchors, distances below 1e-10 -> 1e-10, beyond the
//             search radius -> 1e10, weights 1 / d normalised to sum 1, predicted motion = the weighted sum of the three motions;
//   recall    |p + motion - (rot deformed[metric_index[m]] + trans)| < recall_thr.
// The mask blend_anchor_motion returns is not part of the recall: a point whose three anchors all lie beyond the radius takes three
// equal weights and still counts, as in the reference.
//
// Two launches after a per-pair status pass, all on the caller's stream:
//   nfmr_anchor_kernel   one lane per correspondence, the pair's deformed cloud streamed through LDS in tiles (every lane of a wave
//                        reads the same LDS address: a broadcast), fp32 distances in the difference form (common.h sqdist3, not the
//                        reference's |a|^2 + |b|^2 - 2ab, which only exists to feed a matmul and cancels), ascending scan that
//                        replaces on strictly-less only: THE LOWEST INDEX WINS A TIE;
//   nfmr_blend_kernel    one lane per metric point, the pair's anchors streamed through LDS, a running top-3 of (d^2, index) in
//                        registers (the branch-free v_med3_f32 insertion of pointops_knn.hip; strict comparisons: the lowest index
//                        wins here too -- np.argpartition's choice among equal distances is implementation-defined, and anchors repeat
//                        whenever correspondences share a source point), then weights, blend, ground-truth warp and error per lane,
//                        and the pair's hit count: ballot + popcount per wave, one integer atomicAdd per block and pair.
// Lanes are laid out flat over the batch's rows; a block whose lanes belong to several pairs walks those pairs one after the other,
// so a lane's result depends only on its own pair's data scanned in index order: results are bitwise independent of the batch and
// of the block size.  Offsets are clamped to the totals the host was given before anything is read through them.
#include "common.h"
#include "roitr_engine.h"
#include "workspace.h"

#include <math.h>

namespace {

constexpr int NF_TILE = 1024;   // candidates per LDS tile (16 KB)

// one thread per pair: status word and zeroed hit count.  ref_need: anchors a pair must have (3); need_src: the anchors come from
// a search in the pair's source cloud, an empty cloud leaves none
__global__ __launch_bounds__(256) void nfmr_status_kernel(int pairs, int total_src, const int* __restrict__ src_offsets, int total_ref,
                                                          const int* __restrict__ ref_starts, int total_q, const int* __restrict__ q_starts,
                                                          int* __restrict__ hits, int* __restrict__ status)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= pairs) return;
    int st = 0;
    int n_ref = starts_range(ref_starts, p, total_ref).y - starts_range(ref_starts, p, total_ref).x;
    const int2 q = starts_range(q_starts, p, total_q);
    if (starts_bad(ref_starts, p, total_ref) || starts_bad(q_starts, p, total_q)) st |= ROITR_NFMR_BAD_OFFSETS;
    if (src_offsets) {
        if (starts_bad(src_offsets, p, total_src)) st |= ROITR_NFMR_BAD_OFFSETS;
        const int2 s = starts_range(src_offsets, p, total_src);
        if (s.y == s.x) n_ref = 0;
    }
    if (n_ref < 3) st |= ROITR_NFMR_FEW_ANCHORS;
    if (q.y == q.x) st |= ROITR_NFMR_NO_METRIC;
    status[p] = st;
    if (hits) hits[p] = 0;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void nfmr_anchor_kernel(int pairs, int total_src, const int* __restrict__ src_offsets,
                                                              const float* __restrict__ src_raw, const float* __restrict__ src_def,
                                                              int total_corr, const int* __restrict__ corr_starts,
                                                              const float* __restrict__ src_corr, const float* __restrict__ tgt_corr,
                                                              int* __restrict__ anchor_idx, float* __restrict__ anchor, float* __restrict__ motion)
{
    __shared__ float4 tile[NF_TILE];
    const int c_lo = blockIdx.x * THREADS, c_hi = min(c_lo + THREADS, total_corr);
    const int c = c_lo + threadIdx.x;
    const bool live = c < total_corr;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) { qx = src_corr[(size_t)c * 3]; qy = src_corr[(size_t)c * 3 + 1]; qz = src_corr[(size_t)c * 3 + 2]; }
    const int p_first = segment_of(c_lo, corr_starts + 1, pairs), p_last = segment_of(c_hi - 1, corr_starts + 1, pairs);
    for (int p = p_first; p <= p_last; ++p) {   // block-uniform
        const int2 cr = starts_range(corr_starts, p, total_corr);
        if (cr.y <= c_lo || cr.x >= c_hi) continue;
        const int2 sr = starts_range(src_offsets, p, total_src);
        const int n = sr.y - sr.x;
        float best = INFINITY;
        int bi = 0;
        for (int t0 = 0; t0 < n; t0 += NF_TILE) {
            const int cnt = min(NF_TILE, n - t0);
            __syncthreads();   // the previous tile has been read
            for (int j = threadIdx.x; j < cnt; j += THREADS) {
                const float* q = src_def + (size_t)(sr.x + t0 + j) * 3;
                tile[j] = make_float4(q[0], q[1], q[2], 0.f);
            }
            __syncthreads();
#pragma unroll 8
            for (int j = 0; j < cnt; ++j) {
                const float4 v = tile[j];
                const float d = sqdist3(qx, qy, qz, v.x, v.y, v.z);
                const bool lt = d < best;   // strictly less, ascending index: the lowest index keeps a tie
                best = lt ? d : best;
                bi = lt ? t0 + j : bi;
            }
        }
        if (live && c >= cr.x && c < cr.y) {
            if (anchor_idx) anchor_idx[c] = n > 0 ? bi : -1;
            if (n > 0) {
                const float* a = src_raw + (size_t)(sr.x + bi) * 3;
                const float ax = a[0], ay = a[1], az = a[2];
                anchor[(size_t)c * 3] = ax; anchor[(size_t)c * 3 + 1] = ay; anchor[(size_t)c * 3 + 2] = az;
                motion[(size_t)c * 3] = tgt_corr[(size_t)c * 3] - ax;
                motion[(size_t)c * 3 + 1] = tgt_corr[(size_t)c * 3 + 1] - ay;
                motion[(size_t)c * 3 + 2] = tgt_corr[(size_t)c * 3 + 2] - az;
            }
        }
    }
}

// Queries: q_loc (total_q, 3) directly (blend_anchor_motion), or raw[metric_index[m]] of the pair's cloud (NFMR; then the ground
// truth warp, the error and the hit count follow).  Anchors / motions: (total_ref, 3), pair p's at [ref_starts[p], ref_starts[p+1]).
template <int THREADS>
__global__ __launch_bounds__(THREADS) void nfmr_blend_kernel(int pairs, int total_ref, const int* __restrict__ ref_starts,
                                                             const float* __restrict__ anchor, const float* __restrict__ motion, int total_q,
                                                             const int* __restrict__ q_starts, const float* __restrict__ q_loc,
                                                             const int* __restrict__ metric_index, int total_src,
                                                             const int* __restrict__ src_offsets, const float* __restrict__ src_raw,
                                                             const float* __restrict__ src_def, const float* __restrict__ rot,
                                                             const float* __restrict__ trans, float radius, float thr,
                                                             float* __restrict__ flow_out, int* __restrict__ mask_out, float* __restrict__ err,
                                                             int* __restrict__ hits, int* __restrict__ status)
{
    __shared__ float4 tile[NF_TILE];
    __shared__ int red[THREADS / 64];
    const int m_lo = blockIdx.x * THREADS, m_hi = min(m_lo + THREADS, total_q);
    const int m = m_lo + threadIdx.x;
    const bool live = m < total_q;
    const int p_first = segment_of(m_lo, q_starts + 1, pairs), p_last = segment_of(m_hi - 1, q_starts + 1, pairs);
    for (int p = p_first; p <= p_last; ++p) {   // block-uniform
        const int2 qr = starts_range(q_starts, p, total_q);
        if (qr.y <= m_lo || qr.x >= m_hi) continue;
        const int2 rr = starts_range(ref_starts, p, total_ref);
        int2 sr = make_int2(0, 0);
        if (metric_index) sr = starts_range(src_offsets, p, total_src);
        const int n_src = sr.y - sr.x;
        const int n_ref = (metric_index && n_src == 0) ? 0 : rr.y - rr.x;   // no cloud: the anchor pass wrote nothing
        const bool mine = live && m >= qr.x && m < qr.y;
        bool ok = mine;
        int mi = 0;
        float qx = 0.f, qy = 0.f, qz = 0.f;
        if (mine) {
            if (metric_index) {
                mi = metric_index[m];
                ok = mi >= 0 && mi < n_src;
                if (!ok) atomicOr(status + p, ROITR_NFMR_BAD_INDEX);   // never dereferenced
                mi = ok ? mi : 0;
                if (ok) { const float* q = src_raw + (size_t)(sr.x + mi) * 3; qx = q[0]; qy = q[1]; qz = q[2]; }
            } else {
                qx = q_loc[(size_t)m * 3]; qy = q_loc[(size_t)m * 3 + 1]; qz = q_loc[(size_t)m * 3 + 2];
            }
        }
        if (n_ref < 3) {   // the reference raises here (argpartition); the rule of this library: no prediction, 0 hits, status bit
            if (mine) {
                if (err) err[m] = INFINITY;
                if (flow_out) { flow_out[(size_t)m * 3] = 0.f; flow_out[(size_t)m * 3 + 1] = 0.f; flow_out[(size_t)m * 3 + 2] = 0.f; }
                if (mask_out) mask_out[m] = 0;
            }
            continue;
        }
        float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
        int i0 = 0, i1 = 0, i2 = 0;
        for (int t0 = 0; t0 < n_ref; t0 += NF_TILE) {
            const int cnt = min(NF_TILE, n_ref - t0);
            __syncthreads();
            for (int j = threadIdx.x; j < cnt; j += THREADS) {
                const float* a = anchor + (size_t)(rr.x + t0 + j) * 3;
                tile[j] = make_float4(a[0], a[1], a[2], 0.f);
            }
            __syncthreads();
#pragma unroll 4
            for (int j = 0; j < cnt; ++j) {
                const float4 v = tile[j];
                const float dd = sqdist3(qx, qy, qz, v.x, v.y, v.z);
                const int ci = t0 + j;
                // ascending list; the median IS the shifted / inserted / kept value.  Strict comparisons: an equal distance stays
                // behind the entries already there, which have lower indices
                const bool sh2 = d1 > dd, here2 = d2 > dd;
                d2 = __builtin_amdgcn_fmed3f(dd, d1, d2);
                i2 = sh2 ? i1 : (here2 ? ci : i2);
                const bool sh1 = d0 > dd, here1 = d1 > dd;
                d1 = __builtin_amdgcn_fmed3f(dd, d0, d1);
                i1 = sh1 ? i0 : (here1 ? ci : i1);
                d0 = sh1 ? dd : d0;
                i0 = sh1 ? ci : i0;
            }
        }
        bool hit = false;
        if (ok) {
            // evaluate_fdmatch.py:61-67 in fp32, the sums in numpy's order (k = 0, 1, 2)
            float dk[3] = {sqrtf(d0), sqrtf(d1), sqrtf(d2)};
            const int ik[3] = {i0, i1, i2};
            float w[3];
            int beyond = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                dk[k] = dk[k] < 1e-10f ? 1e-10f : dk[k];
                const bool far = dk[k] > radius;
                beyond += far ? 1 : 0;
                dk[k] = far ? 1e10f : dk[k];
                w[k] = 1.0f / dk[k];
            }
            const float wsum = (w[0] + w[1]) + w[2];
            float fx = 0.f, fy = 0.f, fz = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float wk = w[k] / wsum;
                const float* mo = motion + (size_t)(rr.x + ik[k]) * 3;
                const float tx = mo[0] * wk, ty = mo[1] * wk, tz = mo[2] * wk;
                fx = k == 0 ? tx : fx + tx; fy = k == 0 ? ty : fy + ty; fz = k == 0 ? tz : fz + tz;
            }
            if (flow_out) { flow_out[(size_t)m * 3] = fx; flow_out[(size_t)m * 3 + 1] = fy; flow_out[(size_t)m * 3 + 2] = fz; }
            if (mask_out) mask_out[m] = beyond < 3 ? 1 : 0;
            if (metric_index) {
                const float* R = rot + (size_t)p * 9;
                const float* t = trans + (size_t)p * 3;
                const float* g = src_def + (size_t)(sr.x + mi) * 3;
                const float x = g[0], y = g[1], z = g[2];
                const float gx = fmaf(z, R[2], fmaf(y, R[1], x * R[0])) + t[0];
                const float gy = fmaf(z, R[5], fmaf(y, R[4], x * R[3])) + t[1];
                const float gz = fmaf(z, R[8], fmaf(y, R[7], x * R[6])) + t[2];
                const float ex = (qx + fx) - gx, ey = (qy + fy) - gy, ez = (qz + fz) - gz;
                const float e = sqrtf(ex * ex + ey * ey + ez * ez);
                if (err) err[m] = e;
                hit = e < thr;
            }
        } else if (mine && err) {
            err[m] = INFINITY;   // metric index out of range
        }
        if (hits) {   // integer count: the order the blocks arrive in does not matter
            const int wave_hits = __popcll(__ballot(hit));
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wave_hits;
            __syncthreads();
            if (threadIdx.x == 0) {
                int tot = 0;
#pragma unroll
                for (int k = 0; k < THREADS / 64; ++k) tot += red[k];
                if (tot > 0) atomicAdd(hits + p, tot);
            }
            // red is rewritten only after the next pair's first tile barrier
        }
    }
}

struct NfWorkspace { float* anchor; float* motion; size_t bytes; };   // (total_corr, 3) each

NfWorkspace nf_carve(void* ws, int total_corr)
{
    Carve c(ws);
    NfWorkspace w;
    w.anchor = c.take<float>((size_t)total_corr * 3);
    w.motion = c.take<float>((size_t)total_corr * 3);
    w.bytes = c.bytes;
    return w;
}

int nf_block(int block, int rows)
{
    // 256 lanes per block at batch size; below one wave per SIMD of the chip the rows are spread
    // over four times as many blocks
    if (block != 0) return block;
    return rows >= 64 * 1024 ? 256 : 64;
}

template <typename... A>
void launch_anchor(int block, int rows, hipStream_t stream, A... a)
{
    const int g = div_up(rows, block);
    if (block == 64) nfmr_anchor_kernel<64><<<g, 64, 0, stream>>>(a...);
    else if (block == 128) nfmr_anchor_kernel<128><<<g, 128, 0, stream>>>(a...);
    else nfmr_anchor_kernel<256><<<g, 256, 0, stream>>>(a...);
}
template <typename... A>
void launch_blend(int block, int rows, hipStream_t stream, A... a)
{
    const int g = div_up(rows, block);
    if (block == 64) nfmr_blend_kernel<64><<<g, 64, 0, stream>>>(a...);
    else if (block == 128) nfmr_blend_kernel<128><<<g, 128, 0, stream>>>(a...);
    else nfmr_blend_kernel<256><<<g, 256, 0, stream>>>(a...);
}

bool nf_block_ok(int b) { return b == 0 || b == 64 || b == 128 || b == 256; }

}  // namespace

extern "C" size_t roitr_nfmr_workspace_bytes(int pairs, int total_corr, int total_metric)
{
    (void)pairs; (void)total_metric;
    if (total_corr < 0) return 0;
    return nf_carve(nullptr, total_corr).bytes;
}

extern "C" int roitr_nfmr_batch(int pairs, int total_src, const int* src_offsets, const float* src_raw, const float* src_deformed,
                                int total_corr, const int* corr_starts, const float* src_corr, const float* tgt_corr, int total_metric,
                                const int* metric_starts, const int* metric_index, const float* rot, const float* trans,
                                float search_radius, float recall_thr, int block, int* anchor_idx, float* err, int* hits, int* status,
                                void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    if (pairs < 0 || total_src < 0 || total_corr < 0 || total_metric < 0)
        return refuse(ROITR_ERR_ARG, "roitr_nfmr_batch: negative count");
    if (pairs == 0) return ROITR_OK;
    if (!(search_radius > 0.f) || !isfinite(search_radius) || !(recall_thr > 0.f) || !isfinite(recall_thr))
        return refuse(ROITR_ERR_ARG, "roitr_nfmr_batch: search_radius and recall_thr must be finite and positive");
    if (!nf_block_ok(block)) return refuse(ROITR_ERR_ARG, "roitr_nfmr_batch: block must be 0 (automatic), 64, 128 or 256");
    if (!src_offsets || !corr_starts || !metric_starts || !rot || !trans || !hits || !status || (total_src > 0 && (!src_raw || !src_deformed)) ||
        (total_corr > 0 && (!src_corr || !tgt_corr)) || (total_metric > 0 && !metric_index))
        return refuse(ROITR_ERR_ARG, "roitr_nfmr_batch: null pointer");
    const NfWorkspace w = nf_carve(workspace, total_corr);
    if (workspace_bytes < w.bytes || (total_corr > 0 && !workspace))
        return refuse(ROITR_ERR_ARG, "roitr_nfmr_batch: workspace smaller than roitr_nfmr_workspace_bytes()");
    nfmr_status_kernel<<<div_up(pairs, 256), 256, 0, stream>>>(pairs, total_src, src_offsets, total_corr, corr_starts, total_metric,
                                                               metric_starts, hits, status);
    ROITR_LAUNCH_CHECK();
    if (total_corr > 0) {
        launch_anchor(nf_block(block, total_corr), total_corr, stream, pairs, total_src, src_offsets, src_raw, src_deformed, total_corr,
                      corr_starts, src_corr, tgt_corr, anchor_idx, w.anchor, w.motion);
        ROITR_LAUNCH_CHECK();
    }
    if (total_metric > 0) {
        launch_blend(nf_block(block, total_metric), total_metric, stream, pairs, total_corr, corr_starts, (const float*)w.anchor,
                     (const float*)w.motion, total_metric, metric_starts, (const float*)nullptr, metric_index, total_src, src_offsets, src_raw,
                     src_deformed, rot, trans, search_radius, recall_thr, (float*)nullptr, (int*)nullptr, err, hits, status);
        ROITR_LAUNCH_CHECK();
    }
    return ROITR_OK;
}

extern "C" int roitr_blend_anchor_motion(int pairs, int total_ref, const int* ref_starts, const float* ref_loc, const float* ref_flow,
                                         int total_query, const int* query_starts, const float* query_loc, float search_radius, int block,
                                         float* blended_flow, int* mask, int* status, hipStream_t stream)
{
    if (pairs < 0 || total_ref < 0 || total_query < 0) return refuse(ROITR_ERR_ARG, "roitr_blend_anchor_motion: negative count");
    if (pairs == 0) return ROITR_OK;
    if (!(search_radius > 0.f) || !isfinite(search_radius))
        return refuse(ROITR_ERR_ARG, "roitr_blend_anchor_motion: search_radius must be finite and positive");
    if (!nf_block_ok(block)) return refuse(ROITR_ERR_ARG, "roitr_blend_anchor_motion: block must be 0 (automatic), 64, 128 or 256");
    if (!ref_starts || !query_starts || !status || (total_ref > 0 && (!ref_loc || !ref_flow)) ||
        (total_query > 0 && (!query_loc || !blended_flow || !mask)))
        return refuse(ROITR_ERR_ARG, "roitr_blend_anchor_motion: null pointer");
    nfmr_status_kernel<<<div_up(pairs, 256), 256, 0, stream>>>(pairs, 0, (const int*)nullptr, total_ref, ref_starts, total_query, query_starts,
                                                               (int*)nullptr, status);
    ROITR_LAUNCH_CHECK();
    if (total_query > 0) {
        launch_blend(nf_block(block, total_query), total_query, stream, pairs, total_ref, ref_starts, ref_loc, ref_flow, total_query,
                     query_starts, query_loc, (const int*)nullptr, 0, (const int*)nullptr, (const float*)nullptr, (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, search_radius, 1.0f, blended_flow, mask, (float*)nullptr, (int*)nullptr,
                     status);
        ROITR_LAUNCH_CHECK();
    }
    return ROITR_OK;
}
