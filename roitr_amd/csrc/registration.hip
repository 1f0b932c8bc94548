// GPU registration: batched correspondence RANSAC and weighted Procrustes.
//
// Reference: registration/evaluate_registration_c2f.py:78-85 (n_points correspondences drawn without replacement with probability
// proportional to the confidence), registration/benchmark_utils.py:169-215 (Open3D registration_ransac_based_on_correspondence,
// ransac_n = 3, edge-length checker 0.9, distance checker = threshold, 50 000 iterations) and lib/utils.py:159-212
// (weighted_procrustes).  Open3D is not available to this project: its checkers and scoring are restated from the reference's call
// (registration_math.h), parity with Open3D itself is unpinned.
//
// Pair b owns rows [starts[b], starts[b + 1]) of src / tgt / scores.  Three launches for the whole batch on the caller's stream:
//   ransac_select_kernel   one block per pair: at most n_points rows (all / top-k / weighted sampling), compacted into the workspace
//                          at the pair's own row offset, in index order;
//   ransac_hyp_kernel      grid (chunks, pairs): each lane one hypothesis at a time, the pair's selected rows staged through LDS in
//                          tiles (all lanes read the same row: broadcast), a fixed number of iterations, best of the chunk out;
//   ransac_final_kernel    one block per pair: best over the chunks in the total order (most inliers, smaller sum of inlier d^2 at
//                          equal count, i.e. smaller RMSE, then lower iteration), the transform rebuilt from its iteration index,
//                          optional Procrustes refits on the inlier set.
// The order is total and every sum runs in a fixed order, so a pair's result depends neither on the chunk count nor on the batch.
#include "common.h"
#include "registration_math.h"
#include "roitr_engine.h"
#include "workspace.h"

#include <limits.h>

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_TILE = 1024;            // rows per LDS tile of the hypothesis kernel (2 x 16 KB)
constexpr int RG_TARGET_BLOCKS = 2048;   // hypothesis blocks the automatic chunk count aims at (256 CUs x 8)
constexpr int RG_MAX_ITER = 1 << 28;     // iteration << 4 must fit the low 32 bits of the counter

enum { RG_SEL_ALL = 0, RG_SEL_TOPK = 1, RG_SEL_WEIGHTED = 2 };

int ransac_chunks(int pairs, int iterations, int chunks_req)
{
    const int max_chunks = div_up(iterations, RG_THREADS);
    int c = chunks_req > 0 ? chunks_req : div_up(RG_TARGET_BLOCKS, pairs > 0 ? pairs : 1);
    if (c > max_chunks) c = max_chunks;
    if (c > 65535) c = 65535;
    return c < 1 ? 1 : c;
}

struct RgWorkspace {
    float4* sel_s;               // (total_rows) x, y, z, weight
    float4* sel_t;               // (total_rows) x, y, z, 0
    unsigned long long* keys;    // (total_rows) ordered selection keys
    int4* best;                  // (pairs, chunks) {count, sum d^2 bits, iteration, valid hypotheses}
    size_t bytes;
};

RgWorkspace carve(void* ws, int pairs, int total_rows, int chunks)
{
    Carve c(ws);
    RgWorkspace w;
    w.sel_s = c.take<float4>(total_rows);
    w.sel_t = c.take<float4>(total_rows);
    w.keys = c.take<unsigned long long>(total_rows);
    w.best = c.take<int4>((size_t)pairs * chunks);
    w.bytes = c.bytes;
    return w;
}

__device__ __forceinline__ int wave_sum_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide sum of an int (every thread gets it); `red` holds 4 ints
__device__ __forceinline__ int block_sum_i(int v, int* red)
{
    v = wave_sum_i(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// exclusive prefix of a flag over the block in thread order, and the block total; `red` holds 4 ints
__device__ __forceinline__ int block_scan_flag(bool f, int* red, int& total)
{
    const unsigned long long m = __ballot(f);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) red[w] = __popcll(m);
    __syncthreads();
    int pre = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) pre += k < w ? red[k] : 0;
    total = red[0] + red[1] + red[2] + red[3];
    return pre + below;
}

// ordered image of a double (larger double -> larger integer); 0 is kept for "not eligible"
__device__ __forceinline__ unsigned long long ordered_key(double d)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    const unsigned long long o = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return o == 0 ? 1 : o;
}

// (count, sum, iteration) total order: more inliers, then smaller sum of inlier d^2, then lower iteration
__device__ __forceinline__ bool better(int ca, float sa, int ia, int cb, float sb, int ib)
{
    if (ca != cb) return ca > cb;
    if (sa != sb) return sa < sb;
    return ia < ib;
}

__global__ __launch_bounds__(RG_THREADS) void ransac_select_kernel(const int* __restrict__ starts, int total_rows,
                                                                   const float* __restrict__ src, const float* __restrict__ tgt,
                                                                   const float* __restrict__ scores, int mode, int n_points,
                                                                   unsigned long long seed, const unsigned* __restrict__ pair_keys,
                                                                   RgWorkspace ws, int* __restrict__ n_used, int* __restrict__ selected)
{
    __shared__ int red[4];
    const int b = blockIdx.x;
    const int s = min(max(starts[b], 0), total_rows), e = min(max(starts[b + 1], s), total_rows);
    const int n = e - s;
    const unsigned key = pair_keys[b];
    unsigned long long* kb = ws.keys + s;
    // keys and eligibility
    int elig = 0;
    for (int j = threadIdx.x; j < n; j += RG_THREADS) {
        const float w = scores ? scores[s + j] : 1.0f;
        unsigned long long k;
        if (mode == RG_SEL_ALL) k = 1;
        else if (mode == RG_SEL_TOPK) k = ordered_key((double)w);
        else k = (w > 0.f && w <= 3.402823466e38f) ? ordered_key(log(rg_select_uniform(seed, key, (unsigned)j)) / (double)w) : 0;
        kb[j] = k;
        elig += k != 0;
    }
    __syncthreads();   // keys visible to the block (global memory, same block)
    const int n_elig = block_sum_i(elig, red);
    const int k = mode == RG_SEL_ALL ? n_elig : min(n_points, n_elig);
    // threshold: the k-th largest key (MSB-first bisection); rows above it are taken, rows equal to it by lowest index
    unsigned long long thr = 0;
    int need = 0;
    if (k < n_elig) {
        for (int bit = 63; bit >= 0; --bit) {
            const unsigned long long cand = thr | (1ull << bit);
            int c = 0;
            for (int j = threadIdx.x; j < n; j += RG_THREADS) c += kb[j] >= cand;
            if (block_sum_i(c, red) >= k) thr = cand;
        }
        int gt = 0;
        for (int j = threadIdx.x; j < n; j += RG_THREADS) gt += kb[j] > thr;
        need = k - block_sum_i(gt, red);
    }
    // compaction in index order
    int taken = 0, ties = 0;
    for (int j0 = 0; j0 < n; j0 += RG_THREADS) {
        const int j = j0 + threadIdx.x;
        const unsigned long long kj = j < n ? kb[j] : 0;
        int tie_total, sel_total;
        const int tie_rank = ties + block_scan_flag(j < n && thr != 0 && kj == thr, red, tie_total);
        const bool sel = j < n && (kj > thr || (thr != 0 && kj == thr && tie_rank < need));
        const int pos = taken + block_scan_flag(sel, red, sel_total);
        if (sel) {
            const int r = s + j, o = s + pos;
            ws.sel_s[o] = make_float4(src[3 * (size_t)r], src[3 * (size_t)r + 1], src[3 * (size_t)r + 2], scores ? scores[r] : 1.0f);
            ws.sel_t[o] = make_float4(tgt[3 * (size_t)r], tgt[3 * (size_t)r + 1], tgt[3 * (size_t)r + 2], 0.f);
            if (selected) selected[o] = j;
        }
        ties += tie_total;
        taken += sel_total;
    }
    if (threadIdx.x == 0) n_used[b] = taken;
}

__global__ __launch_bounds__(RG_THREADS) void ransac_hyp_kernel(const int* __restrict__ starts, int total_rows, RgWorkspace ws,
                                                                const int* __restrict__ n_used, unsigned long long seed,
                                                                const unsigned* __restrict__ pair_keys, int iterations, int chunks,
                                                                float thr2, double sim)
{
    __shared__ float4 ts[RG_TILE], tt[RG_TILE];
    __shared__ int red_c[RG_THREADS], red_i[RG_THREADS], red_v[RG_THREADS];
    __shared__ float red_s[RG_THREADS];
    const int b = blockIdx.y, c = blockIdx.x;
    const int s = min(max(starts[b], 0), total_rows);
    const int n = n_used[b];
    const unsigned key = pair_keys[b];
    const int per = (iterations + chunks - 1) / chunks;
    const int it0 = c * per, it1 = min(it0 + per, iterations);
    const float4* s4 = ws.sel_s + s;
    const float4* t4 = ws.sel_t + s;
    int bc = -1, bi = INT_MAX, nvalid = 0;
    float bs = 0.f;
    for (int base = it0; base < it1 && n >= 3; base += RG_THREADS) {
        const int it = base + (int)threadIdx.x;
        float T[12];
        const bool valid = it < it1 && rg_hypothesis(seed, key, (unsigned)it, n, s4, t4, thr2, sim, T);
        nvalid += valid;
        if (!__syncthreads_or(valid)) continue;
        int cnt = 0;
        float sum = 0.f;
        for (int r0 = 0; r0 < n; r0 += RG_TILE) {
            const int m = min(RG_TILE, n - r0);
            __syncthreads();
            for (int j = threadIdx.x; j < m; j += RG_THREADS) { ts[j] = s4[r0 + j]; tt[j] = t4[r0 + j]; }
            __syncthreads();
            if (valid) {
#pragma unroll 4
                for (int j = 0; j < m; ++j) {
                    const float4 a = ts[j], g = tt[j];
                    const float d2 = rg_dist2(T, a.x, a.y, a.z, g.x, g.y, g.z);
                    if (d2 < thr2) { cnt += 1; sum += d2; }
                }
            }
        }
        if (valid && better(cnt, sum, it, bc, bs, bi)) { bc = cnt; bs = sum; bi = it; }
    }
    // best of the block (fixed tree) and the number of valid hypotheses
    red_c[threadIdx.x] = bc; red_s[threadIdx.x] = bs; red_i[threadIdx.x] = bi; red_v[threadIdx.x] = nvalid;
    __syncthreads();
    for (int h = RG_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const int o = threadIdx.x + h;
            if (better(red_c[o], red_s[o], red_i[o], red_c[threadIdx.x], red_s[threadIdx.x], red_i[threadIdx.x])) {
                red_c[threadIdx.x] = red_c[o]; red_s[threadIdx.x] = red_s[o]; red_i[threadIdx.x] = red_i[o];
            }
            red_v[threadIdx.x] += red_v[o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) ws.best[(size_t)b * chunks + c] = make_int4(red_c[0], __float_as_int(red_s[0]), red_i[0], red_v[0]);
}

// fixed-tree block sum of NV doubles per thread (every thread gets the totals); red holds RG_THREADS * NV doubles
// (procrustes_block.h's block_sum_d is a wave butterfly that folds in another order: unifying the two would change result bits)
template <int NV>
__device__ __forceinline__ void block_sum_d(double (&v)[NV], double* red)
{
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) red[k * RG_THREADS + threadIdx.x] = v[k];
    __syncthreads();
    for (int h = RG_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
#pragma unroll
            for (int k = 0; k < NV; ++k) red[k * RG_THREADS + threadIdx.x] += red[k * RG_THREADS + threadIdx.x + h];
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = red[k * RG_THREADS];
}

// One weighted Procrustes step over rows of a block (row r: source p(r), target q(r), weight w(r), 0 = left out), the
// centroids normalised by (sum w + eps) as lib/utils.py:190-193 does: T out.  Two passes (centroids, then centred products).
template <class Row>
__device__ __forceinline__ void block_procrustes(int n, Row row, double eps, double* red, float (&T)[12], double& wsum)
{
    double a[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int j = threadIdx.x; j < n; j += RG_THREADS) {
        float p[3], q[3], w;
        row(j, p, q, w);
        a[0] += w;
        a[1] += (double)w * p[0]; a[2] += (double)w * p[1]; a[3] += (double)w * p[2];
        a[4] += (double)w * q[0]; a[5] += (double)w * q[1]; a[6] += (double)w * q[2];
    }
    block_sum_d<7>(a, red);
    wsum = a[0];
    const double den = a[0] + eps;
    const double cs[3] = {a[1] / den, a[2] / den, a[3] / den}, ct[3] = {a[4] / den, a[5] / den, a[6] / den};
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = threadIdx.x; j < n; j += RG_THREADS) {
        float p[3], q[3], w;
        row(j, p, q, w);
        if (w == 0.f) continue;
        const double ps[3] = {p[0] - cs[0], p[1] - cs[1], p[2] - cs[2]}, qs[3] = {q[0] - ct[0], q[1] - ct[1], q[2] - ct[2]};
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) H[3 * x + y] += (double)w * ps[x] * qs[y];
    }
    block_sum_d<9>(H, red);
    rg_solve_rigid(H, cs, ct, T);
}

__device__ __forceinline__ void write_transform(float* out, const float (&T)[12])
{
    if (threadIdx.x < 16) {
        const int r = threadIdx.x >> 2, c = threadIdx.x & 3;
        float v = r == 3 ? (c == 3 ? 1.f : 0.f) : 0.f;
#pragma unroll
        for (int k = 0; k < 12; ++k) v = (r < 3 && k == 4 * r + c) ? T[k] : v;
        out[threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(RG_THREADS) void ransac_final_kernel(const int* __restrict__ starts, int total_rows, RgWorkspace ws,
                                                                  const int* __restrict__ n_used, unsigned long long seed,
                                                                  const unsigned* __restrict__ pair_keys, int chunks, float thr2,
                                                                  double sim, int refine_iters, int refine_weighted,
                                                                  float* __restrict__ T_out, int* __restrict__ inliers,
                                                                  int* __restrict__ best_iteration, int* __restrict__ valid_out)
{
    __shared__ double red[9 * RG_THREADS];
    __shared__ int red_c[RG_THREADS], red_i[RG_THREADS], red_v[RG_THREADS];
    __shared__ float red_s[RG_THREADS];
    __shared__ int red4[4];
    const int b = blockIdx.x;
    const int s = min(max(starts[b], 0), total_rows);
    const int n = n_used[b];
    int bc = -1, bi = INT_MAX, nv = 0;
    float bs = 0.f;
    for (int c = threadIdx.x; c < chunks; c += RG_THREADS) {
        const int4 q = ws.best[(size_t)b * chunks + c];
        if (better(q.x, __int_as_float(q.y), q.z, bc, bs, bi)) { bc = q.x; bs = __int_as_float(q.y); bi = q.z; }
        nv += q.w;
    }
    red_c[threadIdx.x] = bc; red_s[threadIdx.x] = bs; red_i[threadIdx.x] = bi; red_v[threadIdx.x] = nv;
    __syncthreads();
    for (int h = RG_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const int o = threadIdx.x + h;
            if (better(red_c[o], red_s[o], red_i[o], red_c[threadIdx.x], red_s[threadIdx.x], red_i[threadIdx.x])) {
                red_c[threadIdx.x] = red_c[o]; red_s[threadIdx.x] = red_s[o]; red_i[threadIdx.x] = red_i[o];
            }
            red_v[threadIdx.x] += red_v[o];
        }
        __syncthreads();
    }
    bc = red_c[0]; bi = red_i[0]; nv = red_v[0];
    float T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const float4* s4 = ws.sel_s + s;
    const float4* t4 = ws.sel_t + s;
    if (n < 3 || nv == 0 || bc < 0) {
        bc = 0; bi = -1; nv = 0;
    } else {
        float Th[12];
        if (rg_hypothesis(seed, pair_keys[b], (unsigned)bi, n, s4, t4, thr2, sim, Th)) {
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = Th[k];
        }
        bool refined = false;
        for (int r = 0; r < refine_iters; ++r) {
            const float Tc[12] = {T[0], T[1], T[2], T[3], T[4], T[5], T[6], T[7], T[8], T[9], T[10], T[11]};
            int cnt = 0;
            for (int j = threadIdx.x; j < n; j += RG_THREADS) {
                const float4 a = s4[j], g = t4[j];
                cnt += rg_dist2(Tc, a.x, a.y, a.z, g.x, g.y, g.z) < thr2;
            }
            if (block_sum_i(cnt, red4) < 3) break;
            auto row = [&](int j, float (&p)[3], float (&q)[3], float& w) {
                const float4 a = s4[j], g = t4[j];
                p[0] = a.x; p[1] = a.y; p[2] = a.z; q[0] = g.x; q[1] = g.y; q[2] = g.z;
                const bool in = rg_dist2(Tc, a.x, a.y, a.z, g.x, g.y, g.z) < thr2;
                w = in ? (refine_weighted ? a.w : 1.0f) : 0.f;
            };
            double wsum;
            float Tn[12];
            block_procrustes(n, row, 0.0, red, Tn, wsum);
            if (!(wsum > 0.0)) break;
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = Tn[k];
            refined = true;
        }
        if (refined) {
            int cnt = 0;
            for (int j = threadIdx.x; j < n; j += RG_THREADS) {
                const float4 a = s4[j], g = t4[j];
                cnt += rg_dist2(T, a.x, a.y, a.z, g.x, g.y, g.z) < thr2;
            }
            bc = block_sum_i(cnt, red4);
        }
    }
    write_transform(T_out + (size_t)b * 16, T);
    if (threadIdx.x == 0) { inliers[b] = bc; best_iteration[b] = bi; valid_out[b] = nv; }
}

__global__ __launch_bounds__(RG_THREADS) void procrustes_kernel(int N, const float* __restrict__ src, const float* __restrict__ tgt,
                                                                const float* __restrict__ weights, float weight_thresh, float eps,
                                                                float* __restrict__ T_out)
{
    __shared__ double red[9 * RG_THREADS];
    const int b = blockIdx.x;
    const float* p0 = src + (size_t)b * N * 3;
    const float* q0 = tgt + (size_t)b * N * 3;
    const float* w0 = weights ? weights + (size_t)b * N : nullptr;
    auto row = [&](int j, float (&p)[3], float (&q)[3], float& w) {
        p[0] = p0[3 * (size_t)j]; p[1] = p0[3 * (size_t)j + 1]; p[2] = p0[3 * (size_t)j + 2];
        q[0] = q0[3 * (size_t)j]; q[1] = q0[3 * (size_t)j + 1]; q[2] = q0[3 * (size_t)j + 2];
        const float wr = w0 ? w0[j] : 1.0f;
        w = wr < weight_thresh ? 0.f : wr;   // lib/utils.py:187 torch.where(weights < weight_thresh, 0, weights)
    };
    float T[12];
    double wsum;
    block_procrustes(N, row, (double)eps, red, T, wsum);
    write_transform(T_out + (size_t)b * 16, T);
}

__global__ void ransac_samples_kernel(int pairs, const int* __restrict__ n, const unsigned* __restrict__ pair_keys,
                                      unsigned long long seed, int it0, int count, int* __restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)pairs * count) return;
    const int b = (int)(i / count), it = it0 + (int)(i % count);
    int a0, a1, a2;
    const int nb = n[b];
    if (nb < 3 || !rg_triple(seed, pair_keys[b], (unsigned)it, nb, a0, a1, a2)) a0 = a1 = a2 = -1;
    out[3 * i] = a0; out[3 * i + 1] = a1; out[3 * i + 2] = a2;
}

}  // namespace

extern "C" size_t roitr_registration_workspace_bytes(int pairs, int total_rows, int iterations, int chunks)
{
    if (pairs <= 0 || total_rows < 0 || iterations < 1) return 0;
    return carve(nullptr, pairs, total_rows, ransac_chunks(pairs, iterations, chunks)).bytes;
}

extern "C" int roitr_ransac_correspondences(int pairs, const int* starts, int total_rows, const float* src_pts, const float* tgt_pts,
                                            const float* scores, const unsigned* pair_keys, int sample_mode, int n_points, int ransac_n,
                                            float distance_threshold, float edge_similarity, int iterations, int refine_iters,
                                            int refine_weighted, unsigned long long seed, int chunks, void* workspace,
                                            size_t workspace_bytes_given, float* transforms, int* inliers, int* best_iteration,
                                            int* valid_hypotheses, int* n_used, int* selected, hipStream_t stream)
{
    if (ransac_n != 3) return refuse(ROITR_ERR_UNSUPPORTED, "roitr_ransac_correspondences: only ransac_n = 3 is supported");
    if (iterations < 1 || iterations > RG_MAX_ITER)
        return refuse(ROITR_ERR_ARG, "roitr_ransac_correspondences: iterations must be in [1, 2^28]");
    if (!(distance_threshold > 0.f) || !(distance_threshold <= 3.402823466e38f))
        return refuse(ROITR_ERR_ARG, "roitr_ransac_correspondences: distance_threshold must be finite and positive");
    if (!(edge_similarity > 0.f) || !(edge_similarity <= 1.f))
        return refuse(ROITR_ERR_ARG, "roitr_ransac_correspondences: edge_similarity must be in (0, 1]");
    if (sample_mode < RG_SEL_ALL || sample_mode > RG_SEL_WEIGHTED)
        return refuse(ROITR_ERR_ARG, "roitr_ransac_correspondences: sample_mode must be 0 (all), 1 (topk) or 2 (weighted)");
    if (sample_mode != RG_SEL_ALL && n_points < 1) return refuse(ROITR_ERR_ARG, "roitr_ransac_correspondences: n_points < 1");
    if (refine_iters < 0) return refuse(ROITR_ERR_ARG, "roitr_ransac_correspondences: refine_iters < 0");
    if (pairs <= 0) return ROITR_OK;
    if (total_rows < 0 || pairs > 65535) return refuse(ROITR_ERR_ARG, "roitr_ransac_correspondences: total_rows < 0 or pairs > 65535");
    if (!starts || !pair_keys || !workspace || !transforms || !inliers || !best_iteration || !valid_hypotheses || !n_used ||
        (total_rows > 0 && (!src_pts || !tgt_pts)))
        return refuse(ROITR_ERR_ARG, "roitr_ransac_correspondences: null pointer");
    const int ch = ransac_chunks(pairs, iterations, chunks);
    const RgWorkspace ws = carve(workspace, pairs, total_rows, ch);
    if (workspace_bytes_given < ws.bytes)
        return refuse(ROITR_ERR_ARG, "roitr_ransac_correspondences: workspace smaller than roitr_registration_workspace_bytes()");
    const float thr2 = distance_threshold * distance_threshold;
    ransac_select_kernel<<<pairs, RG_THREADS, 0, stream>>>(starts, total_rows, src_pts, tgt_pts, scores, sample_mode, n_points, seed,
                                                           pair_keys, ws, n_used, selected);
    ROITR_LAUNCH_CHECK();
    ransac_hyp_kernel<<<dim3(ch, pairs), RG_THREADS, 0, stream>>>(starts, total_rows, ws, n_used, seed, pair_keys, iterations, ch, thr2,
                                                                  (double)edge_similarity);
    ROITR_LAUNCH_CHECK();
    ransac_final_kernel<<<pairs, RG_THREADS, 0, stream>>>(starts, total_rows, ws, n_used, seed, pair_keys, ch, thr2,
                                                          (double)edge_similarity, refine_iters, refine_weighted, transforms, inliers,
                                                          best_iteration, valid_hypotheses);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}

extern "C" int roitr_ransac_samples(int pairs, const int* n, const unsigned* pair_keys, unsigned long long seed, int it0, int count,
                                    int* out, hipStream_t stream)
{
    if (it0 < 0 || count < 0 || (long)it0 + count > RG_MAX_ITER)
        return refuse(ROITR_ERR_ARG, "roitr_ransac_samples: iterations must lie in [0, 2^28)");
    if (pairs <= 0 || count == 0) return ROITR_OK;
    if (!n || !pair_keys || !out) return refuse(ROITR_ERR_ARG, "roitr_ransac_samples: null pointer");
    const long total = (long)pairs * count;
    if (total > 0x7fffffffL / 3) return refuse(ROITR_ERR_ARG, "roitr_ransac_samples: pairs x count too large");
    ransac_samples_kernel<<<div_up(total, 256), 256, 0, stream>>>(pairs, n, pair_keys, seed, it0, count, out);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}

extern "C" int roitr_weighted_procrustes(int batch, int n, const float* src_pts, const float* tgt_pts, const float* weights,
                                         float weight_thresh, float eps, float* transforms, hipStream_t stream)
{
    if (batch <= 0) return ROITR_OK;
    if (n < 0 || batch > 0x7fffffff / 16) return refuse(ROITR_ERR_ARG, "roitr_weighted_procrustes: n < 0 or batch too large");
    if (!transforms || (n > 0 && (!src_pts || !tgt_pts))) return refuse(ROITR_ERR_ARG, "roitr_weighted_procrustes: null pointer");
    procrustes_kernel<<<batch, RG_THREADS, 0, stream>>>(n, src_pts, tgt_pts, weights, weight_thresh, eps, transforms);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}
