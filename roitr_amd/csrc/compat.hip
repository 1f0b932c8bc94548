// Spatial-compatibility registration: pose hypotheses from the second-order compatibility
// graph of a correspondence set, for sets without patch structure.  The rules are stated in include/roitr_engine.h above
// roitr_compat_batch.
//
// Pair b owns rows [starts[b], starts[b + 1]); its m = min(n, max_rows) selected rows are numbered a in [0, m).  Everything a pair
// needs lives in the workspace at offsets that are multiples of b: m entries of max_rows, hypothesis slots [b * max_seeds, ...).
// The compatibility matrix C is bit-packed, row a = W = ceil(max_rows / 64) words of 64 bits.  Six launches on the caller's stream:
//   compat_select_kernel     one block per pair: the selected rows (all, or the max_rows of largest (score, -row) by an MSB-first
//                            bisection on float_image(score) and an ordered compaction), their points gathered as float4;
//   compat_graph_kernel      one block per 32 rows a of a pair: a wave owns 8 rows, lane l of chunk c holds point b = 64 c + l in
//                            registers and tests it against the wave's rows; the ballot of the float64 comparison IS word c of row a
//                            (one lane stores it), its population count adds to deg_a.  The b points are staged in LDS 512 at a time;
//   compat_seed_kernel       one block per pair: the S rows of largest (deg, -a) by bisection on the unique key deg << 13 | 8191 - a,
//                            their ranks by counting larger keys among the S chosen;
//   compat_consensus_kernel  one block per 16 seeds of a pair: the 16 seed rows of C sit in LDS; 16 lanes share a candidate row b,
//                            read its words once (one 128-byte line per step) and AND + popcount them against all 16 seed rows, a
//                            4-step exchange leaves lane t with c_b of seed t.  Then a wave per seed takes the exact top k - 1 in
//                            the order of the unique key c_b << 13 | 8191 - b (the (k-1)-th largest c by bisection, ties at it in
//                            index order by a quota), compacts the members in ascending order, 16 lanes
//                            per hypothesis sum the float64 moments and one lane per hypothesis runs the Jacobi solve;
//   compat_verify_kernel     verify_tile of procrustes_block.h, the body lgr_verify_kernel has too: one block per 512 rows of the
//                            concatenated array, one hypothesis per lane; here a slot with the count -1 (invalid) is skipped;
//   compat_global_kernel     arg-max of the counts among the valid hypotheses, then global_refit of procrustes_block.h, as
//                            lgr_global_kernel: `steps` reweighted solves, the final count.
// Every decision up to the member sets is an integer or one float64 comparison per (a, b); the float64 sums run over the member
// index (16 lanes) or the pair's local row index (256 lanes) with fixed butterflies; the only atomics add integer counts.
#include "common.h"
#include "procrustes_block.h"
#include "registration_math.h"
#include "roitr_engine.h"
#include "workspace.h"

namespace {

constexpr int CP_MAX_ROWS = 8192, CP_MAX_SEEDS = 1024, CP_MAX_K = 64;
constexpr int CP_WORDS = CP_MAX_ROWS / 64;   // words of one row of C at the largest max_rows
constexpr int CP_GROWS = 32;                 // rows a per graph block (8 per wave)
constexpr int CP_GTILE = 512;                // points b per LDS tile of the graph kernel (2 x 8 KB)
constexpr int CP_TILE = 16;                  // seeds per consensus block = lanes per candidate row = hypotheses per moment pass

struct CpWorkspace {
    int* m;                      // (pairs) selected rows
    int* sel;                    // (pairs, max_rows) local row of selected row a, ascending
    float4* ps;                  // (pairs, max_rows) selected source points
    float4* pt;                  // (pairs, max_rows) selected target points
    unsigned long long* C;       // (pairs, max_rows, W) bit-packed compatibility
    int* deg;                    // (pairs, max_rows)
    int* seed_a;                 // (pairs, max_seeds) selected row of the seed of every rank
    unsigned short* cw;          // (pairs, max_seeds, max_rows) c_b of every seed
    int* hyp_count;              // (pairs, max_seeds) inliers over the pair's rows, -1: invalid
    float* hyp_T;                // (pairs, max_seeds, 12)
    double* moments;             // (pairs, max_seeds, 15)
    size_t bytes;
};

CpWorkspace carve(void* ws, int pairs, int max_rows, int max_seeds)
{
    const size_t P = (size_t)pairs, M = (size_t)max_rows, S = (size_t)max_seeds, W = (M + 63) / 64;
    Carve c(ws);
    CpWorkspace w;
    w.m = c.take<int>(P);
    w.sel = c.take<int>(P * M);
    w.ps = c.take<float4>(P * M);
    w.pt = c.take<float4>(P * M);
    w.C = c.take<unsigned long long>(P * M * W);
    w.deg = c.take<int>(P * M);
    w.seed_a = c.take<int>(P * S);
    w.cw = c.take<unsigned short>(P * S * M);
    w.hyp_count = c.take<int>(P * S);
    w.hyp_T = c.take<float>(12 * P * S);
    w.moments = c.take<double>(15 * P * S);
    w.bytes = c.bytes;
    return w;
}

// ------------------------------------------------------------------------------------------------------------------ selection
__global__ __launch_bounds__(LG_THREADS) void compat_select_kernel(const int* __restrict__ starts, int total_rows,
                                                                   const float* __restrict__ src, const float* __restrict__ tgt,
                                                                   const float* __restrict__ scores, int max_rows, CpWorkspace ws,
                                                                   int* __restrict__ degree)
{
    __shared__ int wsum[LG_THREADS / 64];
    __shared__ int red4[4];
    __shared__ int carry, carry_eq;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int2 rg = starts_range(starts, b, total_rows);
    const int s = rg.x, n = rg.y - rg.x;
    const int m = min(n, max_rows);
    int* sel = ws.sel + (size_t)b * max_rows;
    float4* ps = ws.ps + (size_t)b * max_rows;
    float4* pt = ws.pt + (size_t)b * max_rows;
    if (tid == 0) ws.m[b] = m;
    if (degree)
        for (int j = tid; j < n; j += LG_THREADS) degree[s + j] = -1;
    auto put = [&](int a, int j) {
        const size_t r = (size_t)(s + j);
        sel[a] = j;
        ps[a] = make_float4(src[3 * r], src[3 * r + 1], src[3 * r + 2], 0.f);
        pt[a] = make_float4(tgt[3 * r], tgt[3 * r + 1], tgt[3 * r + 2], 0.f);
    };
    if (n <= max_rows || !scores) {   // all rows, or the first max_rows rows (equal scores: the lower row wins)
        for (int j = tid; j < m; j += LG_THREADS) put(j, j);
        return;
    }
    // the max_rows-th largest key, MSB first: the largest value v with #{key >= v} >= max_rows
    unsigned thr = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = thr | (1u << bit);
        int c = 0;
        for (int j = tid; j < n; j += LG_THREADS) c += float_image(scores[s + j]) >= cand;
        if (block_sum_i(c, red4) >= max_rows) thr = cand;
    }
    int c = 0;
    for (int j = tid; j < n; j += LG_THREADS) c += float_image(scores[s + j]) > thr;
    const int quota = max_rows - block_sum_i(c, red4);   // rows at the threshold that are taken: the first `quota` in row order
    if (tid == 0) { carry = 0; carry_eq = 0; }
    __syncthreads();
    for (int j0 = 0; j0 < n; j0 += LG_THREADS) {
        const int j = j0 + tid;
        const unsigned key = j < n ? float_image(scores[s + j]) : 0u;
        const bool eq = j < n && key == thr;
        const int eq_end = block_running_scan<LG_THREADS>(eq ? 1 : 0, wsum, &carry_eq);
        const bool take = j < n && (key > thr || (eq && eq_end <= quota));
        const int end = block_running_scan<LG_THREADS>(take ? 1 : 0, wsum, &carry);
        if (take) put(end - 1, j);
    }
}

// ------------------------------------------------------------------------------------------------------------------ graph
__global__ __launch_bounds__(LG_THREADS) void compat_graph_kernel(int max_rows, int words, double compat_dist, CpWorkspace ws)
{
    __shared__ float4 bs[CP_GTILE], bt[CP_GTILE];
    __shared__ float4 as[CP_GROWS], at[CP_GROWS];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = ws.m[b];
    const int a0 = blockIdx.x * CP_GROWS;
    if (a0 >= m) return;
    const float4* ps = ws.ps + (size_t)b * max_rows;
    const float4* pt = ws.pt + (size_t)b * max_rows;
    unsigned long long* C = ws.C + (size_t)b * max_rows * words;
    constexpr int RPW = CP_GROWS / 4;   // rows per wave
    if (tid < CP_GROWS && a0 + tid < m) { as[tid] = ps[a0 + tid]; at[tid] = pt[a0 + tid]; }
    int deg[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) deg[r] = 0;
    for (int t0 = 0; t0 < m; t0 += CP_GTILE) {
        const int tn = min(CP_GTILE, m - t0);
        __syncthreads();   // the previous tile has been read (first round: the a rows are written)
        for (int j = tid; j < tn; j += LG_THREADS) { bs[j] = ps[t0 + j]; bt[j] = pt[t0 + j]; }
        __syncthreads();
        for (int c0 = 0; c0 < tn; c0 += 64) {
            const int jb = c0 + lane, bb = t0 + jb;
            const bool live = jb < tn;
            const float4 p = bs[live ? jb : 0], q = bt[live ? jb : 0];
            const double px = p.x, py = p.y, pz = p.z, qx = q.x, qy = q.y, qz = q.z;
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const int ar = wave * RPW + r, a = a0 + ar;   // the same in every lane of the wave
                if (a < m) {
                    const float4 u = as[ar], v = at[ar];
                    const double d = fabs(rg_len(u.x, u.y, u.z, px, py, pz) - rg_len(v.x, v.y, v.z, qx, qy, qz));
                    const unsigned long long word = __ballot(live && bb != a && d < compat_dist);
                    if (lane == 0) C[(size_t)a * words + ((t0 + c0) >> 6)] = word;
                    deg[r] += __popcll(word);
                }
            }
        }
    }
    if (lane == 0)
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int a = a0 + wave * RPW + r;
            if (a < m) ws.deg[(size_t)b * max_rows + a] = deg[r];
        }
}

// ------------------------------------------------------------------------------------------------------------------ seeds
__global__ __launch_bounds__(LG_THREADS) void compat_seed_kernel(const int* __restrict__ starts, int total_rows, int max_rows,
                                                                 int max_seeds, CpWorkspace ws, int* __restrict__ seeds,
                                                                 int* __restrict__ degree, int* __restrict__ seed_rows)
{
    __shared__ int key[CP_MAX_ROWS];
    __shared__ int chosen[CP_MAX_SEEDS];
    __shared__ int red4[4];
    __shared__ int filled;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int s = starts_range(starts, b, total_rows).x;
    const int m = ws.m[b], S = min(max_seeds, m);
    const int* deg = ws.deg + (size_t)b * max_rows;
    const int* sel = ws.sel + (size_t)b * max_rows;
    for (int a = tid; a < m; a += LG_THREADS) {
        key[a] = deg[a] << 13 | (CP_MAX_ROWS - 1 - a);
        if (degree) degree[s + sel[a]] = deg[a];
    }
    if (tid == 0) { filled = 0; seeds[b] = S; }
    if (seed_rows)
        for (int r = S + tid; r < max_seeds; r += LG_THREADS) seed_rows[(size_t)b * max_seeds + r] = -1;
    __syncthreads();
    if (S == 0) return;
    // the S-th largest key (the keys are distinct): 26 bits, MSB first
    int thr = 0;
    for (int bit = 25; bit >= 0; --bit) {
        const int cand = thr | (1 << bit);
        int c = 0;
        for (int a = tid; a < m; a += LG_THREADS) c += key[a] >= cand;
        if (block_sum_i(c, red4) >= S) thr = cand;
    }
    for (int a = tid; a < m; a += LG_THREADS)
        if (key[a] >= thr) chosen[atomicAdd(&filled, 1)] = key[a];   // any order: the rank below does not depend on it
    __syncthreads();
    for (int i = tid; i < S; i += LG_THREADS) {
        const int mine = chosen[i];
        int rank = 0;
        for (int j = 0; j < S; ++j) rank += chosen[j] > mine;
        const int a = CP_MAX_ROWS - 1 - (mine & (CP_MAX_ROWS - 1));
        ws.seed_a[(size_t)b * max_seeds + rank] = a;
        if (seed_rows) seed_rows[(size_t)b * max_seeds + rank] = sel[a];
    }
}

// ------------------------------------------------------------------------------------------------------------------ consensus
// sum of 16 ints per lane over the 16 lanes of a group, transposed: lane l of the group ends with the total of v[l]
__device__ __forceinline__ int group16_transpose_sum(const int (&v)[16], int l)
{
    const bool b3 = l & 8, b2 = l & 4, b1 = l & 2, b0 = l & 1;
    int w[8], u[4], t[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = (b3 ? v[8 + i] : v[i]) + __shfl_xor(b3 ? v[i] : v[8 + i], 8, 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = (b2 ? w[4 + i] : w[i]) + __shfl_xor(b2 ? w[i] : w[4 + i], 4, 16);
#pragma unroll
    for (int i = 0; i < 2; ++i) t[i] = (b1 ? u[2 + i] : u[i]) + __shfl_xor(b1 ? u[i] : u[2 + i], 2, 16);
    return (b0 ? t[1] : t[0]) + __shfl_xor(b0 ? t[0] : t[1], 1, 16);
}

__global__ __launch_bounds__(LG_THREADS) void compat_consensus_kernel(int max_rows, int words, int max_seeds, int k, CpWorkspace ws,
                                                                      int* __restrict__ seed_members)
{
    __shared__ unsigned long long srow[CP_TILE][CP_WORDS];   // the seed rows of C, 16 KB
    __shared__ int seed_of[CP_TILE];
    __shared__ int member[CP_TILE][CP_MAX_K];
    __shared__ float weight[CP_TILE][CP_MAX_K];
    __shared__ int members[CP_TILE];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = ws.m[b], S = min(max_seeds, m);
    const int r0 = blockIdx.x * CP_TILE;   // first rank of the tile
    if (r0 >= S) return;
    const int live = min(CP_TILE, S - r0), mw = (m + 63) >> 6;
    const unsigned long long* C = ws.C + (size_t)b * max_rows * words;
    const size_t slot0 = (size_t)b * max_seeds + r0;
    unsigned short* cw = ws.cw + slot0 * max_rows;
    if (tid < CP_TILE) seed_of[tid] = tid < live ? ws.seed_a[slot0 + tid] : -1;
    __syncthreads();
    for (int i = tid; i < CP_TILE * mw; i += LG_THREADS) {
        const int t = i / mw, x = i - t * mw;
        srow[t][x] = t < live ? C[(size_t)seed_of[t] * words + x] : 0ull;
    }
    __syncthreads();
    // c_b of the 16 seeds for every candidate row b: 16 lanes per candidate, lane l reads words l, l + 16, ... of row b
    const int g = tid / CP_TILE, l = tid % CP_TILE;
    for (int b0 = 0; b0 < m; b0 += LG_THREADS / CP_TILE) {
        const int cb = b0 + g;                       // the same in the 16 lanes of a group
        const bool row = cb < m;
        unsigned long long any = 0;
        if (row)
#pragma unroll
            for (int t = 0; t < CP_TILE; ++t) any |= srow[t][cb >> 6];
        int c = 0;
        if (row && ((any >> (cb & 63)) & 1)) {       // a candidate no seed of the tile is compatible with has c_b = 0 for all of them
            int part[CP_TILE];
#pragma unroll
            for (int t = 0; t < CP_TILE; ++t) part[t] = 0;
            for (int x = l; x < mw; x += CP_TILE) {
                const unsigned long long w = C[(size_t)cb * words + x];
#pragma unroll
                for (int t = 0; t < CP_TILE; ++t) part[t] += __popcll(w & srow[t][x]);
            }
            c = group16_transpose_sum(part, l);      // lane l: the common neighbours of seed l and the candidate
            c = ((srow[l][cb >> 6] >> (cb & 63)) & 1) ? c : 0;
        }
        if (row && l < live) cw[(size_t)l * max_rows + cb] = (unsigned short)c;
    }
    __syncthreads();   // the block's own writes to cw are visible to all of its waves
    // members: a wave per seed
    const int kk = k - 1;
    for (int t = wave; t < live; t += LG_THREADS / 64) {
        const unsigned short* ct = cw + (size_t)t * max_rows;
        const int sa = seed_of[t];
        // The order (c_b, -b) without a key per candidate: the kk-th largest VALUE of c by bisection (as many passes as the largest c
        // has bits; the loads of a pass are independent, one reduction per pass), then the candidates above it and the first `quota`
        // at it in index order, which the ordered compaction counts as it goes.
        int positive = 0, top = 0;
        for (int bb = lane; bb < m; bb += 64) {
            const int c = ct[bb];
            positive += c > 0;
            top = max(top, c);
        }
        positive = wave_sum_i(positive);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
        int thr = 1, quota = kk;                      // at most kk candidates with c_b > 0: all of them
        if (positive > kk) {
            thr = 0;
            for (int bit = 31 - __clz(top); bit >= 0; --bit) {
                const int cand = thr | (1 << bit);
                int cnt = 0;
#pragma unroll 4
                for (int bb = lane; bb < m; bb += 64) cnt += ct[bb] >= cand;
                if (wave_sum_i(cnt) >= kk) thr = cand;   // v = 1 holds, so thr >= 1
            }
            int above = 0;
#pragma unroll 4
            for (int bb = lane; bb < m; bb += 64) above += ct[bb] > thr;
            quota = kk - wave_sum_i(above);
        }
        int base = 0, at_thr = 0;
        for (int c0 = 0; c0 < m; c0 += 64) {          // ordered compaction: the seed and the taken candidates, ascending
            const int bb = c0 + lane;
            const int c = bb < m ? ct[bb] : 0;
            const unsigned long long below = (1ull << lane) - 1ull;
            const unsigned long long eq = __ballot(c == thr);
            const bool in = bb < m && (bb == sa || c > thr || (c == thr && at_thr + __popcll(eq & below) < quota));
            const unsigned long long mask = __ballot(in);
            if (in) {
                const int pos = base + __popcll(mask & below);
                member[t][pos] = bb;
                weight[t][pos] = (float)(bb == sa ? top : c);
            }
            base += __popcll(mask);
            at_thr += __popcll(eq);
        }
        if (lane == 0) members[t] = base;             // take + 1 <= k
    }
    __syncthreads();
    // moments: 16 lanes per hypothesis, as lgr_local_kernel; a hypothesis without 3 members runs on an empty set
    {
        const int t = g;
        const bool ok = t < live && members[t] >= 3;
        const int len = ok ? members[t] : 0;
        const float4* ps = ws.ps + (size_t)b * max_rows;
        const float4* pt = ws.pt + (size_t)b * max_rows;
        auto rowf = [&](int j, float (&p)[3], float (&q)[3], float& w) {
            const float4 u = ps[member[t][j]], v = pt[member[t][j]];
            p[0] = u.x; p[1] = u.y; p[2] = u.z;
            q[0] = v.x; q[1] = v.y; q[2] = v.z;
            w = weight[t][j];
        };
        double a[7], cs[3], ct[3], Hm[9];
        moments_first(len, l, LG_GROUP, rowf, a);
#pragma unroll
        for (int i = 0; i < 7; ++i) a[i] = lanes_sum_d<LG_GROUP>(a[i]);
        centroids(a, cs, ct);
        moments_second(len, l, LG_GROUP, rowf, cs, ct, Hm);
#pragma unroll
        for (int i = 0; i < 9; ++i) Hm[i] = lanes_sum_d<LG_GROUP>(Hm[i]);
        if (ok && l == 0) {
            double* mo = ws.moments + 15 * (slot0 + t);
#pragma unroll
            for (int i = 0; i < 3; ++i) { mo[i] = cs[i]; mo[3 + i] = ct[i]; }
#pragma unroll
            for (int i = 0; i < 9; ++i) mo[6 + i] = Hm[i];
        }
        if (seed_members && t < live) {
            const int* sel = ws.sel + (size_t)b * max_rows;
            for (int j = l; j < k; j += LG_GROUP) seed_members[(slot0 + t) * k + j] = j < members[t] ? sel[member[t][j]] : -1;
        }
    }
    __syncthreads();
    // solves: one hypothesis per lane
    if (tid < live) {
        const bool ok = members[tid] >= 3;
        float T[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (ok) {
            const double* mo = ws.moments + 15 * (slot0 + tid);
            const double cs[3] = {mo[0], mo[1], mo[2]}, ct[3] = {mo[3], mo[4], mo[5]};
            const double Hm[9] = {mo[6], mo[7], mo[8], mo[9], mo[10], mo[11], mo[12], mo[13], mo[14]};
            rg_solve_rigid(Hm, cs, ct, T);
        }
        float* o = ws.hyp_T + 12 * (slot0 + tid);
#pragma unroll
        for (int i = 0; i < 12; ++i) o[i] = T[i];
        ws.hyp_count[slot0 + tid] = ok ? 0 : -1;
    }
}

// ------------------------------------------------------------------------------------------------------------------ verification
__global__ __launch_bounds__(LG_THREADS) void compat_verify_kernel(int pairs, const int* __restrict__ starts, int total_rows,
                                                                   const float* __restrict__ src, const float* __restrict__ tgt,
                                                                   int max_seeds, CpWorkspace ws, float thr2)
{
    auto slots = [&](int p, int) { return HypSlots<size_t>{min(max_seeds, ws.m[p]), (size_t)p * max_seeds}; };
    verify_tile<true>(pairs, starts, total_rows, src, tgt, slots, ws.hyp_T, ws.hyp_count, thr2);
}

// ------------------------------------------------------------------------------------------------------------------ global stage
__global__ __launch_bounds__(LG_THREADS) void compat_global_kernel(const int* __restrict__ starts, int total_rows,
                                                                   const float* __restrict__ src, const float* __restrict__ tgt,
                                                                   const float* __restrict__ scores, int max_rows, int max_seeds,
                                                                   int steps, float thr2, CpWorkspace ws,
                                                                   float* __restrict__ T_out, int* __restrict__ inliers,
                                                                   int* __restrict__ best_rank, int* __restrict__ best_seed_row,
                                                                   int* __restrict__ hypotheses, int* __restrict__ local_inliers,
                                                                   int* __restrict__ status, float* __restrict__ hyp_transforms,
                                                                   int* __restrict__ hyp_counts, int k, int* __restrict__ seed_members)
{
    __shared__ double red[4 * 9];
    __shared__ unsigned long long redk[LG_THREADS / 64];
    __shared__ int red4[4];
    __shared__ float Ts[12];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int2 rg = starts_range(starts, b, total_rows);
    const int s = rg.x, n = rg.y - rg.x;
    const int H = min(max_seeds, ws.m[b]);
    const size_t hb = (size_t)b * max_seeds;
    // winner: most inliers among the valid hypotheses, the lower rank at equal counts = the largest (count + 1, ~rank) key
    unsigned long long key = 0;
    int valid = 0;
    for (int h = tid; h < H; h += LG_THREADS) {
        const int c = ws.hyp_count[hb + h];
        valid += c >= 0;
        const unsigned long long kq = ((unsigned long long)(unsigned)(c + 1) << 32) | (unsigned)(0x7fffffff - h);
        key = kq > key ? kq : key;
    }
    key = block_winner(key, redk);
    valid = block_sum_i(valid, red4);
    const int best = valid > 0 ? 0x7fffffff - (int)(unsigned)(key & 0xffffffffu) : -1;
    for (int h = tid; h < max_seeds; h += LG_THREADS) {   // every slot of the pair: ranks without a seed read -1 / 0
        if (hyp_counts) hyp_counts[hb + h] = h < H ? ws.hyp_count[hb + h] : -1;
        if (hyp_transforms)
            for (int i = 0; i < 12; ++i) hyp_transforms[12 * (hb + h) + i] = h < H ? ws.hyp_T[12 * (hb + h) + i] : 0.f;
        if (seed_members && h >= H)
            for (int i = 0; i < k; ++i) seed_members[(hb + h) * k + i] = -1;
    }

    float T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    int local, final_count;
    const bool won = best >= 0;
    int st = global_refit(s, n, src, tgt, scores, steps, thr2, won ? ws.hyp_T + 12 * (hb + best) : nullptr,
                          won ? ws.hyp_count + hb + best : nullptr, T, local, final_count, red, red4, Ts);
    if (n > max_rows) st |= ROITR_COMPAT_TRUNCATED;
    write_T44(T_out + 16 * (size_t)b, T);
    if (tid == 0) {
        inliers[b] = final_count;
        best_rank[b] = best;
        best_seed_row[b] = best >= 0 ? ws.sel[(size_t)b * max_rows + ws.seed_a[hb + best]] : -1;
        hypotheses[b] = valid;
        local_inliers[b] = local;
        status[b] = st;
    }
}

bool params_ok(int max_rows, int max_seeds, int k)
{
    return max_rows >= 3 && max_rows <= CP_MAX_ROWS && max_seeds >= 1 && max_seeds <= CP_MAX_SEEDS && k >= 3 && k <= CP_MAX_K;
}

}  // namespace

extern "C" size_t roitr_compat_workspace_bytes(int pairs, int total_rows, int max_rows, int max_seeds, int k)
{
    if (pairs <= 0 || total_rows < 0 || !params_ok(max_rows, max_seeds, k)) return 0;
    return carve(nullptr, pairs, max_rows, max_seeds).bytes;
}

extern "C" int roitr_compat_batch(int pairs, const int* starts, int total_rows, const float* src_pts, const float* tgt_pts,
                                  const float* scores, float compat_dist, float radius, int max_rows, int max_seeds, int k, int steps,
                                  void* workspace, size_t workspace_bytes_given, float* transforms, int* inliers, int* best_rank,
                                  int* best_seed_row, int* seeds, int* hypotheses, int* local_inliers, int* status, int* degree,
                                  int* seed_rows, int* seed_members, float* hyp_transforms, int* hyp_counts, hipStream_t stream)
{
    if (!(compat_dist > 0.f) || !(compat_dist <= 3.402823466e38f))
        return refuse(ROITR_ERR_ARG, "roitr_compat_batch: compat_dist must be finite and positive");
    if (!(radius > 0.f) || !(radius <= 3.402823466e38f)) return refuse(ROITR_ERR_ARG, "roitr_compat_batch: radius must be finite and positive");
    if (max_rows < 3 || max_rows > CP_MAX_ROWS) return refuse(ROITR_ERR_ARG, "roitr_compat_batch: max_rows outside 3 ... 8192");
    if (max_seeds < 1 || max_seeds > CP_MAX_SEEDS) return refuse(ROITR_ERR_ARG, "roitr_compat_batch: max_seeds outside 1 ... 1024");
    if (k < 3 || k > CP_MAX_K) return refuse(ROITR_ERR_ARG, "roitr_compat_batch: k outside 3 ... 64");
    if (steps < 1) return refuse(ROITR_ERR_ARG, "roitr_compat_batch: steps < 1");
    if (pairs <= 0) return ROITR_OK;
    if (total_rows < 0 || pairs > 65535) return refuse(ROITR_ERR_ARG, "roitr_compat_batch: total_rows < 0 or pairs > 65535");
    if (!starts || !transforms || !inliers || !best_rank || !best_seed_row || !seeds || !hypotheses || !local_inliers || !status ||
        (total_rows > 0 && (!src_pts || !tgt_pts)))
        return refuse(ROITR_ERR_ARG, "roitr_compat_batch: null pointer");
    const CpWorkspace ws = carve(workspace, pairs, max_rows, max_seeds);
    if (workspace_bytes_given < ws.bytes || !workspace)
        return refuse(ROITR_ERR_ARG, "roitr_compat_batch: workspace smaller than roitr_compat_workspace_bytes()");
    const float thr2 = radius * radius;
    const int words = (max_rows + 63) / 64;
    compat_select_kernel<<<pairs, LG_THREADS, 0, stream>>>(starts, total_rows, src_pts, tgt_pts, scores, max_rows, ws, degree);
    ROITR_LAUNCH_CHECK();
    compat_graph_kernel<<<dim3(div_up(max_rows, CP_GROWS), pairs), LG_THREADS, 0, stream>>>(max_rows, words, (double)compat_dist, ws);
    ROITR_LAUNCH_CHECK();
    compat_seed_kernel<<<pairs, LG_THREADS, 0, stream>>>(starts, total_rows, max_rows, max_seeds, ws, seeds, degree, seed_rows);
    ROITR_LAUNCH_CHECK();
    compat_consensus_kernel<<<dim3(div_up(max_seeds, CP_TILE), pairs), LG_THREADS, 0, stream>>>(max_rows, words, max_seeds, k, ws,
                                                                                                seed_members);
    ROITR_LAUNCH_CHECK();
    if (total_rows > 0) {
        compat_verify_kernel<<<div_up(total_rows, LG_ROWS), LG_THREADS, 0, stream>>>(pairs, starts, total_rows, src_pts, tgt_pts,
                                                                                    max_seeds, ws, thr2);
        ROITR_LAUNCH_CHECK();
    }
    compat_global_kernel<<<pairs, LG_THREADS, 0, stream>>>(starts, total_rows, src_pts, tgt_pts, scores, max_rows, max_seeds, steps, thr2,
                                                           ws, transforms, inliers, best_rank, best_seed_row, hypotheses, local_inliers,
                                                           status, hyp_transforms, hyp_counts, k, seed_members);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}
