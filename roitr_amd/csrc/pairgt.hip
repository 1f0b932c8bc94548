// Pair ground truth: for B ragged pairs of clouds under their ground-truth transforms, the target
// points within a radius of every moved source point -- counts, the nearest one, the ragged ordered correspondence list
// (lib/utils.py:72-96 get_correspondences: an Open3D KD-tree radius search per point, optional idx[:K]) -- and the per-pair
// reductions on top: the overlap ratio (gt_overlap.log) and the 6x6 Redwood information matrix (gt.info).
//
// The decision is defined in float64 on the fp32 inputs, every product and sum rounded on its own (contraction is off
// for this file), so results are bit-reproducible and equal tests/pairgt_util.py:
//     forward:  p'[c] = ((R[c][0] px + R[c][1] py) + R[c][2] pz) + t[c]
//     inverse:  d = q - t (per component);  q'[c] = (R[0][c] dx + R[1][c] dy) + R[2][c] dz          (target-side overlap)
//     d2 = ((p'x - qx)^2 + (p'y - qy)^2) + (p'z - qz)^2;  (i, j) is a correspondence iff d2 < (double)r * (double)r  (strict)
// Parity with Open3D / nanoflann at the boundary is unpinned.
//
// Search: the per-cloud uniform grid of pointops_knn.hip over the searched clouds, one LANE per query walking the cell rows under the
// ball's bounding box (the shape of knn_within_kernel).  Every candidate of those cells takes the float64 test; there is no fp32
// distance filter.  The list: count pass, exclusive scan (tile sums, one-wave scan, positions), fill pass into a candidate buffer in
// walk order, then one WAVE per run ranks its candidates by (d2, j) and scatters the first K to their final places -- a long run
// occupies one wave's 64 lanes, never one lane.  No host synchronisation, no float atomics, no workgroup waits for another.
#include "cloud_status.h"
#include "common.h"
#include "knn_grid.h"
#include "roitr_pointops.h"
#include "workspace.h"
#include <cmath>

#define PG_NONFINITE 1
#define PG_EMPTY 2
#define PG_OVERFLOW 4
#define PG_THREADS 256
#define PG_ITEMS 8
#define PG_TILE (PG_THREADS * PG_ITEMS)
#define PG_MAX_PAIRS 65536

typedef long long i64;

// hipcc's __dmul_rn / __dadd_rn are plain operators that -ffp-contract=fast would fuse again: contraction is off for the whole file
// and the float64 rule is written with these three.
#pragma clang fp contract(off)

#include "ball_walk.h"   // pg_mul / pg_add / pg_sub, cell_of_axis, ball_cells

namespace {

struct PgWs {
    void* knn;        // grid workspace of the searched clouds
    float* clean;     // (m, 3) searched points with non-finite coordinates zeroed: what the grid is built on
    int* cnt;         // (n) within-radius count per query
    i64* upos;        // (n) first candidate slot of every run (before the cap)
    i64* cpos;        // (n) first list row of every run (after the cap)
    i64* tile;        // (2, ntile) tile sums -> exclusive tile bases: uncapped, capped
    double* cand_d2;  // (capacity) candidate keys, walk order
    int* cand_j;      // (capacity)
    size_t bytes;
};

PgWs carve(void* ws, int b, int n, int m, i64 capacity)
{
    Carve c(Carve::aligned(ws));
    PgWs w;
    const int ntile = div_up(n > 0 ? n : 1, PG_TILE);
    w.knn = c.take<char>(roitr_knn_workspace_bytes(b, m, 0));
    w.clean = c.take<float>((size_t)m * 3);
    w.cnt = c.take<int>(n);
    w.upos = c.take<i64>(n);
    w.cpos = c.take<i64>(n);
    w.tile = c.take<i64>((size_t)ntile * 2);
    w.cand_d2 = c.take<double>(capacity);
    w.cand_j = c.take<int>(capacity);
    w.bytes = c.bytes + 256;   // room to align the caller's pointer
    return w;
}

// One thread per pair, per query point and per searched point: the status bits (integer atomicOr on a word the host zeroed), and the
// copy of the searched points the grid is built on (store_clean of cloud_status.h).
__global__ __launch_bounds__(PG_THREADS) void pairgt_prepare_kernel(int b, int n, int m, const float* __restrict__ src,
                                                                    const int* __restrict__ src_offset, const float* __restrict__ tgt,
                                                                    const int* __restrict__ tgt_offset, const float* __restrict__ rot,
                                                                    const float* __restrict__ trans, float* __restrict__ clean,
                                                                    int* __restrict__ status)
{
    const int t = blockIdx.x * PG_THREADS + threadIdx.x;
    if (t < b) {
        bool ok = true;
        for (int k = 0; k < 9; ++k) ok &= isfinite(rot[(size_t)t * 9 + k]);
        for (int k = 0; k < 3; ++k) ok &= isfinite(trans[(size_t)t * 3 + k]);
        const int ns = src_offset[t] - (t ? src_offset[t - 1] : 0), nt = tgt_offset[t] - (t ? tgt_offset[t - 1] : 0);
        const int bits = (ok ? 0 : PG_NONFINITE) | ((ns <= 0 || nt <= 0) ? PG_EMPTY : 0);
        if (bits) atomicOr(&status[t], bits);
    }
    if (t < n && !finite3(src[(size_t)t * 3], src[(size_t)t * 3 + 1], src[(size_t)t * 3 + 2]))
        atomicOr(&status[segment_of(t, src_offset, b)], PG_NONFINITE);
    if (t < m) {
        const float x = tgt[(size_t)t * 3], y = tgt[(size_t)t * 3 + 1], z = tgt[(size_t)t * 3 + 2];
        const bool ok = finite3(x, y, z);
        if (!ok) atomicOr(&status[segment_of(t, tgt_offset, b)], PG_NONFINITE);
        store_clean(clean, t, x, y, z, ok);
    }
}

// The query in the searched cloud's frame, float64, every operation rounded on its own.
__device__ __forceinline__ void move_point(const float* __restrict__ R, const float* __restrict__ T, bool inverse, double px, double py,
                                           double pz, double (&o)[3])
{
    if (!inverse) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            o[c] = pg_add(pg_add(pg_add(pg_mul((double)R[c * 3], px), pg_mul((double)R[c * 3 + 1], py)),
                                       pg_mul((double)R[c * 3 + 2], pz)), (double)T[c]);
    } else {
        const double dx = pg_sub(px, (double)T[0]), dy = pg_sub(py, (double)T[1]), dz = pg_sub(pz, (double)T[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            o[c] = pg_add(pg_add(pg_mul((double)R[c], dx), pg_mul((double)R[3 + c], dy)), pg_mul((double)R[6 + c], dz));
    }
}

// One lane per query.  FILL = false: count, nearest (d2, j) with ties to the lower j.  FILL = true: the candidates of the run, in walk
// order, into its slots [upos, upos + cnt) of the candidate buffer (a run that does not fit below `capacity` is skipped as a whole).
template <bool FILL>
__global__ __launch_bounds__(PG_THREADS) void pairgt_search_kernel(int b, int n, const float* __restrict__ src,
                                                                   const int* __restrict__ src_offset, const int* __restrict__ tgt_offset,
                                                                   const float* __restrict__ rot, const float* __restrict__ trans,
                                                                   int inverse, double r, const int* __restrict__ status,
                                                                   const RoitrGrid* __restrict__ grids, const int* __restrict__ cell_start,
                                                                   const float4* __restrict__ sorted, int* __restrict__ cnt,
                                                                   int* __restrict__ count, int* __restrict__ nn_idx,
                                                                   double* __restrict__ nn_dist2, const i64* __restrict__ upos, i64 capacity,
                                                                   double* __restrict__ cand_d2, int* __restrict__ cand_j)
{
    const int i = blockIdx.x * PG_THREADS + threadIdx.x;
    if (i >= n) return;
    const int seg = segment_of(i, src_offset, b);
    int have = 0, best_j = -1;
    double best = INFINITY;
    i64 slot = 0;
    int room = 0;
    bool run = !(status[seg] & (PG_NONFINITE | PG_EMPTY));
    if (FILL) {
        room = cnt[i];
        slot = upos[i];
        run = run && room > 0 && slot + room <= capacity;
    }
    if (run) {
        const int t0 = seg ? tgt_offset[seg - 1] : 0;
        const RoitrGrid g = grids[seg];
        const int* cs = cell_start + (size_t)seg * (GRID_MAX_CELLS + 1);
        double q[3];
        move_point(rot + (size_t)seg * 9, trans + (size_t)seg * 3, inverse != 0, (double)src[(size_t)i * 3], (double)src[(size_t)i * 3 + 1],
                   (double)src[(size_t)i * 3 + 2], q);
        const double r2 = pg_mul(r, r);
        int x0, x1, y0, y1, z0, z1;
        float hx, hy, hz;
        ball_cells(q[0], r, g.ox, g.inv_h, g.nx, x0, x1, hx);
        ball_cells(q[1], r, g.oy, g.inv_h, g.ny, y0, y1, hy);
        ball_cells(q[2], r, g.oz, g.inv_h, g.nz, z0, z1, hz);
        // g.ox is the cloud's exact minimum: with fhi < g.ox (see ball_cells: q <= fhi for every accepted q) nothing can be accepted.
        // The far side has no exact bound in the grid; there the clamped edge cells are walked and every candidate fails the test.
        if (!(hx < g.ox || hy < g.oy || hz < g.oz))
            for (int cz = z0; cz <= z1; ++cz)
                for (int cy = y0; cy <= y1; ++cy) {
                    const int rowbase = (cz * g.ny + cy) * g.nx;
                    const int s = cs[rowbase + x0], e = cs[rowbase + x1 + 1];
                    constexpr int NF = 4;
                    for (int p = s; p < e; p += NF) {
                        float4 c[NF];
#pragma unroll
                        for (int u = 0; u < NF; ++u) c[u] = sorted[min(p + u, e - 1)];
#pragma unroll
                        for (int u = 0; u < NF; ++u) {
                            const double dx = pg_sub(q[0], (double)c[u].x), dy = pg_sub(q[1], (double)c[u].y),
                                         dz = pg_sub(q[2], (double)c[u].z);
                            const double d2 = pg_add(pg_add(pg_mul(dx, dx), pg_mul(dy, dy)), pg_mul(dz, dz));
                            if (p + u < e && d2 < r2) {
                                const int j = __float_as_int(c[u].w) - t0;
                                if (FILL) {
                                    if (have < room) { cand_d2[slot + have] = d2; cand_j[slot + have] = j; }
                                } else if (d2 < best || (d2 == best && j < best_j)) {
                                    best = d2; best_j = j;
                                }
                                ++have;
                            }
                        }
                    }
                }
    }
    if (!FILL) {
        cnt[i] = have;
        if (count) count[i] = have;
        if (nn_idx) nn_idx[i] = best_j;
        if (nn_dist2) nn_dist2[i] = best;
    }
}

// One workgroup per pair: hit count, ratio and information matrix.  Thread t sums the pair's points t, t + 256, ... in that order and
// the 256 partial sums fold in a fixed binary tree, so the result depends on the pair alone, not on its slot or the batch.
// info = sum of G^T G, G = [ I3 | -2 [p]x ], p the fp32 query point in its own frame (products of two fp32 values are exact in
// float64): n, sum p and the six second moments, laid out as gt.info (translation block first).
__global__ __launch_bounds__(PG_THREADS) void pairgt_reduce_kernel(const float* __restrict__ src, const int* __restrict__ src_offset,
                                                                   const int* __restrict__ cnt, const int* __restrict__ status,
                                                                   int* __restrict__ n_hit, double* __restrict__ overlap,
                                                                   double* __restrict__ info)
{
    __shared__ double red[10][PG_THREADS];
    const int pr = blockIdx.x, tid = threadIdx.x;
    const int s0 = pr ? src_offset[pr - 1] : 0, ns = src_offset[pr] - s0;
    const bool skip = status[pr] & (PG_NONFINITE | PG_EMPTY);
    double a[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) a[k] = 0.0;
    if (!skip)
        for (int k = tid; k < ns; k += PG_THREADS)
            if (cnt[s0 + k] > 0) {
                const double x = src[(size_t)(s0 + k) * 3], y = src[(size_t)(s0 + k) * 3 + 1], z = src[(size_t)(s0 + k) * 3 + 2];
                a[0] = pg_add(a[0], 1.0);
                a[1] = pg_add(a[1], x); a[2] = pg_add(a[2], y); a[3] = pg_add(a[3], z);
                a[4] = pg_add(a[4], pg_mul(x, x)); a[5] = pg_add(a[5], pg_mul(y, y)); a[6] = pg_add(a[6], pg_mul(z, z));
                a[7] = pg_add(a[7], pg_mul(x, y)); a[8] = pg_add(a[8], pg_mul(x, z)); a[9] = pg_add(a[9], pg_mul(y, z));
            }
#pragma unroll
    for (int k = 0; k < 10; ++k) red[k][tid] = a[k];
    __syncthreads();
    for (int s = PG_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s)
#pragma unroll
            for (int k = 0; k < 10; ++k) red[k][tid] = pg_add(red[k][tid], red[k][tid + s]);
        __syncthreads();
    }
    if (tid == 0) {
        const double cn = red[0][0];   // a count below 2^53: exact
        n_hit[pr] = (int)cn;
        overlap[pr] = skip ? (double)NAN : cn / (double)ns;
    }
    if (info && tid == 0) {
        const double N = red[0][0], sx = red[1][0], sy = red[2][0], sz = red[3][0];
        const double xx = red[4][0], yy = red[5][0], zz = red[6][0], xy = red[7][0], xz = red[8][0], yz = red[9][0];
        // top right: -2 [sum p]x, bottom left its transpose;  bottom right: 4 sum(|p|^2 I - p p^T)
        const double v[36] = {N, 0.0, 0.0, 0.0, 2.0 * sz, -2.0 * sy,
                              0.0, N, 0.0, -2.0 * sz, 0.0, 2.0 * sx,
                              0.0, 0.0, N, 2.0 * sy, -2.0 * sx, 0.0,
                              0.0, -2.0 * sz, 2.0 * sy, 4.0 * (yy + zz), -4.0 * xy, -4.0 * xz,
                              2.0 * sz, 0.0, -2.0 * sx, -4.0 * xy, 4.0 * (xx + zz), -4.0 * yz,
                              -2.0 * sy, 2.0 * sx, 0.0, -4.0 * xz, -4.0 * yz, 4.0 * (xx + yy)};
#pragma unroll
        for (int k = 0; k < 36; ++k) info[(size_t)pr * 36 + k] = v[k];
    }
}

// ------------------------------------------------------------------ run positions: tile sums, one-wave scan, positions
__device__ __forceinline__ i64 wave_incl_scan64(i64 v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const i64 t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
    return v;
}

// Inclusive scan of (u, c) over the block's threads; *tot_u / *tot_c: the block totals.  wsum: 2 * PG_THREADS / 64 words of LDS.
__device__ __forceinline__ void block_scan2(i64& u, i64& c, i64* wsum, i64& tot_u, i64& tot_c)
{
    constexpr int NW = PG_THREADS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u = wave_incl_scan64(u, lane); c = wave_incl_scan64(c, lane);
    if (lane == 63) { wsum[wave] = u; wsum[NW + wave] = c; }
    __syncthreads();
    i64 bu = 0, bc = 0;
    tot_u = 0; tot_c = 0;
    for (int w = 0; w < NW; ++w) {
        if (w < wave) { bu += wsum[w]; bc += wsum[NW + w]; }
        tot_u += wsum[w]; tot_c += wsum[NW + w];
    }
    u += bu; c += bc;
}

template <bool WRITE>
__global__ __launch_bounds__(PG_THREADS) void pairgt_positions_kernel(int n, int ntile, int cap_k, const int* __restrict__ cnt,
                                                                      i64* __restrict__ tile, i64* __restrict__ upos, i64* __restrict__ cpos)
{
    __shared__ i64 wsum[2 * PG_THREADS / 64];
    const int base = blockIdx.x * PG_TILE + threadIdx.x * PG_ITEMS;
    int v[PG_ITEMS];
    i64 u = 0, c = 0;
#pragma unroll
    for (int k = 0; k < PG_ITEMS; ++k) {
        v[k] = base + k < n ? cnt[base + k] : 0;
        u += v[k];
        c += cap_k > 0 ? min(v[k], cap_k) : v[k];
    }
    const i64 mu = u, mc = c;
    i64 tu, tc;
    block_scan2(u, c, wsum, tu, tc);
    if (!WRITE) {
        if (threadIdx.x == 0) { tile[blockIdx.x] = tu; tile[ntile + blockIdx.x] = tc; }
        return;
    }
    i64 ru = tile[blockIdx.x] + u - mu, rc = tile[ntile + blockIdx.x] + c - mc;
#pragma unroll
    for (int k = 0; k < PG_ITEMS; ++k)
        if (base + k < n) {
            upos[base + k] = ru; cpos[base + k] = rc;
            ru += v[k];
            rc += cap_k > 0 ? min(v[k], cap_k) : v[k];
        }
}

// one wave: the tile sums become exclusive tile bases; total[0] = rows of the list, total[1] = candidates before the cap
__global__ __launch_bounds__(64) void pairgt_tile_scan_kernel(int ntile, i64* __restrict__ tile, i64* __restrict__ total)
{
    const int lane = threadIdx.x;
    for (int h = 0; h < 2; ++h) {
        i64 carry = 0;
        for (int t0 = 0; t0 < ntile; t0 += 64) {
            const int t = t0 + lane;
            const i64 v = t < ntile ? tile[(size_t)h * ntile + t] : 0;
            const i64 incl = wave_incl_scan64(v, lane);
            if (t < ntile) tile[(size_t)h * ntile + t] = carry + incl - v;
            carry += __shfl(incl, 63, 64);
        }
        if (lane == 0) total[h == 0 ? 1 : 0] = carry;
    }
}

// one thread per pair: the cumulative list offset (saturated at INT_MAX) and the overflow bit of a pair whose candidates do not all
// lie below `capacity`
__global__ __launch_bounds__(PG_THREADS) void pairgt_offsets_kernel(int b, int n, const int* __restrict__ src_offset,
                                                                    const i64* __restrict__ upos, const i64* __restrict__ cpos,
                                                                    const i64* __restrict__ total, i64 capacity,
                                                                    int* __restrict__ corr_offset, int* __restrict__ status)
{
    const int pr = blockIdx.x * PG_THREADS + threadIdx.x;
    if (pr >= b) return;
    const int s0 = pr ? src_offset[pr - 1] : 0, e = src_offset[pr];
    const i64 end_u = e < n ? upos[e] : total[1], end_c = e < n ? cpos[e] : total[0];
    const i64 begin_u = s0 < n ? upos[s0] : total[1];
    corr_offset[pr] = (int)(end_c < (i64)0x7fffffff ? end_c : (i64)0x7fffffff);
    if (end_u > capacity && end_u > begin_u) atomicOr(&status[pr], PG_OVERFLOW);
}

// One wave per run: every candidate's rank under (d2, j) -- all j of a run differ, so the ranks are a permutation -- by comparing it
// with all candidates of the run, 64 at a time through lane broadcasts; rank < keep goes to list row cpos + rank.  Run length 0 leaves
// at once; a run of L candidates costs ceil(L / 64)^2 * 64 broadcast steps of the one wave that owns it.
__global__ __launch_bounds__(PG_THREADS) void pairgt_rank_kernel(int b, int n, int cap_k, const int* __restrict__ src_offset,
                                                                 const int* __restrict__ cnt, const i64* __restrict__ upos,
                                                                 const i64* __restrict__ cpos, i64 capacity,
                                                                 const double* __restrict__ cand_d2, const int* __restrict__ cand_j,
                                                                 int2* __restrict__ corr)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (PG_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    const int len = cnt[i];
    if (len <= 0) return;
    const i64 u0 = upos[i], c0 = cpos[i];
    if (u0 + len > capacity) return;
    const int keep = cap_k > 0 ? min(len, cap_k) : len;
    const int seg = segment_of(i, src_offset, b);
    const int il = i - (seg ? src_offset[seg - 1] : 0);
    for (int own0 = 0; own0 < len; own0 += 64) {
        const int own = own0 + lane;
        const bool valid = own < len;
        const double d = valid ? cand_d2[u0 + own] : INFINITY;
        const int j = valid ? cand_j[u0 + own] : 0x7fffffff;
        int rank = 0;
        for (int c = 0; c < len; c += 64) {
            const int of = c + lane;
            const double od = of < len ? cand_d2[u0 + of] : INFINITY;
            const int oj = of < len ? cand_j[u0 + of] : 0x7fffffff;
            const int steps = min(64, len - c);
            for (int t = 0; t < steps; ++t) {
                const double bd = __shfl(od, t, 64);
                const int bj = __shfl(oj, t, 64);
                rank += (bd < d || (bd == d && bj < j)) ? 1 : 0;
            }
        }
        if (valid && rank < keep) corr[c0 + rank] = make_int2(il, j);
    }
}

bool common_args_bad(const char* who, int b, int n, int m, float radius, const void* p0, const void* p1, const void* p2, const void* p3,
                     const void* p4, const void* p5, const void* status, const void* ws)
{
    char msg[160];
    if (!(radius > 0.f) || !std::isfinite(radius)) {
        snprintf(msg, sizeof msg, "%s: radius must be finite and positive", who);
    } else if (b <= 0 || b > PG_MAX_PAIRS) {
        snprintf(msg, sizeof msg, "%s: 1 <= B <= %d pairs", who, PG_MAX_PAIRS);
    } else if (n < 0 || m < 0 || n > 0x7fffffff - PG_TILE || m > 0x7fffffff - PG_TILE) {
        snprintf(msg, sizeof msg, "%s: point counts out of range", who);
    } else if (!p2 || !p3 || !p4 || !p5 || !status || !ws || (n > 0 && !p0) || (m > 0 && !p1)) {
        snprintf(msg, sizeof msg, "%s: null pointer", who);
    } else {
        return false;
    }
    roitr_set_error(msg, __FILE__, __LINE__);
    return true;
}

// status, the clean copy, the grid and the count pass: what both entry points start with
int search_front(const PgWs& w, int b, int n, int m, const float* src, const int* src_offset, const float* tgt, const int* tgt_offset,
                 const float* rot, const float* trans, float radius, int inverse, int* count, int* nn_idx, double* nn_dist2, int* status,
                 RoitrGridView& gv, hipStream_t stream)
{
    ROITR_HIP(hipMemsetAsync(status, 0, (size_t)b * 4, stream));
    const int most = n > m ? (n > b ? n : b) : (m > b ? m : b);
    pairgt_prepare_kernel<<<div_up(most, PG_THREADS), PG_THREADS, 0, stream>>>(b, n, m, src, src_offset, tgt, tgt_offset, rot, trans, w.clean,
                                                                             status);
    ROITR_LAUNCH_CHECK();
    gv = roitr_knn_grid_view(b, m, 0, w.knn);
    if (m > 0) {
        const int rc = roitr_knn_build_grid_ex(b, m, 0, w.clean, tgt_offset, w.knn, 0.f, stream);
        if (rc != ROITR_OK) return rc;
    }
    if (n > 0) {
        // m == 0: every pair carries PG_EMPTY and no lane reads the (unbuilt) grid
        pairgt_search_kernel<false><<<div_up(n, PG_THREADS), PG_THREADS, 0, stream>>>(b, n, src, src_offset, tgt_offset, rot, trans, inverse,
                                                                                      (double)radius, status, gv.grids, gv.cell_start, gv.sorted,
                                                                                      w.cnt, count, nn_idx, nn_dist2, nullptr, 0, nullptr, nullptr);
        ROITR_LAUNCH_CHECK();
    }
    return ROITR_OK;
}

}  // namespace

extern "C" size_t roitr_pairgt_workspace_bytes(int b, int n, int m, long long capacity)
{
    if (b <= 0 || n < 0 || m < 0 || capacity < 0) return 0;
    return carve(nullptr, b, n, m, capacity).bytes;
}

extern "C" int roitr_pairgt_stats(int b, int n, int m, const float* src, const int* src_offset, const float* tgt, const int* tgt_offset,
                                  const float* rot, const float* trans, float radius, int inverse, int* count, int* nn_idx,
                                  double* nn_dist2, int* n_hit, double* overlap, double* info, int* status, void* ws, hipStream_t stream)
{
    if (common_args_bad("pairgt_stats", b, n, m, radius, src, tgt, src_offset, tgt_offset, rot, trans, status, ws)) return ROITR_ERR_ARG;
    if (!n_hit || !overlap) {
        roitr_set_error("pairgt_stats: null pointer", __FILE__, __LINE__);
        return ROITR_ERR_ARG;
    }
    const PgWs w = carve(ws, b, n, m, 0);
    RoitrGridView gv;
    const int rc = search_front(w, b, n, m, src, src_offset, tgt, tgt_offset, rot, trans, radius, inverse, count, nn_idx, nn_dist2, status, gv,
                                stream);
    if (rc != ROITR_OK) return rc;
    pairgt_reduce_kernel<<<b, PG_THREADS, 0, stream>>>(src, src_offset, w.cnt, status, n_hit, overlap, info);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}

extern "C" int roitr_pairgt_correspondences(int b, int n, int m, const float* src, const int* src_offset, const float* tgt,
                                            const int* tgt_offset, const float* rot, const float* trans, float radius, int k,
                                            long long capacity, int* corr, int* corr_offset, long long* total, int* status, void* ws,
                                            hipStream_t stream)
{
    if (common_args_bad("pairgt_correspondences", b, n, m, radius, src, tgt, src_offset, tgt_offset, rot, trans, status, ws))
        return ROITR_ERR_ARG;
    if (k < 0 || capacity < 0 || capacity > 0x7fffffffLL || !corr_offset || !total || (capacity > 0 && !corr)) {
        roitr_set_error("pairgt_correspondences: K >= 0 (0: no cap), 0 <= capacity < 2^31, non-null outputs", __FILE__, __LINE__);
        return ROITR_ERR_ARG;
    }
    const PgWs w = carve(ws, b, n, m, capacity);
    RoitrGridView gv;
    const int rc = search_front(w, b, n, m, src, src_offset, tgt, tgt_offset, rot, trans, radius, 0, nullptr, nullptr, nullptr, status, gv,
                                stream);
    if (rc != ROITR_OK) return rc;
    if (n == 0) {
        ROITR_HIP(hipMemsetAsync(corr_offset, 0, (size_t)b * 4, stream));
        ROITR_HIP(hipMemsetAsync(total, 0, 16, stream));
        return ROITR_OK;
    }
    const int ntile = div_up(n, PG_TILE);
    pairgt_positions_kernel<false><<<ntile, PG_THREADS, 0, stream>>>(n, ntile, k, w.cnt, w.tile, w.upos, w.cpos);
    pairgt_tile_scan_kernel<<<1, 64, 0, stream>>>(ntile, w.tile, (i64*)total);
    pairgt_positions_kernel<true><<<ntile, PG_THREADS, 0, stream>>>(n, ntile, k, w.cnt, w.tile, w.upos, w.cpos);
    pairgt_offsets_kernel<<<div_up(b, PG_THREADS), PG_THREADS, 0, stream>>>(b, n, src_offset, w.upos, w.cpos, (const i64*)total, capacity,
                                                                            corr_offset, status);
    ROITR_LAUNCH_CHECK();
    if (capacity > 0) {
        pairgt_search_kernel<true><<<div_up(n, PG_THREADS), PG_THREADS, 0, stream>>>(b, n, src, src_offset, tgt_offset, rot, trans, 0,
                                                                                     (double)radius, status, gv.grids, gv.cell_start, gv.sorted,
                                                                                     w.cnt, nullptr, nullptr, nullptr, w.upos, capacity,
                                                                                     w.cand_d2, w.cand_j);
        pairgt_rank_kernel<<<div_up(n, PG_THREADS / 64), PG_THREADS, 0, stream>>>(b, n, k, src_offset, w.cnt, w.upos, w.cpos, capacity,
                                                                                  w.cand_d2, w.cand_j, (int2*)corr);
        ROITR_LAUNCH_CHECK();
    }
    return ROITR_OK;
}
