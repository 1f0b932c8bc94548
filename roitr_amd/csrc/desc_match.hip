// Descriptor matching: the best target of every source descriptor and the best source of every target
// descriptor, for every pair of a batch, from one fp32 MFMA product per pair whose score matrix never reaches memory.
//
// Reference: lib/utils.py:99-156 (matching_descriptors over square_distance), registration/benchmark_utils.py:42-121
// (mutual_selection, get_inlier_ratio: arg-maxima of src_feat @ tgt_feat^T).  Both build the (N, M) matrix -- 100 MB at 5000 x 5000 --
// and read N + M indices of it.
//
//   dm_prep_kernel     zeroes the per-row and per-column keys, and for metric 1 computes |s|^2 and |t|^2 once (16 lanes per row);
//   dm_tiles_kernel    one block: the prefix sum of ceil(n_b / 64) over the pairs -- the flat (pair, row tile) block map, computed on
//                      the device (no per-pair maximum from the host, no round trip before the launch);
//   dm_match_kernel    gemm.hip's 64 x 64 tile in its TN form (both operands row-major, K contiguous): 4 waves, one 32 x 32
//                      v_mfma_f32_32x32x2_f32 accumulator each, BK = 32, the [kh][row][kk] LDS image, the next slab's staging loads
//                      issued one at a time between the MFMAs.  A block owns one row tile of one pair and walks that pair's column
//                      tiles (every gridDim.y-th one, see below); the store epilogue is replaced by two reductions:
//                        rows     a lane keeps (best score, column) for its 16 accumulator rows across the whole walk, in registers;
//                                 after the walk one butterfly over the 32 lanes that share the rows, then one 64-bit atomicMax per row;
//                        columns  per tile a lane reduces its 16 rows, combines with the lane that holds the other 16 rows of the
//                                 same column, and issues one 64-bit atomicMax per column -- after a plain load of the key has shown
//                                 that it would raise it (keys only grow, so a stale value can only let a redundant atomic through);
//   dm_decode_kernel   key -> (index, value) for every row and column.
//
// KEY = (order-preserving bits of the score << 32) | ~index, scores negated for metric 1 (the smallest distance is the largest key).
// The maximum of a set of keys does not depend on the order of arrival, and among equal scores the larger ~index -- THE LOWEST INDEX
// -- wins.  Inside the block the same (score, index) order is carried as a pair: ascending scans replace on strictly-greater only,
// cross-lane steps compare lexicographically.  -0 is folded into +0 before anything is compared, so the float order inside the block
// and the integer order of the keys agree.  A score is one fixed chain of fp32 FMAs over k, the same in every tile: every output is
// bitwise independent of the batch, of the split of the column walk, of the order blocks finish in and of a repeat of the call.
//
// Column walk split (gridDim.y): one pair of 5000 rows has 79 row tiles, a third of the chip's CUs; the host spreads the column
// tiles of every row tile over up to 16 blocks when the row tiles alone do not fill the chip (a function of the totals, never of
// device data).  That is what the row keys are for: the row side then merges across blocks exactly as the column side does.
#include "common.h"
#include "roitr_engine.h"
#include "gemm_tile.h"
#include "workspace.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int DM_BK = 32, DM_LDR = 20;   // the slab and the row pitch of gemm.hip's [kh][row][kk] LDS image
typedef unsigned long long dm_key;

__device__ __attribute__((aligned(16))) float dm_zero4[4];

struct DmWorkspace { dm_key* row_keys; dm_key* col_keys; float* norm_s; float* norm_t; int* tiles; size_t bytes; };

DmWorkspace dm_carve(void* ws, int pairs, int total_src, int total_tgt)
{
    Carve c(ws);
    DmWorkspace w;
    w.row_keys = c.take<dm_key>(total_src);
    w.col_keys = c.take<dm_key>(total_tgt);
    w.norm_s = c.take<float>(total_src);
    w.norm_t = c.take<float>(total_tgt);
    w.tiles = c.take<int>((size_t)pairs + 1);
    w.bytes = c.bytes;
    return w;
}

__device__ __forceinline__ dm_key dm_make_key(float v, int idx) { return ((dm_key)float_image(v) << 32) | (unsigned)~idx; }

// keys only grow: a value read earlier is a lower bound of the value now, so skipping on `key <= seen` never loses a maximum
__device__ __forceinline__ void dm_raise(dm_key* __restrict__ slot, dm_key key)
{
    const dm_key seen = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (key > seen) atomicMax(slot, key);
}

// (ov, oi) beats (v, i): a larger score, or the same score at a lower index; -1 marks "nothing yet"
__device__ __forceinline__ bool dm_beats(float ov, int oi, float v, int i)
{
    return oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i));
}

__global__ __launch_bounds__(256) void dm_prep_kernel(int dim, int total_src, const float* __restrict__ src_desc, int total_tgt,
                                                      const float* __restrict__ tgt_desc, int want_norms, dm_key* __restrict__ row_keys,
                                                      dm_key* __restrict__ col_keys, float* __restrict__ norm_s, float* __restrict__ norm_t)
{
    const long row = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;   // 16 lanes per row; all 16 take the same branches
    const int sub = threadIdx.x & 15;
    if (row >= (long)total_src + total_tgt) return;
    const bool is_src = row < total_src;
    const long r = is_src ? row : row - total_src;
    if (sub == 0) (is_src ? row_keys : col_keys)[r] = 0;
    if (!want_norms) return;
    const float* x = (is_src ? src_desc : tgt_desc) + (size_t)r * dim;
    float s = 0.f;
    for (int k = sub * 4; k < dim; k += 64) {
        const float4 v = *reinterpret_cast<const float4*>(x + k);
        s = fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, s))));
    }
    s += __shfl_xor(s, 8, 16);
    s += __shfl_xor(s, 4, 16);
    s += __shfl_xor(s, 2, 16);
    s += __shfl_xor(s, 1, 16);
    if (sub == 0) (is_src ? norm_s : norm_t)[r] = s;
}

// tile_starts[p] = sum over q < p of ceil(n_q / 64); one block
__global__ __launch_bounds__(256) void dm_tiles_kernel(int pairs, const int* __restrict__ src_offsets, int total_src, int* __restrict__ tile_starts)
{
    __shared__ int part[256];
    const int chunk = (pairs + 255) / 256;
    const int lo = min(threadIdx.x * chunk, pairs), hi = min(lo + chunk, pairs);
    int s = 0;
    for (int p = lo; p < hi; ++p) { const int2 r = starts_range(src_offsets, p, total_src); s += (r.y - r.x + 63) >> 6; }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = run; run += v; }
        tile_starts[pairs] = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int p = lo; p < hi; ++p) {
        tile_starts[p] = run;
        const int2 r = starts_range(src_offsets, p, total_src);
        run += (r.y - r.x + 63) >> 6;
    }
}

template <bool DIST>
__global__ __launch_bounds__(256) void dm_match_kernel(int pairs, int dim, const int* __restrict__ src_offsets, int total_src,
                                                       const float* __restrict__ src_desc, const int* __restrict__ tgt_offsets, int total_tgt,
                                                       const float* __restrict__ tgt_desc, const int* __restrict__ tile_starts,
                                                       const float* __restrict__ norm_s, const float* __restrict__ norm_t,
                                                       dm_key* __restrict__ row_keys, dm_key* __restrict__ col_keys)
{
    __shared__ __attribute__((aligned(16))) float smem[4 * 64 * DM_LDR];
    float* As = smem;
    float* Bs = smem + 2 * 64 * DM_LDR;
    const int tile = blockIdx.x;
    if (tile >= tile_starts[pairs]) return;   // block-uniform
    const int p = segment_of(tile, tile_starts + 1, pairs);
    const int2 sr = starts_range(src_offsets, p, total_src), tr = starts_range(tgt_offsets, p, total_tgt);
    const int n = sr.y - sr.x, m = tr.y - tr.x;
    const int m0 = (tile - tile_starts[p]) * 64;
    const int nct = (m + 63) >> 6, S = gridDim.y;
    int ct = blockIdx.y;
    if (m0 >= n || ct >= nct) return;   // block-uniform; a pair without targets keeps its zero keys: index -1

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, kh = lane >> 5, ml = lane & 31;
    const int r = tid >> 2, kq = (tid & 3) * 8, kf = (tid & 3) * 4;
    // rows past the tile's end are staged from the pair's last row (resident memory) and masked by index in the epilogue
    const float* arow = src_desc + (size_t)(sr.x + min(m0 + r, n - 1)) * dim;
    auto b_row = [&](int c) { return tgt_desc + (size_t)(tr.x + min(c * 64 + r, m - 1)) * dim; };
    // a lane stages floats kf.. and 16 + kf.. of the slab (two fully used 64-byte segments per row); a float4 lies wholly inside
    // or wholly outside dim (dim % 4 == 0), an outside one reads the resident zeros
    auto src4 = [&](const float* row, int k) { return k < dim ? row + k : (const float*)dm_zero4; };

    const int rbase = m0 + wm * 32 + 4 * kh;   // local row of acc[i]: rbase + (i & 3) + 8 * (i >> 2)
    float sn[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int rr = rbase + (i & 3) + 8 * (i >> 2);
        sn[i] = DIST ? norm_s[sr.x + min(rr, n - 1)] : 0.f;
    }
    float rb[16]; int ri[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { rb[i] = -INFINITY; ri[i] = -1; }
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;

    const float4* ar = reinterpret_cast<const float4*>(As + (kh * 64 + wm * 32 + ml) * DM_LDR);
    const float4* br = reinterpret_cast<const float4*>(Bs + (kh * 64 + wn * 32 + ml) * DM_LDR);
    float4* aw0 = reinterpret_cast<float4*>(As + (0 * 64 + r) * DM_LDR + (kq >> 1));
    float4* aw1 = reinterpret_cast<float4*>(As + (1 * 64 + r) * DM_LDR + (kq >> 1));
    float4* bw0 = reinterpret_cast<float4*>(Bs + (0 * 64 + r) * DM_LDR + (kq >> 1));
    float4* bw1 = reinterpret_cast<float4*>(Bs + (1 * 64 + r) * DM_LDR + (kq >> 1));

    const float* brow = b_row(ct);
    float4 st[4];   // staged: A low, A high, B low, B high
    st[0] = *reinterpret_cast<const float4*>(src4(arow, kf));
    st[1] = *reinterpret_cast<const float4*>(src4(arow, kf + 16));
    st[2] = *reinterpret_cast<const float4*>(src4(brow, kf));
    st[3] = *reinterpret_cast<const float4*>(src4(brow, kf + 16));
    int k0 = 0;
    while (ct < nct) {   // one K slab of one column tile per trip
        __syncthreads();
        *aw0 = make_float4(st[0].x, st[0].z, st[1].x, st[1].z); *aw1 = make_float4(st[0].y, st[0].w, st[1].y, st[1].w);
        *bw0 = make_float4(st[2].x, st[2].z, st[3].x, st[3].z); *bw1 = make_float4(st[2].y, st[2].w, st[3].y, st[3].w);
        __syncthreads();
        // the next trip: the next slab of this tile, or the first slab of the next tile; the last trip re-fetches its own slab
        // (no branch in the instruction stream below)
        int kn = k0 + DM_BK, ctn = ct;
        if (kn >= dim) { kn = 0; ctn = ct + S; }
        const bool more = ctn < nct;
        const float* brn = (more && ctn != ct) ? b_row(ctn) : brow;
        const int kl = (more ? kn : k0) + kf;
        const float* nx[4] = {src4(arow, kl), src4(arow, kl + 16), src4(brn, kl), src4(brn, kl + 16)};
        float af[16], bf[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 a = ar[q], b = br[q];
            af[4 * q] = a.x; af[4 * q + 1] = a.y; af[4 * q + 2] = a.z; af[4 * q + 3] = a.w;
            bf[4 * q] = b.x; bf[4 * q + 1] = b.y; bf[4 * q + 2] = b.z; bf[4 * q + 3] = b.w;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], bf[s], acc, 0, 0, 0);
            if ((s & 3) == 2) {   // gemm.hip, round 4: every staging load hides under a running MFMA
                __builtin_amdgcn_sched_barrier(0);
                st[s >> 2] = *reinterpret_cast<const float4*>(nx[s >> 2]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);   // consumers of the prefetched registers stay below the MFMAs
        if (kn == 0) {   // the tile's scores are complete (block-uniform)
            const int c = ct * 64 + wn * 32 + ml;   // this lane's column, local to the pair
            float cb = -INFINITY;
            int cbi = -1;
            if (c < m) {
                const float tn = DIST ? norm_t[tr.x + c] : 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    // metric 1: square_distance's order, (-2 s.t + |s|^2) + |t|^2, clamped, negated: the smallest distance is the
                    // largest v.  metric 0: + 0 turns -0 into +0 (see the file comment)
                    const float v = DIST ? -fmaxf((fmaf(-2.f, acc[i], sn[i])) + tn, 1e-12f) : acc[i] + 0.f;
                    const int rr = rbase + (i & 3) + 8 * (i >> 2);
                    const bool up = v > rb[i];   // the lane's columns ascend over the walk: strictly greater keeps the lowest
                    rb[i] = up ? v : rb[i];
                    ri[i] = up ? c : ri[i];
                    const bool cu = rr < n && v > cb;   // the lane's rows ascend with i
                    cb = cu ? v : cb;
                    cbi = cu ? rr : cbi;
                }
            }
            const float ov = __shfl_xor(cb, 32);   // the other 16 rows of the same column
            const int oi = __shfl_xor(cbi, 32);
            if (dm_beats(ov, oi, cb, cbi)) { cb = ov; cbi = oi; }
            if (kh == 0 && cbi >= 0) dm_raise(col_keys + tr.x + c, dm_make_key(cb, cbi));
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        }
        if (!more) break;
        ct = ctn; k0 = kn; brow = brn;
    }
    // rows: the 32 lanes of a half wave hold 32 column classes of the same 16 rows
#pragma unroll
    for (int i = 0; i < 16; ++i) {
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(rb[i], off);
            const int oi = __shfl_xor(ri[i], off);
            if (dm_beats(ov, oi, rb[i], ri[i])) { rb[i] = ov; ri[i] = oi; }
        }
        const int rr = rbase + (i & 3) + 8 * (i >> 2);
        if (ml == 0 && rr < n && ri[i] >= 0) dm_raise(row_keys + sr.x + rr, dm_make_key(rb[i], ri[i]));
    }
}

__global__ __launch_bounds__(256) void dm_decode_kernel(int total_src, int total_tgt, int metric, const dm_key* __restrict__ row_keys,
                                                        const dm_key* __restrict__ col_keys, int* __restrict__ row_idx, float* __restrict__ row_val,
                                                        int* __restrict__ col_idx, float* __restrict__ col_val)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)total_src + total_tgt) return;
    const bool is_src = e < total_src;
    const long r = is_src ? e : e - total_src;
    const dm_key k = (is_src ? row_keys : col_keys)[r];
    int idx = -1;
    float val = 0.f;
    if (k != 0) {   // no real key is 0: ~index of an index below 2^31 has its top bit set
        idx = (int)~(unsigned)(k & 0xFFFFFFFFu);
        val = image_float((unsigned)(k >> 32));
        if (metric == 1) val = -val;
    }
    (is_src ? row_idx : col_idx)[r] = idx;
    (is_src ? row_val : col_val)[r] = val;
}

// ---------------------------------------------------------------------------------------------------------------- selection
// element e of pair p under `mode`: does it emit, and which (source, target) pair
__device__ __forceinline__ bool dm_emit(int mode, int e, int n, int m, const int* __restrict__ row_idx, const int* __restrict__ col_idx, int& i, int& j)
{
    if (mode == 1) {
        j = e; i = col_idx[e];
        return i >= 0 && i < n;
    }
    i = e; j = row_idx[e];
    if (j < 0 || j >= m) return false;
    return mode == 0 || col_idx[j] == i;
}

__device__ __forceinline__ int2 dm_sel_range(const int* __restrict__ off, int p)
{
    const int s = max(off[p], 0);
    return make_int2(s, max(off[p + 1], s));
}

// one block per pair.  WRITE = false: corr_starts[p + 1] = the pair's count;  WRITE = true: ordered compaction at corr_starts[p]
template <bool WRITE>
__global__ __launch_bounds__(256) void dm_select_kernel(const int* __restrict__ src_offsets, const int* __restrict__ tgt_offsets,
                                                        const int* __restrict__ row_idx, const int* __restrict__ col_idx, int mode,
                                                        int* __restrict__ corr_starts, int* __restrict__ corr, int capacity)
{
    __shared__ int wsum[4];
    const int p = blockIdx.x;
    const int2 sr = dm_sel_range(src_offsets, p), tr = dm_sel_range(tgt_offsets, p);
    const int n = sr.y - sr.x, m = tr.y - tr.x;
    const int cnt = mode == 1 ? m : n;
    const int* ri = row_idx + sr.x;
    const int* ci = col_idx + tr.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = WRITE ? corr_starts[p] : 0;
    for (int e0 = 0; e0 < cnt; e0 += 256) {   // block-uniform
        const int e = e0 + threadIdx.x;
        int i = 0, j = 0;
        const bool on = e < cnt && dm_emit(mode, e, n, m, ri, ci, i, j);
        const unsigned long long b = __ballot(on);
        if (lane == 0) wsum[wave] = __popcll(b);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { before += w < wave ? wsum[w] : 0; all += wsum[w]; }
        if (WRITE && on) {
            const int slot = base + before + __popcll(b & ((1ull << lane) - 1ull));
            if (slot < capacity) { corr[(size_t)slot * 2] = i; corr[(size_t)slot * 2 + 1] = j; }
        }
        base += all;
        __syncthreads();   // wsum is rewritten in the next trip
    }
    if (!WRITE && threadIdx.x == 0) corr_starts[p + 1] = base;
}

// in place: counts at [1, pairs] -> starts; one block
__global__ __launch_bounds__(256) void dm_scan_kernel(int pairs, int* __restrict__ corr_starts, int* __restrict__ n_out)
{
    __shared__ int part[256];
    const int chunk = (pairs + 255) / 256;
    const int lo = min(threadIdx.x * chunk, pairs), hi = min(lo + chunk, pairs);
    int s = 0;
    for (int p = lo; p < hi; ++p) s += corr_starts[p + 1];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = run; run += v; }
        corr_starts[0] = 0;
        *n_out = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int p = lo; p < hi; ++p) { run += corr_starts[p + 1]; corr_starts[p + 1] = run; }
}

}  // namespace

extern "C" size_t roitr_desc_match_workspace_bytes(int pairs, int total_src, int total_tgt)
{
    if (pairs < 0 || total_src < 0 || total_tgt < 0) return 0;
    return dm_carve(nullptr, pairs, total_src, total_tgt).bytes;
}

extern "C" int roitr_desc_match_batch(int pairs, int dim, const int* src_offsets, int total_src, const float* src_desc,
                                      const int* tgt_offsets, int total_tgt, const float* tgt_desc, int metric, int* row_idx, float* row_val,
                                      int* col_idx, float* col_val, void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    if (pairs < 0 || total_src < 0 || total_tgt < 0) return refuse(ROITR_ERR_ARG, "roitr_desc_match_batch: negative count");
    if (metric != 0 && metric != 1) return refuse(ROITR_ERR_ARG, "roitr_desc_match_batch: metric must be 0 (dot product) or 1 (squared distance)");
    if (dim < 4 || dim > 1024 || dim % 4 != 0)
        return refuse(ROITR_ERR_UNSUPPORTED, "roitr_desc_match_batch: dim must be a multiple of 4 in [4, 1024]");
    if ((pairs > 0 && (!src_offsets || !tgt_offsets)) || (total_src > 0 && (!src_desc || !row_idx || !row_val)) ||
        (total_tgt > 0 && (!tgt_desc || !col_idx || !col_val)))
        return refuse(ROITR_ERR_ARG, "roitr_desc_match_batch: null pointer");
    if ((((uintptr_t)src_desc) | ((uintptr_t)tgt_desc)) & 15)
        return refuse(ROITR_ERR_ARG, "roitr_desc_match_batch: descriptors must be 16-byte aligned");
    const DmWorkspace w = dm_carve(workspace, pairs, total_src, total_tgt);
    if (workspace_bytes < w.bytes || !workspace)
        return refuse(ROITR_ERR_ARG, "roitr_desc_match_batch: workspace smaller than roitr_desc_match_workspace_bytes()");
    const long rows = (long)total_src + total_tgt;
    if (rows == 0) return ROITR_OK;
    dm_key *row_keys = w.row_keys, *col_keys = w.col_keys;
    float *norm_s = w.norm_s, *norm_t = w.norm_t;
    int* tiles = w.tiles;
    dm_prep_kernel<<<div_up(rows * 16, 256), 256, 0, stream>>>(dim, total_src, src_desc, total_tgt, tgt_desc, metric, row_keys, col_keys, norm_s,
                                                               norm_t);
    ROITR_LAUNCH_CHECK();
    if (pairs > 0 && total_src > 0 && total_tgt > 0) {
        dm_tiles_kernel<<<1, 256, 0, stream>>>(pairs, src_offsets, total_src, tiles);
        ROITR_LAUNCH_CHECK();
        // every pair adds at most one partial row tile.  Column walk split: a function of the totals alone
        const int max_tiles = div_up(total_src, 64) + pairs;
        const int col_tiles = div_up(total_tgt, 64);
        int split = 1;
        if (max_tiles < 1024) split = min(min(div_up(1024, max_tiles), 16), col_tiles);
        const dim3 grid(max_tiles, split);
        if (metric == 1)
            dm_match_kernel<true><<<grid, 256, 0, stream>>>(pairs, dim, src_offsets, total_src, src_desc, tgt_offsets, total_tgt, tgt_desc, tiles,
                                                            norm_s, norm_t, row_keys, col_keys);
        else
            dm_match_kernel<false><<<grid, 256, 0, stream>>>(pairs, dim, src_offsets, total_src, src_desc, tgt_offsets, total_tgt, tgt_desc, tiles,
                                                             norm_s, norm_t, row_keys, col_keys);
        ROITR_LAUNCH_CHECK();
    }
    dm_decode_kernel<<<div_up(rows, 256), 256, 0, stream>>>(total_src, total_tgt, metric, row_keys, col_keys, row_idx, row_val, col_idx, col_val);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}

extern "C" int roitr_desc_match_select(int pairs, const int* src_offsets, const int* tgt_offsets, const int* row_idx, const int* col_idx, int mode,
                                       int* corr_starts, int* corr, int capacity, int* n_out, hipStream_t stream)
{
    if (pairs < 0 || capacity < 0) return refuse(ROITR_ERR_ARG, "roitr_desc_match_select: negative count");
    if (mode < 0 || mode > 2) return refuse(ROITR_ERR_ARG, "roitr_desc_match_select: mode must be 0 (row-major), 1 (col-major) or 2 (mutual)");
    if (!corr_starts || !n_out || (pairs > 0 && (!src_offsets || !tgt_offsets || !row_idx || !col_idx)) || (capacity > 0 && !corr))
        return refuse(ROITR_ERR_ARG, "roitr_desc_match_select: null pointer");
    if (pairs > 0) {
        dm_select_kernel<false><<<pairs, 256, 0, stream>>>(src_offsets, tgt_offsets, row_idx, col_idx, mode, corr_starts, (int*)nullptr, 0);
        ROITR_LAUNCH_CHECK();
    }
    dm_scan_kernel<<<1, 256, 0, stream>>>(pairs, corr_starts, n_out);
    ROITR_LAUNCH_CHECK();
    if (pairs > 0 && capacity > 0) {
        dm_select_kernel<true><<<pairs, 256, 0, stream>>>(src_offsets, tgt_offsets, row_idx, col_idx, mode, corr_starts, corr, capacity);
        ROITR_LAUNCH_CHECK();
    }
    return ROITR_OK;
}
