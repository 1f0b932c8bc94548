// Input preparation in front of the normals: voxel-grid downsampling of raw scans and the point cap.
//
// Reference call sites: the 3DMatch .pth files the reference loads were voxel-downsampled at 2.5 cm beforehand, and
// dataset/tdmatch.py:41,72-78 / dataset/fdmatch.py:49-56 cap every cloud at `points_lim` by np.random.permutation(n)[:points_lim].
//
// (1) roitr_voxel_downsample: Open3D's voxel_down_sample, restated from its published algorithm (Open3D is not vendored in the
// reference tree, parity with the original is unpinned, as for the PCA normals of prep.hip).  Per cloud, float64 on the fp32 inputs:
//     vmb = min_bound - voxel_size * 0.5;  ijk = floor((p - vmb) / voxel_size);  one output per occupied voxel = the sum of the voxel's
//     points IN INPUT ORDER / their count, rounded once to fp32.
// Open3D leaves the output order to a hash map; here it is defined: clouds in input order, voxels ascending in (ix, iy, iz).
//
// Key: cloud (16 bits) | ix (16) | iy (16) | iz (16), payload = the global point index.  A STABLE least-significant-digit radix sort
// (8-bit digits; per pass the classical three kernels: tile histograms, scan, ranked scatter; no workgroup waits for another one inside a
// launch) brings equal keys together and keeps the points of a voxel in input order, which makes the float64 sum reproducible bit for
// bit -- a hash table filled with atomics, or float atomics for the sums, would make it depend on arrival order.  Digits that are the
// same in every key of the call (all_and == all_or over the keys, two device words) are skipped: every pass kernel reads those words,
// returns at once on a dead digit, and derives from them which of the two buffers holds the current order.  No host synchronisation.
//
// (2) roitr_random_subsample: uniform without replacement, per cloud: u(j) = splitmix64(seed ^ VX_SUB_DOMAIN ^ splitmix64(key << 32 | j))
// >> 16 (48 bits), the `limit` points of smallest (u, j) are kept, reported as ascending global row indices.  The same sort on
// cloud | u (stable: ties fall to the smaller j).  The selection is a function of (seed, key, cloud size, limit) alone.
#include "common.h"
#include "flag_compact.h"
#include "registration_math.h"
#include "roitr_pointops.h"
#include "workspace.h"

#include <cmath>

namespace {

typedef unsigned long long u64;

constexpr int VX_THREADS = FLAG_THREADS;
constexpr int VX_ITEMS = FLAG_ITEMS;
constexpr int VX_TILE = FLAG_TILE;   // items per workgroup of every tiled kernel here: the sort's tiles are the flag tiles
constexpr int VX_WAVES = VX_THREADS / 64;
constexpr int VX_RADIX = 256;
constexpr int VX_PASSES = 8;
constexpr int VX_AXIS_MAX = 65535;
constexpr int VX_MAX_CLOUDS = 65536;
#define VX_SUB_DOMAIN 0xE7037ED1A0B428DBull   // the cap's own domain of the counter-based generator (distinct from RG_SEL_DOMAIN)

// ------------------------------------------------------------------ workspace
struct Workspace {
    u64* key[2];
    unsigned* pay[2];
    int* hist;          // (VX_RADIX, nblk) tile histograms, bin-major; exclusive row scans after the scan kernel
    int* bintotal;      // VX_RADIX
    u64* andor;         // all_and, all_or over the keys of the call
    unsigned* bounds;   // (b, 3) order-preserving images of the per-cloud minima
    unsigned char* flag;   // n, no padding is read
    int* blocksum;      // tile sums of the flags -> exclusive bases (flag_compact.h), the last entry: total
    int* start;         // n: first sorted position of every voxel
    size_t bytes;
};

static Workspace carve(void* ws, int b, int n)
{
    const size_t nblk = (size_t)div_up(n > 0 ? n : 1, VX_TILE);
    Carve c(Carve::aligned(ws));
    Workspace w;
    w.key[0] = c.take<u64>(n);
    w.key[1] = c.take<u64>(n);
    w.pay[0] = c.take<unsigned>(n);
    w.pay[1] = c.take<unsigned>(n);
    w.hist = c.take<int>((size_t)VX_RADIX * nblk);
    w.bintotal = c.take<int>(VX_RADIX);
    w.andor = c.take<u64>(2);
    w.bounds = c.take<unsigned>((size_t)(b > 0 ? b : 1) * 3);
    w.flag = c.take<unsigned char>(nblk * VX_TILE);   // n of them are used; the size callers are told stays what it has always been
    w.blocksum = c.take<int>((size_t)flag_tiles(n) + 1);
    w.start = c.take<int>(n);
    w.bytes = c.bytes + 256;   // room to align the caller's pointer
    return w;
}

// ------------------------------------------------------------------ small device helpers
// common.h float_image written with a select: the same function, kept for voxel_bounds_kernel alone, whose generated code differs
// with the shared xor form (614 instead of 639 instructions, 25 instead of 24 VGPRs: not measured on a device, so not taken in a change
// that promises identical device code; profiles/eval_layer_refactor_isa.txt)
__device__ __forceinline__ unsigned bounds_image(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ bool pass_live(const u64* __restrict__ andor, int p) { return (((andor[0] ^ andor[1]) >> (8 * p)) & 0xffu) != 0; }
// number of live passes below p: its parity names the buffer that holds the order pass p reads
__device__ __forceinline__ int live_below(const u64* __restrict__ andor, int p)
{
    const u64 diff = andor[0] ^ andor[1];
    int k = 0;
    for (int q = 0; q < p; ++q) k += ((diff >> (8 * q)) & 0xffu) != 0;
    return k;
}

// cloud of item i of a tile whose first and last items lie in clouds c0 and c1
__device__ __forceinline__ int tile_cloud(int i, int c0, int c1, const int* __restrict__ offset, int b)
{
    return c0 == c1 ? c0 : segment_of(i, offset, b);
}

// fold the all_and / all_or words of a block into the two device words (one pair of atomics per block)
__device__ __forceinline__ void fold_andor(u64 a, u64 o, u64* __restrict__ andor, u64* lds /* 2 * VX_WAVES */)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { a &= __shfl_xor(a, s, 64); o |= __shfl_xor(o, s, 64); }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { lds[wave] = a; lds[VX_WAVES + wave] = o; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < VX_WAVES; ++w) { a &= lds[w]; o |= lds[VX_WAVES + w]; }
        atomicAnd(&andor[0], a);
        atomicOr(&andor[1], o);
    }
}

// ------------------------------------------------------------------ (1) bounds, keys
// Per-cloud minima.  The minimum does not depend on the order, so atomicMin on the order-preserving image is deterministic.  A tile
// inside one cloud (almost all of them) reduces in registers and LDS and issues three atomics.  Non-finite coordinate: status bit 2.
__global__ __launch_bounds__(VX_THREADS) void voxel_bounds_kernel(int b, int n, const float* __restrict__ xyz, const int* __restrict__ offset,
                                                                  unsigned* __restrict__ bounds, int* __restrict__ status)
{
    __shared__ unsigned red[VX_WAVES * 4];
    const int base = blockIdx.x * VX_TILE, last = min(base + VX_TILE, n) - 1;
    const int c0 = segment_of(base, offset, b), c1 = segment_of(last, offset, b);
    unsigned m[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
    unsigned bad = 0;
    if (c0 != c1) {
        // A tile that straddles clouds.  Per-lane atomics here put thousands of adds on three words per cloud (measured: 1.4 ms of a
        // 3.4 ms call for the 63 such tiles of 64 x 300 000 points): a round whose 64 consecutive points share a cloud reduces in
        // the wave first, only a round that straddles (or the ragged tail) issues per-lane atomics.
        for (int r = 0; r < VX_ITEMS; ++r) {
            const int i = base + r * VX_THREADS + threadIdx.x;
            const bool valid = i < n;
            const int c = valid ? segment_of(i, offset, b) : -1;
            unsigned v[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
            unsigned nf = 0;
            if (valid) {
                const float x = xyz[(size_t)i * 3], y = xyz[(size_t)i * 3 + 1], z = xyz[(size_t)i * 3 + 2];
                if (isfinite(x) && isfinite(y) && isfinite(z)) { v[0] = bounds_image(x); v[1] = bounds_image(y); v[2] = bounds_image(z); }
                else nf = 1;
            }
            const int cf = __builtin_amdgcn_readfirstlane(c);
            if (cf >= 0 && __ballot(c == cf) == ~0ull) {   // wave-uniform: every lane is here, all in cloud cf
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) v[a] = min(v[a], (unsigned)__shfl_xor((int)v[a], s, 64));
                    nf |= (unsigned)__shfl_xor((int)nf, s, 64);
                }
                if ((threadIdx.x & 63) == 0) {
                    atomicMin(&bounds[cf * 3], v[0]); atomicMin(&bounds[cf * 3 + 1], v[1]); atomicMin(&bounds[cf * 3 + 2], v[2]);
                    if (nf) atomicOr(&status[cf], 2);
                }
            } else if (valid) {
                if (nf) atomicOr(&status[c], 2);
                else { atomicMin(&bounds[c * 3], v[0]); atomicMin(&bounds[c * 3 + 1], v[1]); atomicMin(&bounds[c * 3 + 2], v[2]); }
            }
        }
        return;   // block-uniform
    }
    for (int r = 0; r < VX_ITEMS; ++r) {
        const int i = base + r * VX_THREADS + threadIdx.x;
        if (i >= n) break;
        const float x = xyz[(size_t)i * 3], y = xyz[(size_t)i * 3 + 1], z = xyz[(size_t)i * 3 + 2];
        if (isfinite(x) && isfinite(y) && isfinite(z)) { m[0] = min(m[0], bounds_image(x)); m[1] = min(m[1], bounds_image(y)); m[2] = min(m[2], bounds_image(z)); }
        else bad = 1;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) m[a] = min(m[a], (unsigned)__shfl_xor((int)m[a], s, 64));
        bad |= (unsigned)__shfl_xor((int)bad, s, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave * 4] = m[0]; red[wave * 4 + 1] = m[1]; red[wave * 4 + 2] = m[2]; red[wave * 4 + 3] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < VX_WAVES; ++w) {
            m[0] = min(m[0], red[w * 4]); m[1] = min(m[1], red[w * 4 + 1]); m[2] = min(m[2], red[w * 4 + 2]); bad |= red[w * 4 + 3];
        }
        atomicMin(&bounds[c0 * 3], m[0]); atomicMin(&bounds[c0 * 3 + 1], m[1]); atomicMin(&bounds[c0 * 3 + 2], m[2]);
        if (bad) atomicOr(&status[c0], 2);
    }
}

// Voxel index of one coordinate.  Contraction is off for this function: `mn - vs * 0.5` would be safe either way (the product with
// 0.5 is exact), the rest is a subtraction, a correctly rounded division and a floor; the pragma keeps that true if the form changes.
// Returns -1 when the index does not fit the key's 16 bits per axis.
__device__ __forceinline__ int voxel_index(float p, float mn, double vs)
{
#pragma clang fp contract(off)
    const double vmb = (double)mn - vs * 0.5;
    const double q = floor(((double)p - vmb) / vs);
    return (q >= 0.0 && q <= (double)VX_AXIS_MAX) ? (int)q : -1;
}

__global__ __launch_bounds__(VX_THREADS) void voxel_keys_kernel(int b, int n, const float* __restrict__ xyz, const int* __restrict__ offset,
                                                                double vs, const unsigned* __restrict__ bounds, int* __restrict__ status,
                                                                u64* __restrict__ key, unsigned* __restrict__ pay, u64* __restrict__ andor)
{
    __shared__ u64 red[2 * VX_WAVES];
    const int base = blockIdx.x * VX_TILE, last = min(base + VX_TILE, n) - 1;
    const int c0 = segment_of(base, offset, b), c1 = segment_of(last, offset, b);
    u64 a = ~0ull, o = 0ull;
    for (int r = 0; r < VX_ITEMS; ++r) {
        const int i = base + r * VX_THREADS + threadIdx.x;
        if (i >= n) break;
        const int c = tile_cloud(i, c0, c1, offset, b);
        u64 k = (u64)c << 48;
        if (!(status[c] & 2)) {   // bit 2 is complete: the bounds kernel has finished.  Bit 1 is set below and read by later kernels only
            const int ix = voxel_index(xyz[(size_t)i * 3], image_float(bounds[c * 3]), vs);
            const int iy = voxel_index(xyz[(size_t)i * 3 + 1], image_float(bounds[c * 3 + 1]), vs);
            const int iz = voxel_index(xyz[(size_t)i * 3 + 2], image_float(bounds[c * 3 + 2]), vs);
            if ((ix | iy | iz) < 0) atomicOr(&status[c], 1);
            else k |= (u64)ix << 32 | (u64)iy << 16 | (u64)iz;
        }
        key[i] = k;
        pay[i] = (unsigned)i;
        a &= k; o |= k;
    }
    fold_andor(a, o, andor, red);
}

// ------------------------------------------------------------------ (2) keys of the cap
__global__ __launch_bounds__(VX_THREADS) void subsample_keys_kernel(int b, int n, const int* __restrict__ offset, u64 seed,
                                                                    const int* __restrict__ cloud_keys, u64* __restrict__ key,
                                                                    unsigned* __restrict__ pay, u64* __restrict__ andor)
{
    __shared__ u64 red[2 * VX_WAVES];
    const int base = blockIdx.x * VX_TILE, last = min(base + VX_TILE, n) - 1;
    const int c0 = segment_of(base, offset, b), c1 = segment_of(last, offset, b);
    u64 a = ~0ull, o = 0ull;
    for (int r = 0; r < VX_ITEMS; ++r) {
        const int i = base + r * VX_THREADS + threadIdx.x;
        if (i >= n) break;
        const int c = tile_cloud(i, c0, c1, offset, b);
        const unsigned j = (unsigned)(i - (c ? offset[c - 1] : 0));
        const unsigned ck = cloud_keys ? (unsigned)cloud_keys[c] : (unsigned)c;
        const u64 u = rg_splitmix64(seed ^ VX_SUB_DOMAIN ^ rg_splitmix64(((u64)ck << 32) | (u64)j)) >> 16;
        const u64 k = (u64)c << 48 | u;
        key[i] = k;
        pay[i] = (unsigned)i;
        a &= k; o |= k;
    }
    fold_andor(a, o, andor, red);
}

// ------------------------------------------------------------------ the sort: three kernels per 8-bit digit
__global__ __launch_bounds__(VX_THREADS) void sort_hist_kernel(int n, int nblk, int p, const u64* __restrict__ andor, const u64* __restrict__ key0,
                                                               const u64* __restrict__ key1, int* __restrict__ hist)
{
    if (!pass_live(andor, p)) return;
    __shared__ int h[VX_RADIX];
    const u64* __restrict__ src = (live_below(andor, p) & 1) ? key1 : key0;
    h[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * VX_TILE;
    for (int r = 0; r < VX_ITEMS; ++r) {
        const int i = base + r * VX_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&h[(unsigned)(src[i] >> (8 * p)) & 255u], 1);   // integer LDS atomics: the counts do not depend on the order
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

// one block per bin: the row of tile counts becomes its exclusive scan, the row total goes to bintotal
__global__ __launch_bounds__(VX_THREADS) void sort_scan_kernel(int nblk, int p, const u64* __restrict__ andor, int* __restrict__ hist,
                                                               int* __restrict__ bintotal)
{
    if (!pass_live(andor, p)) return;
    __shared__ int wsum[VX_WAVES];
    __shared__ int carry;
    int* __restrict__ row = hist + (size_t)blockIdx.x * nblk;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int s = 0; s < nblk; s += VX_THREADS) {
        const int j = s + threadIdx.x;
        const int v = j < nblk ? row[j] : 0;
        const int end = block_running_scan<VX_THREADS>(v, wsum, &carry);
        if (j < nblk) row[j] = end - v;
    }
    if (threadIdx.x == 0) bintotal[blockIdx.x] = carry;
}

// Stable ranked scatter of one tile.  Wave w owns items [w * 1024, (w + 1) * 1024) of the tile, 16 rounds of 64 consecutive items, so
// (wave, round, lane) order is input order.  Per round the lanes with the same digit find each other with eight ballots; the lowest of
// them advances the wave's counter of that digit in LDS, the rank is that counter plus the number of equal lanes below.  Wave bases and
// digit bases then give every item its place in the tile's digit-ordered image in LDS, which is written out run by run.
__global__ __launch_bounds__(VX_THREADS) void sort_scatter_kernel(int n, int nblk, int p, const u64* __restrict__ andor, u64* __restrict__ key0,
                                                                  u64* __restrict__ key1, unsigned* __restrict__ pay0, unsigned* __restrict__ pay1,
                                                                  const int* __restrict__ hist, const int* __restrict__ bintotal)
{
    if (!pass_live(andor, p)) return;
    __shared__ u64 key_s[VX_TILE];
    __shared__ unsigned pay_s[VX_TILE];
    __shared__ int wave_cnt[VX_WAVES * VX_RADIX];
    __shared__ int lbase[VX_RADIX], gbase[VX_RADIX];
    __shared__ int wsum[VX_WAVES];
    const bool odd = live_below(andor, p) & 1;
    const u64* __restrict__ src = odd ? key1 : key0;
    const unsigned* __restrict__ srcp = odd ? pay1 : pay0;
    u64* __restrict__ dst = odd ? key0 : key1;
    unsigned* __restrict__ dstp = odd ? pay0 : pay1;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int base = blockIdx.x * VX_TILE;
    const int shift = 8 * p;

    const int tot = bintotal[t];
    const int bin_excl = block_incl_scan<VX_THREADS>(tot, wsum) - tot;   // first output position of digit t
    for (int w = 0; w < VX_WAVES; ++w) wave_cnt[w * VX_RADIX + t] = 0;
    __syncthreads();

    u64 key[VX_ITEMS];
    unsigned pay[VX_ITEMS];
    int rank[VX_ITEMS];
    volatile int* wc = wave_cnt + wave * VX_RADIX;
    const u64 below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < VX_ITEMS; ++r) {
        const int i = base + wave * (VX_TILE / VX_WAVES) + r * 64 + lane;
        const bool valid = i < n;
        key[r] = valid ? src[i] : 0ull;
        pay[r] = valid ? srcp[i] : 0u;
    }
#pragma unroll
    for (int r = 0; r < VX_ITEMS; ++r) {
        const bool valid = base + wave * (VX_TILE / VX_WAVES) + r * 64 + lane < n;
        const unsigned d = (unsigned)(key[r] >> shift) & 255u;
        u64 peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1u;
            const u64 m = __ballot(one);
            peers &= one ? m : ~m;
        }
        peers = valid ? peers : 0ull;
        const int leader = peers ? __ffsll((long long)peers) - 1 : lane;
        int old = 0;
        if (valid && lane == leader) { old = wc[d]; wc[d] = old + __popcll(peers); }
        old = __shfl(old, leader, 64);
        rank[r] = old + __popcll(peers & below);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {   // digit t: wave counts -> exclusive wave bases; tile total -> base inside the tile image and in the output
        int run = 0;
        for (int w = 0; w < VX_WAVES; ++w) { const int c = wave_cnt[w * VX_RADIX + t]; wave_cnt[w * VX_RADIX + t] = run; run += c; }
        const int incl = block_incl_scan<VX_THREADS>(run, wsum);
        lbase[t] = incl - run;
        gbase[t] = bin_excl + hist[(size_t)t * nblk + blockIdx.x];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < VX_ITEMS; ++r) {
        const bool valid = base + wave * (VX_TILE / VX_WAVES) + r * 64 + lane < n;
        if (valid) {
            const unsigned d = (unsigned)(key[r] >> shift) & 255u;
            const int lp = lbase[d] + wave_cnt[wave * VX_RADIX + d] + rank[r];
            key_s[lp] = key[r];
            pay_s[lp] = pay[r];
        }
    }
    __syncthreads();
    const int cnt = min(VX_TILE, n - base);
    for (int j = t; j < cnt; j += VX_THREADS) {
        const u64 k = key_s[j];
        const unsigned d = (unsigned)(k >> shift) & 255u;
        const int q = gbase[d] + (j - lbase[d]);
        dst[q] = k;
        dstp[q] = pay_s[j];
    }
}

// ------------------------------------------------------------------ flags -> ordered positions (flag_compact.h: tile sums, scan; the final
// pass of the cap is that file's compaction, the one of the voxels is voxel_assign_kernel on its tile_inclusive)
// voxel heads in the sorted order: the first point of every run of equal keys, none in a cloud with a status bit
__global__ __launch_bounds__(VX_THREADS) void voxel_heads_kernel(int n, const u64* __restrict__ andor, const u64* __restrict__ key0,
                                                                 const u64* __restrict__ key1, const int* __restrict__ status,
                                                                 unsigned char* __restrict__ flag)
{
    const u64* __restrict__ key = (live_below(andor, VX_PASSES) & 1) ? key1 : key0;
    const int i = blockIdx.x * VX_THREADS + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    flag[i] = status[(int)(k >> 48)] == 0 && (i == 0 || key[i - 1] != k);
}

// the cap: sorted position inside the cloud below the limit -> the point is kept (flag in INPUT order; the array arrives zeroed)
__global__ __launch_bounds__(VX_THREADS) void subsample_keep_kernel(int n, int limit, const u64* __restrict__ andor, const u64* __restrict__ key0,
                                                                    const u64* __restrict__ key1, const unsigned* __restrict__ pay0,
                                                                    const unsigned* __restrict__ pay1, const int* __restrict__ offset,
                                                                    unsigned char* __restrict__ flag)
{
    const bool odd = live_below(andor, VX_PASSES) & 1;
    const int i = blockIdx.x * VX_THREADS + threadIdx.x;
    if (i >= n) return;
    const int c = (int)((odd ? key1 : key0)[i] >> 48);
    if (i - (c ? offset[c - 1] : 0) < limit) flag[(odd ? pay1 : pay0)[i]] = 1;
}

// sorted position -> voxel id: inverse, the first position of every voxel, and new_offset at the cloud boundaries (the cloud id is in
// the key, clouds without points take the count of the cloud before them)
__global__ __launch_bounds__(VX_THREADS) void voxel_assign_kernel(int b, int n, const u64* __restrict__ andor, const u64* __restrict__ key0,
                                                                  const u64* __restrict__ key1, const unsigned* __restrict__ pay0,
                                                                  const unsigned* __restrict__ pay1, const int* __restrict__ status,
                                                                  const unsigned char* __restrict__ flag, const int* __restrict__ blocksum,
                                                                  int* __restrict__ inverse, int* __restrict__ start, int* __restrict__ new_offset)
{
    __shared__ int incl_s[VX_TILE];
    __shared__ int wsum[VX_WAVES];
    const bool odd = live_below(andor, VX_PASSES) & 1;
    const u64* __restrict__ key = odd ? key1 : key0;
    const unsigned* __restrict__ pay = odd ? pay1 : pay0;
    tile_inclusive(n, flag, blocksum, incl_s, wsum);
    for (int r = 0; r < VX_ITEMS; ++r) {
        const int j = r * VX_THREADS + threadIdx.x, i = blockIdx.x * VX_TILE + j;
        if (i >= n) break;
        const int s = incl_s[j];
        const int c = (int)(key[i] >> 48);
        inverse[pay[i]] = status[c] == 0 ? s - 1 : -1;
        if (flag[i]) start[s - 1] = i;
        const int cn = i == n - 1 ? b : (int)(key[i + 1] >> 48);
        for (int cc = c; cc < cn; ++cc) new_offset[cc] = s;
        if (i == 0) for (int cc = 0; cc < c; ++cc) new_offset[cc] = 0;
    }
}

// One lane per voxel: the run of its points in the sorted order IS their input order (stable sort, payload = input index), summed in
// float64 one after the other from +0, divided by the count (the correctly rounded fp64 division) and rounded once to fp32.
__global__ __launch_bounds__(VX_THREADS) void voxel_mean_kernel(int n, int c, const u64* __restrict__ andor, const u64* __restrict__ key0,
                                                                const u64* __restrict__ key1, const unsigned* __restrict__ pay0,
                                                                const unsigned* __restrict__ pay1, const int* __restrict__ blocksum, int nblk,
                                                                const int* __restrict__ start, const float* __restrict__ xyz,
                                                                const float* __restrict__ attr, float* __restrict__ out_xyz,
                                                                int* __restrict__ out_count, float* __restrict__ out_attr)
{
    const int v = blockIdx.x * VX_THREADS + threadIdx.x;
    if (v >= blocksum[nblk]) return;
    const bool odd = live_below(andor, VX_PASSES) & 1;
    const u64* __restrict__ key = odd ? key1 : key0;
    const unsigned* __restrict__ pay = odd ? pay1 : pay0;
    const int i0 = start[v];
    const u64 k0 = key[i0];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int cnt = 0;
    for (int i = i0; i < n && key[i] == k0; ++i) {
        const size_t q = pay[i];
        sx += (double)xyz[q * 3]; sy += (double)xyz[q * 3 + 1]; sz += (double)xyz[q * 3 + 2];
        ++cnt;
    }
    const double dn = (double)cnt;
    out_xyz[(size_t)v * 3] = (float)(sx / dn); out_xyz[(size_t)v * 3 + 1] = (float)(sy / dn); out_xyz[(size_t)v * 3 + 2] = (float)(sz / dn);
    out_count[v] = cnt;
    for (int ch = 0; ch < c; ch += 4) {   // attribute channels, four at a time over the same run
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        const int m = min(4, c - ch);
        for (int i = i0; i < i0 + cnt; ++i) {
            const float* __restrict__ a = attr + (size_t)pay[i] * c + ch;
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < m) s[k] += (double)a[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < m) out_attr[(size_t)v * c + ch + k] = (float)(s[k] / dn);
    }
}

// one block: new_offset = cumulative min(cloud size, limit)
__global__ __launch_bounds__(VX_THREADS) void subsample_offset_kernel(int b, int limit, const int* __restrict__ offset, int* __restrict__ new_offset)
{
    __shared__ int wsum[VX_WAVES];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int s = 0; s < b; s += VX_THREADS) {
        const int c = s + threadIdx.x;
        const int v = c < b ? min(offset[c] - (c ? offset[c - 1] : 0), limit) : 0;
        const int end = block_running_scan<VX_THREADS>(max(v, 0), wsum, &carry);
        if (c < b) new_offset[c] = end;
    }
}

// the sort of (key, payload) in w.key[0] / w.pay[0]; the sorted order ends in the buffer live_below(andor, VX_PASSES) & 1 names
static int radix_sort(const Workspace& w, int b, int n, hipStream_t stream)
{
    const int nblk = div_up(n, VX_TILE);
    for (int p = 0; p < VX_PASSES; ++p) {
        // the cloud id starts at bit 48: with b <= 256 no key has a bit of the last digit set, and the host knows it
        if (p == VX_PASSES - 1 && b <= 256) continue;
        sort_hist_kernel<<<nblk, VX_THREADS, 0, stream>>>(n, nblk, p, w.andor, w.key[0], w.key[1], w.hist);
        sort_scan_kernel<<<VX_RADIX, VX_THREADS, 0, stream>>>(nblk, p, w.andor, w.hist, w.bintotal);
        sort_scatter_kernel<<<nblk, VX_THREADS, 0, stream>>>(n, nblk, p, w.andor, w.key[0], w.key[1], w.pay[0], w.pay[1], w.hist, w.bintotal);
        ROITR_LAUNCH_CHECK();
    }
    return ROITR_OK;
}

static int init_andor(const Workspace& w, hipStream_t stream)
{
    ROITR_HIP(hipMemsetAsync(w.andor, 0xff, 8, stream));
    ROITR_HIP(hipMemsetAsync(w.andor + 1, 0, 8, stream));
    return ROITR_OK;
}

}  // namespace

extern "C" size_t roitr_voxel_workspace_bytes(int b, int n, int c)
{
    (void)c;   // the attribute means are written straight to out_attr
    return carve(nullptr, b, n > 0 ? n : 0).bytes;
}

extern "C" size_t roitr_subsample_workspace_bytes(int b, int n) { return carve(nullptr, b, n > 0 ? n : 0).bytes; }

extern "C" int roitr_voxel_downsample(int b, int n, const float* xyz, const int* offset, double voxel_size, int c, const float* attr,
                                      float* out_xyz, int* new_offset, int* out_count, int* inverse, float* out_attr, int* status, void* ws,
                                      hipStream_t stream)
{
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size)) return refuse(ROITR_ERR_ARG, "voxel_downsample: voxel_size must be finite and positive");
    if (b <= 0 || b > VX_MAX_CLOUDS) return refuse(ROITR_ERR_ARG, "voxel_downsample: the key holds 16 bits of cloud id (1 <= b <= 65536)");
    if (n < 0 || c < 0 || n > 0x7fffffff - VX_TILE) return refuse(ROITR_ERR_ARG, "voxel_downsample: point or channel count out of range");
    if (!offset || !new_offset || !status || (n > 0 && (!xyz || !out_xyz || !out_count || !inverse || !ws)) || (n > 0 && c > 0 && (!attr || !out_attr)))
        return refuse(ROITR_ERR_ARG, "voxel_downsample: null pointer");
    ROITR_HIP(hipMemsetAsync(status, 0, (size_t)b * 4, stream));
    if (n == 0) {
        ROITR_HIP(hipMemsetAsync(new_offset, 0, (size_t)b * 4, stream));
        return ROITR_OK;
    }
    const Workspace w = carve(ws, b, n);
    const int nblk = div_up(n, VX_TILE);
    ROITR_HIP(hipMemsetAsync(w.bounds, 0xff, (size_t)b * 12, stream));
    int rc = init_andor(w, stream);
    if (rc != ROITR_OK) return rc;
    voxel_bounds_kernel<<<nblk, VX_THREADS, 0, stream>>>(b, n, xyz, offset, w.bounds, status);
    voxel_keys_kernel<<<nblk, VX_THREADS, 0, stream>>>(b, n, xyz, offset, voxel_size, w.bounds, status, w.key[0], w.pay[0], w.andor);
    ROITR_LAUNCH_CHECK();
    rc = radix_sort(w, b, n, stream);
    if (rc != ROITR_OK) return rc;
    voxel_heads_kernel<<<div_up(n, VX_THREADS), VX_THREADS, 0, stream>>>(n, w.andor, w.key[0], w.key[1], status, w.flag);
    flag_tile_bases(n, w.flag, w.blocksum, stream);
    voxel_assign_kernel<<<nblk, VX_THREADS, 0, stream>>>(b, n, w.andor, w.key[0], w.key[1], w.pay[0], w.pay[1], status, w.flag, w.blocksum, inverse,
                                                         w.start, new_offset);
    // the voxel count stays on the device: the grid covers the capacity, lanes past the total leave at once
    voxel_mean_kernel<<<div_up(n, VX_THREADS), VX_THREADS, 0, stream>>>(n, attr && out_attr ? c : 0, w.andor, w.key[0], w.key[1], w.pay[0], w.pay[1],
                                                                         w.blocksum, nblk, w.start, xyz, attr, out_xyz, out_count, out_attr);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}

extern "C" int roitr_random_subsample(int b, int n, const int* offset, int limit, unsigned long long seed, const int* cloud_keys, int* idx,
                                      int* new_offset, void* ws, hipStream_t stream)
{
    if (b <= 0 || b > VX_MAX_CLOUDS) return refuse(ROITR_ERR_ARG, "random_subsample: the key holds 16 bits of cloud id (1 <= b <= 65536)");
    if (limit <= 0 || n < 0 || n > 0x7fffffff - VX_TILE) return refuse(ROITR_ERR_ARG, "random_subsample: limit must be positive");
    if (!offset || !new_offset || (n > 0 && (!idx || !ws))) return refuse(ROITR_ERR_ARG, "random_subsample: null pointer");
    if (n == 0) {
        ROITR_HIP(hipMemsetAsync(new_offset, 0, (size_t)b * 4, stream));
        return ROITR_OK;
    }
    const Workspace w = carve(ws, b, n);
    const int nblk = div_up(n, VX_TILE);
    int rc = init_andor(w, stream);
    if (rc != ROITR_OK) return rc;
    ROITR_HIP(hipMemsetAsync(w.flag, 0, (size_t)n, stream));
    subsample_keys_kernel<<<nblk, VX_THREADS, 0, stream>>>(b, n, offset, seed, cloud_keys, w.key[0], w.pay[0], w.andor);
    ROITR_LAUNCH_CHECK();
    rc = radix_sort(w, b, n, stream);
    if (rc != ROITR_OK) return rc;
    subsample_keep_kernel<<<div_up(n, VX_THREADS), VX_THREADS, 0, stream>>>(n, limit, w.andor, w.key[0], w.key[1], w.pay[0], w.pay[1], offset, w.flag);
    flag_compact(n, w.flag, w.blocksum, idx, nullptr, stream);
    subsample_offset_kernel<<<1, VX_THREADS, 0, stream>>>(b, limit, offset, new_offset);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}
