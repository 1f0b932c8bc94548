// Flags -> ascending rows: n flags of one byte each (0 / 1) become the inclusive count of set flags up to every row and the list of
// the flagged rows in ascending order.  Three launches over tiles of 4096 flags (256 threads x 16): tile sums, a one-block exclusive
// scan of them with the total behind it, then a pass that rebuilds the inclusive counts of its tile in LDS.  No workgroup waits for
// another inside a launch.  Users: voxel.hip (the voxel heads, whose final pass is its own; the cap) and outlier.hip (the kept rows).
// Every translation unit that includes it gets its own copy of the kernels (anonymous namespace), like icp_common.h.
#pragma once
#include "common.h"

#include <stdint.h>

namespace {

constexpr int FLAG_THREADS = 256;
constexpr int FLAG_ITEMS = 16;
constexpr int FLAG_TILE = FLAG_THREADS * FLAG_ITEMS;

// tiles of n flags: the tile-sum array holds one word more (the total)
inline int flag_tiles(int n) { return div_up(n > 0 ? n : 1, FLAG_TILE); }

// The flags [at, at + 16) of a thread, flag at + k in byte k & 3 of word k >> 2, zero from n on.  One 16-byte load where the whole group
// lies below n and the address allows it (`at` is a multiple of 16, so that is a property of the array: a carved workspace buffer
// always, a caller's array unless it is a view that starts at an odd row), byte by byte otherwise: no padded array is needed.
__device__ __forceinline__ uint4 flags16(const unsigned char* __restrict__ flag, int at, int n)
{
    if (at + FLAG_ITEMS <= n && (reinterpret_cast<uintptr_t>(flag) & 15) == 0) return *reinterpret_cast<const uint4*>(flag + at);
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < FLAG_ITEMS; ++k)
        if (at + k < n) w[k >> 2] |= (unsigned)flag[at + k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ int flag_count(const uint4& v) { return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w); }   // flags are 0 / 1

__global__ __launch_bounds__(FLAG_THREADS) void flag_sums_kernel(int n, const unsigned char* __restrict__ flag, int* __restrict__ tilesum)
{
    __shared__ int wsum[FLAG_THREADS / 64];
    const int s = block_incl_scan<FLAG_THREADS>(flag_count(flags16(flag, blockIdx.x * FLAG_TILE + threadIdx.x * FLAG_ITEMS, n)), wsum);
    if (threadIdx.x == FLAG_THREADS - 1) tilesum[blockIdx.x] = s;
}

// one block: exclusive scan of the tile sums in place, the total behind them
__global__ __launch_bounds__(FLAG_THREADS) void flag_scan_kernel(int ntile, int* __restrict__ tilesum)
{
    __shared__ int wsum[FLAG_THREADS / 64];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int s = 0; s < ntile; s += FLAG_THREADS) {
        const int j = s + threadIdx.x;
        const int v = j < ntile ? tilesum[j] : 0;
        const int end = block_running_scan<FLAG_THREADS>(v, wsum, &carry);
        if (j < ntile) tilesum[j] = end - v;
    }
    if (threadIdx.x == 0) tilesum[ntile] = carry;
}

// inclusive count of flags up to every item of the tile, into LDS (incl_s: FLAG_TILE words, wsum: FLAG_THREADS / 64); ends in a barrier
__device__ __forceinline__ void tile_inclusive(int n, const unsigned char* __restrict__ flag, const int* __restrict__ tilesum, int* incl_s,
                                               int* wsum)
{
    const uint4 v = flags16(flag, blockIdx.x * FLAG_TILE + threadIdx.x * FLAG_ITEMS, n);
    const int mine = flag_count(v);
    int s = tilesum[blockIdx.x] + block_incl_scan<FLAG_THREADS>(mine, wsum) - mine;
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < FLAG_ITEMS; ++k) {
        s += (w[k >> 2] >> (8 * (k & 3))) & 1u;
        incl_s[threadIdx.x * FLAG_ITEMS + k] = s;
    }
    __syncthreads();
}

// flagged rows in ascending order: index[count - 1] = row, nothing behind the total;  incl (nullable): the inclusive count of every row
__global__ __launch_bounds__(FLAG_THREADS) void flag_compact_kernel(int n, const unsigned char* __restrict__ flag, const int* __restrict__ tilesum,
                                                                    int* __restrict__ index, int* __restrict__ incl)
{
    __shared__ int incl_s[FLAG_TILE];
    __shared__ int wsum[FLAG_THREADS / 64];
    tile_inclusive(n, flag, tilesum, incl_s, wsum);
    for (int r = 0; r < FLAG_ITEMS; ++r) {
        const int j = r * FLAG_THREADS + threadIdx.x, i = blockIdx.x * FLAG_TILE + j;
        if (i >= n) break;
        if (incl) incl[i] = incl_s[j];
        if (flag[i]) index[incl_s[j] - 1] = i;   // the count - 1 < the total <= n
    }
}

// tilesum (flag_tiles(n) + 1 words): the exclusive tile bases, the total behind them
inline void flag_tile_bases(int n, const unsigned char* flag, int* tilesum, hipStream_t stream)
{
    const int ntile = div_up(n, FLAG_TILE);
    flag_sums_kernel<<<ntile, FLAG_THREADS, 0, stream>>>(n, flag, tilesum);
    flag_scan_kernel<<<1, FLAG_THREADS, 0, stream>>>(ntile, tilesum);
}

inline void flag_compact(int n, const unsigned char* flag, int* tilesum, int* index, int* incl, hipStream_t stream)
{
    flag_tile_bases(n, flag, tilesum, stream);
    flag_compact_kernel<<<div_up(n, FLAG_TILE), FLAG_THREADS, 0, stream>>>(n, flag, tilesum, index, incl);
}

}  // namespace
