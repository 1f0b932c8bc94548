// The status/clean pass of the point-cloud operators (voxel.hip's successors: pairgt.hip, icp_common.h, fpfh.hip, outlier.hip): is a
// point finite, the copy with non-finite coordinates zeroed that the grid is built on, the cloud of a row, a cloud's clamped row range,
// and the whole pass for the operators that take ONE batch of clouds.  No floating-point arithmetic: it means the same on either side
// of `#pragma clang fp contract(off)`.
#pragma once
#include "common.h"

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// Row t of the copy the grid is built on: a non-finite point becomes the origin.  Its cloud carries a status bit and is skipped by every
// later kernel; the copy only keeps such values away from the grid's cell arithmetic.
__device__ __forceinline__ void store_clean(float* __restrict__ clean, int t, float x, float y, float z, bool ok)
{
    clean[(size_t)t * 3] = ok ? x : 0.f; clean[(size_t)t * 3 + 1] = ok ? y : 0.f; clean[(size_t)t * 3 + 2] = ok ? z : 0.f;
}

// The cloud of row t under the cumulative offsets; -1: a row behind offset[b - 1] belongs to no cloud.
__device__ __forceinline__ int cloud_of_row(int t, const int* __restrict__ offset, int b)
{
    const int c = segment_of(t, offset, b);
    return t >= offset[c] ? -1 : c;
}

// [start, end) of cloud c, clamped into [0, n]: the offsets are the caller's
__device__ __forceinline__ int2 cloud_range(const int* __restrict__ offset, int c, int n)
{
    const int s = min(max(c ? offset[c - 1] : 0, 0), n);
    return make_int2(s, min(max(offset[c], s), n));
}

// The pass of one batch of clouds, for thread t < n: the cloud of the row (the binary search over the offsets is done here, once per
// point, and not by every kernel behind it), the copy, and `bit` into the cloud's status word (integer atomicOr on a word the host
// zeroed) for a non-finite coordinate or, with normals, a non-finite normal.
__device__ __forceinline__ void cloud_prepare(int t, int b, const float* __restrict__ xyz, const float* __restrict__ normals /* nullable */,
                                              const int* __restrict__ offset, float* __restrict__ clean, int* __restrict__ cloud,
                                              int* __restrict__ status, int bit)
{
    const float x = xyz[(size_t)t * 3], y = xyz[(size_t)t * 3 + 1], z = xyz[(size_t)t * 3 + 2];
    const bool ok = finite3(x, y, z);
    store_clean(clean, t, x, y, z, ok);
    const int c = cloud_of_row(t, offset, b);
    cloud[t] = c;
    if (c >= 0 && (!ok || (normals && !finite3(normals[(size_t)t * 3], normals[(size_t)t * 3 + 1], normals[(size_t)t * 3 + 2]))))
        atomicOr(&status[c], bit);
}
