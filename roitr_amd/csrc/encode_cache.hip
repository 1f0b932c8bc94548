// Encode once, match many (include/roitr_encode.h): the two kernels of roitr_engine_match that are not the forward's, and the
// host-only size query of the cloud cache.  Both kernels are plain streaming copies: no LDS, no cross-lane work.
#include "common.h"
#include "roitr_encode.h"

namespace {

constexpr int GATHER_ROWS = 16;   // node rows per workgroup: 4 waves x 4 passes, one wave per 256-float row and pass

// One workgroup per (slot, tile of GATHER_ROWS node rows).  The slot's cloud and that cloud's segment are read from the table on the
// device; a tile past the segment's end leaves at once (the grid is sized by the largest slot).  The C-float rows move as float4
// (global_load_dwordx4 / global_store_dwordx4, 16 bytes per lane, consecutive lanes on consecutive 16 bytes); masks and coordinates
// of the tile's rows are a few dwords, copied by the first lanes.
__global__ __launch_bounds__(256) void cache_gather_nodes_kernel(RoitrCacheGather a, int tiles)
{
    const int slot = blockIdx.x / tiles;
    const RoitrCloudSeg sg = a.seg[a.slot_cloud[slot]];
    const int r0 = (blockIdx.x % tiles) * GATHER_ROWS;
    if (r0 >= sg.n_nodes) return;
    const int rows = min(GATHER_ROWS, sg.n_nodes - r0);
    const size_t src0 = (size_t)sg.node_row0 + r0;
    const size_t dst0 = (size_t)(slot == 0 ? 0 : a.node_offset[slot - 1]) + r0;
    const int c4 = a.C >> 2;
    const float4* __restrict__ in = reinterpret_cast<const float4*>(a.node_geo) + src0 * c4;
    float4* __restrict__ out = reinterpret_cast<float4*>(a.out_geo) + dst0 * c4;
    const int total = rows * c4;
    for (int i = threadIdx.x; i < total; i += 256) out[i] = in[i];
    if ((int)threadIdx.x < rows) a.out_masks[dst0 + threadIdx.x] = a.node_masks[src0 + threadIdx.x];
    if (a.out_xyz && (int)threadIdx.x < rows * 3) a.out_xyz[dst0 * 3 + threadIdx.x] = a.node_xyz[src0 * 3 + threadIdx.x];
}

// patch_gather_kernel (matching.hip) for the strided layout over cached clouds: per (patch slot, position i) and side the cache row
// of the point (-1 = the zero pad row), its mask and its coordinates.  The node row and the point rows of a side come from the
// table entry of the cloud in that side's slot, not from cumulative offsets of the call.
__global__ void cache_patch_gather_kernel(RoitrCachePatch a, long total)
{
    const long t = blockIdx.x * 256L + threadIdx.x;
    if (t >= total) return;
    const int slot = (int)(t / a.limit), i = (int)(t % a.limit);
    const int pair = slot / a.num_corr, p = slot % a.num_corr;
    const bool live = p < a.n_corr[pair];
#pragma unroll
    for (int side = 0; side < 2; ++side) {  // 0 = tgt (rows of the score matrix), 1 = src (columns)
        const int* corr = side == 0 ? a.tgt_corr : a.src_corr;
        int row = -1, mask = 0; float x = 0.f, y = 0.f, z = 0.f;
        if (live) {
            const RoitrCloudSeg sg = a.seg[a.slot_cloud[side == 0 ? a.pairs + pair : pair]];
            const size_t node = (size_t)sg.node_row0 + corr[(size_t)pair * a.num_corr + p];
            const int li = a.knn_idx[node * a.limit + i];
            mask = a.knn_mask[node * a.limit + i];
            if (li >= 0 && li < sg.n_points) {  // index n_c selects the zero pad row (RIGA_v2.py:86-89)
                row = sg.pt_row0 + li;
                const float* q = a.points + (size_t)row * 3;
                x = q[0]; y = q[1]; z = q[2];
            }
        }
        const size_t o = (size_t)t;
        (side == 0 ? a.tgt_rows : a.src_rows)[o] = row;
        (side == 0 ? a.tgt_masks : a.src_masks)[o] = mask;
        float* pp = (side == 0 ? a.tgt_pts : a.src_pts) + o * 3;
        pp[0] = x; pp[1] = y; pp[2] = z;
    }
}

}  // namespace

extern "C" size_t roitr_engine_encode_bytes(int clouds, const int* n_points, int channels, int point_limit, size_t* per_array8)
{
    if (clouds < 1 || !n_points || channels < 1 || point_limit < 1) return 0;
    size_t by[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const size_t C = (size_t)channels, L = (size_t)point_limit;
    for (int c = 0; c < clouds; ++c) {
        if (n_points[c] < 256) return 0;
        const size_t n = (size_t)n_points[c], n4 = n / 4 / 4 / 4;   // roitr_level_sizes
        by[0] += 4 * 3 * n; by[1] += 4 * C * n; by[2] += 4 * 3 * n4; by[3] += 4 * n4;
        by[4] += 4 * L * n4; by[5] += 4 * L * n4; by[6] += 4 * C * n4; by[7] += 4 * C * n4 * n4;
    }
    size_t sum = 0;
    for (int i = 0; i < 8; ++i) { sum += by[i]; if (per_array8) per_array8[i] = by[i]; }
    return sum;
}

extern "C" int roitr_cache_gather_nodes(const RoitrCacheGather* a, hipStream_t stream)
{
    if (a->slots <= 0 || a->n_max <= 0) return ROITR_OK;
    if (a->C <= 0 || a->C % 4 != 0 || ((uintptr_t)a->node_geo & 15) || ((uintptr_t)a->out_geo & 15)) {
        roitr_set_error("cache gather: rows must be whole float4s (C % 4 == 0, 16-byte aligned arrays)", __FILE__, __LINE__);
        return ROITR_ERR_ARG;
    }
    const int tiles = div_up(a->n_max, GATHER_ROWS);
    if ((long)tiles * a->slots > 0x7fffffffL) { roitr_set_error("cache gather: too many (slot, row tile) workgroups for one launch", __FILE__, __LINE__); return ROITR_ERR_ARG; }
    cache_gather_nodes_kernel<<<tiles * a->slots, 256, 0, stream>>>(*a, tiles);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}

extern "C" int roitr_cache_patch_gather(const RoitrCachePatch* a, hipStream_t stream)
{
    const long total = (long)a->pairs * a->num_corr * a->limit;
    if (total <= 0) return ROITR_OK;
    cache_patch_gather_kernel<<<div_up(total, 256), 256, 0, stream>>>(*a, total);
    ROITR_LAUNCH_CHECK();
    return ROITR_OK;
}
