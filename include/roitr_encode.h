/*
 * roitr_encode.h -- C ABI of libroitr_hip.so, part 3: encode once, match many.
 *
 * roitr_engine_forward (roitr_engine.h) takes pairs and runs the whole network on the 2B clouds of a call, so a cloud that takes
 * part in many pairs is encoded once per pair.  The two calls of this header split the forward where its per-cloud half ends:
 *
 *   roitr_engine_encode   NC clouds, no pairing  ->  the cloud cache (every per-cloud result the pair half reads)
 *   roitr_engine_match    B pairs of cached clouds -> the pair-level outputs of RoitrForwardIO
 *
 * Per cloud (encode): the geometry chain (FPS, grids, kNN + PPF, 3-NN, partition), encoder, decoder, the fine head fine_proj, the
 * input projection geo_in of the global transformer and the cloud's n4 x n4 block of the geometric embedding E.
 * Per pair (match): the layers of the global transformer, the coarse head and coarse matching, the patch arrays, the patch score
 * product, optimal transport and fine matching.
 *
 * Both halves queue the stage functions of the forward itself (csrc/engine.cpp) on the same kernels, and every kernel's rows are
 * independent of the rows beside them (tests/test_timed_shape_gpu.py), so a pair matched from cached encodings equals
 * roitr_engine_forward of that pair BIT FOR BIT (tests/test_encode_match_gpu.py compares with torch.equal).
 *
 * Conventions as in roitr_engine.h: device pointers to contiguous fp32 / int32 unless a field says "host"; the caller owns all
 * memory; the calls are asynchronous on `stream` and return 0 or an error code (text via roitr_last_error()).  The structs below are
 * new in this header; no struct of roitr_engine.h changed and roitr_abi_version() stays 4.
 *
 * Scope.  Each of these returns ROITR_ERR_ARG with a message and launches nothing:
 *   - operand_dtype 1 (bf16 operand storage): the pair half would need a bf16 E and a bf16 copy of the point descriptors in the
 *     cache.  operand_dtype 0 and 2 (f32x3) are supported: every GEMM of both halves goes through the engine's one Gemm object,
 *     which routes the K >= 256 layers to the three-way split exactly as the forward does; a match then equals the f32x3 forward.
 *   - adaptive_coarse (4DMatch: the compacted patch layout with its overflow repeat);
 *   - an engine that is not finalized, clouds < 1, pairs < 1 or more pairs than the forward takes in one call (pairs * num_corr
 *     patch slots must stay below 2^31 / point_limit), a cloud of fewer than 256 points (4 superpoints), a cloud index outside
 *     the table, a table whose channels / limit are not the engine's, a table entry whose node count is not the level-4 size of
 *     its point count, a table with a negative row or with point / node rows past 2^31 (patch rows are int32), a node_geo array
 *     that is not 16-byte aligned;
 *   - a `stream` that is capturing a graph (both calls stage descriptors through pinned host memory and may reallocate scratch).
 * Not offered: ground-truth side outputs (a match has no rot / trans), RoitrForwardIO::inputs_ready.
 * A cache is only valid for the weights it was encoded with: after roitr_engine_set_param / roitr_engine_finalize with other
 * weights the caller encodes again (the engine cannot tell; roitr_amd/riga.py compares weight signatures and refuses).
 */
#ifndef ROITR_ENCODE_H
#define ROITR_ENCODE_H

#include <stddef.h>

#include "roitr_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ the cloud cache
 * Eight arrays, the rows of the cached clouds back to back in each (n = points of the cloud, n4 = n / 64 by the floor rule of
 * roitr_level_sizes, C = 256 * factor, L = point_limit):
 *   points        (n, 3)        the points_out coordinates (what the correspondences are reported in)
 *   point_feats   (n, C)        fine_proj(decoder output): the operand rows of the patch score product, read in place
 *   node_xyz      (n4, 3)
 *   node_masks    (n4)          int32 0 / 1
 *   node_knn_idx  (n4, L)       point indices LOCAL to the cloud, pad = n (as RoitrForwardIO::node_knn_idx)
 *   node_knn_mask (n4, L)
 *   node_geo      (n4, C)       geo_in(encoder output of level 4): the rows the first layer of the global transformer starts from
 *   embedding     (n4, n4, C)   the cloud's block of E, read in place by the self-attention layers (RoitrMha::E / eoff)
 * Bytes per cloud: 4 * (3 n + C n + 3 n4 + n4 + 2 L n4 + C n4 + C n4^2); n = 5000, C = 256, L = 64: 11 531 072 (6.2 MB of it E). */
typedef struct RoitrCloudSeg {
    int pt_row0, n_points;     /* first row and rows of the cloud in points / point_feats */
    int node_row0, n_nodes;    /* first row and rows in node_xyz / node_masks / node_knn_* / node_geo */
    long emb0;                 /* first (i, j) entry of the cloud's block in `embedding`, in entries of C floats (the unit of
                                  RoitrMha::eoff), 64 bits: 600 clouds of 5000 points are 3.7 GB of E */
} RoitrCloudSeg;

/* The table of a cache: base pointers and one RoitrCloudSeg per cloud, on the host (the match plans its launches from it) and the
 * same entries on the device (the two gather kernels read them there).  A cache filled by several encode calls has ONE table: each
 * call was given the base pointers advanced by the rows already filled, and the entries are the concatenation. */
typedef struct RoitrCloudTable {
    int n_clouds, channels, limit;   /* C and L the cache was encoded with */
    const float* points; const float* point_feats; const float* node_xyz; const int* node_masks;
    const int* node_knn_idx; const int* node_knn_mask; const float* node_geo; const float* embedding;
    const RoitrCloudSeg* seg;        /* host, n_clouds entries */
    const RoitrCloudSeg* seg_dev;    /* device, the same entries */
} RoitrCloudTable;

/* Host only (no device is touched): bytes of the eight arrays for `clouds` clouds of n_points[c] points, in the order above, into
 * per_array8 (may be NULL); returns their sum, 0 for an argument it refuses (clouds < 1, a cloud below 256 points). */
size_t roitr_engine_encode_bytes(int clouds, const int* n_points, int channels, int point_limit, size_t* per_array8);

/* ------------------------------------------------------------------ encode
 * Inputs: the per-cloud inputs of RoitrForwardIO for `clouds` >= 1 clouds in any order, no pairing.  Outputs: this call's rows of
 * the eight cache arrays (all required; a second call continues where the first ended: pass the pointers advanced by the rows
 * written so far).  Runs the forward's own stages -- geometry chain without its ground-truth part on the engine's geometry stream,
 * encoder, decoder, fine_proj and geo_in on `stream` -- and joins the geometry stream before it returns control of `stream`.
 * Deterministic; a cloud's rows are the same bytes alone and in any call. */
typedef struct RoitrEncodeIO {
    int clouds;
    const int* n_points;       /* host, `clouds` entries */
    const float* points_geom;  /* (T,3) */
    const float* normals;      /* (T,3) */
    const float* feats;        /* (T,1) */
    const float* points_out;   /* (T,3) or NULL = points_geom */
    float* points; float* point_feats; float* node_xyz; int* node_masks;
    int* node_knn_idx; int* node_knn_mask; float* node_geo; float* embedding;
} RoitrEncodeIO;
int roitr_engine_encode(void* engine, const RoitrEncodeIO* io, roitr_stream_t stream);

/* ------------------------------------------------------------------ match
 * Pair b = (src_cloud[b], tgt_cloud[b]), indices into the table; a cloud may appear in any number of pairs on either side, (a, a)
 * included.  The 2B cloud slots of the call are laid out src_0 .. src_{B-1}, tgt_0 .. tgt_{B-1} like a forward's clouds.  Outputs as
 * the fields of the same names of RoitrForwardIO (strided patch layout, any may be NULL); node_xyz / node_feats are in the call's
 * slot layout (T4 = sum of the slots' node counts).  The cloud-level results (points, point_feats, node_knn_*, node_masks) are not
 * copied: they are the cache rows of the slot's cloud.
 * Runs on `stream` only: a segment gather of the slots' node_geo / node_masks (/ node_xyz) rows into the call layout, the global
 * transformer from its first layer on with E read in the cache, coarse head and matching, the cached patch gather, the patch score
 * product on the cached point_feats rows, optimal transport and fine matching.  Deterministic; a pair's results do not depend on
 * its slot or on the other pairs of the call. */
typedef struct RoitrMatchIO {
    int pairs;                 /* B */
    const int* src_cloud;      /* host, B entries */
    const int* tgt_cloud;      /* host, B entries */
    float* node_xyz;           /* (T4,3) */
    float* node_feats;         /* (T4, C) */
    int* tgt_corr; int* src_corr; float* corr_scores; int* n_corr;   /* (B,P) x3, (B) */
    float* tgt_knn_pts; float* src_knn_pts;    /* (B,P,L,3) */
    int* tgt_knn_masks; int* src_knn_masks;    /* (B,P,L) */
    float* matching_scores;    /* (B,P,L+1,L+1) */
    float* out_tgt_pts; float* out_src_pts; float* out_scores; int* out_patch;
    int* fine_offsets;         /* (B*P) */
    int* n_out;                /* (1) */
    int* pair_starts;          /* (B + 1) */
} RoitrMatchIO;
int roitr_engine_match(void* engine, const RoitrCloudTable* table, const RoitrMatchIO* io, roitr_stream_t stream);

/* ------------------------------------------------------------------ the two kernels of the match that are not the forward's
 * (csrc/encode_cache.hip; the engine calls them, they are exported for the tests and for callers that keep their own cache) */

/* One launch: for every slot s of the call (cloud c = slot_cloud[s], its segment read from seg[c] on the device) the rows
 * node_geo[seg.node_row0 ..+ seg.n_nodes) -> out_geo[node_offset[s - 1] ..), the same rows of node_masks -> out_masks and, when
 * out_xyz != NULL, of node_xyz -> out_xyz.  node_offset: cumulative int32 over the slots (the call layout).  One workgroup per
 * (slot, tile of 16 rows), 16-byte accesses on the C-float rows: C % 4 == 0 and 16-byte aligned node_geo / out_geo. */
typedef struct RoitrCacheGather {
    int slots, C, n_max;       /* n_max: the largest node count of a slot (bounds the grid) */
    const RoitrCloudSeg* seg; const int* slot_cloud; const int* node_offset;
    const float* node_geo; const int* node_masks; const float* node_xyz;
    float* out_geo; int* out_masks; float* out_xyz;
} RoitrCacheGather;
int roitr_cache_gather_nodes(const RoitrCacheGather* a, roitr_stream_t stream);

/* roitr_patch_gather for the strided layout with the node and point segment of each side taken from the cloud table: slot
 * pairs + b of the call is the target of pair b, slot b its source.  tgt_rows / src_rows are rows of the CACHE's points /
 * point_feats (-1 = the zero pad row, for the pad index li == n_c and for dead patch slots; mask as stored, point zero). */
typedef struct RoitrCachePatch {
    int pairs, num_corr, limit;
    const int* n_corr; const int* tgt_corr; const int* src_corr;
    const RoitrCloudSeg* seg; const int* slot_cloud;
    const int* knn_idx; const int* knn_mask; const float* points;
    int* tgt_rows; int* src_rows; int* tgt_masks; int* src_masks; float* tgt_pts; float* src_pts;
} RoitrCachePatch;
int roitr_cache_patch_gather(const RoitrCachePatch* a, roitr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
