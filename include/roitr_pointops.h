/*
 * roitr_pointops.h -- C ABI of libroitr_hip.so, part 1: the `pointops` operator boundary.
 *
 * Boundary B1 of SURVEY.md 8(b).  Plain pointers and sizes only; every pointer is a DEVICE pointer
 * to contiguous fp32 / int32 memory owned by the caller; kernels write in place.
 *
 * Two families:
 *  (1) the reference's own `extern "C"` launcher names and signatures, unchanged (void return,
 *      legacy default stream) -- a maintainer can link the reference's *_cuda.cpp ATen wrappers
 *      against this library instead of its .cu objects;
 *  (2) `roitr_*` variants of the same operators that add a hipStream_t, return an int status
 *      (0 = ok; roitr_last_error() has the text) and, for kNN, expose the grid-accelerated search
 *      and the fused queryandgroup + point-pair-feature outputs.
 *
 * All citations are into /root/reference/cpp_wrappers/pointops/src unless stated otherwise.
 */
#ifndef ROITR_POINTOPS_H
#define ROITR_POINTOPS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* roitr_stream_t; /* == hipStream_t; NULL = legacy default stream */

/* ---- diagnostics ---------------------------------------------------------------------------- */
const char* roitr_last_error(void);
int roitr_abi_version(void);

/* ---- (1) reference launcher names, verbatim ------------------------------------------------- */

/* sampling/sampling_cuda_kernel.h:13.  `n` = longest cloud (selects the tie-break block size,
 * cuda_utils.h:11-14); `tmp` (total points) must arrive filled with 1e10 (functions/pointops.py:22);
 * idx[new_offset[i-1]] = offset[i-1] (first point of each cloud is always selected). */
void furthestsampling_cuda_launcher(int b, int n, const float* xyz, const int* offset, const int* new_offset,
                                    float* tmp, int* idx);

/* knnquery/knnquery_cuda_kernel.h:13.  idx (m, nsample) int32 ascending by distance, dist2 SQUARED
 * distances; nsample <= 100 (knnquery_cuda_kernel.cu:86); slots beyond the cloud size keep
 * (offset_start, 1e10). */
void knnquery_cuda_launcher(int m, int nsample, const float* xyz, const float* new_xyz, const int* offset,
                            const int* new_offset, int* idx, float* dist2);

/* grouping/grouping_cuda_kernel.h:13-14 */
void grouping_forward_cuda_launcher(int m, int nsample, int c, const float* input, const int* idx, float* output);
void grouping_backward_cuda_launcher(int m, int nsample, int c, const float* grad_output, const int* idx, float* grad_input);
/* interpolation/interpolation_cuda_kernel.h:13-14 (output must arrive zeroed, pointops.py:199) */
void interpolation_forward_cuda_launcher(int n, int c, int k, const float* input, const int* idx, const float* weight, float* output);
void interpolation_backward_cuda_launcher(int n, int c, int k, const float* grad_output, const int* idx, const float* weight, float* grad_input);
/* subtraction/subtraction_cuda_kernel.h:13-14 */
void subtraction_forward_cuda_launcher(int n, int nsample, int c, const float* input1, const float* input2, const int* idx, float* output);
void subtraction_backward_cuda_launcher(int n, int nsample, int c, const int* idx, const float* grad_output, float* grad_input1, float* grad_input2);
/* aggregation/aggregation_cuda_kernel.h:13-14 (output must arrive zeroed, pointops.py:146) */
void aggregation_forward_cuda_launcher(int n, int nsample, int c, int w_c, const float* input, const float* position, const float* weight, const int* idx, float* output);
void aggregation_backward_cuda_launcher(int n, int nsample, int c, int w_c, const float* input, const float* position, const float* weight, const int* idx, const float* grad_output, float* grad_input, float* grad_position, float* grad_weight);

/* ---- (2) stream + status variants ------------------------------------------------------------ */

int roitr_furthestsampling(int b, int n_max, const float* xyz, const int* offset, const int* new_offset, float* tmp,
                           int* idx, roitr_stream_t stream);
/* The sampling chain of a hierarchy (model/model.py:56-64 called level after level): the next level samples THIS level's picks in
 * pick order from the same first point, so while every arg-max among this level's first m / track_div picks was attained by
 * exactly one point, the next level's result is the prefix 0 .. m'-1 of those picks (csrc/pointops_fps.hip).  tie_out (b ints,
 * device; optional) receives per cloud the first pick index with a shared arg-max (INT_MAX: none in the tracked range);
 * prev_tie (optional) = the tie_out of the call whose picks this call samples: covered clouds are answered with the prefix
 * without running the chain, the others run it.  Results are bit-identical to roitr_furthestsampling either way. */
int roitr_furthestsampling_ex(int b, int n_max, const float* xyz, const int* offset, const int* new_offset, float* tmp, int* idx,
                              const int* prev_tie, int* tie_out, int track_div, roitr_stream_t stream);

/* Workspace for roitr_knn_build_grid / roitr_knnquery_ex: b clouds, n reference points, at most m queries. */
size_t roitr_knn_workspace_bytes(int b, int n, int m);

/* Counting-sorts the reference clouds into per-cloud uniform grids inside `ws`. */
int roitr_knn_build_grid(int b, int n, int m_capacity, const float* xyz, const int* offset, void* ws, roitr_stream_t stream);
/* same, with the mean points-per-cell the cell size is chosen for (<= 0: default 6; ~ (k+1)/3 for the largest k queried) */
int roitr_knn_build_grid_ex(int b, int n, int m_capacity, const float* xyz, const int* offset, void* ws, float target_occupancy,
                            roitr_stream_t stream);

/* The counting-sorted reference points inside a built workspace: float4 (x, y, z, original index as int bits), n entries,
 * cell-major order.  Valid after roitr_knn_build_grid on (b, n, m_capacity, ws). */
const void* roitr_knn_sorted_points(int b, int n, int m_capacity, void* ws);

/* Exact kNN.  Any of idx/dist2/group_idx/ppf may be NULL.
 *   group_idx (m, nsample-1): columns 1.. of idx  == pointops.queryandgroup(nsample-1, ..., return_idx=True)
 *                             (functions/pointops.py:88-89: kNN(k+1), drop column 0)
 *   ppf (m, nsample-1, 4):    lib/utils.py:358-389 calc_ppf_gpu(new_xyz, query_normals, xyz[group_idx],
 *                             ref_normals[group_idx])
 * use_grid != 0 needs a prior roitr_knn_build_grid(b, n, m_capacity, xyz, offset, ws). */
int roitr_knnquery_ex(int b, int n, int m, int nsample, const float* xyz, const float* new_xyz, const int* offset,
                      const int* new_offset, int* idx, float* dist2, int* group_idx, float* ppf,
                      const float* ref_normals, const float* query_normals, int use_grid, int m_capacity, void* ws,
                      roitr_stream_t stream);

/* Which kernel form roitr_knnquery_ex (capped == 0) or roitr_knn_within (capped != 0, nsample 1, outputs = ROITR_KNN_OUT_DIST2) gives a
 * call, chosen by shape alone: the launcher dispatches through the same host function, no pointer is followed, no GPU is needed.
 *   self_query   the queries are the reference points themselves (new_xyz == xyz, new_offset == offset, m == n)
 *   outputs      ROITR_KNN_OUT_* of the outputs that are not NULL;  normals != 0: both normal arrays are given
 * Returns ROITR_KNN_FORM | width << 8 | sort << 16 (read with the three macros), or minus the status the call is refused with.
 *   width   list slots of the kernel's template: L of LANE_BRUTE, LANE and PREFILTER (2, 4, 10, 18, 34), NR of BRUTE (1, 2), else 0
 *   sort    the queries are counting-sorted by grid cell first: ROITR_KNN_SORT_NONE, _4096 or _MAX (the cell cap of the grid,
 *           the one roitr_knn_build_grid_ex built it with: 4096 cells per cloud while n <= 6144 b) */
#define ROITR_KNN_NOTHING 0     /* m <= 0 */
#define ROITR_KNN_BRUTE 1       /* no grid: a wave per query, index order */
#define ROITR_KNN_LANE_BRUTE 2  /* no grid, >= 65536 queries, nsample <= 33: a lane per query, clouds staged in LDS */
#define ROITR_KNN_LANE 3        /* grid, >= 8192 queries, nsample <= 33: a lane per query, ring search */
#define ROITR_KNN_PREFILTER 4   /* as LANE at nsample 4 .. 9, exact k: radius prefilter, then LANE on its retry list */
#define ROITR_KNN_WITHIN 5      /* as LANE for roitr_knn_within's call: one pass over the cells of the ball */
#define ROITR_KNN_CELL 6        /* grid, self query, nsample <= 65: a workgroup per cell, then GRIDSEL on its retry list */
#define ROITR_KNN_GRIDSEL 7     /* grid, everything else: a wave per query with buffered selection */
#define ROITR_KNN_OUT_IDX 1
#define ROITR_KNN_OUT_DIST2 2
#define ROITR_KNN_OUT_GROUP 4
#define ROITR_KNN_OUT_PPF 8
#define ROITR_KNN_SORT_NONE 0
#define ROITR_KNN_SORT_4096 1
#define ROITR_KNN_SORT_MAX 2
#define ROITR_KNN_FORM(v) ((v) & 0xff)
#define ROITR_KNN_WIDTH(v) (((v) >> 8) & 0xff)
#define ROITR_KNN_SORT(v) ((v) >> 16)
int roitr_knn_form(int b, int n, int m, int nsample, int self_query, int outputs, int normals, int use_grid, int capped);

/* ------------------------------------------------------------------ input preparation
 * dataset/tdmatch.py:120-127: open3d estimate_normals(KDTreeSearchParamKNN(knn)) + dataset/common.py:312-320 normal_redirect.
 * normals (n,3) = unit eigenvector of the smallest eigenvalue of the covariance of the knn nearest points (the point
 * itself included), flipped towards view_point (3 host floats; NULL = leave Open3D's arbitrary sign).  use_grid as in
 * roitr_knnquery_ex (this call builds the grid itself).  ws: roitr_normals_workspace_bytes(b, n, knn). */
size_t roitr_normals_workspace_bytes(int b, int n, int knn);
int roitr_estimate_normals(int b, int n, const float* xyz, const int* offset, int knn, int use_grid, const float* view_point,
                           float* normals, void* ws, roitr_stream_t stream);
/* dataset/common.py:312-320 on its own: out = (dot(view_point - p, n) < 0) ? -n : n */
int roitr_normal_redirect(int n, const float* xyz, const float* normals_in, const float* view_point, float* normals_out,
                          roitr_stream_t stream);

/* ------------------------------------------------------------------ FPFH descriptors: the learning-free baseline
 * Open3D's compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn)) restated; parity with the original is unpinned.  b clouds
 * in the `offset` layout of the normals: xyz (n,3), normals (n,3) fp32, offset (b) cumulative int32 with offset[b-1] == n (PRECONDITION,
 * as for roitr_pairgt_stats: the offsets are device memory and are not checked); empty clouds are legal.  All arithmetic is float64 on
 * the fp32 inputs, every product, sum and quotient rounded on its own (no FMA); a dot product is (a0 b0 + a1 b1) + a2 b2, a cross
 * product's component a1 b2 - a2 b1.
 * Neighbours K(i) of point i of cloud c: row i of this library's exact kNN of the cloud against itself with nsample = max_nn
 *   (roitr_knn_build_grid_ex + roitr_knnquery_ex: ascending distance, the lower index first among equal ones).  Slots k >= size(c) are
 *   padding and ignored; entries j == i are dropped; of the rest at most the first max_nn - 1 stay; of those, j is kept iff
 *   d2 = (dx dx + dy dy) + dz dz < radius radius, dp = p_j - p_i = (dx, dy, dz) (strict).  m_i = |K(i)|, in row order.
 * Pair feature of (i, j): d = sqrt(d2).  d == 0: f = (0, 0, 0).  Otherwise a1 = n_i . dp / d, a2 = n_j . dp / d; if |a1| < |a2|:
 *   (n1, n2, dp) = (n_j, n_i, -dp) and f2 = -a2, else (n1, n2) = (n_i, n_j) and f2 = a1.  v = dp x n1; |v| == 0: f = (0, 0, 0).  Otherwise
 *   v /= |v|, w = n1 x v, f1 = v . n2, f0 = atan2(w . n2, n1 . n2).  Normals are used as given, not normalised.
 * Bins: h0 = clamp(floor(11 (f0 + pi) / (2 pi)), 0, 10), h1 = clamp(floor(11 (f1 + 1) / 2), 0, 10), h2 likewise from f2 (a NaN goes to
 *   bin 0); counts_i[h0], counts_i[11 + h1], counts_i[22 + h2] each get +1 per neighbour: integers <= 99.
 * SPFH_i[b] = counts_i[b] (100 / m_i), all zero when m_i == 0.
 * FPFH: for j in K(i) in row order with d2 > 0: val[b] = SPFH_j[b] / d2, F_i[b] += val[b], and S_i[g] += val[b] for the 11 bins b of group
 *   g = b div 11 in ascending b.  Then F_i[b] = (S_i[g] != 0 ? F_i[b] 100 / S_i[g] : F_i[b]) + SPFH_i[b], rounded once to fp32 into
 *   fpfh[i out_stride + b]; columns 33 .. out_stride - 1 are written as 0.
 * Outputs: fpfh (n, out_stride) fp32; spfh_counts (n, 33) int32 and nbr_count (n) int32 = m_i, optional (NULL); status (b): bit 1 = the
 *   cloud holds a non-finite coordinate or normal; all of that cloud's rows (fpfh, spfh_counts, nbr_count) are 0 then and the other
 *   clouds of the call are unaffected.  Nothing is read out of bounds whatever the values are.
 * Host-side errors (ROITR_ERR_ARG, nothing is launched): max_nn outside [2, 100] (the kNN's limit), out_stride < 33, radius not finite
 *   or not positive, b or n negative, b > 65535, b == 0 with n > 0, null required pointers, workspace_bytes below
 *   roitr_fpfh_workspace_bytes(b, n, max_nn).  n == 0 or an empty cloud is not an error.
 * Determinism: counts are integers and every float64 sum is taken in row order by one wave; no floating-point atomics.  A cloud's
 *   outputs are bitwise the same alone, anywhere in a batch and on repeats, with or without the optional outputs, for any out_stride.
 * No host synchronisation, no host read.  The workspace holds the kNN rows: n max_nn 4 bytes dominate. */
size_t roitr_fpfh_workspace_bytes(int b, int n, int max_nn);
int roitr_fpfh_batch(int b, int n, const float* xyz, const float* normals, const int* offset,
                     double radius, int max_nn, int out_stride,
                     float* fpfh,          /* (n, out_stride) */
                     int* spfh_counts,     /* optional (n, 33) */
                     int* nbr_count,       /* optional (n)     */
                     int* status,          /* (b) */
                     void* workspace, size_t workspace_bytes, roitr_stream_t stream);

/* ------------------------------------------------------------------ raw scans: voxel grid + point cap
 * Open3D's voxel_down_sample restated (parity with the original is unpinned, as for the normals).  Per cloud, in float64 on the fp32
 * inputs: vmb = min_bound - voxel_size / 2, ijk = floor((p - vmb) / voxel_size); one output point per occupied voxel = the sum of its
 * points in INPUT order / their count, rounded once to fp32.  Output order (Open3D's is a hash map's): clouds in input order, voxels
 * ascending in (ix, iy, iz).  offset (b) cumulative int32 with offset[b-1] == n; empty clouds are legal.
 *   out_xyz (n,3), out_count (n), out_attr (n,c): capacity buffers, the first new_offset[b-1] rows are written
 *   new_offset (b): cumulative voxel counts;  inverse (n): output row of every input point (-1 in a cloud with a status bit)
 *   attr (n,c) / out_attr: optional per-point channels and their per-voxel means (same summation); c = 0 or NULL: none
 *   status (b): bit 1 = an axis needs a voxel index above 65535 (the key holds 16 bits per axis), bit 2 = a non-finite coordinate.
 *               Such a cloud yields zero voxels; the other clouds of the call are unaffected.
 * Host-side errors (nothing is launched): voxel_size not finite or not positive, b outside 1..65536 (16 bits of cloud id), null
 * pointers.  ws: roitr_voxel_workspace_bytes(b, n, c).  No host synchronisation inside. */
size_t roitr_voxel_workspace_bytes(int b, int n, int c);
int roitr_voxel_downsample(int b, int n, const float* xyz, const int* offset, double voxel_size, int c, const float* attr,
                           float* out_xyz, int* new_offset, int* out_count, int* inverse, float* out_attr, int* status, void* ws,
                           roitr_stream_t stream);
/* The point cap of dataset/tdmatch.py:72-78 (np.random.permutation(n)[:points_lim]) as a distribution: uniform without replacement.
 * Point j (cloud-local) of a cloud with key k draws u = splitmix64(seed ^ 0xE7037ED1A0B428DB ^ splitmix64(k << 32 | j)) >> 16; a cloud
 * with more than `limit` points keeps the `limit` points of smallest (u, j), a smaller one keeps all.  idx (capacity n): the kept GLOBAL
 * rows, ascending (the reference keeps permutation order); new_offset (b) cumulative.  cloud_keys (b, device, optional): k per cloud,
 * default the cloud's position in the call.  The selection depends on (seed, k, cloud size, limit) only.
 * ws: roitr_subsample_workspace_bytes(b, n). */
size_t roitr_subsample_workspace_bytes(int b, int n);
int roitr_random_subsample(int b, int n, const int* offset, int limit, unsigned long long seed, const int* cloud_keys, int* idx,
                           int* new_offset, void* ws, roitr_stream_t stream);

/* ------------------------------------------------------------------ outlier removal: statistical and radius filters
 * Open3D's remove_statistical_outlier(nb_neighbors, std_ratio) and remove_radius_outlier(nb_points, radius) restated; parity with the
 * original is unpinned (Open3D is not part of the build), this text is the definition.  b clouds in the `offset` layout of the normals:
 * xyz (n,3) fp32, offset (b) cumulative int32 with offset[b-1] == n (PRECONDITION, as for roitr_fpfh_batch: the offsets are device
 * memory and are not checked); empty clouds are legal.  All arithmetic is float64 on the fp32 inputs, every product, sum, quotient and
 * square root rounded on its own (no FMA); dp = p_j - p_i = (dx, dy, dz) is taken in float64, d2 = (dx dx + dy dy) + dz dz.
 * Statistical filter (nb_neighbors in [2, 100], std_ratio finite).
 *   Neighbours of point i of cloud c: row i of this library's exact kNN of the cloud against itself with nsample = nb_neighbors
 *     (roitr_knn_build_grid_ex + roitr_knnquery_ex: ascending distance, the lower index first among equal ones).  Point i itself counts
 *     wherever it stands in the row (with more than nb_neighbors copies of a point, not at all); slots k >= size(c) are padding and
 *     ignored: v_i = min(nb_neighbors, size(c)) slots are valid.
 *   mean_i = (the sum over the valid slots, in ROW order from +0, of sqrt(d2)) / v_i.
 *   Per cloud, V = size(c):  S1 = sum_i (mean_i > 0 ? mean_i : 0);  cloud_mean = S1 / V;
 *     S2 = sum_i (mean_i > 0 ? (mean_i - cloud_mean)^2 : 0);  std = sqrt(S2 / (V - 1));  thr = cloud_mean + std_ratio std.
 *     Points with mean_i == 0 (a point with at least nb_neighbors copies of itself) count in V but not in the sums: Open3D's quirk, kept.
 *   Order of a per-cloud sum (fixed): the cloud's points in input order are cut into segments of 256; a segment is summed one term
 *     after the other in input order from +0; the cloud's sum is the sum of its segment sums, one after the other in segment order
 *     from +0.
 *   Point i is kept iff mean_i > 0 && mean_i < thr, both strict.  A cloud of one point gives std = sqrt(0 / 0): a NaN threshold and
 *     nothing kept.  A cloud whose means are all equal and whose sums come out exact (a lattice with nb_neighbors = 2: every mean is half
 *     the step) has std == 0, thr == cloud_mean, and keeps nothing either.
 *   stats of an empty cloud are written as 0, 0, 0 (the formulas would give NaN, -0, NaN).
 * Radius filter (radius finite and positive, nb_points >= 0).
 *   count_i = the number of points j of the same cloud, i included, with d2 < radius radius (strict; the product rounded once).
 *   Point i is kept iff count_i > nb_points.
 * Outputs of both: keep (n) unsigned char 0 / 1;  index (capacity n): the kept GLOBAL rows, ascending, new_offset[b-1] of them, nothing
 *   is written behind those;  new_offset (b) cumulative kept counts;  status (b): bit 1 = the cloud holds a non-finite coordinate -- it
 *   keeps nothing and its optional rows are 0; the other clouds of the call are unaffected (the grid and the kNN run on a copy with
 *   such coordinates zeroed).  Optional (NULL): mean_dist (n) float64 and stats (b,3) float64 = cloud_mean, std, thr for the
 *   statistical filter; count (n) int32 for the radius filter -- without it a query stops walking at nb_points + 1, keep is the same.
 * Host-side errors (ROITR_ERR_ARG, nothing is launched): a parameter outside the ranges above, b or n negative, b > 65535, b == 0 with
 *   n > 0, null required pointers, workspace_bytes below roitr_outlier_workspace_bytes(b, n, nb_neighbors) (nb_neighbors == 0 there:
 *   the radius filter).  n == 0 or an empty cloud is not an error.
 * Determinism: mean_i is summed by one lane in row order, the per-cloud sums in the order above, the counts are integers; no
 *   floating-point atomics.  A cloud's outputs are bitwise the same alone, in any slot of any batch, on repeats, and with or without the
 *   optional outputs.  No host synchronisation, no host read.  The workspace holds the kNN rows: n nb_neighbors 4 bytes dominate. */
#define ROITR_OUTLIER_NONFINITE 1
size_t roitr_outlier_workspace_bytes(int b, int n, int nb_neighbors);
int roitr_remove_statistical_outlier(int b, int n, const float* xyz, const int* offset, int nb_neighbors, double std_ratio,
                                     unsigned char* keep,   /* (n) */
                                     int* index,            /* capacity n */
                                     int* new_offset,       /* (b) */
                                     int* status,           /* (b) */
                                     double* mean_dist,     /* optional (n) */
                                     double* stats,         /* optional (b, 3) */
                                     void* workspace, size_t workspace_bytes, roitr_stream_t stream);
int roitr_remove_radius_outlier(int b, int n, const float* xyz, const int* offset, double radius, int nb_points,
                                unsigned char* keep,        /* (n) */
                                int* index,                 /* capacity n */
                                int* new_offset,            /* (b) */
                                int* status,                /* (b) */
                                int* count,                 /* optional (n) */
                                void* workspace, size_t workspace_bytes, roitr_stream_t stream);

/* kNN(1) distances for a radius test (lib/utils.py:509-521 get_node_occlusion_score): exact when < cap2, otherwise any
 * value >= cap2.  Same workspace / grid rules as roitr_knnquery_ex. */
int roitr_knn_within(int b, int n, int m, const float* xyz, const float* new_xyz, const int* offset, const int* new_offset,
                     float cap2, float* dist2, int use_grid, int m_capacity, void* ws, roitr_stream_t stream);

/* ------------------------------------------------------------------ pair ground truth: radius search under the gt transform
 * lib/utils.py:72-96 get_correspondences (an Open3D KD-tree radius search per source point, optional idx[:K]) restated, with the overlap
 * ratio of gt_overlap.log and the 6x6 information matrix of gt.info as reductions on top.  B ragged pairs: src (n,3) / tgt (m,3) fp32
 * with cumulative int32 offsets src_offset / tgt_offset (B); rot (B,3,3), trans (B,3) fp32, source to target: p' = R p + t.
 * PRECONDITION (not checked: the offsets are device memory): 0 <= offset[0] <= ... <= offset[B-1], src_offset[B-1] == n,
 * tgt_offset[B-1] == m.  The kernels index with them; offsets that break this read out of bounds.
 * The decision, in float64 on the fp32 inputs, every product and sum rounded on its own (no FMA):
 *     p'[c] = ((R[c][0] px + R[c][1] py) + R[c][2] pz) + t[c];   d2 = ((p'x - qx)^2 + (p'y - qy)^2) + (p'z - qz)^2
 *     (i, j) is a correspondence iff d2 < (double)radius * (double)radius            (strict; Open3D's boundary is unpinned)
 *   inverse != 0 (roitr_pairgt_stats): the queries are moved by q'[c] = (R[0][c] dx + R[1][c] dy) + R[2][c] dz, d = q - t, instead:
 *     call it with the target clouds as `src` and the source clouds as `tgt` for the target-side overlap.
 *   count (n), nn_idx (n), nn_dist2 (n, float64): per query the number of searched points within the radius, the nearest one
 *     (pair-local, ties to the lower index; -1 / +inf when none).  Each optional (NULL).
 *   n_hit (B), overlap (B, float64) = n_hit / n_src, info (B,6,6 float64, optional): sum over the hit queries of G^T G,
 *     G = [ I3 | -2 [p]x ], p the query in its own frame: Redwood's gt.info layout (translation block first), info[0][0] = n_hit.
 *     Summed in float64 in a fixed tree per pair: bitwise the same for a pair alone and anywhere in a batch.
 *   status (B): bit 1 = a non-finite coordinate or transform, bit 2 = an empty cloud, bit 4 = list overflow.  A pair with bit 1 or 2 has
 *     no correspondences (count 0, nn -1 / +inf, n_hit 0, overlap NaN, info 0); the other pairs of the call are unaffected.
 * roitr_pairgt_correspondences: corr (capacity, 2) int32 rows (i, j), pair-local, pairs in input order, ascending i, within an i
 *   ascending (d2, j); k > 0 keeps the first k rows of every i (idx[:K]), k = 0 all.  corr_offset (B) cumulative (saturates at INT_MAX),
 *   total (2 x int64, device): [0] rows of the list, [1] candidates before the cap = the capacity the call needs.  Candidates pass
 *   through a buffer of `capacity` entries inside ws: when total[1] > capacity the pairs whose candidates do not all fit carry bit 4 and
 *   their rows are not written (corr_offset and total stay exact): repeat with capacity = total[1].
 * Host-side errors (nothing is launched): radius not finite or not positive, k < 0, B outside 1..65536, capacity outside 0..2^31-1, null
 * pointers.  ws: roitr_pairgt_workspace_bytes(B, n, m, capacity) (capacity 0 for roitr_pairgt_stats).  No host synchronisation. */
size_t roitr_pairgt_workspace_bytes(int b, int n, int m, long long capacity);
int roitr_pairgt_stats(int b, int n, int m, const float* src, const int* src_offset, const float* tgt, const int* tgt_offset,
                       const float* rot, const float* trans, float radius, int inverse, int* count, int* nn_idx, double* nn_dist2,
                       int* n_hit, double* overlap, double* info, int* status, void* ws, roitr_stream_t stream);
int roitr_pairgt_correspondences(int b, int n, int m, const float* src, const int* src_offset, const float* tgt, const int* tgt_offset,
                                 const float* rot, const float* trans, float radius, int k, long long capacity, int* corr,
                                 int* corr_offset, long long* total, int* status, void* ws, roitr_stream_t stream);

/* ------------------------------------------------------------------ ICP pose refinement: point-to-point and point-to-plane
 * Open3D's RegistrationICP restated on the dense clouds; parity with the original is unpinned.
 * Inputs.  B ragged pairs in the layout of roitr_pairgt_stats: src (n,3) / tgt (m,3) fp32, cumulative int32 src_offset / tgt_offset (B)
 *   under the same precondition; tgt_normals (m,3) fp32 or NULL; init_T (B,4,4) fp32 row-major, source to target, only the top three rows
 *   are read; max_dist fp32, finite, > 0; iterations >= 0; rel_fitness, rel_rmse double >= 0 (Open3D's defaults: 1e-6, 1e-6, 30 iterations).
 * Mode.  tgt_normals == NULL: point-to-point; otherwise point-to-plane.
 * State.  Each pair has a state T_s, 12 fp32 values, T_0 = init_T.
 * Evaluation E(T_s): the decision of roitr_pairgt_stats with R, t taken from T_s, in float64 on the fp32 inputs, every product and sum
 *   rounded on its own: p' = ((R[c][0] px + R[c][1] py) + R[c][2] pz) + t[c], d2 as in pairgt.  The match of source point i is the target
 *   point of least (d2, j) with d2 < (double)max_dist^2, strictly.  n_corr = matched points, fitness = n_corr / n_src (float64),
 *   rmse = sqrt(sum d2 / n_corr), 0 when n_corr = 0.
 * Loop.  For s = 0, 1, ...:  1. evaluate E(T_s);  2. if s > 0 and |fitness_s - fitness_{s-1}| < rel_fitness and |rmse_s - rmse_{s-1}| <
 *   rel_rmse, stop with bit CONVERGED;  3. if s == iterations, stop;  4. otherwise compute the update -- if it cannot be computed, stop
 *   with the bits given below;  5. go on with T_{s+1}.  The outputs belong to the last evaluated state: at most iterations + 1 evaluations.
 * Update.  All sums over the matched points, in float64.
 *   Point-to-point: T_{s+1} = Solve(original source points -> matched target points), weights 1: the rigid solve of the registration
 *     operators on centroids and centred cross-covariance, T rounded to fp32.  n_corr < 3: bit TOO_FEW, stop.
 *   Point-to-plane: r_i = (p'_i - q_i) . n_i, J_i = [p'_i x n_i, n_i]; (sum J J^T) x = -sum J r by a float64 Cholesky (L D L^T);
 *     dT from x = (a, b, g, tx, ty, tz) as Open3D's TransformVector6dToMatrix4d, R = Rz(g) Ry(b) Rx(a), t = (tx, ty, tz);
 *     T_{s+1} = fp32(dT T_s), the product in float64.  n_corr < 6: bit TOO_FEW, stop.  A non-positive or non-finite pivot: bit SINGULAR,
 *     T_s is kept, stop.
 * Status bits.  NONFINITE (a non-finite coordinate, normal or init_T entry), EMPTY (an empty cloud), TOO_FEW, SINGULAR, CONVERGED.  A
 *   NONFINITE or EMPTY pair returns init_T, fitness NaN, rmse NaN, n_corr 0, steps 0; the other pairs of the call are unaffected.
 * Outputs (optional unless noted).  T (B,4,4) fp32, last row 0 0 0 1 (required); fitness (B), rmse (B) double; n_corr (B), steps (B) int:
 *   the s at which the pair stopped; status (B) (required); nn_idx (n) int: the match of every source point under the final state,
 *   pair-local, -1 for none; trace_T (iterations + 1, B, 12) fp32 and trace_stat (iterations + 1, B, 2) double (fitness, rmse): one row
 *   per evaluation, rows after a pair's stop repeat its last row.
 * Host-side errors (nothing is launched): max_dist not finite or not positive, negative iterations or tolerances, B outside 1..65536,
 *   null required pointers.
 * Determinism.  The match is an exact decision.  Every float64 sum of a pair is taken in a fixed order that depends on the pair's own
 *   point indices only (thread t of 256 sums points t, t + 256, ..., then the fixed binary tree of the pairgt reduction); no
 *   floating-point atomics: a pair's results are bitwise the same alone, anywhere in a batch, and on repeats.
 * ws: roitr_icp_workspace_bytes(B, n, m, iterations).  No host synchronisation, no host read; 2 launches per evaluation. */
#define ROITR_ICP_NONFINITE 1
#define ROITR_ICP_EMPTY 2
#define ROITR_ICP_TOO_FEW 4
#define ROITR_ICP_SINGULAR 8
#define ROITR_ICP_CONVERGED 16
size_t roitr_icp_workspace_bytes(int b, int n, int m, int iterations);
int    roitr_icp_batch(int b, int n, int m, const float* src, const int* src_offset, const float* tgt, const int* tgt_offset,
                       const float* tgt_normals, const float* init_T, float max_dist, int iterations, double rel_fitness,
                       double rel_rmse, float* T, double* fitness, double* rmse, int* n_corr, int* steps, int* status,
                       int* nn_idx, float* trace_T, double* trace_stat, void* ws, roitr_stream_t stream);

/* ------------------------------------------------------------------ Generalized ICP: plane-to-plane refinement from normals
 * Open3D's RegistrationGeneralizedICP restated on the dense clouds with the covariances fixed by the normals; parity with the original
 * is unpinned.  Deviation stated: Open3D tests convergence on the RMSE of its whitened residuals; this operator tests it on the
 * Euclidean (fitness, rmse) of roitr_icp_batch.  Caller-supplied covariances, robust kernels and point weights are not part of it.
 * Inputs.  As roitr_icp_batch, except: src_normals (n,3) and tgt_normals (m,3) fp32 are both required; epsilon double in [1e-6, 1]
 *   (Open3D's default: 1e-3).
 * Normals.  nh = n / sqrt((nx nx + ny ny) + nz nz), in float64 on the fp32 values, every component divided by the root.  A squared
 *   length of exactly 0 gives nh = 0: an isotropic point, C = I.  The covariance of a point is C = I - (1 - epsilon) nh nh^T:
 *   eigenvalues (epsilon, 1, 1), the normal the epsilon-axis.  A non-finite normal on either side: bit NONFINITE for its pair.
 * State, Evaluation E(T_s), Loop.  Exactly roitr_icp_batch's: the same float64 move, the match the target point of least (d2, j) with
 *   d2 < (double)max_dist^2, n_corr, fitness and the Euclidean rmse, the same convergence rule on (fitness, rmse), at most
 *   iterations + 1 evaluations, the outputs belong to the last evaluated state.
 * Update.  All sums over the matched points, in float64, every product and sum rounded on its own.  Per matched pair (p, q):
 *   p' the moved point, d = p' - q;  a = R nh_s with R from T_s, a[r] = (R[r][0] u0 + R[r][1] u1) + R[r][2] u2;  b = nh_t;
 *   c = 1 - epsilon (computed once, on the host);
 *   M = 2I - c (a a^T + b b^T), symmetric, upper triangle: m_xy = [x == y ? 2 : 0] - c * (a_x a_y + b_x b_y);
 *   W = M^-1 by cofactors: C00 = m11 m22 - m12 m12, C01 = m12 m02 - m01 m22, C02 = m01 m12 - m11 m02, C11 = m00 m22 - m02 m02,
 *     C12 = m01 m02 - m00 m12, C22 = m00 m11 - m01 m01, det = (m00 C00 + m01 C01) + m02 C02, w_xy = C_xy / det;
 *   J = [ -[p']x | I ] (3 x 6), x = (alpha, beta, gamma, tx, ty, tz);
 *   e = W d, e_x = (w_x0 d0 + w_x1 d1) + w_x2 d2;  K = W (-[p']x), row x of K = p' x (row x of W);  G = [p']x K, column y of G =
 *     p' x (column y of K), every cross product component a difference of two products;
 *   A = sum J^T W J = sum [ G  K^T ; K  W ] (upper triangle, 21 sums);  g = sum J^T W d = sum (p' x e, e) (6 sums);
 *   A x = -g by the float64 L D L^T of the point-to-plane mode; dT from x as there (TransformVector6dToMatrix4d);
 *   T_{s+1} = fp32(dT T_s), the product in float64.  n_corr < 6: bit TOO_FEW, stop.  A non-positive or non-finite pivot: bit SINGULAR,
 *   T_s is kept, stop.
 * Status bits.  The ROITR_ICP_* values, with their meaning there.
 * Outputs.  As roitr_icp_batch, and objective (B) double (optional) = sum d^T W d / n_corr of the last evaluated state, d^T W d =
 *   (d0 e0 + d1 e1) + d2 e2, 0 when n_corr = 0, NaN for a NONFINITE or EMPTY pair: the quantity the step minimises.  trace_stat is
 *   (iterations + 1, B, 3) double: fitness, rmse, objective.
 * Host-side errors (nothing is launched): epsilon outside [1e-6, 1] or not finite, either normals pointer null, and roitr_icp_batch's.
 * Determinism.  As roitr_icp_batch: the match is an exact decision; every float64 sum of a pair is taken in the order of the ICP update
 *   (thread t of 256 sums points t, t + 256, ..., then the same binary tree); no floating-point atomics: a pair's results are bitwise
 *   the same alone, anywhere in a ragged batch, and on repeats.
 * ws: roitr_gicp_workspace_bytes(B, n, m, iterations).  No host synchronisation, no host read; 2 launches per evaluation. */
size_t roitr_gicp_workspace_bytes(int b, int n, int m, int iterations);
int    roitr_gicp_batch(int b, int n, int m, const float* src, const int* src_offset, const float* tgt, const int* tgt_offset,
                        const float* src_normals, const float* tgt_normals, const float* init_T, float max_dist, double epsilon,
                        int iterations, double rel_fitness, double rel_rmse, float* T, double* fitness, double* rmse,
                        double* objective, int* n_corr, int* steps, int* status, int* nn_idx, float* trace_T, double* trace_stat,
                        void* ws, roitr_stream_t stream);

int roitr_grouping_forward(int m, int nsample, int c, const float* input, const int* idx, float* output, roitr_stream_t stream);
int roitr_grouping_backward(int m, int nsample, int c, const float* grad_output, const int* idx, float* grad_input, roitr_stream_t stream);
int roitr_interpolation_forward(int n, int c, int k, const float* input, const int* idx, const float* weight, float* output, roitr_stream_t stream);
int roitr_interpolation_backward(int n, int c, int k, const float* grad_output, const int* idx, const float* weight, float* grad_input, roitr_stream_t stream);
int roitr_subtraction_forward(int n, int nsample, int c, const float* input1, const float* input2, const int* idx, float* output, roitr_stream_t stream);
int roitr_subtraction_backward(int n, int nsample, int c, const int* idx, const float* grad_output, float* grad_input1, float* grad_input2, roitr_stream_t stream);
int roitr_aggregation_forward(int n, int nsample, int c, int w_c, const float* input, const float* position, const float* weight, const int* idx, float* output, roitr_stream_t stream);
int roitr_aggregation_backward(int n, int nsample, int c, int w_c, const float* input, const float* position, const float* weight, const int* idx, const float* grad_output, float* grad_input, float* grad_position, float* grad_weight, roitr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROITR_POINTOPS_H */
