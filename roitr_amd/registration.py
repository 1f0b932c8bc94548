"""Registration on the GPU: correspondence RANSAC, weighted Procrustes and the 3DMatch metrics.

`ransac_batch` / `register_handle` run registration/evaluate_registration_c2f.py:78-85 + benchmark_utils.py:169-215 (Open3D's
registration_ransac_based_on_correspondence as the reference calls it) for every pair of a batch in three launches
(csrc/registration.hip; the rules are stated in include/roitr_engine.h).  `ransac_pose_estimation_correspondences` and
`weighted_procrustes` keep the reference's names and signatures (benchmark_utils.py:169, lib/utils.py:159).  The metrics
(registration/benchmark.py) are host float64 code: not a hot path.

Differences from the reference, by design: the iteration count is fixed (50 000, no early exit) and the random stream is a pure
function of (seed, pair key, iteration), so a pair's pose does not depend on the batch it travels in; weighted sampling of fewer
positive-confidence rows than n_points takes all of them (numpy's choice raises there).  Parity with Open3D itself is unpinned.
"""
import math

import numpy as np
import torch

from . import _args as A
from . import _lib as L

SAMPLE_MODES = {"all": 0, "topk": 1, "weighted": 2}


def _keys(pair_keys, B, dev):
    if pair_keys is None:
        k = torch.arange(B, dtype=torch.int64)
    else:
        k = torch.as_tensor(pair_keys, dtype=torch.int64).reshape(-1).cpu()
        if k.numel() != B:
            raise L.RoitrError(f"pair_keys: {k.numel()} keys for {B} pairs")
    k = k & 0xFFFFFFFF
    return torch.where(k >= 2 ** 31, k - 2 ** 32, k).to(torch.int32).to(dev)   # the uint32 bit pattern


@torch.no_grad()
def ransac_batch(starts, src_pts, tgt_pts, scores=None, *, n_points=1000, sample="weighted", distance_threshold=0.05,
                 edge_similarity=0.9, iterations=50000, refine_iters=0, refine_weighted=False, seed=0, pair_keys=None, ransac_n=3,
                 chunks=0):
    """RANSAC over the correspondences of every pair: pair b owns rows [starts[b], starts[b+1]) of src_pts / tgt_pts / scores.

    Returns a dict of device tensors: T (B,4,4) fp32, inliers, best_iteration (-1: none), valid_hypotheses, n_used (B) int32, and
    selected (int32, rows): the local indices of the rows RANSAC used, pair b's at [starts[b], starts[b] + n_used[b]).
    pair_keys (default arange(B)) key the random stream: a pair's result depends on (seed, key), not on its batch.
    chunks: hypothesis workgroups per pair (0: automatic); the result does not depend on it."""
    if sample not in SAMPLE_MODES:
        raise ValueError(f"sample must be one of {sorted(SAMPLE_MODES)}")
    src_pts = src_pts if torch.is_tensor(src_pts) else torch.as_tensor(src_pts)
    dev = src_pts.device if src_pts.is_cuda else torch.device("cuda")
    starts = torch.as_tensor(starts).to(device=dev, dtype=torch.int32).contiguous()
    B = int(starts.shape[0]) - 1
    src = A.upload(src_pts, device=dev).reshape(-1, 3)
    tgt = A.upload(tgt_pts, device=dev).reshape(-1, 3)
    if src.shape != tgt.shape:
        raise ValueError("src_pts and tgt_pts must have the same shape")
    w = None if scores is None else A.upload(scores, device=dev).reshape(-1)
    rows = int(src.shape[0])
    if w is not None and int(w.shape[0]) != rows:
        raise ValueError("scores must have one entry per row")
    keys = _keys(pair_keys, max(B, 0), dev)
    lib = L.lib()
    Bc = max(B, 0)
    out = dict(T=torch.empty((Bc, 4, 4), dtype=torch.float32, device=dev),
               inliers=torch.empty((Bc,), dtype=torch.int32, device=dev),
               best_iteration=torch.empty((Bc,), dtype=torch.int32, device=dev),
               valid_hypotheses=torch.empty((Bc,), dtype=torch.int32, device=dev),
               n_used=torch.empty((Bc,), dtype=torch.int32, device=dev),
               selected=torch.full((rows,), -1, dtype=torch.int32, device=dev))
    nbytes = int(lib.roitr_registration_workspace_bytes(Bc, rows, max(int(iterations), 1), int(chunks))) if Bc > 0 else 0
    ws = A.workspace(nbytes, dev)
    L.check(lib.roitr_ransac_correspondences(
        B, L.ptr(starts).value, rows, src.data_ptr(), tgt.data_ptr(), None if w is None else w.data_ptr(), keys.data_ptr(),
        SAMPLE_MODES[sample], int(n_points), int(ransac_n), float(distance_threshold), float(edge_similarity), int(iterations),
        int(refine_iters), int(bool(refine_weighted)), int(seed) & 0xFFFFFFFFFFFFFFFF, int(chunks), ws.data_ptr(), nbytes,
        out["T"].data_ptr(), out["inliers"].data_ptr(), out["best_iteration"].data_ptr(), out["valid_hypotheses"].data_ptr(),
        out["n_used"].data_ptr(), out["selected"].data_ptr(), L.stream_ptr().value), "ransac_correspondences")
    return out


@torch.no_grad()
def ransac_samples(n, pair_keys=None, seed=0, it0=0, count=1):
    """The triples the RANSAC stream draws for iterations [it0, it0 + count): (pairs, count, 3) int32 on the device, -1 where an
    iteration is invalid.  n: rows per pair (sequence or tensor)."""
    dev = torch.device("cuda")
    n = torch.as_tensor(n).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    B = int(n.shape[0])
    keys = _keys(pair_keys, B, dev)
    out = torch.empty((B, int(count), 3), dtype=torch.int32, device=dev)
    L.check(L.lib().roitr_ransac_samples(B, n.data_ptr(), keys.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF, int(it0), int(count),
                                         out.data_ptr(), L.stream_ptr().value), "ransac_samples")
    return out


@torch.no_grad()
def register_handle(handle, pair_keys=None, **kw):
    """ransac_batch on the correspondences of a RIGA_v2.launch_batch() handle, after finish_batch(handle): pair_starts /
    out_src_pts / out_tgt_pts / out_scores, valid in the strided and the compacted patch layout alike (as
    Evaluator.evaluate_batch reads them).  pair_keys default to the batch positions; pass global pair ids to make the result
    independent of how pairs are grouped into batches."""
    out = handle["out"]
    return ransac_batch(out["pair_starts"], out["out_src_pts"], out["out_tgt_pts"], out["out_scores"], pair_keys=pair_keys, **kw)


def ransac_pose_estimation_correspondences(src_pcd, tgt_pcd, correspondences, mutual=False, distance_threshold=0.05, ransac_n=3, *,
                                           iterations=50000, seed=0):
    """registration/benchmark_utils.py:169-215 on the GPU: src_pcd[correspondences[:, 0]] <-> tgt_pcd[correspondences[:, 1]],
    edge-length checker 0.9, distance checker = distance_threshold, point-to-point, a fixed number of iterations.  Returns the
    4x4 float64 numpy transformation, as Open3D's result.transformation."""
    if mutual:
        raise NotImplementedError
    def arr(x):
        return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    src, tgt, corr = arr(src_pcd).astype(np.float32), arr(tgt_pcd).astype(np.float32), arr(correspondences).astype(np.int64)
    corr = corr.reshape(-1, 2)
    s, t = src[corr[:, 0]], tgt[corr[:, 1]]
    dev = torch.device("cuda")
    r = ransac_batch(A.cumulative([s.shape[0]], dev), torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev), None, sample="all",
                     distance_threshold=distance_threshold, ransac_n=ransac_n, iterations=iterations, seed=seed)
    return r["T"][0].cpu().numpy().astype(np.float64)


def _feature_matches(who, src_pcd, tgt_pcd, src_feat, tgt_feat, mutual):
    """What the *_pose_estimation entries put in front of their estimator: the descriptor matches under the dot product (mutual, or every
    source point with its best target) as (starts of the one pair, matched source points, matched target points, match scores)."""
    from . import descmatch
    src, tgt = A.upload(src_pcd).reshape(-1, 3), A.upload(tgt_pcd).reshape(-1, 3)
    sf, tf = A.upload(src_feat), A.upload(tgt_feat)
    if sf.shape[0] != src.shape[0] or tf.shape[0] != tgt.shape[0]:
        raise L.RoitrError(f"{who}: one descriptor per point is needed")
    m = descmatch.match_batch(A.cumulative([sf.shape[0]], "cuda"), sf, A.cumulative([tf.shape[0]], "cuda"), tf, metric="dot",
                              mode="mutual" if mutual else "row")
    corr = m["corr"].long()
    return m["corr_starts"], src[corr[:, 0]], tgt[corr[:, 1]], m["row_val"][corr[:, 0]]


@torch.no_grad()
def ransac_pose_estimation(src_pcd, tgt_pcd, src_feat, tgt_feat, mutual=False, distance_threshold=0.05, ransac_n=3, *,
                           iterations=50000, seed=0):
    """registration/benchmark_utils.py:124-161 on the GPU: the pose from descriptor matches.  mutual=True: the pairs that are each
    other's best under src_feat @ tgt_feat^T (descmatch, the lowest index at equal scores); mutual=False: every source point with
    its best target (the correspondence list current Open3D's feature-matching RANSAC builds before it runs its correspondence
    RANSAC).  The matched point pairs then go through ransac_batch(sample="all").  Returns the 4x4 float64 numpy transformation.

    Divergences: Open3D is not part of this project's environment, so parity with it is unpinned (as for
    ransac_pose_estimation_correspondences); the reference's mutual=True call passes no checkers, the kernel here always runs the
    edge-length (0.9) and the distance checker; a fixed number of iterations; mutual=False matches under the dot product, as the
    mutual branch does, where Open3D takes the L2 nearest neighbour in feature space -- the same list for equal-norm descriptors
    (the model's are unit-normalised), not otherwise (descmatch.match_batch(metric="sqdist", mode="row") gives the L2 list)."""
    starts, s, t, _ = _feature_matches("ransac_pose_estimation", src_pcd, tgt_pcd, src_feat, tgt_feat, mutual)
    r = ransac_batch(starts, s, t, None, sample="all", distance_threshold=distance_threshold, ransac_n=ransac_n, iterations=iterations,
                     seed=seed)
    return r["T"][0].cpu().numpy().astype(np.float64)


@torch.no_grad()
def compat_pose_estimation(src_pcd, tgt_pcd, src_feat, tgt_feat, mutual=False, **kw):
    """The descriptor-matching twin of ransac_pose_estimation without RANSAC: the same matches (descmatch under the dot product,
    mutual or every source point with its best target), then compat.compat_batch on the matched point pairs with the match scores as
    confidences (they order the rows when there are more than max_rows; the estimator itself is deterministic and takes no seed).
    kw: compat_batch's keyword arguments.  Returns the 4x4 float64 numpy transformation."""
    from .compat import compat_batch
    r = compat_batch(*_feature_matches("compat_pose_estimation", src_pcd, tgt_pcd, src_feat, tgt_feat, mutual), **kw)
    return r["T"][0].cpu().numpy().astype(np.float64)


@torch.no_grad()
def fgr_pose_estimation(src_pcd, tgt_pcd, src_feats, tgt_feats, mutual=True, **kw):
    """Open3D's registration_fgr_based_on_feature_matching in this project's terms: the matches of compat_pose_estimation (descmatch
    under the dot product, mutual or every source point with its best target), then fgr.fgr_batch on the matched point pairs with the
    match scores as confidences.  kw: fgr_batch's keyword arguments (tuples > 0 switches the tuple test on).  Parity with Open3D is
    not claimed (include/roitr_engine.h above roitr_fgr_batch).  Returns the 4x4 float64 numpy transformation."""
    from .fgr import fgr_batch
    r = fgr_batch(*_feature_matches("fgr_pose_estimation", src_pcd, tgt_pcd, src_feats, tgt_feats, mutual), **kw)
    return r["T"][0].cpu().numpy().astype(np.float64)


@torch.no_grad()
def weighted_procrustes(src_points, tgt_points, weights=None, weight_thresh=0., eps=1e-5, return_transform=False):
    """lib/utils.py:159-212 on the GPU (same signature and squeeze rule): (B, N, 3) or (N, 3) -> R, t or the 4x4 transform."""
    squeeze = src_points.ndim == 2
    src = src_points.unsqueeze(0) if squeeze else src_points
    tgt = tgt_points.unsqueeze(0) if squeeze else tgt_points
    w = None if weights is None else (weights.unsqueeze(0) if squeeze else weights)
    dev = src.device if src.is_cuda else torch.device("cuda")
    B, N = int(src.shape[0]), int(src.shape[1])
    src, tgt = A.upload(src, device=dev), A.upload(tgt, device=dev)
    w = None if w is None else A.upload(w, device=dev)
    T = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    L.check(L.lib().roitr_weighted_procrustes(B, N, src.data_ptr(), tgt.data_ptr(), None if w is None else w.data_ptr(),
                                              float(weight_thresh), float(eps), T.data_ptr(), L.stream_ptr().value), "weighted_procrustes")
    if return_transform:
        return T.squeeze(0) if squeeze else T
    R, t = T[:, :3, :3].contiguous(), T[:, :3, 3].contiguous()
    if squeeze:
        R, t = R.squeeze(0), t.squeeze(0)
    return R, t


# ---------------------------------------------------------------------------------------------------- metrics (host, float64)
def rotation_error(R1, R2):
    """registration/benchmark.py:14-37: degrees, (b, 1); the trace term clamped to [-1, 1]."""
    R1, R2 = torch.as_tensor(R1), torch.as_tensor(R2)
    R_ = torch.matmul(R1.transpose(1, 2), R2)
    e = ((R_.diagonal(dim1=1, dim2=2).sum(-1) - 1) / 2).unsqueeze(1)
    e = torch.clamp(e, -1, 1)
    return 180. * torch.acos(e) / math.pi


def translation_error(t1, t2):
    """registration/benchmark.py:40-53: metres, (b,); t1 / t2 (b, 3, 1)."""
    return torch.norm(torch.as_tensor(t1) - torch.as_tensor(t2), dim=(1, 2))


def _mat2quat(M):
    """Unit quaternion (w, x, y, z) of a rotation matrix with w >= 0 (the largest-eigenvector form of nibabel.quaternions.mat2quat)."""
    Qxx, Qyx, Qzx, Qxy, Qyy, Qzy, Qxz, Qyz, Qzz = np.asarray(M, dtype=np.float64).flat
    K = np.array([[Qxx - Qyy - Qzz, 0, 0, 0],
                  [Qyx + Qxy, Qyy - Qxx - Qzz, 0, 0],
                  [Qzx + Qxz, Qzy + Qyz, Qzz - Qxx - Qyy, 0],
                  [Qyz - Qzy, Qzx - Qxz, Qxy - Qyx, Qxx + Qyy + Qzz]]) / 3.0
    vals, vecs = np.linalg.eigh(K)
    q = vecs[[3, 0, 1, 2], np.argmax(vals)]
    return -q if q[0] < 0 else q


def compute_transformation_err(trans, info):
    """registration/benchmark.py:56-75: er = [t, q_xyz] with q the rotation's quaternion (w >= 0); er^T info er / info[0, 0]."""
    trans = np.asarray(trans, dtype=np.float64)
    t = trans[:3, 3]
    q = _mat2quat(trans[:3, :3])
    er = np.concatenate([t, q[1:]], axis=0)
    p = er.reshape(1, 6) @ np.asarray(info, dtype=np.float64) @ er.reshape(6, 1) / info[0, 0]
    return p.item()


def read_trajectory(filename, dim=4):
    """registration/benchmark.py:78-114: (keys (n, 3) str, traj (n, dim, dim) float64) of a 3DMatch / Redwood .log file."""
    with open(filename) as f:
        lines = [ln for ln in f.readlines() if ln.strip()]
    keys = np.asarray([ln.split()[0:3] for ln in lines[0::dim + 1]])
    traj = np.asarray([ln.split()[0:dim] for i, ln in enumerate(lines) if i % (dim + 1) != 0], dtype=np.float64).reshape(-1, dim, dim)
    return keys, traj


def read_trajectory_info(filename, dim=6):
    """registration/benchmark.py:117-145: (n_frame, info (n, dim, dim) float64) of a .info file."""
    with open(filename) as f:
        contents = [ln for ln in f.readlines() if ln.strip()]
    n_pairs = len(contents) // 7
    assert len(contents) == 7 * n_pairs
    info, n_frame = [], 0
    for i in range(n_pairs):
        _, _, n_frame = [int(x) for x in contents[i * 7].split()]
        info.append(np.asarray([[float(v) for v in ln.split()] for ln in contents[i * 7 + 1:i * 7 + 7]]))
    return n_frame, np.asarray(info, dtype=np.float64).reshape(-1, dim, dim)


def write_trajectory(traj, metadata, filename, dim=4):
    """registration/benchmark.py:168-185: the pairs whose metadata[idx][2] is non-zero, in the .log format (12 decimals)."""
    with open(filename, "w") as f:
        for idx in range(traj.shape[0]):
            if metadata[idx][2]:
                p = np.asarray(traj[idx]).tolist()
                f.write("\t".join(map(str, metadata[idx])) + "\n")
                f.write("\n".join("\t".join(map("{0:.12f}".format, p[i])) for i in range(dim)))
                f.write("\n")


def write_trajectory_info(info, metadata, filename, dim=6):
    """The .info counterpart of write_trajectory (the layout read_trajectory_info reads)."""
    with open(filename, "w") as f:
        for idx in range(info.shape[0]):
            f.write("\t".join(map(str, metadata[idx])) + "\n")
            f.write("\n".join("\t".join(map("{0:.12f}".format, row)) for row in np.asarray(info[idx]).tolist()))
            f.write("\n")


def evaluate_registration(num_fragment, result, result_pairs, gt_pairs, gt, gt_info, err2=0.2):
    """registration/benchmark.py:214-260: 3DMatch-protocol precision and recall (only non-consecutive pairs, RMSE <= err2) and the
    per-result flags (0 good, 1 bad, 2 not a tested pair)."""
    err2 = err2 ** 2
    gt_mask = np.zeros((num_fragment, num_fragment), dtype=np.int64)
    flags = []
    for idx in range(gt_pairs.shape[0]):
        i, j = int(gt_pairs[idx, 0]), int(gt_pairs[idx, 1])
        if j - i > 1:   # only non-consecutive pairs are tested
            gt_mask[i, j] = idx
    n_gt = np.sum(gt_mask > 0)
    good, n_res = 0, 0
    for idx in range(result_pairs.shape[0]):
        i, j = int(result_pairs[idx, 0]), int(result_pairs[idx, 1])
        pose = result[idx, :, :]
        if gt_mask[i, j] > 0:
            n_res += 1
            gt_idx = gt_mask[i, j]
            p = compute_transformation_err(np.linalg.inv(gt[gt_idx, :, :]) @ pose, gt_info[gt_idx, :, :])
            if p <= err2:
                good += 1
                flags.append(0)
            else:
                flags.append(1)
        else:
            flags.append(2)
    if n_res == 0:
        n_res += 1e6
    return good * 1.0 / n_res, good * 1.0 / n_gt, flags


def pose_errors(T_est, rot, trans):
    """(RRE degrees, RTE metres) of estimated 4x4 transforms against ground-truth rot (b,3,3) / trans (b,3[,1]), float64."""
    T_est = torch.as_tensor(T_est).double().cpu().reshape(-1, 4, 4)
    rot = torch.as_tensor(rot).double().cpu().reshape(-1, 3, 3)
    trans = torch.as_tensor(trans).double().cpu().reshape(-1, 3, 1)
    rre = rotation_error(T_est[:, :3, :3], rot)[:, 0]
    rte = translation_error(T_est[:, :3, 3:4], trans)
    return rre, rte
