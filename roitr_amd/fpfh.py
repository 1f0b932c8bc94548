"""FPFH descriptors on the GPU and the learning-free registration baseline on top of them (DESIGN.md section 7 row f13, section 7.9;
csrc/fpfh.hip).

Open3D's compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn)) restated (include/roitr_pointops.h states the rules above
roitr_fpfh_batch; parity with the original is unpinned): per point the pair features of its neighbours -- the first max_nn - 1 other
points of the exact kNN row that lie within the radius -- in three 11-bin histograms (SPFH), then the neighbours' histograms blended
by 1 / d2.  Everything downstream is what the learned descriptors go through: descmatch under the squared distance, the
spatial-compatibility estimator or RANSAC, pose_errors.  No CPU fallback.
"""
import numpy as np
import torch

from . import _args as A
from . import _lib as L
from .pairgt import _check_offsets

NONFINITE = 1   # status bit: the cloud holds a non-finite coordinate or normal; its rows are zero
BINS = 33

_lib = L.binder(("roitr_fpfh_workspace_bytes", "roitr_fpfh_batch"))   # the library with this module's two entry points bound from the header


@torch.no_grad()
def compute_fpfh(xyz, normals, offset, radius=0.125, max_nn=100, pad_to=36, return_stages=False, strict=True):
    """xyz (n,3) / normals (n,3) fp32 device tensors of b concatenated clouds, offset (b) cumulative ends (host offsets are checked,
    device offsets trusted) -> fpfh (n, pad_to) fp32: 33 bins and zero columns up to pad_to (descmatch takes dims that are multiples
    of 4; zero columns change neither a dot product nor a distance).  max_nn in [2, 100]: a point has at most max_nn - 1 neighbours.

    return_stages: (fpfh, spfh_counts (n,33) int32, nbr_count (n) int32, status (b) int32).  strict: raise RoitrError naming the first
    cloud with a non-finite coordinate or normal (one host read of the status words); otherwise its rows are zero."""
    xyz, normals = A.points(xyz, "compute_fpfh: xyz"), A.points(normals, "compute_fpfh: normals")
    dev = xyz.device
    normals = normals.to(dev)
    n = int(xyz.shape[0])
    if int(normals.shape[0]) != n:
        raise L.RoitrError("compute_fpfh: normals must have one row per point")
    _check_offsets("offset", offset, n)
    off = torch.as_tensor(offset).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    b, max_nn, pad_to = int(off.shape[0]), int(max_nn), int(pad_to)
    out = torch.empty((n, max(pad_to, 0)), dtype=torch.float32, device=dev)
    counts = torch.empty((n, BINS), dtype=torch.int32, device=dev) if return_stages else None
    nbr = torch.empty((n,), dtype=torch.int32, device=dev) if return_stages else None
    status = torch.zeros((b,), dtype=torch.int32, device=dev)
    lib = _lib()
    nbytes = int(lib.roitr_fpfh_workspace_bytes(b, n, max_nn))
    ws = A.workspace(nbytes, dev)
    L.check(lib.roitr_fpfh_batch(b, n, xyz.data_ptr(), normals.data_ptr(), off.data_ptr(), float(radius), max_nn, pad_to, out.data_ptr(),
                                 None if counts is None else counts.data_ptr(), None if nbr is None else nbr.data_ptr(),
                                 status.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr().value), "fpfh_batch")
    if strict:
        host = status.cpu()
        if bool(host.any()):
            raise L.RoitrError(f"compute_fpfh: cloud {int(torch.nonzero(host)[0])}: a non-finite coordinate or normal")
    return (out, counts, nbr, status) if return_stages else out


@torch.no_grad()
def fpfh_match_batch(src_xyz, src_normals, src_offset, tgt_xyz, tgt_normals, tgt_offset, radius=0.125, max_nn=100, mode="mutual"):
    """FPFH matches of B pairs: ONE compute_fpfh call over the source clouds followed by the target clouds, then
    descmatch.match_batch(metric="sqdist") of every source cloud against its target.  Offsets (B) are cumulative ends per side.

    Returns match_batch's dict (row_idx / row_val / col_idx / col_val, corr_starts (B + 1), corr (n, 2) local indices of `mode`) plus
    fpfh (rows of both sides, 36 columns), src_starts / tgt_starts (B + 1) into it."""
    from . import descmatch
    src, tgt = A.points(src_xyz, "fpfh_match_batch: src_xyz"), A.points(tgt_xyz, "fpfh_match_batch: tgt_xyz")
    dev = src.device
    n_src, n_tgt = int(src.shape[0]), int(tgt.shape[0])
    _check_offsets("src_offset", src_offset, n_src)
    _check_offsets("tgt_offset", tgt_offset, n_tgt)
    so = torch.as_tensor(src_offset).to(device=dev, dtype=torch.int32).reshape(-1)
    to = torch.as_tensor(tgt_offset).to(device=dev, dtype=torch.int32).reshape(-1)
    if so.shape[0] != to.shape[0]:
        raise L.RoitrError("fpfh_match_batch: src_offset and tgt_offset must have one entry per pair")
    nrm = torch.cat([A.points(src_normals, "fpfh_match_batch: src_normals"), A.points(tgt_normals, "fpfh_match_batch: tgt_normals").to(dev)])
    desc = compute_fpfh(torch.cat([src, tgt.to(dev)]), nrm, torch.cat([so, to + n_src]), radius, max_nn)
    zero = torch.zeros((1,), dtype=torch.int32, device=dev)
    src_starts, tgt_starts = torch.cat([zero, so]), torch.cat([zero, to]) + n_src
    m = descmatch.match_batch(src_starts, desc, tgt_starts, desc, metric="sqdist", mode=mode)
    m.update(fpfh=desc, src_starts=src_starts, tgt_starts=tgt_starts)
    return m


def _matched(m, rows):
    """(row of every match's source point, matched source points, matched target points) of a match dict whose starts point into `rows`."""
    corr, starts = m["corr"].long(), m["corr_starts"]
    B = int(starts.shape[0]) - 1
    pair = torch.bucketize(torch.arange(corr.shape[0], device=corr.device), starts[1:].long(), right=True).clamp_max(max(B - 1, 0))
    si = m["src_starts"].long()[pair] + corr[:, 0]
    ti = m["tgt_starts"].long()[pair] + corr[:, 1]
    return si, rows[si].contiguous(), rows[ti].contiguous()


def _estimate(m, matched, estimator, kw, pair_keys=None):
    """Poses from the matches: compat_batch or fgr_batch with 1 / (1 + squared distance) as confidences, or ransac_batch over all of them.  A
    smaller distance is a better match, but the negated distance cannot serve: compat's refits weigh every inlier row by its
    confidence (include/roitr_engine.h), and negative weights mirror the cross-covariance -- an exact copy came back rotated by 180
    degrees.  1 / (1 + d) orders the rows like -d and lies in (0, 1]."""
    if estimator not in ("compat", "ransac", "fgr"):
        raise ValueError("the FPFH baseline runs with estimator 'compat', 'ransac' or 'fgr' (lgr needs the matcher's patches)")
    si, s, t = matched
    if estimator == "fgr":   # the same confidences as compat: the objective weighs every row by its score
        from .fgr import fgr_batch
        return fgr_batch(m["corr_starts"], s, t, 1.0 / (1.0 + m["row_val"][si]), **dict(dict(pair_keys=pair_keys), **kw))
    if estimator == "compat":
        from .compat import compat_batch
        return compat_batch(m["corr_starts"], s, t, 1.0 / (1.0 + m["row_val"][si]), **kw)
    from .registration import ransac_batch
    return ransac_batch(m["corr_starts"], s, t, None, **dict(dict(sample="all", pair_keys=pair_keys), **kw))


@torch.no_grad()
def fpfh_pose_estimation(src_pcd, tgt_pcd, src_normals, tgt_normals, *, radius=0.125, max_nn=100, mutual=True, estimator="compat", **kw):
    """One pair, from points and normals to a pose without a learned descriptor: FPFH, matches under the squared distance (mutual, or
    every source point with its nearest target), then compat.compat_batch or fgr.fgr_batch with 1 / (1 + distance) as confidences, or
    registration.ransac_batch over all matches.  kw: the estimator's keyword arguments (compat's own `radius` keeps its default: the
    name is taken by the FPFH radius here).  Returns the 4x4 float64 numpy transform."""
    src, tgt = A.upload(src_pcd).reshape(-1, 3), A.upload(tgt_pcd).reshape(-1, 3)
    m = fpfh_match_batch(src, A.upload(src_normals).reshape(-1, 3), [int(src.shape[0])], tgt, A.upload(tgt_normals).reshape(-1, 3),
                         [int(tgt.shape[0])], radius, max_nn, mode="mutual" if mutual else "row")
    reg = _estimate(m, _matched(m, torch.cat([src, tgt])), estimator, kw)
    return reg["T"][0].cpu().numpy().astype(np.float64)


@torch.no_grad()
def fpfh_handle(handle, radius=0.125, max_nn=100, mode="mutual", estimator=None, estimator_kw=None, pair_keys=None,
                inlier_distance_threshold=None):
    """The baseline on the clouds and normals an engine call already holds (RIGA_v2.launch_batch() handle, after finish_batch): one
    compute_fpfh over all 2B clouds, one match_batch.  Returns fpfh_match_batch's dict; with estimator ("compat" / "ransac" / "fgr",
    estimator_kw its keyword arguments, pair_keys the keys of RANSAC's random stream and of fgr's tuple test) also reg, the estimator's result dict
    (T (B,4,4), inliers, ...); with inlier_distance_threshold (needs ground-truth transforms in the pairs) also ir (B,) the share of
    the matches within it under the ground truth (nan: no matches) and n_matches (B,) int32."""
    from . import descmatch
    from .riga import handle_layout, handle_normals, handle_poses
    pts, src_starts, tgt_starts = handle_layout(handle, "point")
    B = handle["B"]
    offs = torch.cat([src_starts[1:], tgt_starts[1:]]) if B > 0 else src_starts[1:]
    desc = compute_fpfh(pts, handle_normals(handle), offs, radius, max_nn)
    m = descmatch.match_batch(src_starts, desc, tgt_starts, desc, metric="sqdist", mode=mode)
    m.update(fpfh=desc, src_starts=src_starts, tgt_starts=tgt_starts)
    if estimator is None and inlier_distance_threshold is None:
        return m
    matched = _matched(m, pts)
    if estimator is not None:
        m["reg"] = _estimate(m, matched, estimator, dict(estimator_kw or {}), pair_keys)
    if inlier_distance_threshold is not None:
        from .evaluate import _inlier_counts
        rot, trans = handle_poses(handle, "fpfh_handle")
        inl = _inlier_counts(m["corr_starts"], matched[1], matched[2], rot, trans, inlier_distance_threshold)
        cnt = (m["corr_starts"][1:] - m["corr_starts"][:-1]).to(torch.int32)
        m["n_matches"] = cnt
        m["ir"] = torch.where(cnt > 0, inl.float() / cnt.clamp_min(1).float(), torch.full((B,), float("nan"), device=pts.device))
    return m
