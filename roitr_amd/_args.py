"""Argument preparation shared by the evaluation and preparation operators (registration, nonrigid, descmatch, loss, pairgt, prep,
evaluate): checks that raise RoitrError before anything reaches the library, and the small tensors every call builds.

Two conventions for the rows of B concatenated clouds or lists stay public as they are:
  * `offset`, the reference's pointops convention: B cumulative ENDS, cloud b owns rows [offset[b - 1], offset[b]) with offset[-1] = 0
    (prep.estimate_normals / voxel_down_sample / random_subsample, pairgt.*);
  * `starts`: B + 1 entries, pair b owns rows [starts[b], starts[b + 1]) (registration, nonrigid, descmatch, evaluate, and the
    engine's pair_starts).  `cumulative(sizes)` gives the starts; its [1:] are the offsets.
"""
import numpy as np
import torch

from . import _lib as L


def dev(t, dtype, what):
    """A device tensor as contiguous `dtype`; anything else is an error, not a fallback."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise L.RoitrError(f"{what}: roitr_amd needs ROCm device tensors (no CPU fallback)")
    return t.to(dtype).contiguous()


def points(t, what):
    t = dev(t, torch.float32, what)
    if t.dim() != 2 or t.shape[1] != 3:
        raise L.RoitrError(f"{what} must be (n, 3), got {tuple(t.shape)}")
    return t


def starts(t, what, B=None):
    t = dev(t, torch.int32, what).reshape(-1)
    if t.numel() < 1 or (B is not None and t.numel() != B + 1):
        raise L.RoitrError(f"{what} must hold pairs + 1 entries, got {t.numel()}" + ("" if B is None else f" for {B} pairs"))
    return t


def poses(rot, trans, B):
    """Device tensors rot (B,3,3) / trans (B,3[,1]) as contiguous fp32 (B,3,3) / (B,3)."""
    rot, trans = dev(rot, torch.float32, "rot").reshape(-1, 3, 3), dev(trans, torch.float32, "trans").reshape(-1, 3)
    if rot.shape[0] != B or trans.shape[0] != B:
        raise L.RoitrError(f"rot / trans: {rot.shape[0]} / {trans.shape[0]} poses for {B} pairs")
    return rot, trans


def upload(x, dtype=torch.float32, device="cuda"):
    """A numpy array or a tensor (host or device) as a contiguous device tensor of `dtype`."""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=device, dtype=dtype).contiguous()


def correspondences(starts, src_pts, tgt_pts, scores, per_row="scores"):
    """The row arrays of the hypothesis estimators (lgr, compat), tensors or arrays on either side, as device tensors on src_pts's
    device: (device, starts int32, B, src (rows,3), tgt (rows,3), rows, w (rows) or None).  per_row: what the error about a
    scores length names."""
    src_pts = src_pts if torch.is_tensor(src_pts) else torch.as_tensor(src_pts)
    device = src_pts.device if src_pts.is_cuda else torch.device("cuda")
    starts = torch.as_tensor(starts).to(device=device, dtype=torch.int32).contiguous()
    src = upload(src_pts, device=device).reshape(-1, 3)
    tgt = upload(tgt_pts, device=device).reshape(-1, 3)
    if src.shape != tgt.shape:
        raise ValueError("src_pts and tgt_pts must have the same shape")
    rows = int(src.shape[0])
    w = None if scores is None else upload(scores, device=device).reshape(-1)
    if w is not None and int(w.shape[0]) != rows:
        raise ValueError(f"{per_row} must have one entry per row")
    return device, starts, max(int(starts.shape[0]) - 1, 0), src, tgt, rows, w


def cumulative(sizes, device):
    """starts (len(sizes) + 1) int32 on the device of host-known row counts: [0, n0, n0 + n1, ...]; (n,) gives one pair's [0, n]."""
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), device=device)


def workspace(nbytes, device):
    return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device)
