"""Pair ground truth on the GPU (csrc/pairgt.hip).

For B ragged pairs of clouds under their ground-truth transforms (source to target, p' = R p + t): the target points within a radius
of every moved source point.  One batched fixed-radius search gives the three things the reference only ships as files or loops
over in Python:
  * the overlap ratio of a pair (gt_overlap.log: 3DMatch >= 0.3, 3DLoMatch 0.1 .. 0.3),
  * the 6x6 information matrix of a pair (gt.info, what registration/benchmark.py:56-75 computeTransformationErr needs for the
    registration recall),
  * the point-level ground-truth correspondences (lib/utils.py:72-96 get_correspondences; 4DMatch's entry['correspondences']).
The decision is defined in float64 on the fp32 inputs (include/roitr_pointops.h states it): (i, j) is a correspondence iff
d2 < radius^2, strictly, with radius taken as fp32.  Open3D's KD-tree may decide boundary pairs differently: parity with it is
unpinned.  No CPU fallback.
"""
import collections

import numpy as np
import torch

from . import _args as A
from . import _lib as L
from .riga import handle_layout, handle_poses

STATUS_NONFINITE, STATUS_EMPTY, STATUS_OVERFLOW = 1, 2, 4

PairGroundTruth = collections.namedtuple("PairGroundTruth", "overlap_src overlap_tgt n_src_hit n_tgt_hit info count nn_idx nn_dist2 status")


def _check_offsets(name, offset, rows):
    """Offsets that arrive on the host are checked for free; device offsets are a precondition (checking them would cost a host read):
    non-decreasing, non-negative, the last one equal to the number of rows.  The kernels index with them unchecked."""
    if torch.is_tensor(offset) and offset.is_cuda:
        return
    o = [int(x) for x in torch.as_tensor(offset).reshape(-1).tolist()]
    if not o or o[-1] != rows or any(b < a for a, b in zip([0] + o, o)):
        raise L.RoitrError(f"pairgt: {name} must be cumulative (non-decreasing, >= 0) and end at the number of rows ({rows})")


def _inputs(src, src_offset, tgt, tgt_offset, rot, trans):
    src, tgt = A.dev(src, torch.float32, "pairgt").reshape(-1, 3), A.dev(tgt, torch.float32, "pairgt").reshape(-1, 3)
    dev = src.device
    tgt = tgt.to(dev)
    _check_offsets("src_offset", src_offset, int(src.shape[0]))
    _check_offsets("tgt_offset", tgt_offset, int(tgt.shape[0]))
    so = torch.as_tensor(src_offset).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    to = torch.as_tensor(tgt_offset).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    B = int(so.shape[0])
    if int(to.shape[0]) != B:
        raise L.RoitrError("pairgt: src_offset and tgt_offset must have one entry per pair")
    rot = torch.as_tensor(rot).to(device=dev, dtype=torch.float32).reshape(-1, 3, 3).contiguous()
    trans = torch.as_tensor(trans).to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    if int(rot.shape[0]) != B or int(trans.shape[0]) != B:
        raise L.RoitrError(f"pairgt: {B} pairs need rot (B,3,3) and trans (B,3)")
    return src, so, tgt, to, rot, trans, B, dev


def _stats(lib, src, so, tgt, to, rot, trans, radius, inverse, want_info, B, dev):
    n, m = int(src.shape[0]), int(tgt.shape[0])
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    nn_idx = torch.empty((n,), dtype=torch.int32, device=dev)
    nn_d2 = torch.empty((n,), dtype=torch.float64, device=dev)
    n_hit = torch.empty((B,), dtype=torch.int32, device=dev)
    overlap = torch.empty((B,), dtype=torch.float64, device=dev)
    info = torch.empty((B, 6, 6), dtype=torch.float64, device=dev) if want_info else None
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    ws = A.workspace(lib.roitr_pairgt_workspace_bytes(B, n, m, 0), dev)
    L.check(lib.roitr_pairgt_stats(B, n, m, src.data_ptr(), so.data_ptr(), tgt.data_ptr(), to.data_ptr(), rot.data_ptr(), trans.data_ptr(),
                                   float(radius), int(inverse), count.data_ptr(), nn_idx.data_ptr(), nn_d2.data_ptr(), n_hit.data_ptr(),
                                   overlap.data_ptr(), None if info is None else info.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                   L.stream_ptr().value), "pairgt_stats")
    return count, nn_idx, nn_d2, n_hit, overlap, info, status


@torch.no_grad()
def pair_ground_truth(src, src_offset, tgt, tgt_offset, rot, trans, radius, both_sides=True):
    """src (n,3) / tgt (m,3) fp32 device tensors of B concatenated clouds with cumulative offsets (B), rot (B,3,3), trans (B,3).
    Precondition: the offsets are non-decreasing, non-negative and end at n / m.  Host offsets (lists, CPU tensors) are checked and
    raise RoitrError; offsets already on the device are trusted -- the kernels index with them, a wrong one reads out of bounds.

    Returns PairGroundTruth of device tensors:
      overlap_src (B) float64 = n_src_hit / n_src: the share of source points with a target point within `radius` after the move;
      overlap_tgt (B) float64, n_tgt_hit (B): the same with the roles swapped (target points moved by R^T (q - t), searched in the
        source clouds; a separately defined quantity) -- None with both_sides=False;
      n_src_hit (B) int32;  info (B,6,6) float64: Redwood's gt.info matrix, sum over the hit source points of G^T G,
        G = [ I | -2 [p]x ] (p in the source frame), info[:, 0, 0] == n_src_hit;
      count (n) int32, nn_idx (n) int32 pair-local (-1: none), nn_dist2 (n) float64 (+inf: none): per source point;
      status (B) int32: bit 1 a non-finite coordinate or transform, bit 2 an empty cloud: such a pair has no correspondences and
        nan ratios (both sides' bits are merged)."""
    src, so, tgt, to, rot, trans, B, dev = _inputs(src, src_offset, tgt, tgt_offset, rot, trans)
    lib = L.lib()
    count, nn_idx, nn_d2, n_hit, overlap, info, status = _stats(lib, src, so, tgt, to, rot, trans, radius, 0, True, B, dev)
    ov_t = hit_t = None
    if both_sides:
        _, _, _, hit_t, ov_t, _, st_t = _stats(lib, tgt, to, src, so, rot, trans, radius, 1, False, B, dev)
        status = status | st_t
    return PairGroundTruth(overlap, ov_t, n_hit, hit_t, info, count, nn_idx, nn_d2, status)


def correspondences_once(src, so, tgt, to, rot, trans, radius, K, capacity, B, dev):
    """One roitr_pairgt_correspondences call with a candidate buffer of `capacity` entries on prepared inputs: (corr (capacity,2),
    corr_offset (B), rows, needed, status) with rows / needed read back from the device (the one host read)."""
    lib = L.lib()
    n, m = int(src.shape[0]), int(tgt.shape[0])
    corr = torch.empty((capacity, 2), dtype=torch.int32, device=dev)
    corr_offset = torch.empty((B,), dtype=torch.int32, device=dev)
    total = torch.empty((2,), dtype=torch.int64, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    ws = A.workspace(lib.roitr_pairgt_workspace_bytes(B, n, m, capacity), dev)
    L.check(lib.roitr_pairgt_correspondences(B, n, m, src.data_ptr(), so.data_ptr(), tgt.data_ptr(), to.data_ptr(), rot.data_ptr(),
                                             trans.data_ptr(), float(radius), 0 if K is None else int(K), capacity, corr.data_ptr(),
                                             corr_offset.data_ptr(), total.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                             L.stream_ptr().value), "pairgt_correspondences")
    rows, need = (int(x) for x in total.cpu().tolist())
    return corr, corr_offset, rows, need, status


@torch.no_grad()
def radius_correspondences(src, src_offset, tgt, tgt_offset, rot, trans, radius, K=None, capacity=None, return_status=False):
    """The ground-truth correspondence list: (corr (total,2) int32, corr_offset (B) cumulative int32).

    Rows are (i, j), pair-local; pairs in input order, ascending i, within an i ascending (d2, j) -- the KD-tree's sorted-by-distance
    order with a defined tie-break; K >= 1 keeps the first K rows of every i (the reference's idx[:K]).  The candidates pass through
    a buffer of `capacity` entries (default: 32 per source point): one host read of the totals, and when they did not fit, one exact
    repeat.  return_status: also the per-pair status words (bits as in pair_ground_truth) of the final call."""
    src, so, tgt, to, rot, trans, B, dev = _inputs(src, src_offset, tgt, tgt_offset, rot, trans)
    if K is not None and int(K) < 1:
        raise L.RoitrError("radius_correspondences: K must be at least 1 (None: no cap)")
    cap = max(32 * int(src.shape[0]), 1024) if capacity is None else int(capacity)
    corr, corr_offset, rows, need, status = correspondences_once(src, so, tgt, to, rot, trans, radius, K, cap, B, dev)
    if need > cap:
        if need > 2 ** 31 - 1:
            raise L.RoitrError(f"radius_correspondences: {need} within-radius pairs do not fit a list (2^31 - 1 at most)")
        corr, corr_offset, rows, need, status = correspondences_once(src, so, tgt, to, rot, trans, radius, K, need, B, dev)
    out = (corr[:rows], corr_offset)
    return out + (status,) if return_status else out


def get_correspondences(src_pcd, tgt_pcd, trans, search_voxel_size, K=None):
    """lib/utils.py:72-96 with (N,3) arrays or tensors in place of Open3D clouds and `trans` the 4x4 source-to-target transform:
    the (?, 2) int64 tensor of (source index, target index) with the target within search_voxel_size of the moved source point."""
    def dev32(x):   # numpy arrays are uploaded, host tensors refused
        return (A.dev(x, torch.float32, "get_correspondences") if torch.is_tensor(x) else A.upload(x)).reshape(-1, 3)
    src, tgt = dev32(src_pcd), dev32(tgt_pcd)
    T = torch.as_tensor(np.asarray(trans.detach().cpu() if torch.is_tensor(trans) else trans, dtype=np.float64).reshape(4, 4))
    off = lambda t: torch.tensor([t.shape[0]], dtype=torch.int32, device=src.device)
    corr, _ = radius_correspondences(src, off(src), tgt, off(tgt), T[:3, :3].float().reshape(1, 3, 3), T[:3, 3].float().reshape(1, 3),
                                     search_voxel_size, K=K)
    return corr.long()


def handle_clouds(handle):
    """(src, src_offset, tgt, tgt_offset, rot, trans) of a RIGA_v2.launch_batch() handle: the clouds the model was fed and the
    ground-truth transforms of its pairs."""
    rot, trans = handle_poses(handle, "pairgt_handle")
    pts, src_starts, tgt_starts = handle_layout(handle, "point")
    B = handle["B"]
    n_src = sum(handle["n_all"][:B])
    return pts[:n_src], src_starts[1:], pts[n_src:], tgt_starts[1:] - n_src, rot.reshape(B, 3, 3), trans.reshape(B, 3)


def pairgt_handle(handle, radius, both_sides=True):
    """pair_ground_truth on the clouds and transforms of an engine batch handle (after finish_batch), like register_handle."""
    return pair_ground_truth(*handle_clouds(handle), radius, both_sides=both_sides)
