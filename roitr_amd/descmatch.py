"""Descriptor matching on the GPU: nearest neighbours in descriptor space in both directions, the
mutual check, the descriptor-level inlier ratio and the feature-matching recall's input.

`match_batch` / `descriptor_handle` run one fused fp32 MFMA product per pair (csrc/desc_match.hip; the rules are stated in
include/roitr_engine.h): the (N, M) score matrix never reaches memory, only the best entry of every row and of every column does.
`matching_descriptors` (lib/utils.py:99-136), `mutual_selection` and `get_inlier_ratio` (registration/benchmark_utils.py:42-121)
keep the reference's names, signatures and return types.

Differences from the reference, by design: among equal scores THE LOWEST INDEX wins in both directions (what np.argmax / np.argmin /
torch.max give, so there is none on finite input); scores are fp32 MFMA sums in a fixed k order where the reference has a BLAS
product, so an index can differ where two scores lie within rounding of each other (tests/descmatch_util.py states the bound).
"""
import numpy as np
import torch

from . import _args as A
from . import _lib as L
from .riga import handle_layout, handle_poses

METRICS = {"dot": 0, "sqdist": 1}
MODES = {"row": 0, "col": 1, "mutual": 2}


def _desc(t, what):
    t = A.dev(t, torch.float32, what)
    if t.dim() != 2:
        raise L.RoitrError(f"{what} must be (rows, dim), got {tuple(t.shape)}")
    return t


@torch.no_grad()
def select(src_offsets, tgt_offsets, row_idx, col_idx, mode="mutual", capacity=None):
    """roitr_desc_match_select: the matches of `mode` ("row", "col", "mutual") as (corr_starts (B + 1) int32, corr (n, 2) int32
    local (source, target) indices, needed): pair b's rows are corr[corr_starts[b]:corr_starts[b + 1]].  capacity (default: the
    mode's upper bound, which never cuts) limits the rows written; `needed` is the count the full list has."""
    if mode not in MODES:
        raise L.RoitrError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    src_offsets = A.starts(src_offsets, "src_offsets")
    B = int(src_offsets.numel()) - 1
    tgt_offsets = A.starts(tgt_offsets, "tgt_offsets", B)
    row_idx, col_idx = A.dev(row_idx, torch.int32, "row_idx"), A.dev(col_idx, torch.int32, "col_idx")
    dev = row_idx.device
    if row_idx.numel() == 0:   # a side without rows is never read, but the entry point refuses a null pointer
        row_idx = torch.full((1,), -1, dtype=torch.int32, device=dev)
    if col_idx.numel() == 0:
        col_idx = torch.full((1,), -1, dtype=torch.int32, device=dev)
    bound = int(col_idx.numel()) if mode == "col" else int(row_idx.numel())   # every row emits at most once
    cap = bound if capacity is None else int(capacity)
    corr_starts = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    corr = torch.full((max(cap, 1), 2), -1, dtype=torch.int32, device=dev)
    n_out = torch.empty((1,), dtype=torch.int32, device=dev)
    L.check(L.lib().roitr_desc_match_select(B, src_offsets.data_ptr(), tgt_offsets.data_ptr(), row_idx.data_ptr(), col_idx.data_ptr(),
                                            MODES[mode], corr_starts.data_ptr(), corr.data_ptr(), cap, n_out.data_ptr(),
                                            L.stream_ptr().value), "desc_match_select")
    needed = int(n_out.item())   # the one host round trip: the capacity check
    return corr_starts, corr[:min(needed, cap)], needed


@torch.no_grad()
def match_batch(src_offsets, src_desc, tgt_offsets, tgt_desc, *, metric="dot", mode="mutual"):
    """Matches the descriptors of every pair of a batch.  Pair b owns rows [src_offsets[b], src_offsets[b+1]) of src_desc
    (total_src, dim) and rows [tgt_offsets[b], tgt_offsets[b+1]) of tgt_desc (total_tgt, dim); both may be the same tensor (an
    engine call's point_feats).  Device tensors; dim a multiple of 4 in [4, 1024].
    metric: "dot" (s . t, the largest wins) or "sqdist" (max(|s|^2 + |t|^2 - 2 s.t, 1e-12), the smallest wins).

    Returns a dict of device tensors: row_idx (total_src) int32, the best target of every source row, local to its pair (-1: the
    pair has no targets, or the row belongs to no pair) and row_val, its score; col_idx / col_val (total_tgt) likewise; corr_starts
    (B + 1) and corr (n, 2): the (source, target) matches of `mode` ("row", "col" or "mutual"), local indices, in increasing order."""
    if metric not in METRICS:
        raise L.RoitrError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    if mode not in MODES:
        raise L.RoitrError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    src_offsets = A.starts(src_offsets, "src_offsets")
    B = int(src_offsets.numel()) - 1
    tgt_offsets = A.starts(tgt_offsets, "tgt_offsets", B)
    src_desc, tgt_desc = _desc(src_desc, "src_desc"), _desc(tgt_desc, "tgt_desc")
    if src_desc.shape[1] != tgt_desc.shape[1]:
        raise L.RoitrError(f"src_desc / tgt_desc: dim {src_desc.shape[1]} against {tgt_desc.shape[1]}")
    dev = src_desc.device
    n_src, n_tgt, dim = int(src_desc.shape[0]), int(tgt_desc.shape[0]), int(src_desc.shape[1])
    row_idx = torch.empty((n_src,), dtype=torch.int32, device=dev)
    row_val = torch.empty((n_src,), dtype=torch.float32, device=dev)
    col_idx = torch.empty((n_tgt,), dtype=torch.int32, device=dev)
    col_val = torch.empty((n_tgt,), dtype=torch.float32, device=dev)
    lib = L.lib()
    nbytes = int(lib.roitr_desc_match_workspace_bytes(B, n_src, n_tgt))
    ws = A.workspace(nbytes, dev)
    L.check(lib.roitr_desc_match_batch(B, dim, src_offsets.data_ptr(), n_src, src_desc.data_ptr(), tgt_offsets.data_ptr(), n_tgt,
                                       tgt_desc.data_ptr(), METRICS[metric], row_idx.data_ptr(), row_val.data_ptr(), col_idx.data_ptr(),
                                       col_val.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr().value), "desc_match_batch")
    corr_starts, corr, _ = select(src_offsets, tgt_offsets, row_idx, col_idx, mode)
    return dict(row_idx=row_idx, row_val=row_val, col_idx=col_idx, col_val=col_val, corr_starts=corr_starts, corr=corr)


def _match_one(src_desc, tgt_desc, metric, mode):
    s, t = A.upload(src_desc), A.upload(tgt_desc)
    return match_batch(A.cumulative([s.shape[0]], "cuda"), s, A.cumulative([t.shape[0]], "cuda"), t, metric=metric, mode=mode), s.shape[0], t.shape[0]


@torch.no_grad()
def matching_descriptors(src_desc, tgt_desc, mutual=False, major=None):
    """lib/utils.py:99-136 on the GPU: correspondences (n, 2) as a numpy int64 array, nearest neighbours under the squared
    distance.  major "row": (i, nearest target of i); "col": (nearest source of j, j); None: the union of both in np.nonzero
    order; mutual: the pairs that are each other's nearest (major is not used then, as in the reference)."""
    assert major in ["row", "col"] or major is None
    mode = "mutual" if mutual else ("col" if major == "col" else "row")
    r, n, m = _match_one(src_desc, tgt_desc, "sqdist", mode)
    if mutual or major is not None:
        return r["corr"].cpu().numpy().astype(np.int64)
    # the union (a cold path): keys i * M + j of both directions, sorted, duplicates removed
    i = torch.arange(n, device="cuda", dtype=torch.int64)
    j = torch.arange(m, device="cuda", dtype=torch.int64)
    keys = torch.cat([i * m + r["row_idx"].long(), r["col_idx"].long() * m + j]) if n > 0 and m > 0 else i[:0]
    keys = torch.unique(keys, sorted=True)
    return torch.stack([keys // max(m, 1), keys % max(m, 1)], 1).cpu().numpy().astype(np.int64)


@torch.no_grad()
def mutual_selection(score_mat):
    """registration/benchmark_utils.py:42-66 for a dense score matrix the caller already has ((N, M) or (B, N, M), numpy or
    torch): a bool numpy array of the same batched shape, True where an entry is the maximum of its row and of its column (the first
    one at equal values)."""
    s = score_mat if torch.is_tensor(score_mat) else torch.from_numpy(np.ascontiguousarray(score_mat))
    if s.dim() == 2:
        s = s[None]
    B, N, M = s.shape
    out = torch.zeros((B, N, M), dtype=torch.bool, device=s.device)
    if N > 0 and M > 0:
        r = s.argmax(2)                                   # (B, N)
        c = s.argmax(1)                                   # (B, M)
        rows = torch.arange(N, device=s.device)[None].expand(B, N)
        keep = c.gather(1, r) == rows
        out[torch.arange(B, device=s.device)[:, None].expand(B, N)[keep], rows[keep], r[keep]] = True
    return out.cpu().numpy()


@torch.no_grad()
def get_inlier_ratio(src_pcd, tgt_pcd, src_feat, tgt_feat, rot, trans, inlier_distance_threshold=0.1):
    """registration/benchmark_utils.py:80-121 on the GPU: results['wo' | 'w']['distance' | 'inlier_ratio'], without and with the
    mutual check: the distances (numpy) between rot src + trans and the matched target points, and the share below the threshold
    (a 0-dim tensor; nan for an empty mutual set, the mean of nothing, as in the reference)."""
    r, n, m = _match_one(src_feat, tgt_feat, "dot", "mutual")
    src, tgt = A.upload(src_pcd).reshape(-1, 3), A.upload(tgt_pcd).reshape(-1, 3)
    rot, trans = A.upload(rot).reshape(3, 3), A.upload(trans).reshape(3, 1)
    src = (torch.matmul(rot, src.transpose(0, 1)) + trans).transpose(0, 1)
    results = {"w": {}, "wo": {}}
    for key, si, ti in (("wo", torch.arange(n, device="cuda"), r["row_idx"].long()), ("w", r["corr"][:, 0].long(), r["corr"][:, 1].long())):
        dist = torch.norm(src[si] - tgt[ti], dim=1)
        results[key]["distance"] = dist.cpu().numpy()
        results[key]["inlier_ratio"] = (dist < inlier_distance_threshold).float().mean().cpu()
    return results


@torch.no_grad()
def descriptor_handle(handle, which="point", inlier_distance_threshold=0.1):
    """The descriptor-level evaluation of a whole RIGA_v2.launch_batch() handle, after finish_batch(handle): ONE match_batch over the
    call's descriptor buffer (which = "point": point_feats against the input points; "node": node_feats against node_xyz), source
    and target of every pair matched in place.  Needs ground-truth transforms in the pairs.

    Returns a dict of device tensors: ir_wo (B,) the inlier ratio of every source row's best target, ir_w (B,) the same over the
    mutual matches (nan for a pair without any), n_wo / n_w (B,) int32 the counts of matches, and the mutual correspondences as
    points in the layout registration.ransac_batch takes: starts (B + 1) int32, src_pts / tgt_pts (n, 3) (source points NOT
    transformed), plus corr (n, 2) their local indices."""
    from .evaluate import _inlier_counts
    pts, src_off, tgt_off = handle_layout(handle, which)
    rot, trans = handle_poses(handle, "descriptor_handle")
    B = handle["B"]
    desc = handle["out"]["point_feats" if which == "point" else "node_feats"][:pts.shape[0]]
    dev = desc.device
    r = match_batch(src_off, desc, tgt_off, desc, metric="dot", mode="mutual")
    n_src_rows = sum(handle["n_all" if which == "point" else "n4"][:B])
    n_src = src_off[1:] - src_off[:-1]
    # without the mutual check: source row i of pair b against target tgt_off[b] + row_idx[i]
    pair_of_row = torch.repeat_interleave(torch.arange(B, device=dev), n_src, output_size=n_src_rows)
    ri = r["row_idx"][:n_src_rows].long()
    has = ri >= 0
    tgt_abs = torch.where(has, tgt_off.long()[pair_of_row] + ri, torch.zeros_like(ri))
    # a pair without targets has no matches: its rows are compared with a point at infinity and count as outliers
    tgt_wo = torch.where(has[:, None], pts[tgt_abs], torch.full_like(pts[tgt_abs], float("inf")))
    inl_wo = _inlier_counts(src_off, pts[:n_src_rows].contiguous(), tgt_wo.contiguous(), rot, trans, inlier_distance_threshold)
    n_wo = n_src
    ir_wo = torch.where(n_wo > 0, inl_wo.float() / n_wo.clamp_min(1).float(), torch.full((B,), float("nan"), device=dev))
    # with it
    corr, starts = r["corr"].long(), r["corr_starts"]
    pair_of_corr = torch.bucketize(torch.arange(corr.shape[0], device=dev), starts[1:].long(), right=True).clamp_max(max(B - 1, 0))
    src_pts = pts[src_off.long()[pair_of_corr] + corr[:, 0]].contiguous()
    tgt_pts = pts[tgt_off.long()[pair_of_corr] + corr[:, 1]].contiguous()
    inl_w = _inlier_counts(starts, src_pts, tgt_pts, rot, trans, inlier_distance_threshold)
    n_w = (starts[1:] - starts[:-1]).to(torch.int32)
    ir_w = torch.where(n_w > 0, inl_w.float() / n_w.clamp_min(1).float(), torch.full((B,), float("nan"), device=dev))
    return dict(ir_wo=ir_wo, ir_w=ir_w, n_wo=n_wo, n_w=n_w, starts=starts, src_pts=src_pts, tgt_pts=tgt_pts, corr=r["corr"])
