"""4DMatch non-rigid evaluation on the GPU: NFMR, the non-rigid feature matching recall.

`nfmr_batch` / `nfmr_handle` run registration/evaluate_fdmatch.py:74-115 (compute_nrfmr) for every pair of a batch in two launches
(csrc/nonrigid.hip; the rules are stated in include/roitr_engine.h).  `compute_nrfmr` and `blend_anchor_motion` keep the
reference's names and signatures, so evaluate_fdmatch.py's loop runs on this project's result files with one import changed.

Differences from the reference, by design: both nearest-neighbour searches take the LOWEST INDEX among equal distances (the
reference's np.argpartition leaves the choice among repeated anchors open, so parity is defined for distinct anchors only);
distances are differences in fp32, not the |a|^2 + |b|^2 - 2ab expansion; a pair with fewer than 3 anchors or without metric points
has NFMR 0 and a status bit where the reference raises; only knn = 3.
"""
import torch

from . import _args as A
from . import _lib as L
from .riga import handle_poses

FEW_ANCHORS, NO_METRIC, BAD_INDEX, BAD_OFFSETS = 1, 2, 4, 8


def _check_status(status, what):
    """The one host round trip of the path."""
    bad = int((status & (BAD_INDEX | BAD_OFFSETS)).max().item()) if status.numel() else 0
    if bad & BAD_OFFSETS:
        raise L.RoitrError(f"{what}: an offset array decreases or leaves [0, total] (pairs {_where(status, BAD_OFFSETS)})")
    if bad & BAD_INDEX:
        raise L.RoitrError(f"{what}: metric_index outside the pair's source cloud (pairs {_where(status, BAD_INDEX)})")


def _where(status, bit):
    return torch.nonzero(status & bit).reshape(-1).tolist()[:8]


@torch.no_grad()
def nfmr_batch(src_offsets, src_raw, src_deformed, corr_starts, src_corr, tgt_corr, metric_starts, metric_index, rot, trans, *,
               search_radius=0.1, recall_thr=0.04, return_errors=False, block=0):
    """NFMR of every pair of a batch.  Pair b owns points [src_offsets[b], src_offsets[b+1]) of src_raw / src_deformed,
    correspondences [corr_starts[b], corr_starts[b+1]) of src_corr / tgt_corr and metric points [metric_starts[b],
    metric_starts[b+1]) of metric_index (indices into the pair's own cloud); rot (B,3,3), trans (B,3[,1]).  Device tensors.

    Returns a dict of device tensors: nfmr (B,) float32, hits, n_metric, status (B,) int32 (FEW_ANCHORS / NO_METRIC pairs have
    NFMR 0) and, with return_errors, anchor_idx (rows of src_corr; local to the pair) and err (per metric point, metres).
    block: lanes per workgroup (0: automatic); the result does not depend on it, nor on the batch a pair travels in."""
    src_offsets = A.starts(src_offsets, "src_offsets")
    B = int(src_offsets.numel()) - 1
    corr_starts, metric_starts = A.starts(corr_starts, "corr_starts", B), A.starts(metric_starts, "metric_starts", B)
    src_raw, src_deformed = A.points(src_raw, "src_raw"), A.points(src_deformed, "src_deformed")
    src_corr, tgt_corr = A.points(src_corr, "src_corr"), A.points(tgt_corr, "tgt_corr")
    if src_raw.shape != src_deformed.shape or src_corr.shape != tgt_corr.shape:
        raise L.RoitrError("src_raw / src_deformed and src_corr / tgt_corr must have the same shapes")
    if not torch.is_tensor(metric_index) or not metric_index.is_cuda:
        raise L.RoitrError("metric_index: roitr_amd needs ROCm device tensors (no CPU fallback)")
    # int64 indices beyond the int32 range stay out of range (-1 / 2^31 - 1) instead of wrapping into it
    metric_index = metric_index.reshape(-1).clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()
    rot, trans = A.poses(rot, trans, B)
    dev = src_raw.device
    n_src, n_corr, n_met = int(src_raw.shape[0]), int(src_corr.shape[0]), int(metric_index.shape[0])
    hits = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    anchor_idx = torch.full((n_corr,), -1, dtype=torch.int32, device=dev) if return_errors else None
    err = torch.full((n_met,), float("inf"), dtype=torch.float32, device=dev) if return_errors else None
    lib = L.lib()
    nbytes = int(lib.roitr_nfmr_workspace_bytes(B, n_corr, n_met))
    ws = A.workspace(nbytes, dev)
    L.check(lib.roitr_nfmr_batch(B, n_src, src_offsets.data_ptr(), src_raw.data_ptr(), src_deformed.data_ptr(), n_corr,
                                 corr_starts.data_ptr(), src_corr.data_ptr(), tgt_corr.data_ptr(), n_met, metric_starts.data_ptr(),
                                 metric_index.data_ptr(), rot.data_ptr(), trans.data_ptr(), float(search_radius), float(recall_thr),
                                 int(block), None if anchor_idx is None else anchor_idx.data_ptr(),
                                 None if err is None else err.data_ptr(), hits.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes,
                                 L.stream_ptr().value), "nfmr_batch")
    _check_status(status, "nfmr_batch")
    n_metric = metric_starts[1:] - metric_starts[:-1]
    nfmr = torch.where(n_metric > 0, hits.float() / n_metric.clamp_min(1).float(), torch.zeros_like(hits, dtype=torch.float32))
    out = dict(nfmr=nfmr, hits=hits, n_metric=n_metric, status=status)
    if return_errors:
        out.update(anchor_idx=anchor_idx, err=err)
    return out


@torch.no_grad()
def compute_nrfmr(data, recall_thr=0.04):
    """registration/evaluate_fdmatch.py:74-115 on the GPU: the NFMR of one saved result file (the dict lib/tester.py:56-69 writes,
    with `metric_index_list`), as a 0-dim tensor like the reference's."""
    raw, deformed = A.upload(data["src_raw_pcd"]).reshape(-1, 3), A.upload(data["src_pcd"]).reshape(-1, 3)
    src_corr, tgt_corr = A.upload(data["src_corr_pts"]).reshape(-1, 3), A.upload(data["tgt_corr_pts"]).reshape(-1, 3)
    index = A.upload(torch.as_tensor(data["metric_index_list"]).reshape(-1), torch.int64)
    ends = lambda t: A.cumulative([t.shape[0]], "cuda")
    r = nfmr_batch(ends(raw), raw, deformed, ends(src_corr), src_corr, tgt_corr, ends(index), index,
                   A.upload(data["rot"]).reshape(1, 3, 3), A.upload(data["trans"]).reshape(1, 3), recall_thr=recall_thr)
    return r["nfmr"][0].cpu()


@torch.no_grad()
def blend_anchor_motion(query_loc, reference_loc, reference_flow, knn=3, search_radius=0.1):
    """registration/evaluate_fdmatch.py:50-71 on the GPU (the blend kernel alone): -> (blended_flow [m,3] float32, mask [m] bool) as
    numpy arrays for numpy inputs and as device tensors for device tensors.  Fewer than 3 references: RoitrError (numpy raises)."""
    if knn != 3:
        raise NotImplementedError("blend_anchor_motion: only knn = 3 (the reference's setting)")
    as_numpy = not torch.is_tensor(query_loc)
    i32 = torch.int32
    q, ref, flow = (A.upload(x).reshape(-1, 3) for x in (query_loc, reference_loc, reference_flow))
    if ref.shape != flow.shape:
        raise L.RoitrError("reference_loc and reference_flow must have the same shape")
    if ref.shape[0] < 3:
        raise L.RoitrError(f"blend_anchor_motion: {ref.shape[0]} reference points for knn = 3")
    dev = q.device
    out = torch.empty_like(q)
    mask = torch.empty((q.shape[0],), dtype=i32, device=dev)
    status = torch.empty((1,), dtype=i32, device=dev)
    rs, qs = A.cumulative([ref.shape[0]], dev), A.cumulative([q.shape[0]], dev)
    L.check(L.lib().roitr_blend_anchor_motion(1, int(ref.shape[0]), rs.data_ptr(), ref.data_ptr(), flow.data_ptr(), int(q.shape[0]),
                                              qs.data_ptr(), q.data_ptr(), float(search_radius), 0, out.data_ptr(), mask.data_ptr(),
                                              status.data_ptr(), L.stream_ptr().value), "blend_anchor_motion")
    mask = mask.bool()
    return (out.cpu().numpy(), mask.cpu().numpy()) if as_numpy else (out, mask)


@torch.no_grad()
def nfmr_handle(handle, metric_index_list, **kw):
    """nfmr_batch on the correspondences of a RIGA_v2.launch_batch() handle, after finish_batch(handle): pair_starts / out_src_pts /
    out_tgt_pts, valid in the strided and the compacted patch layout alike (as Evaluator.evaluate_batch and register_handle read
    them); the clouds (src_raw_pcd, src_pcd) and the poses come from handle["pairs"].  metric_index_list: one index tensor per pair."""
    pairs, out, B = handle["pairs"], handle["out"], handle["B"]
    rot, trans = handle_poses(handle, "nfmr_handle")
    if len(metric_index_list) != B:
        raise L.RoitrError(f"nfmr_handle: {len(metric_index_list)} metric index lists for {B} pairs")
    dev = out["pair_starts"].device
    f32 = torch.float32
    raw = torch.cat([p["src_raw_pcd"].to(f32) for p in pairs], 0)
    deformed = torch.cat([p["src_pcd"].to(f32) for p in pairs], 0)
    index = torch.cat([torch.as_tensor(m).reshape(-1).to(device=dev, dtype=torch.int64) for m in metric_index_list], 0)
    rows = int(handle["starts"][-1]) if "starts" in handle else int(out["out_src_pts"].shape[0])   # the buffers are sized for the worst case
    return nfmr_batch(A.cumulative(handle["n_all"][:B], dev), raw, deformed, out["pair_starts"], out["out_src_pts"][:rows],
                      out["out_tgt_pts"][:rows], A.cumulative([int(torch.as_tensor(m).numel()) for m in metric_index_list], dev),
                      index, rot, trans, **kw)
