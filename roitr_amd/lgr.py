"""RANSAC-free registration on the GPU: GeoTransformer's local-to-global registration (LGR).

One pose hypothesis per patch of the coarse-to-fine matcher (a patch's correspondences are a contiguous run of rows), verification
of every hypothesis over all correspondences of the pair, then iterative reweighted Procrustes refits from the winner.  Three
launches for a whole batch (csrc/lgr.hip; the rules are stated in include/roitr_engine.h above roitr_lgr_batch), no random stream,
no seed, no pair keys: a pair's pose depends on its own rows only.  The solver is the reference's weighted_procrustes
(lib/utils.py:159-212), which the reference itself never calls.
"""
import torch

from . import _args as A
from . import _lib as L

NO_ROWS, NO_LOCAL, EMPTY_REFIT = 1, 2, 4   # status bits (ROITR_LGR_* of include/roitr_engine.h)


_lib = L.binder(("roitr_lgr_workspace_bytes", "roitr_lgr_batch"))   # the library with this module's two entry points bound from the header


@torch.no_grad()
def lgr_batch(starts, src_pts, tgt_pts, scores, row_patch, *, radius=0.1, min_rows=3, steps=5, return_hypotheses=False):
    """LGR over the correspondences of every pair: pair b owns rows [starts[b], starts[b+1]) of src_pts / tgt_pts / scores /
    row_patch (scores None: all 1; row_patch: equal for the rows of one patch, only equality of neighbours is read).

    Returns a dict of device tensors: T (B,4,4) fp32 and, (B) int32 each, inliers (under T), best_hypothesis (-1: none),
    best_first_row (local first row of the winning patch), hypotheses (patches with at least min_rows rows), local_inliers (the
    winner's count) and status (bits NO_ROWS, NO_LOCAL, EMPTY_REFIT).  return_hypotheses adds hyp_starts (B+1), hyp_first_row,
    hyp_T (.,3,4) and hyp_counts: pair b's hypotheses are entries [hyp_starts[b], hyp_starts[b] + hypotheses[b])."""
    dev, starts, B, src, tgt, rows, w = A.correspondences(starts, src_pts, tgt_pts, scores, per_row="scores and row_patch")
    patch = A.upload(row_patch, dtype=torch.int32, device=dev).reshape(-1)
    if int(patch.shape[0]) != rows:
        raise ValueError("scores and row_patch must have one entry per row")
    ints = lambda n: torch.empty((n,), dtype=torch.int32, device=dev)
    out = dict(T=torch.empty((B, 4, 4), dtype=torch.float32, device=dev), inliers=ints(B), best_hypothesis=ints(B),
               best_first_row=ints(B), hypotheses=ints(B), local_inliers=ints(B), status=ints(B))
    hyp = [None] * 4
    if return_hypotheses:
        cap = rows // max(int(min_rows), 1)
        out.update(hyp_starts=ints(B + 1), hyp_first_row=ints(cap), hyp_T=torch.empty((cap, 3, 4), dtype=torch.float32, device=dev),
                   hyp_counts=ints(cap))
        hyp = [out[k].data_ptr() for k in ("hyp_starts", "hyp_first_row", "hyp_T", "hyp_counts")]
    lib = _lib()
    nbytes = int(lib.roitr_lgr_workspace_bytes(B, rows))
    ws = A.workspace(nbytes, dev)
    L.check(lib.roitr_lgr_batch(B, starts.data_ptr(), rows, src.data_ptr(), tgt.data_ptr(), None if w is None else w.data_ptr(),
                                patch.data_ptr(), float(radius), int(min_rows), int(steps), ws.data_ptr(), nbytes,
                                out["T"].data_ptr(), out["inliers"].data_ptr(), out["best_hypothesis"].data_ptr(),
                                out["best_first_row"].data_ptr(), out["hypotheses"].data_ptr(), out["local_inliers"].data_ptr(),
                                out["status"].data_ptr(), *hyp, L.stream_ptr().value), "lgr_batch")
    return out


@torch.no_grad()
def lgr_handle(handle, **kw):
    """lgr_batch on the correspondences of a RIGA_v2.launch_batch() handle, after finish_batch(handle): pair_starts / out_src_pts /
    out_tgt_pts / out_scores / out_patch, valid in the strided and the compacted patch layout alike."""
    out = handle["out"]
    return lgr_batch(out["pair_starts"], out["out_src_pts"], out["out_tgt_pts"], out["out_scores"], out["out_patch"], **kw)


@torch.no_grad()
def local_global_registration(ref_knn_points, src_knn_points, score_mat, corr_mat, *, radius=0.1, min_rows=3, steps=5):
    """GeoTransformer's LocalGlobalRegistration.forward for one pair, in its argument order: ref_knn_points (P,K,3), src_knn_points
    (P,K,3), score_mat (P,K,K), corr_mat (P,K,K) bool.  The nonzero entries of corr_mat in (patch, ref, src) order are the
    correspondences, patch by patch.  Returns (ref_corr_points, src_corr_points, corr_scores, estimated_transform): the transform
    maps the source onto the reference."""
    ref_knn_points, src_knn_points = A.upload(ref_knn_points), A.upload(src_knn_points)
    score_mat = A.upload(score_mat)
    b, i, j = torch.nonzero(A.upload(corr_mat, dtype=torch.bool), as_tuple=True)
    ref_pts, src_pts, w = ref_knn_points[b, i].contiguous(), src_knn_points[b, j].contiguous(), score_mat[b, i, j].contiguous()
    r = lgr_batch(A.cumulative([int(b.shape[0])], ref_pts.device), src_pts, ref_pts, w, b.to(torch.int32), radius=radius,
                  min_rows=min_rows, steps=steps)
    return ref_pts, src_pts, w, r["T"][0]
