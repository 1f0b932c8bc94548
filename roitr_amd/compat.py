"""Spatial-compatibility registration on the GPU: a pose from the compatibility graph of
the correspondences themselves, for sets without patch structure (descriptor matches, loaded or subsampled or shuffled sets).

Two correspondences are compatible when they preserve the distance between their points; a seed's consensus set is the k rows that
share the most compatible neighbours with it (the second-order compatibility of SC2-PCR, Chen et al., CVPR 2022; parity with that
method is not claimed, the operator is defined in include/roitr_engine.h above roitr_compat_batch).  A few dozen hypotheses instead
of RANSAC's 50 000, no random stream, no seed, no pair keys; verification and the reweighted refits are those of lgr.py.  Six
launches for a whole batch (csrc/compat.hip), no host round trip.
"""
import torch

from . import _args as A
from . import _lib as L

NO_ROWS, NO_HYPOTHESIS, EMPTY_REFIT, TRUNCATED = 1, 2, 4, 8   # status bits (ROITR_COMPAT_* of include/roitr_engine.h)
MAX_ROWS_DEFAULT = 2048


_lib = L.binder(("roitr_compat_workspace_bytes", "roitr_compat_batch"))   # the library with this module's two entry points bound from the header


@torch.no_grad()
def compat_batch(starts, src_pts, tgt_pts, scores, *, compat_dist=0.1, radius=0.1, max_rows=None, max_seeds=64, k=20, steps=5,
                 return_stages=False):
    """Spatial-compatibility registration of every pair: pair b owns rows [starts[b], starts[b+1]) of src_pts / tgt_pts / scores
    (scores None: all 1).  max_rows: rows per pair that enter the graph (the best-scored ones of a longer pair); None: min(2048,
    rows) and at least 3, from the tensor shape (starts is not read on the host).  The workspace holds the bit-packed graph, pairs x
    max_rows^2 / 8 bytes, and pairs x max_seeds x max_rows x 2 bytes of neighbour counts: with many short pairs, pass their length.

    Returns a dict of device tensors: T (B,4,4) fp32 and, (B) int32 each, inliers (under T), best_rank (-1: none), best_seed_row (the
    winning seed's row, local to the pair), seeds, hypotheses (valid ones), local_inliers (the winner's count) and status (bits
    NO_ROWS, NO_HYPOTHESIS, EMPTY_REFIT, TRUNCATED).  return_stages adds degree (rows; -1: not selected), seed_rows (B, max_seeds),
    seed_members (B, max_seeds, k), hyp_T (B, max_seeds, 3, 4) and hyp_counts (B, max_seeds), by rank, -1 / 0 padded."""
    dev, starts, B, src, tgt, rows, w = A.correspondences(starts, src_pts, tgt_pts, scores)
    if max_rows is None:
        max_rows = max(3, min(MAX_ROWS_DEFAULT, rows))
    max_rows, max_seeds, k = int(max_rows), int(max_seeds), int(k)
    ints = lambda *n: torch.empty(n, dtype=torch.int32, device=dev)
    out = dict(T=torch.empty((B, 4, 4), dtype=torch.float32, device=dev), inliers=ints(B), best_rank=ints(B), best_seed_row=ints(B),
               seeds=ints(B), hypotheses=ints(B), local_inliers=ints(B), status=ints(B))
    stages = [None] * 5
    if return_stages:
        S, K = max(max_seeds, 0), max(k, 0)
        out.update(degree=torch.full((rows,), -1, dtype=torch.int32, device=dev), seed_rows=ints(B, S), seed_members=ints(B, S, K),
                   hyp_T=torch.empty((B, S, 3, 4), dtype=torch.float32, device=dev), hyp_counts=ints(B, S))
        stages = [out[n].data_ptr() for n in ("degree", "seed_rows", "seed_members", "hyp_T", "hyp_counts")]
    lib = _lib()
    nbytes = int(lib.roitr_compat_workspace_bytes(B, rows, max_rows, max_seeds, k))
    ws = A.workspace(nbytes, dev)
    L.check(lib.roitr_compat_batch(B, starts.data_ptr(), rows, src.data_ptr(), tgt.data_ptr(), None if w is None else w.data_ptr(),
                                   float(compat_dist), float(radius), max_rows, max_seeds, k, int(steps), ws.data_ptr(), nbytes,
                                   out["T"].data_ptr(), out["inliers"].data_ptr(), out["best_rank"].data_ptr(),
                                   out["best_seed_row"].data_ptr(), out["seeds"].data_ptr(), out["hypotheses"].data_ptr(),
                                   out["local_inliers"].data_ptr(), out["status"].data_ptr(), *stages, L.stream_ptr().value),
            "compat_batch")
    return out


@torch.no_grad()
def compat_handle(handle, **kw):
    """compat_batch on the correspondences of a RIGA_v2.launch_batch() handle, after finish_batch(handle): pair_starts / out_src_pts /
    out_tgt_pts / out_scores, valid in the strided and the compacted patch layout alike (out_patch is not read)."""
    out = handle["out"]
    return compat_batch(out["pair_starts"], out["out_src_pts"], out["out_tgt_pts"], out["out_scores"], **kw)
