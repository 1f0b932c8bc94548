"""Fast global registration on the GPU: a pose from one robust objective over all
correspondences of a pair, with no hypotheses at all.

The Geman-McClure cost of Fast Global Registration (Zhou, Park and Koltun, ECCV 2016; Open3D's FastGlobalRegistration) is minimised by
a few dozen 6 x 6 Gauss-Newton steps while its scale mu is lowered from the extent of the set to max_dist^2 (graduated
non-convexity).  Optionally the rows are first weighted by a tuple test: triples of the RANSAC stream whose three edges keep their
length add 1 to the multiplicity of their rows.  Parity with Open3D is not claimed; the operator is defined in
include/roitr_engine.h above roitr_fgr_batch.  Two launches for a whole batch whatever the iteration count (csrc/fgr.hip), no host
round trip; besides the pose it returns the final scale and objective, which can be compared across pairs.
"""
import torch

from . import _args as A
from . import _lib as L
from .registration import _keys

NO_ROWS, TOO_FEW, SINGULAR, NO_TUPLES = 1, 2, 4, 8   # status bits (ROITR_FGR_* of include/roitr_engine.h)
LDS_ROWS = 1536                                      # rows of a pair the solve kernel stages in LDS (csrc/fgr.hip FG_LDS_ROWS)


_lib = L.binder(("roitr_fgr_workspace_bytes", "roitr_fgr_batch", "roitr_fgr_batch_staged"))   # bound from the header on first use


@torch.no_grad()
def fgr_batch(starts, src_pts, tgt_pts, scores, *, pair_keys=None, seed=0, max_dist=0.1, division_factor=1.4, iterations=128,
              mu_every=4, tuples=0, tuple_scale=0.95, radius=0.1, return_trace=False, return_multiplicity=False, _lds_rows=None):
    """Fast global registration of every pair: pair b owns rows [starts[b], starts[b+1]) of src_pts / tgt_pts / scores (scores None:
    all 1).  max_dist: the final scale of the robust cost (metres); mu starts at the squared extent of the centred set and is divided
    by division_factor every mu_every iterations down to max_dist^2.  tuples: triples drawn per pair for the tuple test (0: none;
    then pair_keys, one uint32 per pair, and seed select the stream, as for RANSAC); tuple_scale: its edge-length ratio.  radius: only
    for the reported inlier count.

    Returns a dict of device tensors: T (B,4,4) fp32; inliers, n_used, tuples_accepted, steps and status (bits NO_ROWS, TOO_FEW,
    SINGULAR, NO_TUPLES), (B) int32 each; mu and objective (B) float64.  return_multiplicity adds multiplicity (rows) int32 (0 for
    rows outside every pair), return_trace adds trace (B, iterations, 16) float64: the centred state [R | t] before every step, mu,
    the objective, the sum of the weights and 1; rows that were not run are zero.  _lds_rows: the staging capacity, for the tests that
    hold the LDS path against the global one (the results do not depend on it)."""
    dev, starts, B, src, tgt, rows, w = A.correspondences(starts, src_pts, tgt_pts, scores)
    tuples, iterations = int(tuples), int(iterations)
    keys = _keys(pair_keys, B, dev) if tuples > 0 else None   # default: the batch positions, as for RANSAC
    ints = lambda n: torch.empty((n,), dtype=torch.int32, device=dev)
    f64 = lambda *n: torch.empty(n, dtype=torch.float64, device=dev)
    out = dict(T=torch.empty((B, 4, 4), dtype=torch.float32, device=dev), inliers=ints(B), n_used=ints(B), tuples_accepted=ints(B),
               steps=ints(B), mu=f64(B), objective=f64(B), status=ints(B))
    if return_multiplicity:
        out["multiplicity"] = torch.zeros((rows,), dtype=torch.int32, device=dev)
    if return_trace:
        out["trace"] = f64(B, max(iterations, 0), 16)
    opt = [out[k].data_ptr() if k in out else None for k in ("multiplicity", "trace")]
    lib = _lib()
    nbytes = int(lib.roitr_fgr_workspace_bytes(B, rows))
    ws = A.workspace(nbytes, dev)
    head = (B, starts.data_ptr(), rows, src.data_ptr(), tgt.data_ptr(), None if w is None else w.data_ptr(),
            None if keys is None else keys.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF, float(max_dist), float(division_factor), iterations,
            int(mu_every), tuples, float(tuple_scale), float(radius))
    tail = (ws.data_ptr(), nbytes, out["T"].data_ptr(), out["inliers"].data_ptr(), out["n_used"].data_ptr(),
            out["tuples_accepted"].data_ptr(), out["steps"].data_ptr(), out["mu"].data_ptr(), out["objective"].data_ptr(),
            out["status"].data_ptr(), *opt, L.stream_ptr().value)
    if _lds_rows is None:
        L.check(lib.roitr_fgr_batch(*head, *tail), "fgr_batch")
    else:
        L.check(lib.roitr_fgr_batch_staged(*head, int(_lds_rows), *tail), "fgr_batch")
    return out


@torch.no_grad()
def fgr_handle(handle, pair_keys=None, **kw):
    """fgr_batch on the correspondences of a RIGA_v2.launch_batch() handle, after finish_batch(handle): pair_starts / out_src_pts /
    out_tgt_pts / out_scores, valid in the strided and the compacted patch layout alike (out_patch is not read).  pair_keys: the keys
    of the tuple test's stream (the global pair ids), read only with tuples > 0."""
    out = handle["out"]
    return fgr_batch(out["pair_starts"], out["out_src_pts"], out["out_tgt_pts"], out["out_scores"], pair_keys=pair_keys, **kw)
