"""ICP pose refinement on the GPU (csrc/icp.hip): point-to-point and point-to-plane.

The pose estimators (registration.py, lgr.py) stop at the matcher's correspondences; this operator refines their pose on the dense
clouds.  Open3D's registration_icp restated (include/roitr_pointops.h states the rules above roitr_icp_batch; parity with the
original is unpinned): per pair, nearest target point within max_dist of every moved source point (an exact float64 decision),
fitness / rmse, the relative convergence test, then a rigid solve (point-to-point) or a Gauss-Newton step on the point-to-plane
residuals.  The whole loop of a batch runs on the device: two launches per evaluation, no host read, the state rounded to fp32
between steps.  Robust kernels, point weights, colored ICP and a multi-scale schedule are out of scope (generalized ICP: gicp.py).
No CPU fallback.
"""
import numpy as np
import torch

from . import _args as A
from . import _lib as L
from .pairgt import _check_offsets

NONFINITE, EMPTY, TOO_FEW, SINGULAR, CONVERGED = 1, 2, 4, 8, 16   # status bits (ROITR_ICP_* of include/roitr_pointops.h)

_lib = L.binder(("roitr_icp_workspace_bytes", "roitr_icp_batch"))   # the library with this module's two entry points bound from the header


def _prepare(who, src, src_offset, tgt, tgt_offset, init_T, normals, normals_error, iterations, return_matches, return_trace, nstat=2,
             extra=()):
    """Argument preparation and output allocation of icp_batch and gicp.gicp_batch; `who` begins the error texts.  normals:
    (src_normals, tgt_normals), None for a side the call does not read; a side with another row count than its cloud raises
    normals_error.  nstat: the columns of trace_stat; extra: names of further (B,) float64 outputs, placed behind rmse.  Returns
    (B, n, m, src, src_offset, tgt, tgt_offset, init_T, normals, iterations, out, opt): device tensors, the output dict and
    opt(name), an optional output's pointer or None."""
    src, tgt = A.points(src, f"{who}: src"), A.points(tgt, f"{who}: tgt")
    dev = src.device
    tgt = tgt.to(dev)
    n, m = int(src.shape[0]), int(tgt.shape[0])
    _check_offsets("src_offset", src_offset, n)
    _check_offsets("tgt_offset", tgt_offset, m)
    so = torch.as_tensor(src_offset).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    to = torch.as_tensor(tgt_offset).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    B = int(so.shape[0])
    if int(to.shape[0]) != B:
        raise L.RoitrError(f"{who}: src_offset and tgt_offset must have one entry per pair")
    T0 = A.dev(init_T, torch.float32, f"{who}: init_T").to(dev).reshape(-1, 4, 4)
    if int(T0.shape[0]) != B:
        raise L.RoitrError(f"{who}: {B} pairs need init_T (B,4,4)")
    normals = [None if t is None else A.points(t, f"{who}: {side}_normals").to(dev) for t, side in zip(normals, ("src", "tgt"))]
    if any(t is not None and int(t.shape[0]) != count for t, count in zip(normals, (n, m))):
        raise L.RoitrError(normals_error)
    iterations = int(iterations)
    rows = max(iterations, 0) + 1
    f64 = lambda: torch.empty((B,), dtype=torch.float64, device=dev)
    i32 = lambda: torch.empty((B,), dtype=torch.int32, device=dev)
    out = dict(T=torch.empty((B, 4, 4), dtype=torch.float32, device=dev), fitness=f64(), rmse=f64(), **{k: f64() for k in extra},
               n_corr=i32(), steps=i32(), status=i32())
    if return_matches:
        out["nn_idx"] = torch.empty((n,), dtype=torch.int32, device=dev)
    if return_trace:
        out["trace_T"] = torch.empty((rows, B, 3, 4), dtype=torch.float32, device=dev)
        out["trace_stat"] = torch.empty((rows, B, nstat), dtype=torch.float64, device=dev)
    return B, n, m, src, so, tgt, to, T0, normals, iterations, out, lambda k: out[k].data_ptr() if k in out else None


@torch.no_grad()
def icp_batch(src, src_offset, tgt, tgt_offset, init_T, *, tgt_normals=None, max_dist=0.05, iterations=30, rel_fitness=1e-6,
              rel_rmse=1e-6, return_matches=False, return_trace=False):
    """src (n,3) / tgt (m,3) fp32 device tensors of B concatenated clouds with cumulative offsets (B) under pairgt's precondition (host
    offsets are checked, device offsets trusted), init_T (B,4,4) source to target.  tgt_normals (m,3): point-to-plane, None:
    point-to-point.

    Returns a dict of device tensors: T (B,4,4) fp32, fitness (B) / rmse (B) float64 of the last evaluated state, n_corr (B), steps (B)
    int32 (the evaluation at which the pair stopped), status (B) int32 (bits NONFINITE, EMPTY, TOO_FEW, SINGULAR, CONVERGED; a
    NONFINITE or EMPTY pair returns init_T and nan).  return_matches adds nn_idx (n) int32, the pair-local match of every source point
    under the final state (-1: none); return_trace adds trace_T (iterations + 1, B, 3, 4) and trace_stat (iterations + 1, B, 2):
    state, fitness and rmse of every evaluation (rows after a pair's stop repeat its last one)."""
    B, n, m, src, so, tgt, to, T0, (_, nrm), iterations, out, opt = _prepare(
        "icp", src, src_offset, tgt, tgt_offset, init_T, (None, tgt_normals), "icp: tgt_normals must have one row per target point",
        iterations, return_matches, return_trace)
    lib = _lib()
    ws = A.workspace(lib.roitr_icp_workspace_bytes(B, n, m, max(iterations, 0)), src.device)
    L.check(lib.roitr_icp_batch(B, n, m, src.data_ptr(), so.data_ptr(), tgt.data_ptr(), to.data_ptr(),
                                None if nrm is None else nrm.data_ptr(), T0.data_ptr(), float(max_dist), iterations, float(rel_fitness),
                                float(rel_rmse), out["T"].data_ptr(), out["fitness"].data_ptr(), out["rmse"].data_ptr(),
                                out["n_corr"].data_ptr(), out["steps"].data_ptr(), out["status"].data_ptr(), opt("nn_idx"), opt("trace_T"),
                                opt("trace_stat"), ws.data_ptr(), L.stream_ptr().value), "icp_batch")
    return out


@torch.no_grad()
def icp_handle(handle, init_T, *, plane=False, **kw):
    """icp_batch on the clouds of a RIGA_v2.launch_batch() handle (after finish_batch), from init_T (B,4,4), e.g. the "T" of
    register_handle or lgr_handle.  plane: point-to-plane on the normals the model was fed for the target clouds."""
    from .pairgt import handle_clouds
    from .riga import handle_normals
    src, so, tgt, to, _, _ = handle_clouds(handle)
    if plane:
        kw["tgt_normals"] = handle_normals(handle)[int(src.shape[0]):]
    return icp_batch(src, so, tgt, to, init_T, **kw)


def registration_icp(source, target, max_correspondence_distance, init=None, *, target_normals=None, iterations=30,
                     relative_fitness=1e-6, relative_rmse=1e-6):
    """One pair in the argument order of Open3D's registration_icp: source / target (N,3) arrays or tensors, init the 4x4 initial
    transform (identity by default), target_normals (M,3) for point-to-plane.  Returns (T (4,4) tensor, fitness, inlier_rmse,
    correspondence_set (k,2) int64 of (source index, target index))."""
    src, tgt = A.upload(source).reshape(-1, 3), A.upload(target).reshape(-1, 3)
    T0 = np.eye(4) if init is None else np.asarray(init.detach().cpu() if torch.is_tensor(init) else init, dtype=np.float64).reshape(4, 4)
    r = icp_batch(src, [int(src.shape[0])], tgt, [int(tgt.shape[0])], A.upload(T0.astype(np.float32)).reshape(1, 4, 4),
                  tgt_normals=None if target_normals is None else A.upload(target_normals).reshape(-1, 3),
                  max_dist=max_correspondence_distance, iterations=iterations, rel_fitness=relative_fitness, rel_rmse=relative_rmse,
                  return_matches=True)
    nn = r["nn_idx"].long()
    i = torch.nonzero(nn >= 0).reshape(-1)
    return r["T"][0], float(r["fitness"][0]), float(r["rmse"][0]), torch.stack([i, nn[i]], 1)
