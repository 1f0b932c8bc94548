"""Generalized ICP on the GPU (csrc/gicp.hip): plane-to-plane refinement from normals.

Open3D's registration_generalized_icp restated with the covariance of every point fixed by its unit normal, C = I - (1 - epsilon) n n^T
(include/roitr_pointops.h states the rules above roitr_gicp_batch; parity with the original is unpinned).  Evaluation, loop and
convergence rule are icp.icp_batch's -- the exact float64 nearest-neighbour match, fitness / rmse, the relative test on them -- and
the update is one Gauss-Newton step on sum d^T (C_t + R C_s R^T)^-1 d.  The whole loop of a batch runs on the device: two launches per
evaluation, no host read, the state rounded to fp32 between steps.  Robust kernels, point weights, colored ICP, a multi-scale
schedule, caller-supplied covariances and Open3D's convergence test on the whitened RMSE are out of scope.  No CPU fallback.
"""
import numpy as np
import torch

from . import _args as A
from . import _lib as L
from .icp import CONVERGED, EMPTY, NONFINITE, SINGULAR, TOO_FEW, _prepare  # noqa: F401  (the status bits are the ICP operator's)

_lib = L.binder(("roitr_gicp_workspace_bytes", "roitr_gicp_batch"))   # the library with this module's two entry points bound from the header


@torch.no_grad()
def gicp_batch(src, src_offset, tgt, tgt_offset, init_T, *, src_normals, tgt_normals, epsilon=1e-3, max_dist=0.05, iterations=30,
               rel_fitness=1e-6, rel_rmse=1e-6, return_matches=False, return_trace=False):
    """src (n,3) / tgt (m,3) fp32 device tensors of B concatenated clouds with cumulative offsets (B) under pairgt's precondition (host
    offsets are checked, device offsets trusted), init_T (B,4,4) source to target, src_normals (n,3) / tgt_normals (m,3): both
    required, any length (they are normalised in float64; a zero normal makes its point isotropic), epsilon in [1e-6, 1].

    Returns icp_batch's dict of device tensors (T, fitness, rmse, n_corr, steps, status) plus objective (B) float64, the mean of
    d^T W d over the matches of the last evaluated state.  return_matches adds nn_idx (n) int32; return_trace adds trace_T
    (iterations + 1, B, 3, 4) and trace_stat (iterations + 1, B, 3): fitness, rmse and objective of every evaluation."""
    if src_normals is None or tgt_normals is None:
        raise L.RoitrError("gicp: src_normals and tgt_normals are both required")
    B, n, m, src, so, tgt, to, T0, (ns, nt), iterations, out, opt = _prepare(
        "gicp", src, src_offset, tgt, tgt_offset, init_T, (src_normals, tgt_normals),
        "gicp: the normals must have one row per point of their cloud", iterations, return_matches, return_trace, nstat=3,
        extra=("objective",))
    # an empty tensor has a null data pointer: the entry point wants the normals' pointers non-null even when a side has no points
    ptr = lambda t: t.data_ptr() if t.numel() else torch.empty((1, 3), dtype=torch.float32, device=src.device).data_ptr()
    lib = _lib()
    ws = A.workspace(lib.roitr_gicp_workspace_bytes(B, n, m, max(iterations, 0)), src.device)
    L.check(lib.roitr_gicp_batch(B, n, m, src.data_ptr(), so.data_ptr(), tgt.data_ptr(), to.data_ptr(), ptr(ns), ptr(nt), T0.data_ptr(),
                                 float(max_dist), float(epsilon), iterations, float(rel_fitness), float(rel_rmse), out["T"].data_ptr(),
                                 out["fitness"].data_ptr(), out["rmse"].data_ptr(), out["objective"].data_ptr(),
                                 out["n_corr"].data_ptr(), out["steps"].data_ptr(), out["status"].data_ptr(), opt("nn_idx"),
                                 opt("trace_T"), opt("trace_stat"), ws.data_ptr(), L.stream_ptr().value), "gicp_batch")
    return out


@torch.no_grad()
def gicp_handle(handle, init_T, **kw):
    """gicp_batch on the clouds of a RIGA_v2.launch_batch() handle (after finish_batch), from init_T (B,4,4), e.g. the "T" of
    register_handle or lgr_handle, on the normals the model was fed: the source rows of handle_normals first, the target rows after."""
    from .pairgt import handle_clouds
    from .riga import handle_normals
    src, so, tgt, to, _, _ = handle_clouds(handle)
    nrm = handle_normals(handle)
    n = int(src.shape[0])
    return gicp_batch(src, so, tgt, to, init_T, src_normals=nrm[:n], tgt_normals=nrm[n:], **kw)


def registration_generalized_icp(source, target, max_correspondence_distance, init=None, *, source_normals=None, target_normals=None,
                                 epsilon=1e-3, iterations=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """One pair in the argument order of Open3D's registration_generalized_icp: source / target (N,3) arrays or tensors, init the 4x4
    initial transform (identity by default).  A cloud given without normals gets them from prep.estimate_normals(knn=20,
    view_point=None), Open3D's fallback (the sign of a normal does not matter to n n^T).  Returns (T (4,4) tensor, fitness,
    inlier_rmse, correspondence_set (k,2) int64 of (source index, target index))."""
    src, tgt = A.upload(source).reshape(-1, 3), A.upload(target).reshape(-1, 3)

    def normals_of(cloud, given):
        if given is not None:
            return A.upload(given).reshape(-1, 3)
        from .prep import estimate_normals
        return estimate_normals(cloud, torch.tensor([int(cloud.shape[0])], dtype=torch.int32, device=cloud.device), knn=20, view_point=None)
    T0 = np.eye(4) if init is None else np.asarray(init.detach().cpu() if torch.is_tensor(init) else init, dtype=np.float64).reshape(4, 4)
    r = gicp_batch(src, [int(src.shape[0])], tgt, [int(tgt.shape[0])], A.upload(T0.astype(np.float32)).reshape(1, 4, 4),
                   src_normals=normals_of(src, source_normals), tgt_normals=normals_of(tgt, target_normals), epsilon=epsilon,
                   max_dist=max_correspondence_distance, iterations=iterations, rel_fitness=relative_fitness, rel_rmse=relative_rmse,
                   return_matches=True)
    nn = r["nn_idx"].long()
    i = torch.nonzero(nn >= 0).reshape(-1)
    return r["T"][0], float(r["fitness"][0]), float(r["rmse"][0]), torch.stack([i, nn[i]], 1)
