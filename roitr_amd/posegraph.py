"""Multiway registration on the GPU: one pose per fragment of a scene in a common frame from
the scene's pairwise poses, with wrong loop closures switched off by a line process.

The pose-graph optimisation of Choi, Zhou and Koltun (CVPR 2015; Open3D's global_optimization with
GlobalOptimizationLevenbergMarquardt).  Parity with Open3D is not claimed; the operator is defined in include/roitr_engine.h above
roitr_edge_information.  `edge_information` weighs an edge by the correspondences that produced its pose (one launch for a batch of
pairs), `pose_graph_batch` optimises any number of ragged scenes in two launches whatever the iteration count (csrc/posegraph.hip):
one workgroup per scene runs the whole Levenberg-Marquardt loop, the dense system in the caller's workspace.
"""
import numpy as np
import torch

from . import _args as A
from . import _lib as L

ONE_NODE, NO_EDGES, BAD_EDGE, SINGULAR, CONVERGED, BAD_COUNTS = 1, 2, 4, 8, 16, 32   # status bits (ROITR_POSEGRAPH_*)
MAX_NODES = 256                                                                      # ROITR_POSEGRAPH_MAX_NODES

_lib = L.binder(("roitr_edge_information", "roitr_pose_graph_workspace_bytes", "roitr_pose_graph_batch"))


@torch.no_grad()
def edge_information(starts, src_pts, tgt_pts, transforms, *, radius=0.1):
    """The information matrix of every pair's pose: pair b owns rows [starts[b], starts[b+1]) of src_pts / tgt_pts, transforms (B,4,4)
    map source to target.  Returns dict(info (B,6,6) float64, rotation first; n_inlier (B) int32: the rows within `radius` under the
    transform, the count lgr_batch reports for its own pose)."""
    dev, starts, B, src, tgt, rows, _ = A.correspondences(starts, src_pts, tgt_pts, None)
    T = A.upload(transforms, device=dev).reshape(-1, 4, 4)
    if int(T.shape[0]) != B:
        raise ValueError(f"transforms: {int(T.shape[0])} poses for {B} pairs")
    out = dict(info=torch.empty((B, 6, 6), dtype=torch.float64, device=dev), n_inlier=torch.empty((B,), dtype=torch.int32, device=dev))
    L.check(_lib().roitr_edge_information(B, starts.data_ptr(), rows, src.data_ptr(), tgt.data_ptr(), T.data_ptr(), float(radius),
                                          out["info"].data_ptr(), out["n_inlier"].data_ptr(), L.stream_ptr().value), "edge_information")
    return out


def _host_starts(x):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(a.reshape(-1).astype(np.int32))


def workspace_bytes(node_starts, edge_starts):
    """roitr_pose_graph_workspace_bytes of host start arrays (scenes + 1 entries each); host-only, 0 for counts the call refuses."""
    ns, es = _host_starts(node_starts), _host_starts(edge_starts)
    if ns.shape != es.shape or ns.size < 2:
        return 0
    return int(_lib().roitr_pose_graph_workspace_bytes(int(ns.size) - 1, ns.ctypes.data, es.ctypes.data))


@torch.no_grad()
def pose_graph_batch(node_starts, edge_starts, edge_i, edge_j, edge_T, edge_info, edge_uncertain, init_poses, *, mu, tau=1e-3,
                     step_tol=1e-6, prune_threshold=0.25, iterations=100, return_trace=False):
    """Pose-graph optimisation of S ragged scenes.  node_starts / edge_starts (S + 1): HOST sequences (lists, arrays or host tensors;
    the limits are checked and the workspace is laid out from them); scene s owns the nodes [node_starts[s], node_starts[s+1]) of
    init_poses (nodes,4,4) and the edges [edge_starts[s], edge_starts[s+1]) of edge_i / edge_j (node indices local to the scene),
    edge_T (edges,4,4: cloud i into cloud j's frame), edge_info (edges,6,6 float64, rotation first) and edge_uncertain (0: odometry,
    1: a loop closure under the line process).  mu: the line-process scale (line_process_weight); tau: the start damping relative to
    the largest diagonal entry; step_tol: stop when max |delta| falls below it; prune_threshold: on the final line weight.

    Returns a dict of device tensors: poses (nodes,4,4) fp32 in the frame of each scene's node 0; line_weight (edges) float64; pruned
    (edges) int32; steps, solves, status (bits ONE_NODE, NO_EDGES, BAD_EDGE, SINGULAR, CONVERGED, BAD_COUNTS) (S) int32; objective and
    lambda_out (S) float64.  return_trace adds trace_scalars (S, iterations, 8), trace_poses (nodes, iterations, 12) and trace_delta
    (nodes, iterations, 6) float64 (include/roitr_engine.h)."""
    ns, es = _host_starts(node_starts), _host_starts(edge_starts)
    if ns.shape != es.shape or ns.size < 1:
        raise ValueError("node_starts and edge_starts must hold scenes + 1 entries each")
    S = int(ns.size) - 1
    init = init_poses if torch.is_tensor(init_poses) else torch.as_tensor(np.asarray(init_poses))
    dev = init.device if init.is_cuda else torch.device("cuda")
    init = A.upload(init, device=dev).reshape(-1, 4, 4)
    i32, f64 = torch.int32, torch.float64
    ei, ej = A.upload(edge_i, i32, dev).reshape(-1), A.upload(edge_j, i32, dev).reshape(-1)
    unc = A.upload(edge_uncertain, i32, dev).reshape(-1)
    Te = A.upload(edge_T, device=dev).reshape(-1, 4, 4)
    info = A.upload(edge_info, f64, dev).reshape(-1, 6, 6)
    nodes, edges = int(init.shape[0]), int(ei.shape[0])
    if S > 0 and (int(ns[-1]) != nodes or int(es[-1]) != edges):
        raise ValueError(f"the starts end at {int(ns[-1])} nodes / {int(es[-1])} edges, the arrays hold {nodes} / {edges}")
    if not (int(ej.shape[0]) == int(unc.shape[0]) == int(Te.shape[0]) == int(info.shape[0]) == edges):
        raise ValueError("edge_i, edge_j, edge_T, edge_info and edge_uncertain must have one entry per edge")
    iterations = int(iterations)
    ints = lambda n: torch.empty((n,), dtype=i32, device=dev)
    dbl = lambda *n: torch.empty(n, dtype=f64, device=dev)
    out = dict(poses=torch.empty((nodes, 4, 4), dtype=torch.float32, device=dev), line_weight=dbl(edges), pruned=ints(edges),
               steps=ints(S), solves=ints(S), objective=dbl(S), lambda_out=dbl(S), status=ints(S))
    if return_trace:
        k = max(iterations, 0)
        out.update(trace_scalars=dbl(S, k, 8), trace_poses=dbl(nodes, k, 12), trace_delta=dbl(nodes, k, 6))
    if S == 0:
        return out
    trace = [out[k].data_ptr() if k in out else None for k in ("trace_scalars", "trace_poses", "trace_delta")]
    lib = _lib()
    nbytes = int(lib.roitr_pose_graph_workspace_bytes(S, ns.ctypes.data, es.ctypes.data))
    ws = A.workspace(nbytes, dev)
    ns_d, es_d = torch.from_numpy(ns).to(dev), torch.from_numpy(es).to(dev)
    L.check(lib.roitr_pose_graph_batch(S, ns_d.data_ptr(), es_d.data_ptr(), ns.ctypes.data, es.ctypes.data, ei.data_ptr(), ej.data_ptr(),
                                       Te.data_ptr(), info.data_ptr(), unc.data_ptr(), init.data_ptr(), float(mu), float(tau),
                                       float(step_tol), float(prune_threshold), iterations, ws.data_ptr(), nbytes,
                                       out["poses"].data_ptr(), out["line_weight"].data_ptr(), out["pruned"].data_ptr(),
                                       out["steps"].data_ptr(), out["solves"].data_ptr(), out["objective"].data_ptr(),
                                       out["lambda_out"].data_ptr(), out["status"].data_ptr(), *trace, L.stream_ptr().value),
            "pose_graph_batch")
    return out


@torch.no_grad()
def line_process_weight(info, uncertain, max_dist, preference=1.0):
    """Open3D's rule for the line-process scale mu: preference * max_dist^2 * the mean of info[5][5] (the inlier count of
    edge_information) over the uncertain edges, as a 0-dim float64 device tensor; 0 edges uncertain: preference * max_dist^2 alone.
    It runs on the device: nothing is read back."""
    info = A.dev(info, torch.float64, "info").reshape(-1, 6, 6)
    unc = A.dev(uncertain, torch.int32, "uncertain").reshape(-1) != 0
    count = unc.sum()
    mean = torch.where(count > 0, (info[:, 5, 5] * unc).sum() / count.clamp(min=1), torch.ones((), dtype=torch.float64, device=info.device))
    return float(preference) * float(max_dist) ** 2 * mean


def info_from_redwood(info):
    """An information matrix in the pair_ground_truth layout (G = [I3 | -2 [p]x], translation first: the Redwood / 3DMatch gt.info
    files) as this module's (G = [-[p]x | I3], rotation first): the blocks swapped, the rotation block / 4, the mixed blocks / 2.
    Tensors and arrays alike, any leading dimensions."""
    t, r = slice(0, 3), slice(3, 6)
    out = info.clone() if torch.is_tensor(info) else np.array(info, dtype=np.float64)
    out[..., t, t] = info[..., r, r] / 4
    out[..., t, r] = info[..., r, t] / 2
    out[..., r, t] = info[..., t, r] / 2
    out[..., r, r] = info[..., t, t]
    return out
