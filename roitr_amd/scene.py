"""Register a pair list over a set of clouds with every cloud encoded once.

The 3DMatch / 3DLoMatch protocol registers every overlapping pair of a scene's fragments (each fragment takes part in ~7 pairs), loop
closure matches one cloud against dozens: `match_pairs` runs the per-cloud half of the model once per cloud
(RIGA_v2.encode_clouds) and the pair half once per pair (RIGA_v2.launch_match), in calls of `pairs_per_call` with two calls in flight.

    python -m roitr_amd.scene --clouds 16 --points 5000            # all pairs i < j of 16 synthetic clouds, pairs/s

`register_scene` goes on from the pairs to one pose per cloud: lgr_handle on every match call,
posegraph.edge_information for the weight of each pose, posegraph.pose_graph_batch over the scene's graph.

    python -m roitr_amd.scene --multiway --clouds 6 --points 5000  # rigid copies of one cloud: per-edge RRE / RTE before and after
"""
import argparse
import collections
import time


def chunk_pairs(pairs, pairs_per_call):
    """The pair list cut into calls: consecutive slices of at most pairs_per_call pairs, in list order."""
    n = int(pairs_per_call)
    if n < 1:
        raise ValueError(f"pairs_per_call must be >= 1, got {pairs_per_call}")
    pairs = list(pairs)
    return [pairs[i:i + n] for i in range(0, len(pairs), n)]


def match_pairs(model, clouds, pairs, pairs_per_call=512, clouds_per_call=128):
    """Yield (pair, result) for every (src_index, tgt_index) of `pairs`, in list order.  `clouds`: the list of cloud dicts
    RIGA_v2.encode_clouds takes (encoded here, once) or an EncodedClouds made earlier.  Two match calls are kept in flight: call s + 1
    is queued before the host waits for call s, so the device does not idle while the results of s are unpacked."""
    calls = chunk_pairs(pairs, pairs_per_call)
    if not calls:
        return
    enc = clouds if hasattr(clouds, "table") else model.encode_clouds(clouds, clouds_per_call=clouds_per_call)
    flight = collections.deque()
    for call in calls:
        flight.append((call, model.launch_match(enc, call)))
        if len(flight) == 2:
            done, handle = flight.popleft()
            yield from zip(done, model.finish_batch(handle))
    while flight:
        done, handle = flight.popleft()
        yield from zip(done, model.finish_batch(handle))


def synthetic_scene(n_clouds, n_points, config=2):
    """Cloud dicts on the device: the sources and targets of synthetic.make_pair(n_points, config, pair_index = i, normals='field')."""
    import numpy as np
    import torch
    from .synthetic import make_pair
    clouds = []
    for i in range((n_clouds + 1) // 2):
        p = make_pair(n_points, config=config, pair_index=i, normals="field")
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        clouds.append(dict(points=dev(p["raw_src_pcd"]), points_out=dev(p["src_points"]), normals=dev(p["src_normals"]), feats=dev(p["src_feats"])))
        clouds.append(dict(points=dev(p["tgt_points"]), normals=dev(p["tgt_normals"]), feats=dev(p["tgt_feats"])))
    return clouds[:n_clouds]


def _match_calls(model, clouds, pairs, pairs_per_call, clouds_per_call):
    """Yield (call, handle) for every call of the pair list, finished, in list order: the pipeline of match_pairs (two calls in
    flight) for a caller that needs the call's device arrays, not the per-pair views."""
    calls = chunk_pairs(pairs, pairs_per_call)
    if not calls:
        return
    enc = clouds if hasattr(clouds, "table") else model.encode_clouds(clouds, clouds_per_call=clouds_per_call)
    flight = collections.deque()
    for call in calls:
        flight.append((call, model.launch_match(enc, call)))
        if len(flight) == 2:
            done, handle = flight.popleft()
            model.finish_batch(handle)
            yield done, handle
    while flight:
        done, handle = flight.popleft()
        model.finish_batch(handle)
        yield done, handle


def spanning_poses(n, pairs, transforms, inliers):
    """Initial poses (n,4,4) float64 on the host, cloud frame to the frame of cloud 0: a breadth-first tree from cloud 0 over the
    edges, a cloud's edges taken by descending inlier count (ties: list order).  Edge (i, j) with T mapping i into j: X_i = X_j T.  A
    cloud no edge reaches keeps the identity."""
    import numpy as np
    T = np.asarray(transforms, np.float64).reshape(-1, 4, 4)
    adj = [[] for _ in range(n)]
    for e, (i, j) in enumerate(pairs):
        adj[i].append((-int(inliers[e]), e, j, False))
        adj[j].append((-int(inliers[e]), e, i, True))
    X = np.tile(np.eye(4), (n, 1, 1))
    seen, queue = {0}, collections.deque([0])
    while queue:
        k = queue.popleft()
        for _, e, other, k_is_target in sorted(adj[k]):
            if other in seen:
                continue
            X[other] = X[k] @ T[e] if k_is_target else X[k] @ np.linalg.inv(T[e])
            seen.add(other)
            queue.append(other)
    return X


def uncertain_flags(pairs, certain):
    """edge_uncertain of the pair list, 0 / 1 per pair: 1 puts the edge under the line process.  certain: "consecutive" (the pairs of neighbouring fragments are odometry
    edges, as in the 3DMatch scenes), "all", "none", or one flag per pair (true: certain)."""
    if isinstance(certain, str):
        rule = {"consecutive": lambda i, j: abs(i - j) == 1, "all": lambda i, j: True, "none": lambda i, j: False}[certain]
        return [0 if rule(i, j) else 1 for i, j in pairs]
    flags = [0 if c else 1 for c in certain]
    if len(flags) != len(pairs):
        raise ValueError("certain must have one flag per pair")
    return flags


def register_scene(model, clouds, pairs, *, certain="consecutive", pairs_per_call=512, clouds_per_call=128, radius=0.1, min_rows=3,
                   steps=5, max_dist=0.05, preference=1.0, tau=1e-3, step_tol=1e-6, prune_threshold=0.25, iterations=100):
    """Multiway registration of a scene: every pair matched over the cached clouds (match_pairs'
    pipeline), one pose per pair by lgr_handle on each call, its information matrix by edge_information, then one pose per cloud in the
    frame of cloud 0 by pose_graph_batch, from the spanning tree of spanning_poses.  Pair (i, j) is the edge i -> j.  max_dist and
    preference set the line-process scale (posegraph.line_process_weight).

    Returns a dict of device tensors: poses (clouds,4,4); pair_T (pairs,4,4), inliers (pairs), info (pairs,6,6), uncertain (pairs),
    init_poses (clouds,4,4); line_weight, pruned (pairs); steps, solves, status, objective, lambda_out (1); and mu (float)."""
    import torch
    from . import posegraph as PG
    from .lgr import lgr_handle
    pairs = [(int(i), int(j)) for i, j in pairs]
    n = len(clouds)
    if n > PG.MAX_NODES:
        raise ValueError(f"register_scene: {n} clouds, a scene holds at most {PG.MAX_NODES}")
    if not pairs or any(i == j or not (0 <= i < n and 0 <= j < n) for i, j in pairs):
        raise ValueError("register_scene needs pairs (i, j) of two different clouds of the scene")
    Ts, counts, infos = [], [], []
    with torch.no_grad():
        for _, handle in _match_calls(model, clouds, pairs, pairs_per_call, clouds_per_call):
            out = handle["out"]
            r = lgr_handle(handle, radius=radius, min_rows=min_rows, steps=steps)
            e = PG.edge_information(out["pair_starts"], out["out_src_pts"], out["out_tgt_pts"], r["T"], radius=radius)
            Ts.append(r["T"]); counts.append(r["inliers"]); infos.append(e["info"])
        pair_T, inliers, info = torch.cat(Ts), torch.cat(counts), torch.cat(infos)
        dev = pair_T.device
        uncertain = torch.tensor(uncertain_flags(pairs, certain), dtype=torch.int32, device=dev)
        init = torch.from_numpy(spanning_poses(n, pairs, pair_T.cpu().numpy(), inliers.cpu().numpy())).to(torch.float32).to(dev)
        mu = float(PG.line_process_weight(info, uncertain, max_dist, preference))
        ei = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device=dev)
        ej = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device=dev)
        res = PG.pose_graph_batch([0, n], [0, len(pairs)], ei, ej, pair_T, info, uncertain, init, mu=mu, tau=tau, step_tol=step_tol,
                                  prune_threshold=prune_threshold, iterations=iterations)
    res.update(pair_T=pair_T, inliers=inliers, info=info, uncertain=uncertain, init_poses=init, mu=mu)
    return res


def rigid_copies(cloud, n_copies, seed=0, angle=0.6, shift=0.5):
    """(clouds, poses): n_copies rigid copies of one cloud dict as the fragments of a scene, and the planted poses (n,4,4) float64
    that map each copy's frame back into the frame of the first (which is the cloud itself)."""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    clouds, poses = [], []
    for k in range(n_copies):
        X = np.eye(4)
        if k:
            w = rng.normal(size=3)
            w *= angle / np.linalg.norm(w)
            K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / angle
            X[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
            X[:3, 3] = rng.normal(size=3) * shift
        R = torch.from_numpy(X[:3, :3]).to(cloud["points"])
        t = torch.from_numpy(X[:3, 3]).to(cloud["points"])
        clouds.append(dict(points=((cloud["points"] - t) @ R).contiguous(), normals=(cloud["normals"] @ R).contiguous(), feats=cloud["feats"]))
        poses.append(X)
    return clouds, np.stack(poses)


def pose_errors(T, T_true):
    """(RRE in degrees, RTE) of (k,4,4) float64 poses against the true ones."""
    import numpy as np
    R = np.einsum("kij,kil->kjl", T[:, :3, :3], T_true[:, :3, :3])
    rre = np.degrees(np.arccos(np.clip((np.trace(R, axis1=1, axis2=2) - 1) / 2, -1, 1)))
    return rre, np.linalg.norm(T[:, :3, 3] - T_true[:, :3, 3], axis=1)


def multiway_main(model, args):
    import numpy as np
    base = synthetic_scene(2, args.points)[1]
    clouds, planted = rigid_copies(base, args.clouds)
    pairs = [(i, j) for i in range(args.clouds) for j in range(i + 1, args.clouds)]
    res = register_scene(model, clouds, pairs, pairs_per_call=args.pairs_per_call)
    true = np.stack([np.linalg.inv(planted[j]) @ planted[i] for i, j in pairs])
    X = res["poses"].cpu().numpy().astype(np.float64)
    after = np.stack([np.linalg.inv(X[j]) @ X[i] for i, j in pairs])
    before = res["pair_T"].cpu().numpy().astype(np.float64)
    (r0, t0), (r1, t1) = pose_errors(before, true), pose_errors(after, true)
    lw, pr, inl = res["line_weight"].cpu().numpy(), res["pruned"].cpu().numpy(), res["inliers"].cpu().numpy()
    print(f"{args.clouds} fragments, {len(pairs)} edges: {int(res['steps'][0])} accepted steps in {int(res['solves'][0])} solves, "
          f"status {int(res['status'][0])}, mu {res['mu']:.4g}")
    print("edge    inliers  line weight  pruned   RRE before  RTE before   RRE after   RTE after")
    for e, (i, j) in enumerate(pairs):
        print(f"{i:3d}-{j:<3d} {inl[e]:7d}  {lw[e]:11.4f}  {pr[e]:6d}  {r0[e]:10.3f}  {t0[e]:10.4f}  {r1[e]:10.3f}  {t1[e]:10.4f}")


def main(argv=None):
    import torch
    from .harness import build_model
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clouds", type=int, default=16)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--pairs-per-call", type=int, default=512)
    ap.add_argument("--multiway", action="store_true", help="register rigid copies of one synthetic cloud as the fragments of a scene "
                    "(register_scene) and print every edge's RRE / RTE before and after the pose-graph optimisation")
    args = ap.parse_args(argv)
    model = build_model("3DMatch", weights="selective")
    if args.multiway:
        return multiway_main(model, args)
    clouds = synthetic_scene(args.clouds, args.points)
    pairs = [(i, j) for i in range(args.clouds) for j in range(i + 1, args.clouds)]
    with torch.no_grad():
        for _ in range(2):   # the first pass sizes the engine's scratch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n_corr = sum(int(res["corr_scores"].shape[0]) for _, res in match_pairs(model, clouds, pairs, args.pairs_per_call))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
    print(f"{len(pairs)} pairs over {args.clouds} clouds of {args.points} points: {len(pairs) / dt:.0f} pairs/s "
          f"(encode included), {n_corr} correspondences")


if __name__ == "__main__":
    main()
