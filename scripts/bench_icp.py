"""Times the ICP refinement (roitr_amd/icp.py) against what can be written from the project's other
operators: a Python loop of pair_ground_truth (the matches) + a gather + weighted_procrustes (the project's Procrustes), point-to-point
only, the same number of evaluations, no convergence test (that would need a host read per step).  One process, the two alternate.

Seeded scan-like pairs: a room corner (three unit squares) with a sphere patch, source and target independent samples of it with
NOISE metres of Gaussian noise, a share OUTLIERS of the source displaced out of range, the start START_DEG degrees and START_SHIFT
metres off the planted pose.  Shapes a user would run: 512 pairs x 5000 points, one pair x 5000, 64 pairs x 30 000.  Both modes at 30
iterations with the default tolerances (pairs stop when they converge) and with tolerances 0 (every evaluation runs).  Device events
around every call, WARMUP calls first, the median over the repeats with min - max.  Per case: ms per call, ms per evaluation of the
all-steps run, RRE / RTE against the planted pose before and after, and the within-range (source point, target point) pairs of one
evaluation at the start (pair_ground_truth's counts: what a walk of the ball must at least look at) per second of the all-steps run.
Kernel times come from a trace of their own:
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_icp.py --steps 3 --only icp

    python scripts/bench_icp.py [--steps 20] [--warmup 3] [--out profiles/icp_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NOISE, OUTLIERS, START_DEG, START_SHIFT, MAX_DIST, ITERATIONS = 0.003, 0.1, 3.0, 0.04, 0.1, 30


def surface(rng, k):
    """k points on the three unit squares at x = 0, y = 0, z = 0 and on the octant of a sphere (centre 0.55, radius 0.3) that faces
    the corner, with unit normals."""
    which = rng.integers(0, 4, k)
    u, v = rng.uniform(0.0, 1.0, k), rng.uniform(0.0, 1.0, k)
    pts, nrm = np.zeros((k, 3)), np.zeros((k, 3))
    for a in range(3):
        sel = which == a
        pts[sel, (a + 1) % 3], pts[sel, (a + 2) % 3] = u[sel], v[sel]
        nrm[sel, a] = 1.0
    sel = which == 3
    d = -np.abs(rng.normal(size=(int(sel.sum()), 3)))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts[sel], nrm[sel] = 0.55 + 0.3 * d, d
    return pts, nrm


def rotations(rng, pairs, angle=None):
    """(pairs, 3, 3) rotations about random axes, by `angle` radians or a random angle."""
    w = rng.normal(size=(pairs, 3))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    th = (rng.uniform(0.2, 3.0, pairs) if angle is None else np.full(pairs, angle))[:, None, None]
    K = np.zeros((pairs, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def scan_pairs(pairs, n, seed):
    """Device tensors src (pairs n, 3), tgt, tgt normals, offsets, the start (pairs, 4, 4) and the planted rot / trans (numpy)."""
    rng = np.random.default_rng(seed)
    q, nq = surface(rng, pairs * n)
    p, _ = surface(rng, pairs * n)
    q = (q + NOISE * rng.normal(size=q.shape)).reshape(pairs, n, 3)
    p = (p + NOISE * rng.normal(size=p.shape)).reshape(pairs, n, 3)
    p[:, n - int(OUTLIERS * n):] += 3.0
    R, t = rotations(rng, pairs), rng.uniform(-0.5, 0.5, (pairs, 1, 3))
    src = (p - t) @ R                                     # rows R^T (p - t)
    dR = rotations(rng, pairs, np.deg2rad(START_DEG))
    dt = rng.normal(size=(pairs, 3))
    dt *= START_SHIFT / np.linalg.norm(dt, axis=1, keepdims=True)
    T0 = np.tile(np.eye(4), (pairs, 1, 1))
    T0[:, :3, :3], T0[:, :3, 3] = dR @ R, np.einsum("bij,bj->bi", dR, t[:, 0]) + dt
    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    off = torch.arange(n, (pairs + 1) * n, n, dtype=torch.int32, device=dev)
    return up(src.reshape(-1, 3)), up(q.reshape(-1, 3)), up(nq), off, up(T0), R, t[:, 0]


def loop_of_operators(src, off, tgt, T0, pairs, n, evaluations):
    """The comparator: `evaluations` times pair_ground_truth -> gather -> weighted_procrustes; returns (pairs, 4, 4)."""
    from roitr_amd.pairgt import pair_ground_truth
    from roitr_amd.registration import weighted_procrustes
    T = T0.clone()
    base = (off - n).long().repeat_interleave(n)
    for s in range(evaluations):
        gt = pair_ground_truth(src, off, tgt, off, T[:, :3, :3].contiguous(), T[:, :3, 3].contiguous(), MAX_DIST, both_sides=False)
        if s == evaluations - 1:
            break
        hit = gt.nn_idx >= 0
        matched = tgt[base + gt.nn_idx.clamp(min=0).long()]
        T = weighted_procrustes(src.reshape(pairs, n, 3), matched.reshape(pairs, n, 3), hit.reshape(pairs, n).float(), return_transform=True)
    return T


def time_case(name, pairs, n, steps, warmup, only):
    from roitr_amd.icp import icp_batch
    from roitr_amd.pairgt import pair_ground_truth
    from roitr_amd.registration import pose_errors
    src, tgt, nrm, off, T0, rot, trans = scan_pairs(pairs, n, seed=pairs * 11 + n)
    kw = dict(max_dist=MAX_DIST, iterations=ITERATIONS)
    calls = dict(point=lambda: icp_batch(src, off, tgt, off, T0, **kw),
                 plane=lambda: icp_batch(src, off, tgt, off, T0, tgt_normals=nrm, **kw),
                 point_all=lambda: icp_batch(src, off, tgt, off, T0, rel_fitness=0.0, rel_rmse=0.0, **kw),
                 plane_all=lambda: icp_batch(src, off, tgt, off, T0, tgt_normals=nrm, rel_fitness=0.0, rel_rmse=0.0, **kw),
                 loop=lambda: dict(T=loop_of_operators(src, off, tgt, T0, pairs, n, ITERATIONS + 1)))
    if only == "icp":
        del calls["loop"]
    for _ in range(warmup):
        res = {k: f() for k, f in calls.items()}
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(steps):
        for k, f in calls.items():       # the operator and the loop alternate
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res[k] = f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    ball = int(pair_ground_truth(src, off, tgt, off, T0[:, :3, :3].contiguous(), T0[:, :3, 3].contiguous(), MAX_DIST,
                                 both_sides=False).count.long().sum())
    errs = lambda T: tuple(float("%.4g" % x.median()) for x in pose_errors(T, rot, trans))
    out = dict(case=name, pairs=pairs, points_per_cloud=n, max_dist=MAX_DIST, iterations=ITERATIONS, start_median_rre_deg=errs(T0)[0],
               start_median_rte_m=errs(T0)[1], in_range_pairs_per_evaluation_at_start=ball)
    for k in calls:
        med = float(np.median(ms[k]))
        out[k] = dict(ms_per_call=round(med, 4), ms_min=round(min(ms[k]), 4), ms_max=round(max(ms[k]), 4),
                      median_rre_deg=errs(res[k]["T"])[0], median_rte_m=errs(res[k]["T"])[1])
        if k.endswith("_all") or k == "loop":
            out[k]["ms_per_evaluation"] = round(med / (ITERATIONS + 1), 4)
        if k.endswith("_all"):
            out[k]["in_range_pairs_per_s"] = float("%.4g" % (ball * (ITERATIONS + 1) / (med * 1e-3)))
        if k in ("point", "plane"):
            st = res[k]["status"]
            out[k].update(mean_steps=round(float(res[k]["steps"].double().mean()), 2), converged=int(((st & 16) != 0).sum()),
                          mean_fitness=round(float(res[k]["fitness"].mean()), 4), mean_rmse=float("%.4g" % res[k]["rmse"].mean()))
    if "loop" in calls:
        out["loop_over_point_all"] = round(out["loop"]["ms_per_call"] / out["point_all"]["ms_per_call"], 2)
        out["loop_over_point"] = round(out["loop"]["ms_per_call"] / out["point"]["ms_per_call"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("icp",), default=None, help="leave the comparator loop out (kernel traces)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "icp_bench.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    cases = [time_case("512x5000", 512, 5000, args.steps, args.warmup, args.only),
             time_case("1x5000", 1, 5000, args.steps, args.warmup, args.only),
             time_case("64x30000", 64, 30000, args.steps, args.warmup, args.only)]
    result = dict(metric="icp_ms_per_call", device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
