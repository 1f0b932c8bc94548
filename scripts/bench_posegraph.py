"""Times the pose-graph optimisation (roitr_amd/posegraph.py) against the float64 numpy
restatement of tests/posegraph_util.py on the host, in one process, on the seeded graphs of that file:

    8 scenes x 60 nodes x 400 edges, 1 scene x 60 nodes x 400 edges, 512 scenes x 12 nodes x 35 edges.

Both arms run a fixed number of solves (step_tol 0, so nothing stops early), from the chained start.  The device arm is one
pose_graph_batch call between device events; the host arm is posegraph_util.optimise with np.linalg.solve (LAPACK) as its solver, timed
with perf_counter on the first `--host-scenes` scenes of the case and scaled to the case's scene count (the host runs them one after
another).  The arms alternate; medians with min - max.

The share of the factorisation is measured from outside: the same scenes with every edge doubled (each copy with half the information,
so H, b and every step are the same numbers up to rounding) cost the same factorisation, back substitution and barriers but twice the
edge terms and the gather, so T(m) = a + b m gives the part that does not scale with the edges as a = 2 T(m) - T(2m).

No target is fixed: nobody had measured this kernel.  Its factorisation runs on one compute unit per scene, so a single large scene may
lose to LAPACK on the host; where it does, the JSON says so.

    python scripts/bench_posegraph.py [--steps 9] [--warmup 2] [--solves 8] [--out profiles/posegraph_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = (("8x60x400", 8, 60, 341), ("1x60x400", 1, 60, 341), ("512x12x35", 512, 12, 24))   # name, scenes, nodes, loop closures (+ n - 1 odometry edges)


def doubled(g):
    """The scene with every edge twice, each copy with half the information."""
    twice = lambda a: np.concatenate([a, a])
    return dict(g, edge_i=twice(g["edge_i"]), edge_j=twice(g["edge_j"]), edge_T=twice(g["edge_T"]), edge_info=twice(g["edge_info"]) / 2,
                edge_uncertain=twice(g["edge_uncertain"]))


def stats(ms):
    return dict(ms=round(float(np.median(ms)), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))


def device_call(graphs, solves):
    import posegraph_util as U
    from roitr_amd import posegraph as PG
    b = U.batch(graphs)
    dev = {k: torch.from_numpy(b[k]).cuda() for k in ("edge_i", "edge_j", "edge_T", "edge_info", "edge_uncertain", "init_poses")}
    return lambda: PG.pose_graph_batch(b["node_starts"], b["edge_starts"], dev["edge_i"], dev["edge_j"], dev["edge_T"], dev["edge_info"],
                                       dev["edge_uncertain"], dev["init_poses"], mu=graphs[0]["mu"], step_tol=0.0, iterations=solves)


def time_case(name, scenes, nodes, loops, args):
    import posegraph_util as U
    graphs = [U.make_graph(n=nodes, seed=1000 + s, loops=loops, wrong=0.15) for s in range(scenes)]
    host_graphs = graphs[:min(scenes, args.host_scenes)]
    arms = dict(device=device_call(graphs, args.solves), device_edges_doubled=device_call([doubled(g) for g in graphs], args.solves))
    host = lambda: [U.optimise(g, g["mu"], step_tol=0.0, iterations=args.solves, solver="numpy") for g in host_graphs]
    for _ in range(args.warmup):
        res = {k: f() for k, f in arms.items()}
    torch.cuda.synchronize()
    ms = {k: [] for k in list(arms) + ["host"]}
    for _ in range(args.steps):
        for k, f in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res[k] = f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
        t0 = time.perf_counter()
        ref = host()
        ms["host"].append(1e3 * (time.perf_counter() - t0) * scenes / len(host_graphs))
    out = dict(case=name, scenes=scenes, nodes=nodes, edges=nodes - 1 + loops, unknowns=6 * (nodes - 1), solves=args.solves,
               host_scenes_timed=len(host_graphs), **{k: stats(v) for k, v in ms.items()})
    # the two arms did the same work: accepted steps and pruned edges of the scenes the host ran
    steps, pruned = res["device"]["steps"].cpu().numpy(), res["device"]["pruned"].cpu().numpy()
    out["same_steps_as_host"] = bool(all(int(steps[s]) == r["steps"] for s, r in enumerate(ref)))
    e0 = 0
    same = True
    for g, r in zip(host_graphs, ref):
        same &= bool(np.array_equal(pruned[e0:e0 + len(g["edge_i"])], r["pruned"]))
        e0 += len(g["edge_i"])
    out["same_pruned_as_host"] = same
    t1, t2 = out["device"]["ms"], out["device_edges_doubled"]["ms"]
    out["edge_independent_ms"] = round(2 * t1 - t2, 4)
    out["edge_independent_share"] = round((2 * t1 - t2) / t1, 3)
    out["ms_per_solve"] = round(t1 / args.solves, 4)
    out["device_over_host"] = round(t1 / out["host"]["ms"], 3)
    out["slower_than_host"] = bool(t1 > out["host"]["ms"])
    print(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--solves", type=int, default=8)
    ap.add_argument("--host-scenes", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_bench.json"))
    args = ap.parse_args()
    from roitr_amd.build import source_hash
    result = dict(device=torch.cuda.get_device_name(0), source_hash=source_hash(), steps=args.steps, warmup=args.warmup,
                  cases=[time_case(*c, args) for c in CASES])
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
