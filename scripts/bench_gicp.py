"""Times generalized ICP (roitr_amd/gicp.py) against the point-to-plane mode of icp.py, the comparator
the two share everything with but the update kernel.  One process, the two alternate.

The seeded scan-like pairs of scripts/bench_icp.py (a room corner with a sphere patch, noise, a share of outliers, a start
START_DEG degrees and START_SHIFT metres off the planted pose) at its shapes: 512 pairs x 5000 points, one pair x 5000, 64 pairs x
30 000.  The normals of both clouds are estimated on the device (prep.estimate_normals, knn = 33), as a pipeline on raw scans has them;
both operators read the same target normals.  Both at 30 iterations with the default tolerances (pairs stop when they converge) and
with tolerances 0 (every evaluation runs).  Device events around every call, WARMUP calls first, the median over the repeats with
min - max.  Per case: ms per call, ms per evaluation of the all-steps runs, RRE / RTE against the planted pose before and after.
Kernel times come from a trace of their own:
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_gicp.py --steps 3 --warmup 1 --out DIR/bench.json

    python scripts/bench_gicp.py [--steps 10] [--warmup 3] [--out profiles/gicp_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_icp import ITERATIONS, MAX_DIST, scan_pairs  # noqa: E402

EPSILON, KNN = 1e-3, 33


def time_case(name, pairs, n, steps, warmup):
    from roitr_amd.gicp import gicp_batch
    from roitr_amd.icp import icp_batch
    from roitr_amd.prep import estimate_normals
    from roitr_amd.registration import pose_errors
    src, tgt, _, off, T0, rot, trans = scan_pairs(pairs, n, seed=pairs * 11 + n)
    ns, nt = estimate_normals(src, off, knn=KNN), estimate_normals(tgt, off, knn=KNN)
    kw = dict(max_dist=MAX_DIST, iterations=ITERATIONS)
    every = dict(rel_fitness=0.0, rel_rmse=0.0)
    calls = dict(gicp=lambda: gicp_batch(src, off, tgt, off, T0, src_normals=ns, tgt_normals=nt, epsilon=EPSILON, **kw),
                 plane=lambda: icp_batch(src, off, tgt, off, T0, tgt_normals=nt, **kw),
                 gicp_all=lambda: gicp_batch(src, off, tgt, off, T0, src_normals=ns, tgt_normals=nt, epsilon=EPSILON, **every, **kw),
                 plane_all=lambda: icp_batch(src, off, tgt, off, T0, tgt_normals=nt, **every, **kw))
    for _ in range(warmup):
        res = {k: f() for k, f in calls.items()}
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(steps):
        for k, f in calls.items():       # the two operators alternate
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res[k] = f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    errs = lambda T: tuple(float("%.4g" % x.median()) for x in pose_errors(T, rot, trans))
    out = dict(case=name, pairs=pairs, points_per_cloud=n, max_dist=MAX_DIST, iterations=ITERATIONS, epsilon=EPSILON, normals_knn=KNN,
               start_median_rre_deg=errs(T0)[0], start_median_rte_m=errs(T0)[1])
    for k in calls:
        med = float(np.median(ms[k]))
        out[k] = dict(ms_per_call=round(med, 4), ms_min=round(min(ms[k]), 4), ms_max=round(max(ms[k]), 4),
                      median_rre_deg=errs(res[k]["T"])[0], median_rte_m=errs(res[k]["T"])[1])
        if k.endswith("_all"):
            out[k]["ms_per_evaluation"] = round(med / (ITERATIONS + 1), 4)
        else:
            st = res[k]["status"]
            out[k].update(mean_steps=round(float(res[k]["steps"].double().mean()), 2), converged=int(((st & 16) != 0).sum()),
                          mean_fitness=round(float(res[k]["fitness"].mean()), 4), mean_rmse=float("%.4g" % res[k]["rmse"].mean()))
    out["gicp_over_plane_per_evaluation"] = round(out["gicp_all"]["ms_per_evaluation"] / out["plane_all"]["ms_per_evaluation"], 3)
    out["gicp_over_plane_per_call"] = round(out["gicp"]["ms_per_call"] / out["plane"]["ms_per_call"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gicp_bench.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    cases = [time_case("512x5000", 512, 5000, args.steps, args.warmup),
             time_case("1x5000", 1, 5000, args.steps, args.warmup),
             time_case("64x30000", 64, 30000, args.steps, args.warmup)]
    result = dict(metric="gicp_ms_per_call", device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
