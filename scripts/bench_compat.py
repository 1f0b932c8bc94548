"""Times the spatial-compatibility registration (roitr_amd/compat.py) against the correspondence RANSAC
(registration.ransac_batch, 50 000 iterations, n_points 1000) and the local-to-global registration (lgr.py) on the same seeded sets,
in one process.

Sets: those of scripts/bench_lgr.py (256 patches per pair with ragged run lengths, Gaussian noise of 5 mm on the planted rows) with
30 %, 10 % and 5 % of the patches planted, at 512 pairs x 1000 rows, one pair x 1000 rows and 64 pairs x 10 000 rows (max_rows 2048
there: the 2048 best-scored rows of a pair enter the graph), each as generated and with the rows of every pair SHUFFLED -- the patch
labels travel with their rows, so LGR finds runs of one or two rows and has nothing to form a hypothesis from, which is the
situation of a descriptor-matched, loaded or subsampled set.  Warm-up calls, then the estimators alternate; device events around
every call; medians with min - max.  Per case and estimator: ms per call, median RRE / RTE against the planted pose and the share
of pairs within 15 deg / 0.3 m.

The expectation, written down here and not gated on: compat takes less time per call than RANSAC at all three shapes.

    python scripts/bench_compat.py [--steps 10] [--warmup 2] [--only compat] [--out profiles/compat_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_compat.py --steps 3 --only compat --out DIR/bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

RATIOS = (0.30, 0.10, 0.05)
SHAPES = (("512x1000", 512, 1000, None), ("1x1000", 1, 1000, None), ("64x10000", 64, 10000, 2048))


def sets(pairs, n, ratio, shuffled):
    """bench_lgr.patch_sets at another inlier share; shuffled: a permutation of its own for the rows of every pair."""
    import bench_lgr
    bench_lgr.INLIER_SHARE = ratio
    (starts, src, tgt, scores, patch), rot, trans = bench_lgr.patch_sets(pairs, n, seed=pairs * 7 + n + int(1000 * ratio))
    if shuffled:
        rng = np.random.default_rng(pairs + n)
        perm = torch.from_numpy(np.concatenate([b * n + rng.permutation(n) for b in range(pairs)])).to(src.device)
        src, tgt, scores, patch = src[perm].contiguous(), tgt[perm].contiguous(), scores[perm].contiguous(), patch[perm].contiguous()
    return (starts, src, tgt, scores, patch), rot, trans


def time_case(name, pairs, n, max_rows, ratio, shuffled, steps, warmup, only):
    from roitr_amd.compat import compat_batch
    from roitr_amd.lgr import lgr_batch
    from roitr_amd.registration import pose_errors, ransac_batch
    (starts, src, tgt, scores, patch), rot, trans = sets(pairs, n, ratio, shuffled)
    calls = dict(compat=lambda: compat_batch(starts, src, tgt, scores, max_rows=max_rows),
                 ransac=lambda: ransac_batch(starts, src, tgt, scores, n_points=1000, iterations=50000),
                 lgr=lambda: lgr_batch(starts, src, tgt, scores, patch))
    calls = {k: v for k, v in calls.items() if only in (None, k)}
    for _ in range(warmup):
        res = {k: f() for k, f in calls.items()}
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(steps):
        for k, f in calls.items():       # the estimators alternate
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res[k] = f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    out = dict(case=name, pairs=pairs, rows_per_pair=n, max_rows=max_rows, inlier_share=ratio, shuffled=shuffled)
    for k in calls:
        rre, rte = pose_errors(res[k]["T"], rot, trans)
        out[k] = dict(ms_per_call=round(float(np.median(ms[k])), 4), ms_min=round(min(ms[k]), 4), ms_max=round(max(ms[k]), 4),
                      median_rre_deg=float("%.4g" % rre.median()), median_rte_m=float("%.4g" % rte.median()),
                      share_rre15_rte03=round(float(((rre < 15) & (rte < 0.3)).double().mean()), 4))
    if "compat" in calls:
        r = res["compat"]
        out["compat"].update(hypotheses_per_pair=round(float(r["hypotheses"].double().mean()), 1),
                             winner_rank_max=int(r["best_rank"].max()), status_counts={
                                 str(int(v)): int(c) for v, c in zip(*torch.unique(r["status"], return_counts=True))})
    if "lgr" in calls:
        out["lgr"]["hypotheses_per_pair"] = round(float(res["lgr"]["hypotheses"].double().mean()), 1)
    if "compat" in calls and "ransac" in calls:
        out["ransac_over_compat"] = round(out["ransac"]["ms_per_call"] / out["compat"]["ms_per_call"], 2)
    if "compat" in calls and "lgr" in calls:
        out["compat_over_lgr"] = round(out["compat"]["ms_per_call"] / out["lgr"]["ms_per_call"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("compat", "ransac", "lgr"), default=None, help="time one estimator alone (kernel traces)")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES), help="comma-separated subset of the shapes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compat_bench.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    cases = []
    for name, pairs, n, max_rows in SHAPES:
        if name not in args.shapes.split(","):
            continue
        for ratio in RATIOS:
            for shuffled in (False, True):
                cases.append(time_case(name, pairs, n, max_rows, ratio, shuffled, args.steps, args.warmup, args.only))
                print(json.dumps(cases[-1]), flush=True)
    result = dict(metric="compat_vs_ransac_vs_lgr_ms_per_call", device=torch.cuda.get_device_name(0), steps=args.steps,
                  expectation="compat below RANSAC per call at all three shapes (not gated)", cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
