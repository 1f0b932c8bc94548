"""Times fast global registration (roitr_amd/fgr.py) against the correspondence RANSAC
(registration.ransac_batch, 50 000 iterations, n_points 1000) and the spatial-compatibility registration (compat.py) on the seeded sets
of scripts/bench_compat.py, in one process: 512 pairs x 1000 rows at 30 % and 5 % planted, 64 x 10 000 and 1 x 1000 at 30 %.

FGR runs without the tuple test (tuples 0) and, on the 5 % sets, also at the tuple count tests/fgr_util.py found on the CPU
(TUPLES_05 = 131 072); `fgr_unit` is FGR with scores None, since the objective weighs every row by its score and the sets' scores are
what they are.  Warm-up calls, then the estimators alternate; device events around every call; medians with min - max.  Per case and
estimator: ms per call, median RRE / RTE against the planted pose and the share of pairs within 15 deg / 0.3 m.

Two more tables on the 512 x 1000 set at 30 %, FGR alone: the call at iterations 1, 32 and 128 (what an iteration costs), and the rows
staged in LDS against swept from global memory (_lds_rows 0).

Expectations, written down here and not gated on, all unmeasured when they were written: FGR well below RANSAC per call at 512 x 1000
and 64 x 10 000; possibly above it for one pair, where 128 dependent iterations meet one block.

    python scripts/bench_fgr.py [--steps 20] [--warmup 3] [--only fgr] [--out profiles/fgr_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_fgr.py --steps 3 --only fgr --out DIR/bench.json
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

TUPLES_05 = 131072
CASES = (("512x1000", 512, 1000, None, 0.30), ("512x1000", 512, 1000, None, 0.05), ("64x10000", 64, 10000, 2048, 0.30),
         ("1x1000", 1, 1000, None, 0.30))


def timed(calls, steps, warmup):
    """{name: (ms list, last result)} of calls that alternate."""
    for _ in range(warmup):
        res = {k: f() for k, f in calls.items()}
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(steps):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res[k] = f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: (ms[k], res[k]) for k in calls}


def stats(ms):
    return dict(ms_per_call=round(float(np.median(ms)), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))


def time_case(name, pairs, n, max_rows, ratio, steps, warmup, only):
    import bench_compat
    from roitr_amd.compat import compat_batch
    from roitr_amd.fgr import fgr_batch
    from roitr_amd.registration import pose_errors, ransac_batch
    (starts, src, tgt, scores, _), rot, trans = bench_compat.sets(pairs, n, ratio, True)
    keys = list(range(pairs))
    calls = dict(fgr=lambda: fgr_batch(starts, src, tgt, scores),
                 fgr_unit=lambda: fgr_batch(starts, src, tgt, None),
                 ransac=lambda: ransac_batch(starts, src, tgt, scores, n_points=1000, iterations=50000),
                 compat=lambda: compat_batch(starts, src, tgt, scores, max_rows=max_rows))
    if ratio <= 0.05:
        calls["fgr_tuples"] = lambda: fgr_batch(starts, src, tgt, scores, pair_keys=keys, tuples=TUPLES_05)
        calls["fgr_unit_tuples"] = lambda: fgr_batch(starts, src, tgt, None, pair_keys=keys, tuples=TUPLES_05)
    calls = {k: v for k, v in calls.items() if only is None or k.startswith(only)}
    out = dict(case=name, pairs=pairs, rows_per_pair=n, max_rows=max_rows, inlier_share=ratio)
    for k, (ms, res) in timed(calls, steps, warmup).items():
        rre, rte = pose_errors(res["T"], rot, trans)
        out[k] = dict(stats(ms), median_rre_deg=float("%.4g" % rre.median()), median_rte_m=float("%.4g" % rte.median()),
                      share_rre15_rte03=round(float(((rre < 15) & (rte < 0.3)).double().mean()), 4))
        if k.startswith("fgr"):
            out[k].update(status_counts={str(int(v)): int(c) for v, c in zip(*torch.unique(res["status"], return_counts=True))},
                          steps_mean=round(float(res["steps"].double().mean()), 1),
                          tuples_accepted_mean=round(float(res["tuples_accepted"].double().mean()), 1),
                          n_used_mean=round(float(res["n_used"].double().mean()), 1))
    if "fgr" in out and "ransac" in out:
        out["ransac_over_fgr"] = round(out["ransac"]["ms_per_call"] / out["fgr"]["ms_per_call"], 2)
    if "fgr" in out and "compat" in out:
        out["compat_over_fgr"] = round(out["compat"]["ms_per_call"] / out["fgr"]["ms_per_call"], 2)
    return out


def fgr_alone(steps, warmup):
    """FGR on the 512 x 1000 set at 30 %: by iteration count, and LDS against global."""
    import bench_compat
    from roitr_amd.fgr import fgr_batch
    (starts, src, tgt, scores, _), _, _ = bench_compat.sets(512, 1000, 0.30, True)
    calls = {f"iterations_{k}": (lambda k=k: fgr_batch(starts, src, tgt, scores, iterations=k)) for k in (1, 32, 128)}
    calls["lds_128"] = lambda: fgr_batch(starts, src, tgt, scores)
    calls["global_128"] = lambda: fgr_batch(starts, src, tgt, scores, _lds_rows=0)
    r = timed(calls, steps, warmup)
    out = {k: stats(ms) for k, (ms, _) in r.items()}
    out["bitwise_equal_lds_global"] = bool(all(torch.equal(r["lds_128"][1][k], r["global_128"][1][k]) for k in r["lds_128"][1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("fgr", "ransac", "compat"), default=None, help="time one estimator alone (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fgr_bench.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    cases = []
    for name, pairs, n, max_rows, ratio in CASES:
        cases.append(time_case(name, pairs, n, max_rows, ratio, args.steps, args.warmup, args.only))
        print(json.dumps(cases[-1]), flush=True)
    alone = fgr_alone(args.steps, args.warmup) if args.only in (None, "fgr") else None
    print(json.dumps(alone), flush=True)
    result = dict(metric="fgr_vs_ransac_vs_compat_ms_per_call", device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
                  tuples_05=TUPLES_05, expectation="FGR below RANSAC per call at 512x1000 and 64x10000, possibly above at 1x1000 (not gated)",
                  cases=cases, fgr_512x1000=alone)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
