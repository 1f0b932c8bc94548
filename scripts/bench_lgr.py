"""Times the RANSAC-free registration (roitr_amd/lgr.py) against the correspondence RANSAC
(registration.ransac_batch, 50 000 iterations, n_points 1000) on the same seeded sets, in one process.

Sets with patch structure: 256 patches per pair with ragged run lengths (a multinomial split of the pair's rows, so some patches
have fewer than 3 rows and form no hypothesis), INLIER_SHARE of the patches follow the planted pose with Gaussian noise of SIGMA
on the target, the rows of the others are displaced by 0.3 .. 1.5 m in directions of their own.  Shapes as in
scripts/bench_registration.py: 512 pairs x 1000 rows, one pair x 1000 rows, 64 pairs x 10 000 rows.  Warm-up calls, then the two
estimators alternate; device events around every call, the median over the repeats is reported.  Per case: ms per call of both,
median RRE / RTE of both against the planted pose, and the (hypothesis x row) tests one LGR call makes (the verification kernel's
rate is that count over its time in a kernel trace, taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_lgr.py --steps 3 --only lgr).

    python scripts/bench_lgr.py [--steps 20] [--warmup 3] [--out profiles/lgr_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PATCHES, INLIER_SHARE, SIGMA = 256, 0.4, 0.005


def patch_sets(pairs, n, seed):
    """starts, src, tgt, scores, row_patch on the device and the planted rot (pairs,3,3) / trans (pairs,3)."""
    rng = np.random.default_rng(seed)
    S, G, P, rot, trans = [], [], [], [], []
    for _ in range(pairs):
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        t = rng.uniform(-1, 1, 3)
        lengths = rng.multinomial(n, np.ones(PATCHES) / PATCHES)
        patch = np.repeat(np.arange(PATCHES), lengths)
        good = (rng.uniform(size=PATCHES) < INLIER_SHARE)[patch]
        s = rng.uniform(-1.5, 1.5, (PATCHES, 3))[patch] + 0.15 * rng.normal(size=(n, 3))
        u = rng.normal(size=(n, 3))
        u *= rng.uniform(0.3, 1.5, (n, 1)) / np.linalg.norm(u, axis=1, keepdims=True)
        g = s @ R.T + t + np.where(good[:, None], SIGMA * rng.normal(size=(n, 3)), u)
        S.append(s); G.append(g); P.append(patch); rot.append(R); trans.append(t)
    dev = torch.device("cuda")
    up = lambda a, dt: torch.from_numpy(np.concatenate(a).astype(dt)).to(dev)
    starts = torch.arange(0, (pairs + 1) * n, n, dtype=torch.int32, device=dev)
    scores = torch.from_numpy(rng.uniform(0.05, 1, pairs * n).astype(np.float32)).to(dev)
    return (starts, up(S, np.float32), up(G, np.float32), scores, up(P, np.int32)), np.stack(rot), np.stack(trans)


def time_case(name, pairs, n, steps, warmup, only):
    from roitr_amd.lgr import lgr_batch
    from roitr_amd.registration import pose_errors, ransac_batch
    (starts, src, tgt, scores, patch), rot, trans = patch_sets(pairs, n, seed=pairs * 7 + n)
    calls = dict(lgr=lambda: lgr_batch(starts, src, tgt, scores, patch),
                 ransac=lambda: ransac_batch(starts, src, tgt, scores, n_points=1000, iterations=50000))
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
    out = dict(case=name, pairs=pairs, rows_per_pair=n, patches=PATCHES, inlier_share=INLIER_SHARE, sigma=SIGMA)
    for k in calls:
        rre, rte = pose_errors(res[k]["T"], rot, trans)
        out[k] = dict(ms_per_call=round(float(np.median(ms[k])), 4), ms_min=round(min(ms[k]), 4), ms_max=round(max(ms[k]), 4),
                      median_rre_deg=float("%.4g" % rre.median()), median_rte_m=float("%.4g" % rte.median()),
                      share_rre15_rte03=round(float(((rre < 15) & (rte < 0.3)).double().mean()), 4))
    if "lgr" in calls:
        hyp = res["lgr"]["hypotheses"].double()
        out["lgr"]["hypotheses_per_pair"] = round(float(hyp.mean()), 1)
        out["lgr"]["verify_tests_per_call"] = float((hyp * n).sum())
        out["lgr"]["status_nonzero"] = int((res["lgr"]["status"] != 0).sum())
    if len(calls) == 2:
        out["ransac_over_lgr"] = round(out["ransac"]["ms_per_call"] / out["lgr"]["ms_per_call"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("lgr", "ransac"), default=None, help="time one estimator alone (kernel traces)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lgr_bench.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    cases = [time_case("512x1000", 512, 1000, args.steps, args.warmup, args.only),
             time_case("1x1000", 1, 1000, args.steps, args.warmup, args.only),
             time_case("64x10000", 64, 10000, args.steps, args.warmup, args.only)]
    result = dict(metric="lgr_vs_ransac_ms_per_call", device=torch.cuda.get_device_name(0), steps=args.steps, cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
