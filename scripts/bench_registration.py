"""Times the GPU correspondence RANSAC (roitr_amd/registration.py) on seeded constructed sets.

Cases: 512 pairs x 1000 correspondences x 50 000 iterations (the reference's setting), the same for one pair alone, and 64 pairs
x 10 000 correspondences with n_points = 5000.  Device events around each timed call after warm-up calls; prints one JSON line
with ms per call, pairs/s and the achieved (hypothesis x correspondence) tests per second against the VALU-issue floor
(256 CU x 4 SIMD x 32 lanes x 2.4 GHz / 17 lane-operations per test).

    python scripts/bench_registration.py [--steps 5] [--warmup 2] [--iterations 50000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VALU_LANE_OPS = 256 * 4 * 32 * 2.4e9
OPS_PER_TEST = 17


def constructed(pairs, n, seed, inlier_frac=0.3, sigma=0.005):
    rng = np.random.default_rng(seed)
    src, tgt = [], []
    for _ in range(pairs):
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        s = rng.uniform(-1, 1, (n, 3))
        t = s @ R.T + rng.uniform(-1, 1, 3) + rng.normal(0, sigma, (n, 3))
        k = int(inlier_frac * n)
        t[k:] = rng.uniform(t.min(0), t.max(0), (n - k, 3))
        src.append(s)
        tgt.append(t)
    dev = torch.device("cuda")
    starts = torch.arange(0, (pairs + 1) * n, n, dtype=torch.int32, device=dev)
    conf = torch.from_numpy(rng.uniform(0.05, 1, pairs * n).astype(np.float32)).to(dev)
    return (starts, torch.from_numpy(np.concatenate(src).astype(np.float32)).to(dev),
            torch.from_numpy(np.concatenate(tgt).astype(np.float32)).to(dev), conf)


def time_case(name, pairs, n, n_points, iterations, steps, warmup):
    from roitr_amd.registration import ransac_batch
    starts, src, tgt, conf = constructed(pairs, n, seed=pairs * 7 + n)
    kw = dict(n_points=n_points, iterations=iterations, sample="weighted")
    for _ in range(warmup):
        r = ransac_batch(starts, src, tgt, conf, **kw)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = ransac_batch(starts, src, tgt, conf, **kw)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    used = r["n_used"].double()
    valid = r["valid_hypotheses"].double()
    med = float(np.median(ms))
    tests_all = float((used * iterations).sum())            # every hypothesis x every selected row
    tests_valid = float((used * valid).sum())               # the ones the kernel actually counts (checkers passed)
    floor_ms = tests_all * OPS_PER_TEST / VALU_LANE_OPS * 1e3
    return dict(case=name, pairs=pairs, n=n, n_points=n_points, iterations=iterations, ms_per_call=round(med, 3),
                ms_min=round(min(ms), 3), pairs_per_s=round(pairs / med * 1e3, 1),
                tests_per_s=float("%.3e" % (tests_all / med * 1e3)), valid_fraction=round(float(valid.sum()) / (pairs * iterations), 4),
                counted_tests_per_s=float("%.3e" % (tests_valid / med * 1e3)),
                valu_floor_ms=round(floor_ms, 3), fraction_of_floor=round(floor_ms / med, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=50000)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    it = args.iterations
    cases = [time_case("512x1000", 512, 1000, 1000, it, args.steps, args.warmup),
             time_case("1x1000", 1, 1000, 1000, it, args.steps, args.warmup),
             time_case("64x10000_np5000", 64, 10000, 5000, it, args.steps, args.warmup)]
    print(json.dumps(dict(metric="ransac_ms_per_call", cases=cases)))


if __name__ == "__main__":
    main()
