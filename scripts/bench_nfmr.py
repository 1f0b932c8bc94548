"""Times the batched NFMR (roitr_amd/nonrigid.py) on seeded constructed pairs.

Cases: 64 pairs x (N 8000 source points, C 6000 correspondences, M 2500 metric points) -- the shape of a 4DMatch test batch at the
flagship size -- and one pair of that shape, each with the automatic block size and with 64 / 128 / 256 lanes per workgroup.  Device
events around each timed call after warm-up calls; the call includes the wrapper's one host round trip (the status check).  Prints one
JSON line with ms per call, pairs/s and the achieved distance evaluations per second against the VALU-issue floor
(256 CU x 4 SIMD x 32 lanes x 2.4 GHz; 9 lane-operations per anchor candidate, 16 per blend candidate).

    python scripts/bench_nfmr.py [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VALU_LANE_OPS = 256 * 4 * 32 * 2.4e9
OPS_ANCHOR, OPS_BLEND = 9, 16


def constructed(pairs, n, c, m, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = torch.device("cuda")
    u = lambda *shape: torch.rand(*shape, generator=g, device=dev)
    raw = u(pairs, n, 3) * 2.0
    deformed = raw + 0.08 * torch.sin(1.7 * raw.roll(1, 2) + 0.3)
    idx = torch.randint(0, n, (pairs, c), generator=g, device=dev)
    q = torch.nn.functional.normalize(u(pairs, 4) - 0.5, dim=1)
    w, x, y, z = q.unbind(1)
    rot = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                       2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(pairs, 3, 3)
    trans = u(pairs, 3) * 2.0 - 1.0
    src_corr = torch.gather(deformed, 1, idx[:, :, None].expand(-1, -1, 3))
    tgt_corr = src_corr @ rot.transpose(1, 2) + trans[:, None, :] + 0.004 * (u(pairs, c, 3) - 0.5)
    metric = torch.stack([torch.randperm(n, generator=g, device=dev)[:m] for _ in range(pairs)])
    off = lambda k: torch.arange(0, (pairs + 1) * k, k, dtype=torch.int32, device=dev)
    return (off(n), raw.reshape(-1, 3), deformed.reshape(-1, 3), off(c), src_corr.reshape(-1, 3), tgt_corr.reshape(-1, 3).contiguous(), off(m),
            metric.reshape(-1), rot, trans)


def time_case(pairs, n, c, m, block, steps, warmup):
    from roitr_amd.nonrigid import nfmr_batch
    args = constructed(pairs, n, c, m, seed=pairs * 11 + 1)
    for _ in range(warmup):
        r = nfmr_batch(*args, block=block)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = nfmr_batch(*args, block=block)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    med = float(np.median(ms))
    evals = pairs * (c * n + m * c)
    floor_ms = pairs * (c * n * OPS_ANCHOR + m * c * OPS_BLEND) / VALU_LANE_OPS * 1e3
    return dict(case=f"{pairs}x(N{n},C{c},M{m})", block=block, ms_per_call=round(med, 4), ms_min=round(min(ms), 4),
                pairs_per_s=round(pairs / med * 1e3, 1), distance_evals_per_s=float("%.3e" % (evals / med * 1e3)),
                valu_floor_ms=round(floor_ms, 4), fraction_of_floor=round(floor_ms / med, 3), mean_nfmr=round(float(r["nfmr"].mean()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    cases = [time_case(pairs, 8000, 6000, 2500, block, args.steps, args.warmup) for pairs in (64, 1) for block in (0, 64, 128, 256)]
    print(json.dumps(dict(metric="nfmr_ms_per_call", cases=cases)))


if __name__ == "__main__":
    main()
