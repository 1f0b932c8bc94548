"""Times descriptor matching (descmatch.match_batch: the fused score-argmax kernel) against the baseline a
user has without it: per pair `s @ t.T`, then `.max(1)` and `.max(0)` with torch on the same device, which materialises the (N, M)
matrix (for --metric sqdist too: on unit-norm rows the smallest distance is the largest dot product, so the baseline stays the
cheapest thing a user could run).  Device events around the whole call, the median of 20 after 5 warm-up calls, seeded unit-norm descriptors.

    python scripts/bench_descmatch.py [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TFLOPS = 157.3   # fp32 MFMA peak of the MI355X, as in README.md
CASES = [(64, 5000, 5000, 256), (1, 5000, 5000, 256), (8, 8000, 8000, 512)]


def timed(fn, warmup=5, reps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--metric", default="dot", choices=["dot", "sqdist"])
    args = ap.parse_args()
    from roitr_amd.descmatch import match_batch
    rows = []
    for pairs, n, m, d in CASES:
        g = torch.Generator(device="cuda").manual_seed(pairs * 1000 + d)
        s = torch.nn.functional.normalize(torch.randn((pairs * n, d), device="cuda", generator=g), dim=1)
        t = torch.nn.functional.normalize(torch.randn((pairs * m, d), device="cuda", generator=g), dim=1)
        so = torch.arange(pairs + 1, device="cuda", dtype=torch.int32) * n
        to = torch.arange(pairs + 1, device="cuda", dtype=torch.int32) * m
        fused = lambda: match_batch(so, s, to, t, metric=args.metric, mode="mutual")
        def baseline():
            out = []
            for b in range(pairs):
                sc = s[b * n:(b + 1) * n] @ t[b * m:(b + 1) * m].T
                out.append((sc.max(1), sc.max(0)))
            return out
        r = fused()
        base = baseline()
        agree = sum(int((r["row_idx"][b * n:(b + 1) * n].long() == base[b][0][1]).sum()) for b in range(pairs)) / (pairs * n)
        ms_f, ms_b = timed(fused), timed(baseline)
        flop = 2.0 * pairs * n * m * d
        row = dict(pairs=pairs, n=n, m=m, dim=d, metric=args.metric, fused_ms=ms_f, baseline_ms=ms_b, speedup=ms_b / ms_f,
                   fused_pairs_per_s=pairs / ms_f * 1e3, fused_tflops=flop / ms_f / 1e9, fused_peak_fraction=flop / ms_f / 1e9 / PEAK_TFLOPS,
                   baseline_tflops=flop / ms_b / 1e9, matrix_bytes_per_pair_avoided=n * m * 4, row_index_agreement=agree)
        rows.append(row)
        print(f"{pairs:3d} x ({n}, {m}, {d}) {args.metric}: fused {ms_f:8.3f} ms  {row['fused_pairs_per_s']:9.1f} pairs/s  "
              f"{row['fused_tflops']:6.1f} TFLOP/s ({row['fused_peak_fraction']:.3f} of {PEAK_TFLOPS})   torch baseline {ms_b:8.3f} ms "
              f"({row['baseline_tflops']:.1f} TFLOP/s)   x{row['speedup']:.2f}   row indices equal to torch's: {agree:.6f}")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
