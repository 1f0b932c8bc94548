"""Times the pair ground truth (pairgt.pair_ground_truth and pairgt.radius_correspondences: csrc/pairgt.hip)
against a dense torch formulation on the same device: per pair, chunked torch.cdist of the moved source against the target + a
threshold + nonzero (fp32, unordered within a source point, boundary pairs decided in fp32: not the same definition, only the same
work).  Device events around the whole public call (allocations and its host read included), the median of `--reps` after `--warmup`.

Pairs: synthetic.make_pair(cloud="surface"), scan-like clouds of a 2 m room with 60 % overlap.  Cases:
  batched  64 pairs x (30 000, 30 000), r = 0.0375        single  one such pair
  raw       8 pairs x (300 000, 300 000), r = 0.0375 (raw-scan density; no torch baseline: 7e11 distances)
  list     16 pairs x (30 000, 30 000), r = 0.1 (list-heavy: tens of rows per source point)
Printed per case: ms of the statistics call (both sides) and of the list call, source points per second, rows of the list, GB/s on
the algorithmic bytes counted below and that rate's share of the MI355X's 8 TB/s, and the ratio to the torch formulation.

    python scripts/bench_pairgt.py [--json out.json] [--txt out.txt] [--cases batched,single,raw,list] [--no-torch]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_GBS = 8000.0   # HBM3E peak of the MI355X, as in README.md
CASES = {"batched": (64, 30000, 0.0375), "single": (1, 30000, 0.0375), "raw": (8, 300000, 0.0375), "list": (16, 30000, 0.1)}


def timed(fn, warmup, reps):
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
    return sorted(ms)[len(ms) // 2], min(ms), max(ms)


def pairs(b, n):
    from roitr_amd.synthetic import make_pair
    ps = [make_pair(n, config=1, pair_index=i, cloud="surface") for i in range(b)]
    cat = lambda k: torch.from_numpy(np.concatenate([p[k] for p in ps]).astype(np.float32)).cuda()
    off = lambda k: torch.from_numpy(np.cumsum([len(p[k]) for p in ps]).astype(np.int32)).cuda()
    rot = torch.from_numpy(np.stack([p["rot"].reshape(3, 3) for p in ps]).astype(np.float32)).cuda()
    trans = torch.from_numpy(np.stack([p["trans"].reshape(3) for p in ps]).astype(np.float32)).cuda()
    return cat("src_points"), off("src_points"), cat("tgt_points"), off("tgt_points"), rot, trans


def torch_formulation(src, so, tgt, to, rot, trans, r, chunk=8192):
    lo_s, lo_t = [0] + so.tolist(), [0] + to.tolist()
    out = []
    for b in range(len(lo_s) - 1):
        s = src[lo_s[b]:lo_s[b + 1]] @ rot[b].T + trans[b]
        t = tgt[lo_t[b]:lo_t[b + 1]]
        for c in range(0, s.shape[0], chunk):
            nz = (torch.cdist(s[c:c + chunk], t) < r).nonzero()
            nz[:, 0] += c
            out.append(nz)
    return out


def stats_bytes(n, m):
    """One side of pair_ground_truth, n queries into m searched points, without the candidates the walk reads (data dependent: 16 B
    each): prepare 12 n + 12 m read, 12 m written; grid 12 m read three times + 16 m written; search 12 n read, 4 + 4 + 4 + 8 n
    written; reduction 4 n + 12 n read."""
    return n * (12 + 12 + 20 + 16) + m * (24 + 36 + 16)


def list_bytes(n, m, cand, rows):
    """radius_correspondences: the front of stats_bytes; positions 4 n read twice, 16 n written; fill 12 n + 20 n read, 12 B per
    candidate written; ranking 20 n read, 12 B per candidate read (once per 64 of its run), 8 B per row written."""
    return n * (12 + 12 + 4) + m * (24 + 36 + 16) + n * (8 + 16 + 32 + 20) + 24 * cand + 8 * rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    ap.add_argument("--cases", default="batched,single,raw,list")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch formulation (the kernel-trace run)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pairgt.py measures on the GPU only"
    from roitr_amd.pairgt import pair_ground_truth, radius_correspondences
    rows, lines = [], []
    for case in args.cases.split(","):
        b, npts, r = CASES[case]
        a = pairs(b, npts)
        n, m = int(a[0].shape[0]), int(a[2].shape[0])
        g = pair_ground_truth(*a, r)
        corr, off = radius_correspondences(*a, r)
        n_rows = int(corr.shape[0])
        cap = max(n_rows, 1)
        assert int(g.count.long().sum()) == n_rows and int(off[-1]) == n_rows
        row = dict(case=case, pairs=b, src_points=n, tgt_points=m, radius=r, rows=n_rows, rows_per_hit=n_rows / max(int(g.n_src_hit.sum()), 1),
                   longest_run=int(g.count.max()), overlap_src_mean=float(g.overlap_src.mean()), overlap_tgt_mean=float(g.overlap_tgt.mean()))
        del g, corr, off
        s_ms, s_lo, s_hi = timed(lambda: pair_ground_truth(*a, r), args.warmup, args.reps)
        c_ms, c_lo, c_hi = timed(lambda: radius_correspondences(*a, r, capacity=cap), args.warmup, args.reps)
        sb, lb = stats_bytes(n, m) + stats_bytes(m, n), list_bytes(n, m, n_rows, n_rows)
        row.update(stats_ms=s_ms, stats_ms_min=s_lo, stats_ms_max=s_hi, list_ms=c_ms, list_ms_min=c_lo, list_ms_max=c_hi,
                   stats_points_per_s=(n + m) / s_ms * 1e3, list_rows_per_s=n_rows / c_ms * 1e3, stats_bytes=sb, list_bytes=lb,
                   stats_gbs=sb / s_ms / 1e6, list_gbs=lb / c_ms / 1e6, stats_hbm_fraction=sb / s_ms / 1e6 / PEAK_GBS,
                   list_hbm_fraction=lb / c_ms / 1e6 / PEAK_GBS)
        line = (f"{case:8s} {b:3d} pairs {n:8d} + {m:8d} points r {r:g}: stats (both sides) {s_ms:8.3f} ms (min {s_lo:.3f}, max {s_hi:.3f}) "
                f"{row['stats_points_per_s'] / 1e9:5.2f} G queries/s {row['stats_gbs']:6.1f} GB/s ({row['stats_hbm_fraction']:.3f} of "
                f"{PEAK_GBS / 1000:g} TB/s);  list {c_ms:8.3f} ms (min {c_lo:.3f}, max {c_hi:.3f}) {n_rows} rows, "
                f"{row['rows_per_hit']:.1f} per hit point, longest run {row['longest_run']}, {row['list_rows_per_s'] / 1e9:5.2f} G rows/s "
                f"{row['list_gbs']:6.1f} GB/s ({row['list_hbm_fraction']:.3f})")
        if not args.no_torch and case != "raw":
            ref = torch_formulation(*a, r)
            t_rows = sum(int(x.shape[0]) for x in ref)
            del ref
            t_ms, t_lo, t_hi = timed(lambda: torch_formulation(*a, r), 1, 3)
            row.update(torch_ms=t_ms, torch_ms_min=t_lo, torch_ms_max=t_hi, torch_rows=t_rows, torch_over_list=t_ms / c_ms)
            line += f"   torch cdist + nonzero {t_ms:9.3f} ms (min {t_lo:.3f}, max {t_hi:.3f}), {t_rows} rows (fp32 boundary)   x{t_ms / c_ms:.1f}"
        rows.append(row)
        print(line, flush=True)
        lines.append(line)
        del a
        torch.cuda.empty_cache()
    for path, text in ((args.json, json.dumps(rows, indent=1)), (args.txt, "\n".join(lines) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
