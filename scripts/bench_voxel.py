"""Times the raw-scan preparation (prep.voxel_down_sample and prep.random_subsample: csrc/voxel.hip) against the
plain torch formulation of the voxel grid on the same device: torch.unique(keys, return_inverse=True) + index_add_ in float64 + a
divide (not bit-reproducible: index_add_ uses float atomics; unique sorts twice inside).  The torch side is timed on keys built
beforehand -- those three operations alone, which favours it: the library call builds its keys (bounds, indices) inside its time.
Device events around the whole public call (allocations and its one host read included), the median of `--reps` after `--warmup` calls.

Clouds: seeded, scan-like (synthetic.surface_points, a 2 m room), 300 000 points each.  Cases:
  batched   64 clouds in one call at voxel 0.025          single   one such cloud alone          cap   64 x 300 000 -> 30 000
Printed per case: ms, points per second, GB/s on the algorithmic bytes (counted below from the shapes and the number of live sort
passes) and that rate's share of the MI355X's 8 TB/s, and the ratio to the torch formulation.

    python scripts/bench_voxel.py [--json out.json] [--txt out.txt] [--cases batched,single,cap] [--no-torch]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_GBS = 8000.0   # HBM3E peak of the MI355X, as in README.md
N_POINTS, N_CLOUDS, VOXEL, CAP = 300000, 64, 0.025, 30000


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


def clouds(b):
    from roitr_amd.synthetic import surface_points
    xyz = np.concatenate([surface_points(np.random.default_rng(5000 + i), N_POINTS, 0.0, 2.0).astype(np.float32) for i in range(b)])
    off = (np.arange(1, b + 1) * N_POINTS).astype(np.int32)
    return torch.from_numpy(xyz).cuda(), torch.from_numpy(off).cuda()


def torch_keys(xyz, off, vs):
    sizes = torch.diff(off.long(), prepend=off.new_zeros(1, dtype=torch.long))
    cloud = torch.repeat_interleave(torch.arange(off.shape[0], device=xyz.device), sizes)
    mn = torch.full((off.shape[0], 3), float("inf"), device=xyz.device).scatter_reduce(0, cloud[:, None].expand(-1, 3), xyz, "amin")
    vmb = mn.double() - vs * 0.5
    ijk = torch.floor((xyz.double() - vmb[cloud]) / vs).long()
    return (cloud << 48) | (ijk[:, 0] << 32) | (ijk[:, 1] << 16) | ijk[:, 2]


def torch_formulation(keys, xyz):
    uniq, inverse = torch.unique(keys, return_inverse=True)
    m = uniq.shape[0]
    sums = torch.zeros((m, 3), dtype=torch.float64, device=xyz.device).index_add_(0, inverse, xyz.double())
    counts = torch.bincount(inverse, minlength=m)
    return (sums / counts[:, None]).float(), inverse, counts


def live_passes(keys):
    return sum(1 for p in range(8) if int(((keys >> (8 * p)) & 255).min()) != int(((keys >> (8 * p)) & 255).max()))


def voxel_bytes(n, m, passes):
    """Algorithmic bytes of one voxel_down_sample call without attributes: n points, m voxels, `passes` live 8-bit sort passes.
    bounds 12 n; keys 12 n read + 12 n written; per pass 8 n (histogram) + 12 n read + 12 n written (scatter); heads 8 n + n; tile sums
    n; assign n + 12 n read + 4 n (inverse) + 4 m (start); means 12 n (sorted keys, payload) + 12 n (gathered points) + 20 m."""
    return n * (12 + 24 + 32 * passes + 9 + 1 + 17 + 24) + m * 24


def cap_bytes(n, kept, passes):
    """keys 12 n written; per pass 32 n; keep 12 n read + n written; tile sums n; compaction n read + 4 kept written."""
    return n * (12 + 32 * passes + 13 + 1 + 1) + 4 * kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    ap.add_argument("--cases", default="batched,single,cap")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch formulation (the kernel-trace run)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_voxel.py measures on the GPU only"
    from roitr_amd.prep import random_subsample, voxel_down_sample
    rows, lines = [], []
    for case in args.cases.split(","):
        b = 1 if case == "single" else N_CLOUDS
        xyz, off = clouds(b)
        n = int(xyz.shape[0])
        row = dict(case=case, clouds=b, points=n)
        if case == "cap":
            idx, _ = random_subsample(off, CAP, 0)
            sizes = torch.diff(off.long(), prepend=off.new_zeros(1, dtype=torch.long))
            u_bits = 7 if b > 1 else 6     # 48 bits of u are live, plus the cloud digit
            ms, lo, hi = timed(lambda: random_subsample(off, CAP, 0), args.warmup, args.reps)
            nbytes = cap_bytes(n, int(idx.shape[0]), u_bits)
            row.update(kept=int(idx.shape[0]), live_passes=u_bits)
            assert int(idx.shape[0]) == int(sizes.clamp(max=CAP).sum())
        else:
            r = voxel_down_sample(xyz, off, VOXEL)
            keys = torch_keys(xyz, off, VOXEL)
            passes = live_passes(keys)
            m = int(r.points.shape[0])
            ms, lo, hi = timed(lambda: voxel_down_sample(xyz, off, VOXEL), args.warmup, args.reps)
            nbytes = voxel_bytes(n, m, passes)
            row.update(voxels=m, live_passes=passes)
            if not args.no_torch:
                pts, inverse, counts = torch_formulation(keys, xyz)
                # the same voxels in the same order (unique sorts the same keys); the sums differ in the last bits at most
                assert pts.shape[0] == m and torch.equal(inverse.int(), r.inverse) and torch.equal(counts.int(), r.counts)
                row["max_abs_diff_to_torch"] = float((pts - r.points).abs().max())
                del pts, inverse, counts
                t_ms, t_lo, t_hi = timed(lambda: torch_formulation(keys, xyz), args.warmup, args.reps)
                row.update(torch_ms=t_ms, torch_ms_min=t_lo, torch_ms_max=t_hi, torch_over_kernel=t_ms / ms)
            del r, keys
        row.update(ms=ms, ms_min=lo, ms_max=hi, points_per_s=n / ms * 1e3, algorithmic_bytes=nbytes, gbs=nbytes / ms / 1e6,
                   hbm_fraction=nbytes / ms / 1e6 / PEAK_GBS)
        rows.append(row)
        line = (f"{case:8s} {b:3d} clouds {n:9d} points: {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f})  {row['points_per_s'] / 1e9:6.2f} G points/s  "
                f"{row['gbs']:7.1f} GB/s on {nbytes / n:.0f} B/point ({row['hbm_fraction']:.3f} of {PEAK_GBS / 1000:g} TB/s), "
                f"{row['live_passes']} live passes")
        if "voxels" in row:
            line += f", {row['voxels']} voxels"
        if "torch_ms" in row:
            line += (f"   torch formulation {row['torch_ms']:8.3f} ms (min {row['torch_ms_min']:.3f}, max {row['torch_ms_max']:.3f})   "
                     f"x{row['torch_over_kernel']:.2f}   max |diff| {row['max_abs_diff_to_torch']:.1e}")
        print(line, flush=True)
        lines.append(line)
        del xyz, off
        torch.cuda.empty_cache()
    for path, text in ((args.json, json.dumps(rows, indent=1)), (args.txt, "\n".join(lines) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
