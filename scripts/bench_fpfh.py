"""Times the FPFH operator (roitr_amd/fpfh.py compute_fpfh) against a torch formulation of the same
definition on the device: pointops.knnquery for the rows, then gathers, elementwise float64 operations and scatter_add for the
histograms, in chunks of points (the (points, neighbours, 33) blend operand does not fit otherwise).  It is the only comparator this
environment has; Open3D is not part of it.

Clouds: scan-like (synthetic.surface_points, the room-like surfaces of `bench.py --cloud surface`) with normals from
prep.estimate_normals(knn=33), radius 0.125, max_nn 100, at 1024 clouds x 5000 points (a 512-pair call), one cloud of 5000 points and
64 clouds x 30 000 points.  Warm-up calls, then the two alternate; device events around every call; medians with min - max.  The kNN
call alone (grid build + query, pointops.knnquery_raw on the same clouds) is timed beside them; the split between the kNN kernels,
fpfh_spfh_kernel and fpfh_blend_kernel comes from a kernel trace collected in a run of its own and summarised by --trace-dir:

    python scripts/bench_fpfh.py [--steps 10] [--warmup 2] [--only fpfh] [--shapes 1024x5000,...] [--out profiles/fpfh_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_fpfh.py --steps 3 --warmup 1 --only fpfh --shapes SHAPE --out DIR/bench.json
    python scripts/bench_fpfh.py --trace-dir DIR --trace-shape SHAPE          (appends the shape's rows to profiles/fpfh_kernels.csv)
    python scripts/bench_fpfh.py --sweep-occupancy profiles/fpfh_knn_occupancy.json   (the kNN call alone against the grid's target occupancy)

No target time was fixed in advance; nothing here is gated.
"""
import argparse
import csv
import glob
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RADIUS, MAX_NN = 0.125, 100
SHAPES = (("1024x5000", 1024, 5000), ("1x5000", 1, 5000), ("64x30000", 64, 30000))
KERNEL_CSV = os.path.join(ROOT, "profiles", "fpfh_kernels.csv")


def clouds(b, n):
    """b scan-like clouds of n points (at most 64 distinct ones, repeated) and their estimated normals, on the device."""
    from roitr_amd.prep import estimate_normals
    from roitr_amd.synthetic import surface_points
    distinct = [surface_points(np.random.default_rng(1000 * n + i), n, 0.0, 2.0).astype(np.float32) for i in range(min(b, 64))]
    xyz = torch.from_numpy(np.concatenate([distinct[i % len(distinct)] for i in range(b)])).cuda()
    offset = torch.arange(1, b + 1, dtype=torch.int32, device="cuda") * n
    return xyz, estimate_normals(xyz, offset, 33, (1.0, 1.0, 1.0)), offset


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    """Component by component, every product and difference a rounded operation of its own as in the definition: torch.cross contracts
    them, and on planar patches with mirrored normals the sign of a rounding residue then decides between the first and the last bin."""
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


@torch.no_grad()
def torch_fpfh(xyz, normals, offset, radius=RADIUS, max_nn=MAX_NN, chunk=32768):
    """The definition of include/roitr_pointops.h in torch float64 (sums in torch's order, not in row order)."""
    from roitr_amd import pointops
    n, dev = xyz.shape[0], xyz.device
    idx = pointops.knnquery_raw(max_nn, xyz, xyz, offset, offset, use_grid=True)[0].long()
    off = offset.long()
    cloud = torch.bucketize(torch.arange(n, device=dev), off, right=True)
    size = (off - torch.cat([off.new_zeros(1), off[:-1]]))[cloud]
    p, nr = xyz.double(), normals.double()
    counts = torch.zeros((n * 33,), dtype=torch.float64, device=dev)
    keep_all = torch.empty((n, max_nn), dtype=torch.bool, device=dev)
    d2_all = torch.empty((n, max_nn), dtype=torch.float64, device=dev)
    slots = torch.arange(max_nn, device=dev)[None, :]
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        j = idx[s:e]
        rows = torch.arange(s, e, device=dev)[:, None]
        notself = (slots < size[s:e, None]) & (j != rows)
        cand = notself & (torch.cumsum(notself, 1) - 1 < max_nn - 1)
        dp = p[j] - p[s:e, None, :]
        d2 = dot(dp, dp)
        keep = cand & (d2 < radius * radius)
        d = torch.sqrt(d2)
        nz = d != 0
        ds = torch.where(nz, d, torch.ones_like(d))
        ni, nj = nr[s:e, None, :].expand_as(dp), nr[j]
        a1, a2 = dot(ni, dp) / ds, dot(nj, dp) / ds
        swap = (a1.abs() < a2.abs())[..., None]
        n1, n2, dps = torch.where(swap, nj, ni), torch.where(swap, ni, nj), torch.where(swap, -dp, dp)
        v = cross(dps, n1)
        vn = torch.sqrt(dot(v, v))
        ok = nz & (vn != 0)
        v = v / torch.where(ok, vn, torch.ones_like(vn))[..., None]
        w = cross(n1, v)
        zero = torch.zeros_like(d)
        f2 = torch.where(ok, torch.where(swap[..., 0], -a2, a1), zero)
        f1 = torch.where(ok, dot(v, n2), zero)
        f0 = torch.where(ok, torch.atan2(dot(w, n2), dot(n1, n2)), zero)
        x = torch.stack([11.0 * (f0 + np.pi) / (2.0 * np.pi), 11.0 * (f1 + 1.0) / 2.0, 11.0 * (f2 + 1.0) / 2.0], -1)
        h = torch.floor(x).clamp(0, 10).long() + torch.tensor([0, 11, 22], device=dev)
        flat = (rows[..., None] * 33 + h)[keep]
        counts.scatter_add_(0, flat.reshape(-1), torch.ones_like(flat.reshape(-1), dtype=torch.float64))
        keep_all[s:e], d2_all[s:e] = keep, d2
    counts = counts.reshape(n, 33)
    m = keep_all.sum(1)
    spfh = torch.where(m[:, None] > 0, counts * (100.0 / m.clamp_min(1).double())[:, None], torch.zeros_like(counts))
    out = torch.empty((n, 36), dtype=torch.float32, device=dev)
    out[:, 33:] = 0
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        sel = keep_all[s:e] & (d2_all[s:e] > 0)
        val = spfh[idx[s:e]] / torch.where(sel, d2_all[s:e], torch.ones_like(d2_all[s:e]))[..., None]
        F = (val * sel[..., None]).sum(1)
        S = F.reshape(-1, 3, 11).sum(2).repeat_interleave(11, dim=1)
        out[s:e, :33] = (torch.where(S != 0, F * 100.0 / torch.where(S != 0, S, torch.ones_like(S)), F) + spfh[s:e]).float()
    return out


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def kernel_split(shape):
    """ms per compute_fpfh call by kernel family from profiles/fpfh_kernels.csv (None when the shape has no rows there).  The traced
    process also estimates the normals once: kernels with fewer launches than fpfh_spfh_kernel belong to that call alone and are left
    out; a kernel with one launch more (grid build, tie replay) had its shortest launch there (kNN(33) against kNN(100))."""
    if not os.path.exists(KERNEL_CSV):
        return None
    rows = [r for r in csv.DictReader(open(KERNEL_CSV)) if r["shape"] == shape]
    calls = [int(r["calls"]) for r in rows if r["kernel"] == "fpfh_spfh_kernel"]
    if not calls:
        return None
    fam = lambda k: "spfh" if k == "fpfh_spfh_kernel" else "blend" if k == "fpfh_blend_kernel" else "prepare" if k == "fpfh_prepare_kernel" \
        else "knn" if k.startswith(("knn_", "grid_build", "sort_queries")) else None
    out = {}
    for r in rows:
        c, avg = int(r["calls"]), float(r["avg_us"])
        if not fam(r["kernel"]) or c < calls[0]:
            continue
        total = c * avg - (float(r["min_us"]) if c == calls[0] + 1 else 0.0)
        out[fam(r["kernel"])] = out.get(fam(r["kernel"]), 0.0) + total / calls[0] / 1000.0
    return {k: round(v, 4) for k, v in out.items()}


def time_case(name, b, n, steps, warmup, only):
    from roitr_amd import pointops
    from roitr_amd.fpfh import compute_fpfh
    xyz, normals, offset = clouds(b, n)
    calls = dict(fpfh=lambda: compute_fpfh(xyz, normals, offset, RADIUS, MAX_NN, strict=False),
                 knn=lambda: pointops.knnquery_raw(MAX_NN, xyz, xyz, offset, offset, use_grid=True)[0],
                 torch=lambda: torch_fpfh(xyz, normals, offset))
    calls = {k: v for k, v in calls.items() if only in (None, k)}
    res = {}
    for _ in range(warmup):
        res = {k: f() for k, f in calls.items()}
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(steps):
        for k, f in calls.items():       # the variants alternate
            if k == "torch" and len(ms[k]) >= max(2, steps // 4):
                continue                 # the comparator takes seconds at the large shapes: a few calls of it
            t, res[k] = timed(f)
            ms[k].append(t)
    out = dict(case=name, clouds=b, points_per_cloud=n, radius=RADIUS, max_nn=MAX_NN)
    for k in calls:
        out[k] = dict(ms_per_call=round(float(np.median(ms[k])), 4), ms_min=round(min(ms[k]), 4), ms_max=round(max(ms[k]), 4), calls=len(ms[k]))
    if "fpfh" in calls:
        _, _, nbr, _ = compute_fpfh(xyz, normals, offset, RADIUS, MAX_NN, return_stages=True, strict=False)
        out["fpfh"].update(neighbours_mean=round(float(nbr.double().mean()), 2), neighbours_max=int(nbr.max()),
                           ns_per_point=round(1e6 * out["fpfh"]["ms_per_call"] / (b * n), 3))
        if "knn" in calls:
            out["fpfh_minus_knn_ms"] = round(out["fpfh"]["ms_per_call"] - out["knn"]["ms_per_call"], 4)
        if "torch" in calls:
            out["torch_over_fpfh"] = round(out["torch"]["ms_per_call"] / out["fpfh"]["ms_per_call"], 2)
            diff = (res["fpfh"] - res["torch"]).abs()
            out["max_abs_diff_to_torch"] = float(diff.max())
            out["rows_off_by_more_than_1e-3"] = int((diff.max(1).values > 1e-3).sum())
        split = kernel_split(name)
        if split:
            out["kernel_trace_ms_per_call"] = split
    return out


def summarise_trace(trace_dir, shape):
    """Appends `shape,kernel,calls,avg_us,min_us,max_us` rows of a rocprofv3 --stats run to profiles/fpfh_kernels.csv."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {trace_dir}")
    rows = []
    for r in csv.DictReader(open(files[0])):
        name = re.match(r"\w+", r["Name"].replace("(anonymous namespace)::", "").replace("void ", "")).group(0)
        if name.startswith(("fpfh_", "knn_", "grid_build", "sort_queries")):
            rows.append((shape, name, int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3, float(r["TotalDurationNs"])))
    rows.sort(key=lambda r: -r[6])
    new = not os.path.exists(KERNEL_CSV)
    with open(KERNEL_CSV, "a") as f:
        if new:
            f.write("shape,kernel,calls,avg_us,min_us,max_us\n")
        for r in rows:
            f.write("%s,%s,%d,%.1f,%.1f,%.1f\n" % r[:6])


def sweep_occupancy(out_path, shapes):
    """Grid build + kNN(100) of the clouds against themselves, rows only, as the operator calls it, at several target occupancies of the
    grid (points per cell): ms per call (median of 4) and whether the rows equal those of the first occupancy (they must: the search
    is exact).  The operator uses (max_nn + 1) / 3 = 33.67; pointops.knnquery sizes its grid for 0.4 (k + 2) = 40.4."""
    import ctypes
    from roitr_amd import _lib as L
    lib, rows = L.lib(), []
    for name, b, n in SHAPES:
        if name not in shapes:
            continue
        xyz, _, off = clouds(b, n)
        total = xyz.shape[0]
        ws = torch.empty(lib.roitr_knn_workspace_bytes(b, total, total), dtype=torch.uint8, device="cuda")
        idx = torch.empty((total, MAX_NN), dtype=torch.int32, device="cuda")
        st, ref = L.stream_ptr(), None
        for rho in (6.0, 9.0, 12.0, 17.0, 25.0, 33.67, 40.4):
            def call():
                L.check(lib.roitr_knn_build_grid_ex(b, total, total, L.ptr(xyz), L.ptr(off), L.ptr(ws), ctypes.c_float(rho), st), "grid")
                L.check(lib.roitr_knnquery_ex(b, total, total, MAX_NN, L.ptr(xyz), L.ptr(xyz), L.ptr(off), L.ptr(off), L.ptr(idx), None, None, None,
                                              None, None, 1, total, L.ptr(ws), st), "knn")
            call()
            torch.cuda.synchronize()
            ms = [timed(call)[0] for _ in range(4)]
            same = True if ref is None else bool(torch.equal(ref, idx))
            ref = idx.clone() if ref is None else ref
            rows.append(dict(shape=name, rho=rho, ms=round(float(np.median(ms)), 3), same_rows=same))
            print(json.dumps(rows[-1]), flush=True)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("fpfh", "knn", "torch"), default=None, help="time one variant alone (kernel traces)")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES), help="comma-separated subset of the shapes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_bench.json"))
    ap.add_argument("--trace-dir", default=None, help="summarise a rocprofv3 --kernel-trace --stats output directory instead of timing")
    ap.add_argument("--trace-shape", default=None)
    ap.add_argument("--sweep-occupancy", default=None, metavar="JSON", help="time the kNN(100) call at several grid occupancies instead")
    args = ap.parse_args()
    if args.trace_dir:
        summarise_trace(args.trace_dir, args.trace_shape or "?")
        return
    torch.cuda.set_device(0)
    if args.sweep_occupancy:
        sweep_occupancy(args.sweep_occupancy, args.shapes.split(","))
        return
    cases = []
    for name, b, n in SHAPES:
        if name in args.shapes.split(","):
            cases.append(time_case(name, b, n, args.steps, args.warmup, args.only))
            print(json.dumps(cases[-1]), flush=True)
    result = dict(metric="fpfh_ms_per_call", device=torch.cuda.get_device_name(0), steps=args.steps,
                  comparator="torch float64 formulation of the same definition (pointops.knnquery, gather, scatter_add), chunked",
                  expectation="none fixed in advance (not gated)", cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
