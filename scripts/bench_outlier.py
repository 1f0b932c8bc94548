"""Times the outlier filters (roitr_amd/prep.py remove_statistical_outlier / remove_radius_outlier) against
their two yardsticks: the grid build + roitr_knnquery_ex of the same clouds alone (what the statistical filter's new kernels follow),
and a torch formulation on the device (chunked cdist + topk per cloud, then mean, std and mask).  Open3D is not part of this
environment.

Clouds: scan-like (synthetic.surface_points) scaled to one point per (2.5 cm)^2 of surface, with 2 % of the points replaced by uniform
points of the bounding box; 64 clouds x 30 000 points and 8 x 300 000.  Statistical filter: k = 20, std_ratio 2; radius filter: more
than 16 points within 5 cm.  Warm-up calls, then the variants alternate; device events around every call; medians with min - max.
Besides the times: the share of the planted points removed and of the surface points lost.  The split between the kNN kernels and the
kernels of csrc/outlier.hip comes from a kernel trace collected in a run of its own and summarised by --trace-dir:

    python scripts/bench_outlier.py [--steps 10] [--warmup 2] [--only statistical] [--shapes 64x30000,...] [--out profiles/outlier_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_outlier.py --steps 3 --warmup 1 --only filters --shapes SHAPE --out DIR/bench.json
    python scripts/bench_outlier.py --trace-dir DIR --trace-shape SHAPE       (appends the shape's rows to profiles/outlier_kernels.csv)

No target time was fixed in advance; nothing here is gated.
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, STD_RATIO, NB_POINTS, RADIUS, SPACING, PLANTED = 20, 2.0, 16, 0.05, 0.025, 0.02
ROOM_AREA = 27.0   # m^2 of surface in synthetic.surface_points(0, 2): the corridor's six rectangles and the furniture, nominal
SHAPES = (("64x30000", 64, 30000), ("8x300000", 8, 300000))
KERNEL_CSV = os.path.join(ROOT, "profiles", "outlier_kernels.csv")


def clouds(b, n):
    """b clouds of n points (at most 8 distinct ones, repeated) on the device, and the mask of the planted points."""
    from roitr_amd.synthetic import surface_points
    scale = SPACING * (n / ROOM_AREA) ** 0.5
    m = int(round(PLANTED * n))
    distinct = []
    for i in range(min(b, 8)):
        rng = np.random.default_rng(7000 * n + i)
        p = surface_points(rng, n, 0.0, 2.0) * scale
        rows = rng.choice(n, m, replace=False)
        p[rows] = rng.uniform(p.min(0), p.max(0), (m, 3))
        mask = np.zeros(n, bool)
        mask[rows] = True
        distinct.append((p.astype(np.float32), mask))
    xyz = torch.from_numpy(np.concatenate([distinct[i % len(distinct)][0] for i in range(b)])).cuda()
    planted = torch.from_numpy(np.concatenate([distinct[i % len(distinct)][1] for i in range(b)])).cuda()
    return xyz, torch.arange(1, b + 1, dtype=torch.int32, device="cuda") * n, planted


@torch.no_grad()
def torch_statistical(xyz, offset, k=K, std_ratio=STD_RATIO, chunk_elems=1 << 27):
    """The statistical filter in torch: per cloud, chunked cdist + topk (fp32), then mean, std and mask in float64 (torch's sum order;
    the zero-mean quirk of the definition is not restated)."""
    keep = torch.empty((xyz.shape[0],), dtype=torch.bool, device=xyz.device)
    ends = [0] + offset.tolist()
    for s, e in zip(ends[:-1], ends[1:]):
        p = xyz[s:e]
        rows = max(1, chunk_elems // max(e - s, 1))
        mean = torch.cat([torch.cdist(p[r:r + rows], p).topk(min(k, e - s), dim=1, largest=False).values.double().mean(1)
                          for r in range(0, e - s, rows)])
        keep[s:e] = mean < mean.mean() + std_ratio * mean.std()
    return keep


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def knn_alone(xyz, offset):
    """The grid build and the kNN(K) rows exactly as the statistical filter calls them."""
    from roitr_amd import _lib as L
    lib = L.lib()
    n, b = int(xyz.shape[0]), int(offset.shape[0])
    ws = torch.empty(lib.roitr_knn_workspace_bytes(b, n, n), dtype=torch.uint8, device="cuda")
    idx = torch.empty((n, K), dtype=torch.int32, device="cuda")

    def call():
        st = L.stream_ptr()
        L.check(lib.roitr_knn_build_grid_ex(b, n, n, L.ptr(xyz), L.ptr(offset), L.ptr(ws), ctypes.c_float((K + 1) / 3.0), st), "grid")
        L.check(lib.roitr_knnquery_ex(b, n, n, K, L.ptr(xyz), L.ptr(xyz), L.ptr(offset), L.ptr(offset), L.ptr(idx), None, None, None, None, None, 1,
                                      n, L.ptr(ws), st), "knn")
        return idx
    return call


def kernel_split(shape):
    """ms by kernel family from profiles/outlier_kernels.csv (None when the shape has no rows there).  The traced run makes the same
    number of statistical and radius calls and every family is divided by the launches of outlier_mean_kernel: knn_query, mean and
    stats belong to a statistical call, radius to a radius call, and grid_build, prepare and the four compaction kernels are the sum
    over one call of each."""
    if not os.path.exists(KERNEL_CSV):
        return None
    rows = [r for r in csv.DictReader(open(KERNEL_CSV)) if r["shape"] == shape]
    calls = [int(r["calls"]) for r in rows if r["kernel"] == "outlier_mean_kernel"]
    if not calls:
        return None
    out = {}
    for r in rows:
        k = r["kernel"]
        fam = k[len("outlier_"):-len("_kernel")] if k.startswith("outlier_") else "knn_query" if k.startswith(("knn_", "sort_queries")) else "grid_build"
        out[fam] = out.get(fam, 0.0) + int(r["calls"]) * float(r["avg_us"]) / calls[0] / 1000.0
    return {k: round(v, 4) for k, v in out.items()}


def shares(keep, planted):
    return dict(planted_removed=round(float((~keep[planted]).double().mean()), 4), surface_lost=round(float((~keep[~planted]).double().mean()), 4))


def time_case(name, b, n, steps, warmup, only):
    from roitr_amd import prep
    xyz, offset, planted = clouds(b, n)
    calls = dict(statistical=lambda: prep.remove_statistical_outlier(xyz, offset, K, STD_RATIO, max_workspace_bytes=1 << 40).keep,
                 radius=lambda: prep.remove_radius_outlier(xyz, offset, NB_POINTS, RADIUS).keep,
                 radius_counts=lambda: prep.remove_radius_outlier(xyz, offset, NB_POINTS, RADIUS, return_counts=True).keep,
                 knn=knn_alone(xyz, offset),
                 torch=lambda: torch_statistical(xyz, offset))
    pick = dict(filters=("statistical", "radius"))
    calls = {k: v for k, v in calls.items() if only is None or k in pick.get(only, (only,))}
    res = {}
    for _ in range(warmup):
        res = {k: f() for k, f in calls.items() if k != "torch"}
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(steps):
        for k, f in calls.items():       # the variants alternate
            if k == "torch" and len(ms[k]) >= (2 if n <= 30000 else 1):
                continue                 # the comparator takes seconds: one or two calls of it
            t, res[k] = timed(f)
            ms[k].append(t)
    out = dict(case=name, clouds=b, points_per_cloud=n, nb_neighbors=K, std_ratio=STD_RATIO, nb_points=NB_POINTS, radius_m=RADIUS,
               spacing_m=SPACING, planted_share=PLANTED, knn_row_bytes=b * n * K * 4)
    for k in calls:
        out[k] = dict(ms_per_call=round(float(np.median(ms[k])), 4), ms_min=round(min(ms[k]), 4), ms_max=round(max(ms[k]), 4), calls=len(ms[k]))
    for k in ("statistical", "radius", "torch"):
        if k in calls:
            out[k].update(shares(res[k], planted))
    if "statistical" in calls and "knn" in calls:
        out["statistical_minus_knn_ms"] = round(out["statistical"]["ms_per_call"] - out["knn"]["ms_per_call"], 4)
    if "statistical" in calls and "torch" in calls:
        out["torch_over_statistical"] = round(out["torch"]["ms_per_call"] / out["statistical"]["ms_per_call"], 2)
        out["flags_equal_to_torch"] = round(float((res["statistical"] == res["torch"]).double().mean()), 6)
    split = kernel_split(name)
    if split:
        out["kernel_trace_ms_per_call"] = split
    return out


def summarise_trace(trace_dir, shape):
    """Appends `shape,kernel,calls,avg_us,min_us,max_us` rows of a rocprofv3 --stats run to profiles/outlier_kernels.csv."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {trace_dir}")
    rows = []
    for r in csv.DictReader(open(files[0])):
        name = re.match(r"\w+", r["Name"].replace("(anonymous namespace)::", "").replace("void ", "")).group(0)
        if name.startswith(("outlier_", "knn_", "grid_build", "sort_queries")):
            rows.append((shape, name, int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3, float(r["TotalDurationNs"])))
    rows.sort(key=lambda r: -r[6])
    new = not os.path.exists(KERNEL_CSV)
    with open(KERNEL_CSV, "a") as f:
        if new:
            f.write("shape,kernel,calls,avg_us,min_us,max_us\n")
        for r in rows:
            f.write("%s,%s,%d,%.1f,%.1f,%.1f\n" % r[:6])


def main():
    global NB_POINTS
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("statistical", "radius", "radius_counts", "knn", "torch", "filters"), default=None,
                    help="time one variant alone; filters: the statistical and the radius filter (kernel traces)")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES), help="comma-separated subset of the shapes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlier_bench.json"))
    ap.add_argument("--nb-points", type=int, default=NB_POINTS, help="the radius filter's nb_points (default: Open3D's tutorial value)")
    ap.add_argument("--trace-dir", default=None, help="summarise a rocprofv3 --kernel-trace --stats output directory instead of timing")
    ap.add_argument("--trace-shape", default=None)
    args = ap.parse_args()
    if args.trace_dir:
        summarise_trace(args.trace_dir, args.trace_shape or "?")
        return
    torch.cuda.set_device(0)
    NB_POINTS = args.nb_points
    cases = []
    for name, b, n in SHAPES:
        if name in args.shapes.split(","):
            cases.append(time_case(name, b, n, args.steps, args.warmup, args.only))
            print(json.dumps(cases[-1]), flush=True)
    result = dict(metric="outlier_ms_per_call", device=torch.cuda.get_device_name(0), steps=args.steps,
                  yardsticks="the grid build + kNN(20) rows alone at the same shape; a torch formulation (chunked cdist + topk, mean, std, mask)",
                  expectation="none fixed in advance (not gated)", cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
