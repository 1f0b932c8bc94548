"""Every output of the kNN entry points on seeded inputs, saved to one .npz: run it on two builds, then `--compare a.npz b.npz` (no GPU)
lists the keys and fails unless every one is bitwise equal.

    python scripts/dump_knn.py out.npz
    python scripts/dump_knn.py --compare parent.npz branch.npz

  ex/       roitr_knnquery_ex on every shape of tests/test_knn_fused_gpu.py (CASES, the one-column, nsample-1 and ppf-alone shapes) in all
            four cloud kinds: the engine's call (group_idx + ppf) and the call with all four outputs, from one workspace
  within/   roitr_knn_within on the shapes and caps of test_knn_within_matches_oracle_below_the_cap
  legacy/   knnquery_cuda_launcher on one small shape
  sorted/   roitr_knn_sorted_points after a build with each grid cap (every cloud's rows ordered by their index: the order inside a
            cell is not reproducible), where they lie in the workspace, and roitr_knn_workspace_bytes of a few shapes

The package and the tests are taken from the tree the script lies in, so a copy of another commit's tree dumps that commit; the
shapes are read from that tree's test module, the extra ones are spelled out here.  profiles/knn_refactor.txt records the comparison
made when the dispatch became one plan."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch

    import knn_util as U
    import test_knn_fused_gpu as T
    from roitr_amd import _lib as L
    from roitr_amd import pointops
    from test_pointops_gpu import cloud
    out = {}

    # ---- roitr_knnquery_ex
    shapes = []
    for _, use_grid, sizes, take, ns, _, _ in T.CASES:
        shapes.append((use_grid, sizes, take, ns, "gp"))
    shapes += [(True, T.R8, None, 2, "gp"), (False, T.RLB, None, 1, ""), (True, T.R8, None, 17, "p"), (False, T.RLB, None, 17, "p")]
    seen = set()
    for use_grid, sizes, take, ns, engine in shapes:
        key = (use_grid, tuple(sizes), None if take is None else tuple(take), ns, engine)
        if key in seen:
            continue
        seen.add(key)
        n, m = sum(sizes), sum(take) if take else sum(sizes)
        for kind in T.KINDS:
            inp = T.make_inputs(1000 * T.KINDS.index(kind) + 13 * ns + n + 7 * m + int(use_grid), sizes, kind, take)
            g = U.Grid(inp["xyz"], inp["off"], inp["r_nrm"], m_capacity=m, use_grid=use_grid,
                       occupancy=max(6.0, 0.4 * (ns + 1) if ns + 1 >= 35 else 0.0))
            q = g.queries(None if take is None else inp["q_xyz"], inp["q_off"], inp["q_nrm"])
            name = f"ex/{'grid' if use_grid else 'nogrid'}_{len(sizes)}x{sizes[0]}_{n}{'_sub' if take else ''}_k{ns}_{kind}"
            for want in filter(None, (engine, "idgp" if ns > 1 else "id")):
                r = g.query(ns, q, want)
                for c, a in zip("idgp", (r.idx, r.dist2, r.group, r.ppf)):
                    if a is not None:
                        out[f"{name}/{want}/{c}"] = a

    # ---- roitr_knn_within: lane-sized and wave-sized, with and without a grid
    rng = np.random.default_rng(9)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for nc, n in ((6, 5000), (1, 3000)):
        sizes = [n - i for i in range(nc)]
        xyz = np.concatenate([cloud(rng, m) for m in sizes])
        q = np.concatenate([cloud(rng, m) * 1.1 - 0.05 for m in sizes]).astype(np.float32)
        off = dev(np.cumsum(sizes).astype(np.int32))
        for cap in (0.0375, 0.08, 0.5):
            for use_grid in (True, False):
                d2 = pointops.knn_within(dev(xyz), dev(q), off, off, cap * cap * 1.01, use_grid=use_grid)
                out[f"within/{nc}x{n}_cap{cap}_{'grid' if use_grid else 'nogrid'}"] = d2.cpu().numpy()

    # ---- knnquery_cuda_launcher
    rng = np.random.default_rng(4)
    xyz = cloud(rng, 700)
    sel = np.sort(rng.choice(700, 175, replace=False))
    txyz, tnew = dev(xyz), dev(xyz[sel])
    toff, tnoff = dev(np.array([300, 700], np.int32)), dev(np.array([75, 175], np.int32))
    for ns in (17, 70):
        kidx = torch.full((175, ns), -1, dtype=torch.int32, device="cuda")
        kd2 = torch.full((175, ns), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        L.lib().knnquery_cuda_launcher(175, ns, L.ptr(txyz), L.ptr(tnew), L.ptr(toff), L.ptr(tnoff), L.ptr(kidx), L.ptr(kd2))
        torch.cuda.synchronize()
        out[f"legacy/k{ns}/i"], out[f"legacy/k{ns}/d"] = kidx.cpu().numpy(), kd2.cpu().numpy()

    # ---- the grid: sorted points with each cap, where they lie in the workspace, the workspace size
    lib = L.bind(["roitr_knn_sorted_points"])
    for sizes in ([1250, 1247, 900], [9000, 8997, 700]):
        rng = np.random.default_rng(sum(sizes))
        xyz = np.concatenate([cloud(rng, s) for s in sizes])
        n, b = xyz.shape[0], len(sizes)
        g = U.Grid(xyz, np.cumsum(sizes).astype(np.int32), None, m_capacity=n + 37, use_grid=True, occupancy=6.0)
        at = lib.roitr_knn_sorted_points(b, n, n + 37, L.ptr(g.ws)) - g.ws.data_ptr()
        torch.cuda.synchronize()
        # a point's position inside its cell comes from an LDS atomic (grid_build_kernel) and changes from run to run of one build:
        # every cloud's rows are stored ordered by the index they carry (a cloud keeps its own range of rows)
        pts = g.ws[at:at + 16 * n].clone().view(torch.float32).cpu().numpy().reshape(n, 4)
        w, lo = pts[:, 3].copy().view(np.int32), 0
        for s in sizes:
            pts[lo:lo + s] = pts[lo:lo + s][np.argsort(w[lo:lo + s], kind="stable")]
            lo += s
        out[f"sorted/{sizes[0]}/points"] = pts
        out[f"sorted/{sizes[0]}/at"] = np.array([at - (-g.ws.data_ptr() % 16)], np.int64)   # from the 16-byte aligned base
    out["sorted/workspace_bytes"] = np.array([L.lib().roitr_knn_workspace_bytes(b, n, m) for b, n, m in
                                              ((0, 0, 175), (1, 1, 1), (3, 3397, 3434), (8, 40000, 9999), (256, 66000, 70001), (1024, 5120000, 5120000))], np.int64)

    # the 65536-query shapes make 1 GB of rows: an array above 1 MiB is kept as the SHA-256 of its bytes behind its dtype and shape
    # (equal digests = equal bits; stricter than array_equal, to which -0 == +0 and every NaN is the same)
    packed = {}
    for k, a in out.items():
        a = np.ascontiguousarray(a)
        if a.nbytes <= 1 << 20:
            packed[k] = a
        else:
            packed[k + "#sha256"] = np.frombuffer((f"{a.dtype}{a.shape}".encode() + hashlib.sha256(a.tobytes()).digest()), np.uint8)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **packed)
    print(len(packed), "arrays ->", path, f"({sum(k.endswith('#sha256') for k in packed)} as digests)")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    per_op, bad = {}, sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        equal = a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")
        n = per_op.setdefault(k.split("/")[0], [0, 0])
        n[0] += 1
        n[1] += equal
        if not equal:
            bad.append(k)
    for op, (n, eq) in per_op.items():
        print(f"{op}: {eq} of {n} keys bitwise equal")
    if bad:
        sys.exit("NOT EQUAL or missing on one side: " + ", ".join(bad))


if __name__ == "__main__":
    compare(*sys.argv[2:4]) if sys.argv[1] == "--compare" else dump(sys.argv[1])
