"""Helpers of the NFMR tests (tests/test_nfmr_cpu.py, tests/test_nfmr_gpu.py, tests/golden/make_nfmr_golden.py): a seeded generator
of small non-rigid cases, a float64 restatement of registration/evaluate_fdmatch.py:50-115 with the lowest-index tie rule, and the
test for metric points whose outcome fp32 cannot be held to.

Everything the generator computes is elementwise +, -, * on seeded uniform numbers (no matmul, no transcendental function), so the
float32 inputs are the same bits on every host and the checksums in tests/golden/nfmr_ref.npz hold."""
import hashlib

import numpy as np

RADIUS, THR = 0.1, 0.04
SIDE = 0.8
KEYS = ("src_raw", "src_deformed", "src_corr", "tgt_corr", "metric_index", "rot", "trans")


def _rotation(rng):
    q = rng.uniform(-1.0, 1.0, 4)
    while not 0.1 < float(np.sum(q * q)) <= 1.0:
        q = rng.uniform(-1.0, 1.0, 4)
    w, x, y, z = q
    s = 1.0 / (w * w + x * x + y * y + z * z)   # the rotation of a non-unit quaternion: no square root
    return np.array([[1 - 2 * s * (y * y + z * z), 2 * s * (x * y - z * w), 2 * s * (x * z + y * w)],
                     [2 * s * (x * y + z * w), 1 - 2 * s * (x * x + z * z), 2 * s * (y * z - x * w)],
                     [2 * s * (x * z - y * w), 2 * s * (y * z + x * w), 1 - 2 * s * (x * x + y * y)]])


def _apply(rot, trans, p):
    """p @ rot.T + trans, written out (a BLAS matmul may contract differently from host to host)."""
    return np.stack([p[:, 0] * rot[i, 0] + p[:, 1] * rot[i, 1] + p[:, 2] * rot[i, 2] + trans[i] for i in range(3)], 1)


def _flow(rng, p):
    """A smooth quadratic displacement field, up to ~0.06 m on the cube."""
    a = rng.uniform(-0.05, 0.05, (3, 3))
    b = rng.uniform(-0.06, 0.06, (3, 3))
    u = p / SIDE - 0.5
    return np.stack([a[i, 0] * u[:, 0] + a[i, 1] * u[:, 1] + a[i, 2] * u[:, 2] +
                     b[i, 0] * u[:, 1] * u[:, 2] + b[i, 1] * u[:, 0] * u[:, 2] + b[i, 2] * u[:, 0] * u[:, 1] for i in range(3)], 1)


def make_case(seed, distinct=True, n=2048, c=1500, m=600, outliers=0.2, dup_points=False, repeat_corr=False):
    """One pair: n points in a cube of side 0.8, c correspondences (20 % outliers), m metric points; float32 / int64 arrays.
    distinct: the correspondences' source indices are drawn without (True) or with replacement.  Half of the source points of the
    correspondences are exact points of the deformed cloud (what the engine emits), half carry 2 mm of noise.
    dup_points: 64 points of the deformed cloud are overwritten with copies of lower-index points that correspondences use (the
    argmin must name the lower index).  repeat_corr: every correspondence appears twice (every anchor is a duplicate)."""
    rng = np.random.default_rng(77000 + 10 * seed + (0 if distinct else 1))
    raw = rng.uniform(0.0, SIDE, (n, 3))
    deformed = raw + _flow(rng, raw)
    rot = _rotation(rng)
    trans = rng.uniform(-1.0, 1.0, 3)
    idx = rng.choice(n, size=c, replace=not distinct)
    if dup_points:
        lo = np.sort(idx[:64])
        hi = n - 1 - np.arange(64)
        deformed[hi] = deformed[np.minimum(lo, n - 65)]
    noise = rng.uniform(-0.002, 0.002, (c, 3))
    noise[: c // 2] = 0.0
    src_corr = deformed[idx] + noise
    tgt_corr = _apply(rot, trans, deformed[idx]) + rng.uniform(-0.003, 0.003, (c, 3))
    n_out = int(outliers * c)
    tgt_corr[c - n_out:] = _apply(rot, trans, rng.uniform(0.0, SIDE, (n_out, 3)))
    metric_index = np.sort(rng.choice(n, size=m, replace=False)).astype(np.int64)
    if repeat_corr:
        src_corr, tgt_corr = np.concatenate([src_corr, src_corr]), np.concatenate([tgt_corr, tgt_corr])
    f32 = np.float32
    return dict(src_raw=raw.astype(f32), src_deformed=deformed.astype(f32), src_corr=src_corr.astype(f32), tgt_corr=tgt_corr.astype(f32),
                metric_index=metric_index, rot=rot.astype(f32), trans=trans.astype(f32))


def twelve_cases():
    """Seeds 0-5 with distinct anchors at the default size (the golden cases), then seeds 0-5 with repeated anchors at differing
    sizes: one with duplicate points in the deformed cloud, one with every correspondence repeated."""
    cases = [make_case(s, True) for s in range(6)]
    sizes = ((2048, 1500, 600), (1500, 1200, 450), (2600, 2000, 700), (1024, 900, 300), (2048, 1500, 600), (3000, 1100, 512))
    for s, (n, c, m) in enumerate(sizes):
        cases.append(make_case(s, False, n, c, m, dup_points=s == 1, repeat_corr=s == 2))
    return cases


def truncated(case, c):
    out = dict(case)
    out["src_corr"], out["tgt_corr"] = case["src_corr"][:c], case["tgt_corr"][:c]
    return out


def checksum(case):
    h = hashlib.sha256()
    for k in KEYS:
        h.update(np.ascontiguousarray(case[k]).tobytes())
    return h.hexdigest()[:16]


def nfmr_f64(case, radius=RADIUS, thr=THR):
    """The three steps in float64 on the case's float32 inputs, the lowest index winning every tie (np.argmin returns the first
    minimum, the stable argsort keeps equal distances in index order)."""
    f = {k: np.asarray(case[k], np.float64) for k in KEYS if k != "metric_index"}
    mi = np.asarray(case["metric_index"], np.int64)
    d2 = ((f["src_corr"][:, None, :] - f["src_deformed"][None, :, :]) ** 2).sum(-1)
    anchor_idx = np.argmin(d2, axis=1)
    anchor = f["src_raw"][anchor_idx]
    motion = f["tgt_corr"] - anchor
    p = f["src_raw"][mi]
    out = blend_f64(p, anchor, motion, radius)
    gt = _apply(f["rot"], f["trans"], f["src_deformed"][mi])
    err = np.sqrt((((p + out["flow"]) - gt) ** 2).sum(-1))
    out.update(anchor_idx=anchor_idx, err=err, hits=int((err < thr).sum()), nfmr=float((err < thr).sum()) / max(len(err), 1))
    return out


def blend_f64(query, ref, flow, radius=RADIUS):
    """blend_anchor_motion (knn = 3) in float64, lowest index on ties; also the four nearest distances of every query."""
    query, ref, flow = (np.asarray(x, np.float64) for x in (query, ref, flow))
    dist = np.sqrt(((query[:, None, :] - ref[None, :, :]) ** 2).sum(-1))
    order = np.argsort(dist, axis=1, kind="stable")[:, :4]
    d4 = np.take_along_axis(dist, order, axis=1)
    if d4.shape[1] < 4:
        d4 = np.concatenate([d4, np.full((d4.shape[0], 4 - d4.shape[1]), np.inf)], 1)
    d = d4[:, :3].copy()
    d[d < 1e-10] = 1e-10
    far = d > radius
    d[far] = 1e10
    w = 1.0 / d
    w = w / w.sum(-1, keepdims=True)
    return dict(flow=(flow[order[:, :3]] * w[:, :, None]).sum(1), mask=far.sum(1) < 3, nn_idx=order[:, :3], d4=d4)


def ambiguous(case, res=None, radius=RADIUS, thr=THR, query_only=False):
    """Metric points fp32 cannot be held to: 0 < d4 - d3 < 1e-6 (which anchor is third is a matter of rounding; exact ties among
    duplicate anchors are NOT ambiguous, their fp32 distances are bit-equal and the index rule decides), one of the four nearest
    distances within 1e-6 of the radius, or the error within 1e-5 of the threshold."""
    res = nfmr_f64(case, radius, thr) if res is None else res
    d4 = res["d4"]
    gap = d4[:, 3] - d4[:, 2]
    amb = ((gap > 0) & (gap < 1e-6)) | (np.abs(d4 - radius) < 1e-6).any(1)
    if not query_only:
        amb |= np.abs(res["err"] - thr) < 1e-5
    return amb
