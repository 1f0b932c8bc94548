"""The float64 numpy restatement of the FPFH operator defined in include/roitr_pointops.h (above roitr_fpfh_batch), the fixtures of
tests/test_fpfh_cpu.py / test_fpfh_gpu.py and the test that a fixture is DECIDED: no radius test, swap test or bin lies within 1e-9 of
its border, so a last-bit difference between numpy's and the device's sqrt / atan2 / quotient cannot change an integer.

The kNN rows come from oracle.pointops_cpu.knnquery_raw, which is bit-exact with the device kNN (tests/test_pointops_gpu.py)."""
import functools

import numpy as np

from oracle import pointops_cpu as O

BINS = 33
MARGIN = 1e-9


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def clamp_bin(x):
    return np.clip(np.floor(x), 0, 10).astype(np.int64)


def neighbours(xyz, offset, radius, max_nn):
    """(idx (n, max_nn) kNN rows, cand, keep (n, max_nn) bool, dp (n, max_nn, 3), d2 (n, max_nn)): cand = the entries the radius
    test sees (a real slot, not the point itself, among the first max_nn - 1 of those), keep = K(i)."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    offset = np.asarray(offset, np.int32)
    n = xyz.shape[0]
    idx, _ = O.knnquery_raw(max_nn, xyz, xyz, offset, offset, threads=4)
    idx = idx.astype(np.int64)
    cloud = np.searchsorted(offset, np.arange(n), side="right")
    size = np.diff(np.concatenate([[0], offset]))[cloud]
    slot = np.arange(max_nn)[None, :] < size[:, None]
    notself = slot & (idx != np.arange(n)[:, None])
    cand = notself & (np.cumsum(notself, 1) - 1 < max_nn - 1)
    p = xyz.astype(np.float64)
    dp = p[np.where(slot, idx, 0)] - p[:, None, :]
    d2 = (dp[..., 0] * dp[..., 0] + dp[..., 1] * dp[..., 1]) + dp[..., 2] * dp[..., 2]
    keep = cand & (d2 < float(radius) * float(radius))
    return np.where(slot, idx, 0), cand, keep, dp, d2


def pair_features(ni, nj, dp, d2):
    """f (.., 3), the scaled bin operands x (.., 3), and |a1| - |a2| (nan where the swap test is not taken: d == 0)."""
    with np.errstate(all="ignore"):
        d = np.sqrt(d2)
        nz = d != 0
        ds = np.where(nz, d, 1.0)
        a1, a2 = dot3(ni, dp) / ds, dot3(nj, dp) / ds
        swap = np.abs(a1) < np.abs(a2)
        n1 = np.where(swap[..., None], nj, ni)
        n2 = np.where(swap[..., None], ni, nj)
        dps = np.where(swap[..., None], -dp, dp)
        v = cross3(dps, n1)
        vn = np.sqrt(dot3(v, v))
        ok = nz & (vn != 0)
        v = v / np.where(ok, vn, 1.0)[..., None]
        w = cross3(n1, v)
        f2 = np.where(ok, np.where(swap, -a2, a1), 0.0)
        f1 = np.where(ok, dot3(v, n2), 0.0)
        f0 = np.where(ok, np.arctan2(dot3(w, n2), dot3(n1, n2)), 0.0)
        x = np.stack([11.0 * (f0 + np.pi) / (2.0 * np.pi), 11.0 * (f1 + 1.0) / 2.0, 11.0 * (f2 + 1.0) / 2.0], -1)
    return np.stack([f0, f1, f2], -1), x, np.where(nz, np.abs(a1) - np.abs(a2), np.nan)


def fpfh_ref(xyz, normals, offset, radius, max_nn):
    """The operator on finite input: dict(counts (n,33) int32, m (n) int32, spfh, fpfh (n,33) float64, keep, idx, and the smallest
    margins of the radius tests, swap tests and bins)."""
    xyz, normals = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(normals, np.float32)
    n = xyz.shape[0]
    idx, cand, keep, dp, d2 = neighbours(xyz, offset, radius, max_nn)
    nrm = normals.astype(np.float64)
    r2 = float(radius) * float(radius)
    _, x, swap_gap = pair_features(nrm[:, None, :], nrm[idx], dp, d2)
    h = clamp_bin(x)
    counts = np.zeros((n, BINS), np.int64)
    rows = np.broadcast_to(np.arange(n)[:, None], keep.shape)[keep]
    for g in range(3):
        np.add.at(counts, (rows, 11 * g + h[..., g][keep]), 1)
    m = keep.sum(1)
    with np.errstate(all="ignore"):
        spfh = np.where(m[:, None] > 0, counts * (100.0 / np.where(m > 0, m, 1))[:, None], 0.0)
        F, S = np.zeros((n, BINS)), np.zeros((n, 3))
        for k in range(idx.shape[1]):     # row order
            sel = keep[:, k] & (d2[:, k] > 0)
            if not sel.any():
                continue
            val = np.where(sel[:, None], spfh[idx[:, k]] / np.where(sel, d2[:, k], 1.0)[:, None], 0.0)
            F += val
            for b in range(BINS):
                S[:, b // 11] += val[:, b]
        Sg = np.repeat(S, 11, axis=1)
        fpfh = np.where(Sg != 0, F * 100.0 / np.where(Sg != 0, Sg, 1.0), F) + spfh
        radius_margin = np.min(np.abs(d2 - r2)[cand] / np.maximum(d2[cand], 1e-300), initial=np.inf)
        gaps = np.abs(swap_gap[keep])
        swap_margin = np.min(gaps[~np.isnan(gaps)], initial=np.inf)
        xk = x[keep]
        bins_stable = bool((clamp_bin(xk - MARGIN) == clamp_bin(xk + MARGIN)).all())
    return dict(counts=counts.astype(np.int32), m=m.astype(np.int32), spfh=spfh, fpfh=fpfh, keep=keep, idx=idx,
                radius_margin=float(radius_margin), swap_margin=float(swap_margin), bins_stable=bins_stable)


def is_decided(fixture):
    r = reference(fixture) if isinstance(fixture, str) else fpfh_ref(**fixture)
    return r["radius_margin"] > MARGIN and r["swap_margin"] > MARGIN and r["bins_stable"]


# ---------------------------------------------------------------------------------------------------------------- fixtures
def surface(rng, n, normal_noise=0.15):
    """A surface-like cloud over the unit square, z = a smooth bump field plus a little thickness, with noisy unit normals."""
    u = rng.uniform(0, 1, (n, 2))
    z = 0.15 * np.sin(5.0 * u[:, 0]) * np.cos(4.0 * u[:, 1]) + 0.1 * u[:, 0] * u[:, 1] + 0.004 * rng.normal(size=n)
    gx = 0.75 * np.cos(5.0 * u[:, 0]) * np.cos(4.0 * u[:, 1]) + 0.1 * u[:, 1]
    gy = -0.6 * np.sin(5.0 * u[:, 0]) * np.sin(4.0 * u[:, 1]) + 0.1 * u[:, 0]
    nrm = np.stack([-gx, -gy, np.ones(n)], 1) + normal_noise * rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.stack([u[:, 0], u[:, 1], z], 1).astype(np.float32), nrm.astype(np.float32)


def batch(seed, sizes, radius, max_nn, scale=None):
    """Clouds of the given sizes, each a surface of its own; a small cloud is scaled down so that the radius still reaches neighbours."""
    rng = np.random.default_rng(seed)
    pts, nrm = [], []
    for s in sizes:
        p, q = surface(rng, s)
        pts.append(p * np.float32(scale if scale is not None else min(1.0, (max(s, 1) / 300.0) ** 0.5)))
        nrm.append(q)
    return dict(xyz=np.concatenate(pts).reshape(-1, 3), normals=np.concatenate(nrm).reshape(-1, 3),
                offset=np.cumsum(sizes).astype(np.int32), radius=radius, max_nn=max_nn)


def duplicates(seed, max_nn=16):
    """400 points; 30 of them sit on another point, and one point has max_nn + 4 copies (more copies than the kNN row holds: the later
    copies do not find themselves in their own row)."""
    rng = np.random.default_rng(seed)
    f = batch(seed, [400], 0.12, max_nn)
    x = f["xyz"]
    src = rng.choice(200, 30, replace=False)
    x[200:230] = x[src]
    x[300:300 + max_nn + 4] = x[7]
    return f


def lattice(side=12, step=1.0 / 64, radius=2.5 / 64, max_nn=16):
    """A planar lattice with exact coordinates (multiples of 1/64), normal (0, 0, 1), plus three isolated points."""
    g = np.arange(side) * step
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    pts = np.concatenate([np.concatenate([xy, np.zeros((len(xy), 1))], 1), [[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [3.0, 3.0, 0.0]]])
    nrm = np.tile([[0.0, 0.0, 1.0]], (len(pts), 1))
    return dict(xyz=pts.astype(np.float32), normals=nrm.astype(np.float32), offset=np.array([len(pts)], np.int32), radius=radius, max_nn=max_nn)


def end_to_end(seed, n=1500):
    """A non-symmetric cloud with coordinates on a 2^-16 grid, so that the transform of moved() is exact in fp32; the radius cuts
    every row before max_nn - 1 (asserted in test_fpfh_cpu.py), so K(i) is the set of points within the radius, whatever the row order."""
    f = batch(seed, [n], 0.1, 100)
    f["xyz"] = (np.round(f["xyz"].astype(np.float64) * 65536.0) / 65536.0).astype(np.float32)
    return f


FIXTURES = {
    "nn2": lambda: batch(1, [300], 0.2, 2),
    "nn16_cut": lambda: batch(2, [1000], 0.05, 16),          # about 8 points within the radius: it cuts most rows
    "nn16_full": lambda: batch(3, [1000], 0.3, 16),          # the radius cuts nothing: every point keeps 15 neighbours
    "nn65": lambda: batch(4, [1200], 0.13, 65),              # 65 slots: the second lane round; about 60 points within the radius
    "nn100": lambda: batch(5, [2000], 0.125, 100),           # about 98 within the radius
    "sizes16": lambda: batch(6, [1, 2, 15, 0, 16, 17, 300], 0.3, 16),
    "sizes100": lambda: batch(7, [99, 0, 100, 101, 1], 0.5, 100, scale=1.0),
    "ragged": lambda: batch(8, [300, 0, 700, 450], 0.11, 33),
    "dups": lambda: duplicates(9),
    "e2e": lambda: end_to_end(10),
}
DECIDED = sorted(FIXTURES)


@functools.lru_cache(maxsize=None)
def fixture(name):
    f = FIXTURES[name]()
    for v in f.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference(name):
    return fpfh_ref(**fixture(name))


def split(f, c):
    """Cloud c of a batch fixture as a fixture of its own."""
    off = np.concatenate([[0], f["offset"]])
    s, e = int(off[c]), int(off[c + 1])
    return dict(xyz=f["xyz"][s:e], normals=f["normals"][s:e], offset=np.array([e - s], np.int32), radius=f["radius"], max_nn=f["max_nn"])


# the exact transform of the end-to-end test: a coordinate permutation with signs (det +1) and a translation by powers of two
E2E_R = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
E2E_T = np.array([0.5, -0.25, 2.0])


def moved(f):
    """The fixture under the exact transform: every coordinate and normal component is a signed copy, the translation adds exactly."""
    x = (f["xyz"].astype(np.float64) @ E2E_R.T + E2E_T).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) - E2E_T, f["xyz"].astype(np.float64) @ E2E_R.T)
    return dict(f, xyz=x, normals=(f["normals"].astype(np.float64) @ E2E_R.T).astype(np.float32))
