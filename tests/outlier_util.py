"""The float64 numpy restatement of the outlier filters defined in include/roitr_pointops.h (above roitr_remove_statistical_outlier), the
fixtures of tests/test_outlier_cpu.py / test_outlier_gpu.py / test_outlier_tester_gpu.py, and the test that a fixture is DECIDED.

The kNN rows come from oracle.pointops_cpu.knnquery_raw (a float32 brute force with the library's tie rule, bit-exact with the device
kNN: tests/test_pointops_gpu.py), as in tests/fpfh_util.py.  Every sum that the definition orders is taken with np.cumsum(...)[-1] or a
loop: np.add.reduce is pairwise.

Decided (statistical filter; the radius filter has no square root, its arithmetic must be bit-equal and nothing can be undecided):
  * no mean_i of a cloud with std > 0 lies within 1e-9 thr of thr, so a last-bit difference between numpy's and the device's sqrt
    cannot change a flag.  A cloud of one point has a NaN threshold and keeps nothing whatever the bits.  A cloud of two points has
    thr == mean_i by construction: both means are the half of the same sqrt(d2) (dp and -dp have the same squares), S1 = 2 mean is
    exact, cloud_mean == mean, S2 == 0 -- on any correctly or incorrectly rounded sqrt alike -- so it keeps nothing and counts as
    decided.  Any other cloud with std == 0 is undecided.
  * no fp32 kNN decision that changes the k-set sits on a tie broken by rounding: in float64 no row entry is farther than a point the
    row leaves out (equal is an exact tie of the coordinates: duplicates, lattice neighbours; the index rule decides it in any
    precision)."""
import functools

import numpy as np

from oracle import pointops_cpu as O

MARGIN = 1e-9
SEG = 256
NONFINITE = 1


def seq_sum(a):
    """The sum of a, one term after the other from +0."""
    return float(np.cumsum(np.concatenate([[0.0], a]))[-1])


def cloud_sum(terms):
    """The definition's order: segments of 256 in input order, each summed sequentially, then the segment sums sequentially."""
    return seq_sum(np.array([seq_sum(terms[s:s + SEG]) for s in range(0, len(terms), SEG)], np.float64))


def d2_of(p, i, j):
    dp = p[j] - p[i]
    return (dp[..., 0] * dp[..., 0] + dp[..., 1] * dp[..., 1]) + dp[..., 2] * dp[..., 2]


def _prepare(xyz, offset):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    offset = np.asarray(offset, np.int32)
    ends = np.concatenate([[0], offset]).astype(np.int64)
    fin = np.isfinite(xyz).all(1)
    status = np.array([0 if fin[ends[c]:ends[c + 1]].all() else NONFINITE for c in range(len(offset))], np.int32)
    clean = np.where(fin[:, None], xyz, np.float32(0))
    return xyz, offset, ends, status, clean


def _finish(keep, ends):
    index = np.flatnonzero(keep).astype(np.int32)
    new_offset = np.array([int(keep[:e].sum()) for e in ends[1:]], np.int32)
    return index, new_offset


def statistical_ref(xyz, offset, nb_neighbors=20, std_ratio=2.0, **_):
    """dict(keep (n) bool, index, new_offset, status, mean (n) float64, stats (b,3), idx (n,k) the kNN rows, thr_margin: the smallest
    |mean_i - thr| / |thr| over the clouds with std > 0, std_zero_ok: every cloud with std == 0 has at most two points)."""
    xyz, offset, ends, status, clean = _prepare(xyz, offset)
    n, k = xyz.shape[0], int(nb_neighbors)
    idx = np.zeros((n, k), np.int64)
    if n:
        idx = O.knnquery_raw(k, clean, clean, offset, offset, threads=4)[0].astype(np.int64)
    p = xyz.astype(np.float64)
    mean, keep, stats = np.zeros(n), np.zeros(n, bool), np.zeros((len(offset), 3))
    thr_margin, std_zero_ok = np.inf, True
    for c in range(len(offset)):
        s, e = int(ends[c]), int(ends[c + 1])
        if e == s or status[c]:
            continue
        v = min(k, e - s)
        acc = np.zeros(e - s)
        with np.errstate(all="ignore"):
            for slot in range(v):      # row order
                acc = acc + np.sqrt(d2_of(p, np.arange(s, e), idx[s:e, slot]))
            m = acc / float(v)
            mean[s:e] = m
            V = float(e - s)
            cloud_mean = cloud_sum(np.where(m > 0, m, 0.0)) / V
            s2 = cloud_sum(np.where(m > 0, (m - cloud_mean) * (m - cloud_mean), 0.0))
            std = np.sqrt(np.float64(s2) / np.float64(V - 1.0))
            thr = cloud_mean + float(std_ratio) * std
            keep[s:e] = (m > 0) & (m < thr)
            stats[c] = cloud_mean, std, thr
            if std > 0 and (m > 0).any():
                thr_margin = min(thr_margin, float(np.min(np.abs(m[m > 0] - thr)) / abs(thr)))
            elif std == 0 and e - s > 2:
                std_zero_ok = False
    index, new_offset = _finish(keep, ends)
    return dict(keep=keep, index=index, new_offset=new_offset, status=status, mean=mean, stats=stats, idx=idx, thr_margin=thr_margin,
                std_zero_ok=std_zero_ok)


def pair_d2(p, s, e, rows):
    """float64 d2 of the points `rows` of cloud [s, e) against the whole cloud: (len(rows), e - s), the definition's arithmetic."""
    dp = p[None, s:e, :] - p[rows, None, :]
    return (dp[..., 0] * dp[..., 0] + dp[..., 1] * dp[..., 1]) + dp[..., 2] * dp[..., 2]


def radius_ref(xyz, offset, nb_points=16, radius=0.05, **_):
    """dict(keep, index, new_offset, status, count (n) int32)."""
    xyz, offset, ends, status, _ = _prepare(xyz, offset)
    n = xyz.shape[0]
    p = xyz.astype(np.float64)
    r2 = float(radius) * float(radius)
    count = np.zeros(n, np.int32)
    for c in range(len(offset)):
        s, e = int(ends[c]), int(ends[c + 1])
        if status[c]:
            continue
        for lo in range(s, e, 512):
            rows = np.arange(lo, min(lo + 512, e))
            count[rows] = (pair_d2(p, s, e, rows) < r2).sum(1)
    keep = count > int(nb_points)
    index, new_offset = _finish(keep, ends)
    return dict(keep=keep, index=index, new_offset=new_offset, status=status, count=count)


def knn_set_decided(xyz, offset, idx, status=None):
    """In float64 no entry of a point's row is farther than a point of its cloud that the row leaves out."""
    xyz, offset, ends, st, clean = _prepare(xyz, offset)
    p = clean.astype(np.float64)
    k = idx.shape[1]
    for c in range(len(offset)):
        s, e = int(ends[c]), int(ends[c + 1])
        if e - s <= k or st[c]:
            continue
        for lo in range(s, e, 512):
            rows = np.arange(lo, min(lo + 512, e))
            D = pair_d2(p, s, e, rows)
            member = np.zeros(D.shape, bool)
            np.put_along_axis(member, idx[rows] - s, True, 1)
            if member.sum(1).min() != k:
                return False
            if (np.where(member, D, -np.inf).max(1) > np.where(member, np.inf, D).min(1)).any():
                return False
    return True


def is_decided(fixture):
    f = fixture_of(fixture)
    r = reference(fixture, "statistical") if isinstance(fixture, str) else statistical_ref(**f)
    return r["thr_margin"] > MARGIN and r["std_zero_ok"] and knn_set_decided(f["xyz"], f["offset"], r["idx"])


# ---------------------------------------------------------------------------------------------------------------- fixtures
def surface(rng, n):
    """A surface-like cloud over the unit square: z = a smooth bump field plus a little thickness."""
    u = rng.uniform(0, 1, (n, 2))
    z = 0.15 * np.sin(5.0 * u[:, 0]) * np.cos(4.0 * u[:, 1]) + 0.1 * u[:, 0] * u[:, 1] + 0.004 * rng.normal(size=n)
    return np.stack([u[:, 0], u[:, 1], z], 1).astype(np.float32)


def planted(rng, pts, share):
    """`pts` with round(share * n) uniform points of its bounding box appended (the flying pixels)."""
    m = int(round(share * len(pts)))
    lo, hi = pts.min(0), pts.max(0)
    return np.concatenate([pts, rng.uniform(lo, hi, (m, 3)).astype(np.float32)])


def params(**kw):
    return dict(dict(nb_neighbors=20, std_ratio=2.0, nb_points=4, radius=0.1), **kw)


def batch(seed, sizes, **kw):
    """Clouds of the given sizes, each a surface of its own; a small cloud is scaled down so that the radius still reaches neighbours."""
    rng = np.random.default_rng(seed)
    pts = [surface(rng, s) * np.float32(min(1.0, (max(s, 1) / 300.0) ** 0.5)) for s in sizes]
    return dict(xyz=np.concatenate(pts).reshape(-1, 3), offset=np.cumsum(sizes).astype(np.int32), **params(**kw))


def duplicates(seed, k=20):
    """400 points; 30 of them sit on another point, and one point has k + 4 copies: their rows hold copies only, mean == 0 -- counted in
    V, absent from the sums, removed."""
    rng = np.random.default_rng(seed)
    f = batch(seed, [400], nb_neighbors=k)
    x = f["xyz"]
    x[200:230] = x[rng.choice(200, 30, replace=False)]
    x[300:300 + k + 4] = x[7]
    return f


def lattice(side=12, step=1.0 / 64, isolated=True, **kw):
    """A planar lattice with exact coordinates (multiples of 1/64), plus three isolated points.  radius == 2 / 64 exactly: the lattice
    points at distance 2 / 64 fail the strict test, an interior point counts 9, an edge point 6, a corner 4, an isolated point 1."""
    g = np.arange(side) * step
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    pts = np.concatenate([xy, np.zeros((len(xy), 1))], 1)
    if isolated:
        pts = np.concatenate([pts, [[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [3.0, 3.0, 0.0]]])
    return dict(xyz=pts.astype(np.float32), offset=np.array([len(pts)], np.int32), **params(**dict(dict(radius=2.0 / 64, nb_points=5), **kw)))


def scan(seed, n=3000, share=0.05, **kw):
    """n surface points plus `share` planted uniform points of the bounding box."""
    rng = np.random.default_rng(seed)
    pts = planted(rng, surface(rng, n), share)
    return dict(xyz=pts, offset=np.array([len(pts)], np.int32), **params(**dict(dict(radius=0.05, nb_points=8), **kw)))


def nonfinite(seed):
    """Three clouds; the first holds a NaN, the last an inf, the middle one is clean."""
    f = batch(seed, [300, 200, 250])
    f["xyz"][17, 1] = np.nan
    f["xyz"][500 + 240, 2] = np.inf
    return f


SIZES = [0, 1, 2, 5, 19, 20, 21, 64, 257, 700]   # empty, NaN threshold, padding slots, exactly k, a wave boundary, the 256 / 257 segment boundary
FIXTURES = {
    "sizes": lambda: batch(11, SIZES),
    "dups": lambda: duplicates(12),
    "lattice": lambda: lattice(),
    "surface": lambda: scan(13),
    "nonfinite": lambda: nonfinite(14),
}
NAMES = sorted(FIXTURES)


@functools.lru_cache(maxsize=None)
def fixture(name):
    f = FIXTURES[name]()
    for v in f.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return f


def fixture_of(f):
    return fixture(f) if isinstance(f, str) else f


@functools.lru_cache(maxsize=None)
def reference(name, method):
    return (statistical_ref if method == "statistical" else radius_ref)(**fixture(name))


def split(f, c):
    """Cloud c of a batch fixture as a fixture of its own."""
    off = np.concatenate([[0], f["offset"]])
    s, e = int(off[c]), int(off[c + 1])
    return dict(f, xyz=f["xyz"][s:e], offset=np.array([e - s], np.int32))


def reorder(f, order):
    """The clouds of a batch fixture in another order."""
    parts = [split(f, c) for c in order]
    return dict(f, xyz=np.concatenate([q["xyz"] for q in parts]).reshape(-1, 3),
                offset=np.cumsum([q["xyz"].shape[0] for q in parts]).astype(np.int32))
