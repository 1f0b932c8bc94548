"""Shared by the descriptor-matching tests: a seeded case generator and a float64 restatement of
lib/utils.py:99-156 (matching_descriptors over square_distance) and registration/benchmark_utils.py:42-121 (mutual_selection,
get_inlier_ratio) with the lowest index winning every tie (np.argmax / np.argmin return the first).

DECIDED / UNDECIDED.  The kernel sums D fp32 products per score; the float64 score of the same fp32 inputs differs from any fp32
summation order by at most D * 2^-24 * sum|s_k t_k| * (1 + small) <= E with
    metric 0 (dot):      E_i = D * 2^-23 * |s_i| * max_j |t_j|                  (Cauchy-Schwarz on sum|s_k t_k|)
    metric 1 (sqdist):   E_i = D * 2^-23 * (|s_i| + max_j |t_j|)^2              (the three terms |s|^2, |t|^2, 2 s.t together)
and columns likewise with the roles swapped.  A row is UNDECIDED when its float64 best and second best lie within 2 E: there either
index is a correct answer in fp32.  Decided entries must match the float64 index exactly; on undecided ones the chosen index's
float64 score must lie within 2 E of the best; reported values lie within E of the float64 score of the chosen index.
"""
import hashlib

import numpy as np

N, M = 333, 301
MAX_UNDECIDED = 0.03
# chosen on the float64 restatement alone: the first multiple of 1000 at which seeds 0-5 at D = 64 (the golden's cases) have no
# undecided row or column, so the golden's index sets can be compared exactly
SEED_BASE = 4000


def make_case(seed, D=64, n=N, m=M, scale="unit"):
    """s (n, D), t (m, D) float32: standard normal, two thirds of min(n, m) target rows planted as a permuted source row plus
    0.3 * normal noise, then every row unit-normalised (scale "unit") or multiplied by 2 ("x2").  Points: src_pcd uniform in the
    unit cube, the planted targets at rot src + trans + 5 mm noise, the others uniform; rot / trans a seeded rigid motion."""
    rng = np.random.default_rng(SEED_BASE + seed)
    s = rng.standard_normal((n, D))
    t = rng.standard_normal((m, D))
    k = (2 * min(n, m)) // 3
    src_of = rng.permutation(n)[:k]
    tgt_of = rng.permutation(m)[:k]
    t[tgt_of] = s[src_of] + 0.3 * rng.standard_normal((k, D))
    if scale == "unit":
        s /= np.linalg.norm(s, axis=1, keepdims=True)
        t /= np.linalg.norm(t, axis=1, keepdims=True)
    else:
        s *= 2.0
        t *= 2.0
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    rot = q * np.sign(np.linalg.det(q))
    trans = rng.uniform(-0.5, 0.5, (3, 1))
    src_pcd = rng.uniform(0, 1, (n, 3))
    tgt_pcd = rng.uniform(0, 1, (m, 3)) + 3.0
    tgt_pcd[tgt_of] = src_pcd[src_of] @ rot.T + trans.T + 0.005 * rng.standard_normal((k, 3))
    f = np.float32
    return dict(src_desc=s.astype(f), tgt_desc=t.astype(f), src_pcd=src_pcd.astype(f), tgt_pcd=tgt_pcd.astype(f), rot=rot.astype(f),
                trans=trans.astype(f))


def make_int_case(seed, n, m, D=256, r=3):
    """Descriptors of small integers in [-r, r]: every product, every partial sum, both norms and the distance are exact in fp32 in
    any order (|score| <= 4 D r^2 < 2^24), and ties are everywhere."""
    rng = np.random.default_rng(2000 + seed)
    return dict(src_desc=rng.integers(-r, r + 1, (n, D)).astype(np.float32), tgt_desc=rng.integers(-r, r + 1, (m, D)).astype(np.float32))


KEYS = ("src_desc", "tgt_desc", "src_pcd", "tgt_pcd", "rot", "trans")


def checksum(case):
    h = hashlib.sha256()
    for k in KEYS:
        h.update(np.ascontiguousarray(case[k]).tobytes())
    return h.hexdigest()[:16]


def scores_f64(s, t, metric):
    """metric 0: s . t (larger is better); metric 1: square_distance(normalized=False) in its order, (-2 s.t + |s|^2) + |t|^2,
    clamped at 1e-12 (smaller is better)."""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    dot = s @ t.T
    if metric == 0:
        return dot
    d = (-2.0 * dot + (s ** 2).sum(1)[:, None]) + (t ** 2).sum(1)[None, :]
    return np.maximum(d, 1e-12)


def arg_best(score, metric):
    """(row_idx (n,), col_idx (m,)): the lowest index among equal scores; -1 where the other side is empty."""
    n, m = score.shape
    f = np.argmax if metric == 0 else np.argmin
    row = f(score, axis=1) if m > 0 else np.full(n, -1)
    col = f(score, axis=0) if n > 0 else np.full(m, -1)
    return row.astype(np.int64), col.astype(np.int64)


def select(row, col, mode):
    """The (source, target) matches of mode "row", "col", "mutual", "union", in the order the reference emits them."""
    n, m = len(row), len(col)
    if mode == "row":
        keep = row >= 0
        return np.stack([np.arange(n)[keep], row[keep]], 1).reshape(-1, 2)
    if mode == "col":
        keep = col >= 0
        return np.stack([col[keep], np.arange(m)[keep]], 1).reshape(-1, 2)
    if n == 0 or m == 0:
        return np.zeros((0, 2), np.int64)
    a = np.zeros((n, m), bool)
    b = np.zeros((n, m), bool)
    a[np.arange(n), row] = True
    b[col, np.arange(m)] = True
    mask = (a & b) if mode == "mutual" else (a | b)
    return np.stack(np.nonzero(mask), 1)


def match_f64(s, t, metric):
    sc = scores_f64(s, t, metric)
    row, col = arg_best(sc, metric)
    return dict(score=sc, row_idx=row, col_idx=col)


def bounds(s, t, metric):
    """(E per row, E per column), the module docstring's bound."""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    D = s.shape[1]
    ns, nt = np.linalg.norm(s, axis=1), np.linalg.norm(t, axis=1)
    u = D * 2.0 ** -23
    if metric == 0:
        return u * ns * (nt.max() if len(nt) else 0.0), u * nt * (ns.max() if len(ns) else 0.0)
    return u * (ns + (nt.max() if len(nt) else 0.0)) ** 2, u * (nt + (ns.max() if len(ns) else 0.0)) ** 2


def undecided(score, metric, e_row, e_col):
    """(rows, columns) bool: best and second best within 2 E."""
    sg = score if metric == 1 else -score   # ascending: the best first
    def gap(a):
        if a.shape[1] < 2:
            return np.full(a.shape[0], np.inf)
        p = np.partition(a, 1, axis=1)
        return p[:, 1] - p[:, 0]
    return gap(sg) <= 2 * e_row, gap(sg.T) <= 2 * e_col


def check_against_f64(s, t, metric, row_idx, row_val, col_idx, col_val):
    """The decided / undecided rule of the module docstring; returns (undecided rows, undecided columns) for the report."""
    ref = match_f64(s, t, metric)
    sc = ref["score"]
    n, m = sc.shape
    e_row, e_col = bounds(s, t, metric)
    u_row, u_col = undecided(sc, metric, e_row, e_col)
    print(f"metric {metric} D {np.asarray(s).shape[1]}: undecided rows {int(u_row.sum())} / {n}, columns {int(u_col.sum())} / {m}")
    assert u_row.mean() <= MAX_UNDECIDED and u_col.mean() <= MAX_UNDECIDED, (u_row.sum(), u_col.sum())
    row_idx, col_idx = np.asarray(row_idx, np.int64), np.asarray(col_idx, np.int64)
    assert row_idx.min() >= 0 and row_idx.max() < m and col_idx.min() >= 0 and col_idx.max() < n
    assert np.array_equal(row_idx[~u_row], ref["row_idx"][~u_row])
    assert np.array_equal(col_idx[~u_col], ref["col_idx"][~u_col])
    got_r, got_c = sc[np.arange(n), row_idx], sc[col_idx, np.arange(m)]
    best_r, best_c = sc[np.arange(n), ref["row_idx"]], sc[ref["col_idx"], np.arange(m)]
    assert (np.abs(got_r - best_r) <= 2 * e_row).all() and (np.abs(got_c - best_c) <= 2 * e_col).all()
    assert (np.abs(np.asarray(row_val, np.float64) - got_r) <= e_row).all(), np.abs(np.asarray(row_val, np.float64) - got_r).max()
    assert (np.abs(np.asarray(col_val, np.float64) - got_c) <= e_col).all(), np.abs(np.asarray(col_val, np.float64) - got_c).max()
    return int(u_row.sum()), int(u_col.sum())


def inlier_ratio_f64(case, thr=0.1):
    """registration/benchmark_utils.py:80-121: {'wo' | 'w': (distances, ratio)}; the mean of an empty mutual set is nan."""
    ref = match_f64(case["src_desc"], case["tgt_desc"], 0)
    src = case["src_pcd"].astype(np.float64) @ case["rot"].astype(np.float64).T + case["trans"].astype(np.float64).reshape(1, 3)
    tgt = case["tgt_pcd"].astype(np.float64)
    out = {}
    for key, corr in (("wo", select(ref["row_idx"], ref["col_idx"], "row")), ("w", select(ref["row_idx"], ref["col_idx"], "mutual"))):
        d = np.linalg.norm(src[corr[:, 0]] - tgt[corr[:, 1]], axis=1)
        out[key] = (d, float((d < thr).mean()) if len(d) else float("nan"))
    return out
