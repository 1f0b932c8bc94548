"""float64 numpy restatement of roitr_compat_batch (include/roitr_engine.h) and the seeded sets its tests share.

compat_ref follows the header's five stages and returns every one of them.  The solver, the residual, the near-row rule and
well_posed are those of tests/lgr_util.py (SVD Kabsch where the kernels use Horn's quaternion form).  The seed rows of C . C are one
float32 matmul: the entries are counts below 2^24, exact in fp32.

A fixture is DECIDED (decided()) when
  * every |d_ab - compat_dist| over the selected pairs a != b is at least 1e-9: the float64 comparison of the graph stage gives the
    same bit under any rounding of the two square roots (their error is ~1e-15 at these extents);
  * the inlier margin rule of lgr_util holds: no near row (|d^2 - r^2| < 1e-4 r^2) at any global step, none for a hypothesis whose
    count could reach the maximum;
  * the scores at the truncation threshold are distinct (unless the fixture is about that tie: ties=True).
On a decided fixture every integer output is the same for any arithmetic that meets the fp32 bounds, so the GPU tests compare them
exactly.  A hypothesis whose member set is not well_posed (lgr_util) is left out of the by-value comparison of hyp_T and hyp_counts
only: at most 5 % of a fixture's valid hypotheses and never the winner (tests/test_compat_cpu.py asserts this for every fixture).
"""
import numpy as np

import lgr_util as LU

COMPAT_DIST, RADIUS, MAX_SEEDS, K, STEPS = 0.1, 0.1, 64, 20, 5
NO_ROWS, NO_HYPOTHESIS, EMPTY_REFIT, TRUNCATED = 1, 2, 4, 8
MARGIN = 1e-9


# ---------------------------------------------------------------------------------------------------- restatement
def select(n, scores, max_rows):
    """The selected rows, ascending: all, or the max_rows of largest (score, -row)."""
    if n <= max_rows:
        return np.arange(n)
    if scores is None:
        return np.arange(max_rows)
    order = np.lexsort((np.arange(n), -scores.astype(np.float64)))      # by score descending, then row ascending
    return np.sort(order[:max_rows])


def lengths(p):
    d = p[:, None, :] - p[None, :, :]
    return np.sqrt((d * d).sum(2))


def graph(P, Q, compat_dist):
    """(C bool (m,m), the smallest distance of an off-diagonal |d - compat_dist| from 0)"""
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    d = np.abs(lengths(P) - lengths(Q))
    C = d < float(np.float32(compat_dist))
    np.fill_diagonal(C, False)
    off = np.abs(d - float(np.float32(compat_dist)))
    np.fill_diagonal(off, np.inf)
    return C, (float(off.min()) if C.shape[0] > 1 else np.inf)


def graph_rows(P, Q, rows, compat_dist, chunk=128):
    """Rows `rows` of C without the whole matrix (for sets too large to restate in full): (C_rows bool (len(rows), m), margin)."""
    P, Q, thr = P.astype(np.float64), Q.astype(np.float64), float(np.float32(compat_dist))
    out, margin = np.zeros((len(rows), len(P)), bool), np.inf
    for i in range(0, len(rows), chunk):
        r = np.asarray(rows[i:i + chunk])
        dp = np.sqrt(((P[r][:, None, :] - P[None, :, :]) ** 2).sum(2))
        dq = np.sqrt(((Q[r][:, None, :] - Q[None, :, :]) ** 2).sum(2))
        d = np.abs(dp - dq)
        off = np.abs(d - thr)
        off[np.arange(len(r)), r] = np.inf
        margin = min(margin, float(off.min()))
        c = d < thr
        c[np.arange(len(r)), r] = False
        out[i:i + chunk] = c
    return out, margin


def common_neighbours(C, seeds):
    """c (S, m): c[i, b] = C[s_i, b] * sum_x C[s_i, x] C[b, x]"""
    Cf = C.astype(np.float32)
    return (C[seeds] * (Cf[seeds] @ Cf)).astype(np.int64)


def members_of(c_row, seed, k):
    """(members ascending, weights) of one seed; fewer than 3 members make no hypothesis."""
    cand = np.flatnonzero(c_row > 0)
    cand = cand[np.lexsort((cand, -c_row[cand]))][:k - 1]                # by c descending, then index ascending
    mem = np.sort(np.concatenate([cand, [seed]]))
    w = c_row[mem].astype(np.float32)
    w[mem == seed] = np.float32(c_row.max())
    return mem, w


def compat_ref(src, tgt, scores, compat_dist=COMPAT_DIST, radius=RADIUS, max_rows=None, max_seeds=MAX_SEEDS, k=K, steps=STEPS):
    """One pair.  Returns a dict with every stage: sel, C, deg, margin, seeds (selected indices by rank), seed_rows, members (list per
    rank: local rows ascending; fewer than 3 when invalid), hyp_T (S,3,4; zeros when invalid), hyp_counts (-1 when invalid), hyp_near,
    hyp_well (well_posed of the member set), best (rank), best_seed_row, hypotheses (valid), local_inliers, T (4,4), inliers, mask,
    status, step_near and decided_counts (the inlier margin rule)."""
    n = src.shape[0]
    max_rows = max(3, min(2048, n)) if max_rows is None else max_rows
    w_all = np.ones(n, np.float32) if scores is None else scores
    out = dict(sel=np.zeros(0, int), C=np.zeros((0, 0), bool), deg=np.zeros(0, int), margin=np.inf, seeds=np.zeros(0, int),
               seed_rows=[], members=[], hyp_T=np.zeros((0, 3, 4)), hyp_counts=[], hyp_near=[], hyp_well=[], best=-1, best_seed_row=-1,
               hypotheses=0, local_inliers=0, T=np.eye(4), inliers=0, mask=np.zeros(n, bool), status=0, step_near=[],
               decided_counts=True)
    if n == 0:
        out["status"] = NO_ROWS
        return out
    if n > max_rows:
        out["status"] |= TRUNCATED
    sel = select(n, scores, max_rows)
    m = len(sel)
    P, Q = src[sel], tgt[sel]
    C, margin = graph(P, Q, compat_dist)
    deg = C.sum(1)
    S = min(max_seeds, m)
    seeds = np.lexsort((np.arange(m), -deg))[:S]                          # by degree descending, then index ascending
    c = common_neighbours(C, seeds)
    out.update(sel=sel, C=C, deg=deg, margin=margin, seeds=seeds, seed_rows=[int(sel[a]) for a in seeds], c=c)
    I = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    Ts, cnt, near, well, mems, stats = [], [], [], [], [], []
    for i, s in enumerate(seeds):
        mem, w = members_of(c[i], int(s), k)
        if len(mem) < 3:
            mems.append([int(sel[a]) for a in mem]); Ts.append(np.zeros((3, 4))); cnt.append(-1); near.append(0); well.append(False); stats.append(None)
            continue
        T = LU.solve(P[mem], Q[mem], w)
        st = LU.counts(T, src, tgt, radius)
        mems.append([int(sel[a]) for a in mem]); Ts.append(T); cnt.append(st[0]); near.append(st[1]); stats.append(st)
        well.append(bool(len(mem) >= 3 and LU.well_posed(P[mem], Q[mem], w)))
    out.update(members=mems, hyp_T=np.stack(Ts), hyp_counts=cnt, hyp_near=near, hyp_well=well)
    valid = [i for i, x in enumerate(cnt) if x >= 0]
    out["hypotheses"] = len(valid)
    T, alive = I, True
    if valid:
        best = max(valid, key=lambda i: (cnt[i], -i))                     # the largest count, the lower rank at equal counts
        top_lower = max(stats[i][2] for i in valid)
        out["decided_counts"] = all(stats[i][1] == 0 for i in valid if stats[i][3] >= top_lower)
        out["best"], out["best_seed_row"], out["local_inliers"], T = best, int(sel[seeds[best]]), cnt[best], Ts[best]
    else:
        out["status"] |= NO_HYPOTHESIS
        T0 = LU.solve(src, tgt, w_all)
        alive = T0 is not None
        if alive:
            T = T0
            out["local_inliers"] = LU.counts(T, src, tgt, radius)[0]
    for _ in range(steps):
        if not alive:
            break
        st = LU.counts(T, src, tgt, radius)
        out["step_near"].append(st[1])
        Tn = LU.solve(src, tgt, w_all * st[4])
        alive = Tn is not None
        T = Tn if alive else T
    if not alive:
        out["status"] |= EMPTY_REFIT
    st = LU.counts(T, src, tgt, radius)
    out["step_near"].append(st[1])
    out["decided_counts"] = out["decided_counts"] and not any(out["step_near"])
    out["T"][:3] = T
    out["inliers"], out["mask"] = st[0], st[4]
    return out


def decided(ref, scores=None, max_rows=None, ties=False):
    """The three rules of the module docstring on a compat_ref result."""
    ok = ref["margin"] >= MARGIN and ref["decided_counts"]
    if ok and scores is not None and max_rows is not None and len(scores) > max_rows and not ties:
        srt = np.sort(scores.astype(np.float64))[::-1]
        ok = srt[max_rows - 1] != srt[max_rows]                          # the last row taken and the first one left differ
    return bool(ok)


def excluded(ref):
    """Ranks left out of the by-value comparison: valid hypotheses whose member set is not well_posed."""
    return [i for i, c in enumerate(ref["hyp_counts"]) if c >= 0 and not ref["hyp_well"][i]]


def within_cap(ref):
    ex = excluded(ref)
    return len(ex) <= 0.05 * max(ref["hypotheses"], 1) and ref["best"] not in ex


# ---------------------------------------------------------------------------------------------------- generator
def make_set(seed, n, ratio, noise=0.005, extent=3.0):
    """n correspondences, round(ratio n) of them planted (tgt = R s + t + noise), the others with a target drawn in the same box, in a
    random order.  Returns src, tgt (fp32), scores, the planted mask and the pose."""
    rng = np.random.default_rng(seed)
    R, t = LU.random_pose(rng)
    src = rng.uniform(-extent / 2, extent / 2, (n, 3)).astype(np.float32)
    tgt = src.astype(np.float64) @ R.T + t
    mask = np.zeros(n, bool)
    mask[rng.permutation(n)[:int(round(ratio * n))]] = True
    tgt[mask] += noise * rng.normal(size=(int(mask.sum()), 3))
    tgt[~mask] = rng.uniform(-extent / 2, extent / 2, (int((~mask).sum()), 3)) @ R.T + t
    scores = rng.permutation(n).astype(np.float32) / n * 0.8 + 0.2     # distinct
    return src, tgt.astype(np.float32), scores.astype(np.float32), mask, (R, t)


def lattice_set(seed, n_in=40, n_out=24, side=6):
    """An exact integer lattice: planted rows map under a lattice rotation plus an integer shift (every planted d_ab is exactly 0, many
    degrees and many c_b are equal), the others to another lattice point.  Distinct source points."""
    rng = np.random.default_rng(seed)
    pts = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    src = pts[rng.permutation(len(pts))[:n_in + n_out]].astype(np.float64)
    R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], float)
    t = np.array([3.0, -2.0, 5.0])
    tgt = src @ R.T + t
    mask = np.zeros(n_in + n_out, bool)
    mask[rng.permutation(n_in + n_out)[:n_in]] = True
    tgt[~mask] = pts[rng.integers(0, len(pts), int((~mask).sum()))] @ R.T + t + np.array([0.0, 0.0, 9.0])
    scores = np.ones(n_in + n_out, np.float32)
    return src.astype(np.float32), tgt.astype(np.float32), scores, mask, (R, t)


def incompatible_set(n=12):
    """Rows that are mutually incompatible: the targets are the sources scaled by 3, so every |d_ab| is twice a source distance, and
    the source points keep more than compat_dist between them."""
    rng = np.random.default_rng(21)
    while True:
        src = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
        d = lengths(src.astype(np.float64)) + 9 * np.eye(n)
        if d.min() > 0.2:
            break
    tgt = (3.0 * src).astype(np.float32)
    return src, tgt, np.linspace(0.5, 1.0, n).astype(np.float32), np.zeros(n, bool), None


# name -> (builder, keyword arguments of the call).  Ratios 30 / 10 / 5 %; m around the 64-bit word, the 16-word line, the 512-point
# tile and the 32-row block; a truncated pair; k and max_seeds at their borders.
def _ratio_for(m):
    return 0.3 if m >= 63 else 1.0


CASES = {}
for _m in (3, 4, 63, 64, 65, 127, 128, 129, 257):
    CASES[f"m_{_m}"] = (lambda m=_m: make_set(10 + m, m, _ratio_for(m), noise=0.003 if m < 63 else 0.005), {})
CASES["m_1000"] = (lambda: make_set(3, 1000, 0.1), {})
CASES["ratio_30"] = (lambda: make_set(5, 400, 0.30), {})
CASES["ratio_10"] = (lambda: make_set(6, 600, 0.10), {})
CASES["ratio_05"] = (lambda: make_set(7, 800, 0.05), {})
CASES["trunc_2049"] = (lambda: make_set(8, 2049, 0.1), dict(max_rows=2048))
CASES["trunc_300"] = (lambda: make_set(9, 300, 0.3), dict(max_rows=200))
CASES["k_3"] = (lambda: make_set(11, 200, 0.3), dict(k=3))
CASES["k_64"] = (lambda: make_set(12, 300, 0.4), dict(k=64))
CASES["k_over"] = (lambda: make_set(13, 80, 0.2), dict(k=64))            # 16 planted rows: fewer members than k
CASES["seeds_1"] = (lambda: make_set(14, 200, 0.3), dict(max_seeds=1))
CASES["seeds_over"] = (lambda: make_set(15, 100, 0.3), dict(max_seeds=128))   # more seeds than rows
CASES["seeds_1024"] = (lambda: make_set(16, 1100, 0.2), dict(max_seeds=1024, k=8))
CASES["lattice"] = (lambda: lattice_set(1), dict(compat_dist=0.05, radius=0.05))
CASES["lattice_k5"] = (lambda: lattice_set(2, 30, 30), dict(compat_dist=0.05, radius=0.05, k=5, max_seeds=16))
CASES["incompatible"] = (incompatible_set, {})
CASES["two_rows"] = (lambda: tuple(x[:2] if isinstance(x, np.ndarray) else x for x in make_set(17, 10, 1.0)), {})
PLANTED = [n for n in CASES if n.startswith(("m_", "ratio_", "trunc_", "k_", "seeds_")) and n not in ("m_3", "m_4")]

_cache = {}


def fixture(name):
    """(src, tgt, scores, mask, pose), kw"""
    if name not in _cache:
        build, kw = CASES[name]
        _cache[name] = (build(), kw)
    return _cache[name]


def reference(name):
    """compat_ref of a fixture, computed once per process and never changed."""
    key = ("ref", name)
    if key not in _cache:
        (src, tgt, w, _, _), kw = fixture(name)
        _cache[key] = compat_ref(src, tgt, w, **kw)
    return _cache[key]
