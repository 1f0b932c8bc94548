"""float64 numpy restatement of roitr_fgr_batch (include/roitr_engine.h) and the seeded sets its tests share.

fgr_ref follows the header's definition with full 3 x 6 Jacobians and np.linalg.solve where the kernel carries the 17 distinct sums of
A, g, the objective and sum_omega and solves by L D L^T.  The tuple test runs on the numpy restatement of the RANSAC stream that
tests/test_registration_gpu.py holds against roitr_ransac_samples bit for bit.

A fixture is WELL POSED (well_posed()) when
  * every evaluated step's A has a 2-norm condition number below COND_BOUND = 1e6: the float64 solve then keeps about ten digits, one
    more than the 1e-9 the GPU tests ask of the trace (a singular step, which the restatement finds by an exact zero on the diagonal
    of A, is exempt: it is decided by exact arithmetic on the lattice inputs of that fixture);
  * every edge comparison of every drawn triple, ls * s < lt and lt * s < ls, has a margin of at least 1e-12 relative to the longer
    edge: the decision is then the same under any rounding of the two square roots (their error is ~1e-16 relative);
  * no row is near the inlier radius under the final transform (|d^2 - r^2| < 1e-4 r^2, the margin rule of tests/lgr_util.py), so
    the fp32 count is decided.
On a well-posed fixture every integer output is the same for any arithmetic that meets these bounds, so the GPU tests compare them
exactly.
"""
import numpy as np

import compat_util as CU
import lgr_util as LU
from test_registration_gpu import triples

MAX_DIST, DIVISION, ITERATIONS, MU_EVERY, TUPLE_SCALE, RADIUS = 0.1, 1.4, 128, 4, 0.95, 0.1
NO_ROWS, TOO_FEW, SINGULAR, NO_TUPLES = 1, 2, 4, 8
COND_BOUND, EDGE_MARGIN = 1e6, 1e-12
LDS_ROWS = 1536


# ---------------------------------------------------------------------------------------------------- restatement
def multiplicity(src, tgt, key, seed, tuples, scale=TUPLE_SCALE, chunk=1 << 16):
    """(m int64 (n), accepted triples, the smallest relative margin of an edge comparison) of the tuple test; m is the raw count."""
    n = src.shape[0]
    m, accepted, margin = np.zeros(n, np.int64), 0, np.inf
    if tuples == 0 or n < 3:
        return m, 0, margin
    P, Q, s = src.astype(np.float64), tgt.astype(np.float64), float(np.float32(scale))
    for it0 in range(0, tuples, chunk):
        tr = triples(seed, key, np.arange(it0, min(it0 + chunk, tuples)), n)
        tr = tr[tr[:, 0] >= 0]
        ok = np.ones(len(tr), bool)
        for a, b in ((0, 1), (0, 2), (1, 2)):
            ls = np.sqrt(((P[tr[:, a]] - P[tr[:, b]]) ** 2).sum(1))
            lt = np.sqrt(((Q[tr[:, a]] - Q[tr[:, b]]) ** 2).sum(1))
            ok &= (ls * s < lt) & (lt * s < ls)
            big = np.maximum(np.maximum(ls, lt), 1e-300)
            if len(tr):
                margin = min(margin, float((np.abs(ls * s - lt) / big).min()), float((np.abs(lt * s - ls) / big).min()))
        np.add.at(m, tr[ok].reshape(-1), 1)
        accepted += int(ok.sum())
    return m, accepted, margin


def delta(x):
    """(R (3,3), t (3)) of the step x: Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5 (Open3D's TransformVector6dToMatrix4d)."""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    R = np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                  [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                  [-sb, cb * sa, cb * ca]])
    return R, np.asarray(x[3:6], np.float64)


def sums(S, mu, Pc, Qc, w):
    """(A (6,6), g (6), objective, sum_omega) of one evaluation at the centred state S (3,4) over the used rows."""
    y = Pc @ S[:, :3].T + S[:, 3]
    r = y - Qc
    e = (r * r).sum(1)
    om = w * (mu / (e + mu)) ** 2
    J = np.zeros((len(y), 3, 6))
    J[:, 0, 1], J[:, 0, 2] = y[:, 2], -y[:, 1]           # -[y]x
    J[:, 1, 0], J[:, 1, 2] = -y[:, 2], y[:, 0]
    J[:, 2, 0], J[:, 2, 1] = y[:, 1], -y[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
    A = np.einsum("n,nki,nkj->ij", om, J, J)
    g = np.einsum("n,nki,nk->i", om, J, r)
    return A, g, float((w * mu * e / (e + mu)).sum()), float(om.sum())


def advance(S, mu, A, g, k, md2, division=DIVISION, mu_every=MU_EVERY):
    """The state and scale after step k from its sums, or None when the step is singular (an exact zero or a negative on the diagonal,
    or a solve numpy refuses)."""
    if not np.isfinite(A).all() or (np.diag(A) <= 0).any():
        return None
    try:
        x = np.linalg.solve(A, -g)
    except np.linalg.LinAlgError:
        return None
    R, t = delta(x)
    Sn = np.concatenate([R @ S[:, :3], (R @ S[:, 3] + t)[:, None]], 1)
    if (k + 1) % mu_every == 0 and mu > md2:
        mu = max(mu / division, md2)
    return Sn, mu


def fgr_ref(src, tgt, scores, key=0, seed=0, max_dist=MAX_DIST, division_factor=DIVISION, iterations=ITERATIONS, mu_every=MU_EVERY,
            tuples=0, tuple_scale=TUPLE_SCALE, radius=RADIUS):
    """One pair.  Returns a dict: T (4,4; fp32 values), inliers, near, n_used, tuples_accepted, steps, mu, objective, status,
    multiplicity (as used), trace (iterations, 16), conds (per evaluated non-singular step), margin (tuple edges), cs, ct and T64
    (3,4), the transform before its rounding to fp32."""
    n = src.shape[0]
    out = dict(T=np.eye(4), inliers=0, near=0, n_used=0, tuples_accepted=0, steps=0, mu=0.0, objective=0.0, status=0,
               multiplicity=np.ones(n, np.int64), trace=np.zeros((iterations, 16)), conds=[], margin=np.inf, cs=np.zeros(3), ct=np.zeros(3))
    if n == 0:
        out["status"] = NO_ROWS
        return out
    P, Q = src.astype(np.float64), tgt.astype(np.float64)
    m, acc, out["margin"] = multiplicity(src, tgt, key, seed, tuples, tuple_scale)
    if tuples > 0 and n >= 3 and acc == 0:
        out["status"] |= NO_TUPLES
    if acc > 0:
        out["multiplicity"], out["tuples_accepted"] = m, acc
    sc = np.ones(n) if scores is None else scores.astype(np.float64)
    w = sc * out["multiplicity"]
    used = w > 0
    out["n_used"] = int(used.sum())
    S, cs, ct = np.concatenate([np.eye(3), np.zeros((3, 1))], 1), np.zeros(3), np.zeros(3)
    if out["n_used"] < 3:
        out["status"] |= TOO_FEW
    else:
        cs, ct = P[used].mean(0), Q[used].mean(0)
        Pc, Qc, wu = P[used] - cs, Q[used] - ct, w[used]
        md2 = float(np.float32(max_dist)) ** 2
        mu = max(float(max((Pc * Pc).sum(1).max(), (Qc * Qc).sum(1).max())), md2)
        for k in range(iterations):
            A, g, obj, so = sums(S, mu, Pc, Qc, wu)
            out["trace"][k] = np.concatenate([S.reshape(-1), [mu, obj, so, 1.0]])
            out["objective"] = obj
            nxt = advance(S, mu, A, g, k, md2, division_factor, mu_every)
            if nxt is None:
                out["status"] |= SINGULAR
                break
            out["conds"].append(float(np.linalg.cond(A)))
            S, mu = nxt
            out["steps"] += 1
        out["mu"] = mu
    T64 = np.concatenate([S[:, :3], (ct + S[:, 3] - S[:, :3] @ cs)[:, None]], 1)
    T = T64.astype(np.float32).astype(np.float64)
    c = LU.counts(T, src, tgt, float(np.float32(radius)))
    out["T"][:3] = T
    out.update(inliers=c[0], near=c[1], cs=cs, ct=ct, T64=T64)
    return out


def well_posed(ref):
    """The three rules of the module docstring on an fgr_ref result."""
    return bool(all(c < COND_BOUND for c in ref["conds"]) and ref["margin"] >= EDGE_MARGIN and ref["near"] == 0)


def pose_errors(T, pose):
    """(RRE degrees, RTE metres) of T (4,4) against the planted (R, t)."""
    R, t = pose
    rre = np.degrees(np.arccos(np.clip((np.trace(T[:3, :3].T @ R) - 1) / 2, -1, 1)))
    return float(rre), float(np.linalg.norm(T[:3, 3] - t))


# ---------------------------------------------------------------------------------------------------- fixtures
def line_set(n=12):
    """Rows on a line parallel to the x axis, the targets shifted: the centred y and z are exactly 0 (the mean of equal values is
    exact), so A(0,0) = sum omega (y1^2 + y2^2) is exactly 0 at step 0."""
    x = np.arange(n, dtype=np.float32) * 0.25
    src = np.stack([x, np.full(n, 0.5, np.float32), np.full(n, -1.25, np.float32)], 1)
    tgt = src + np.array([2.0, -0.75, 0.5], np.float32)
    return src, tgt, np.ones(n, np.float32), np.ones(n, bool), (np.eye(3), np.array([2.0, -0.75, 0.5]))


def stretched_set(n=40):
    """Targets = the sources scaled by 2: no edge keeps its length within 0.95, so no triple is accepted."""
    src, _, w, mask, _ = CU.make_set(31, n, 1.0)
    return src, (2.0 * src).astype(np.float32), w, mask, None


def zero_score_set():
    """Half of the outliers carry score 0: they are not used, but a planted row among them still counts as an inlier."""
    src, tgt, w, mask, pose = CU.make_set(32, 300, 0.5)
    w = w.copy()
    w[::3] = 0.0
    return src, tgt, w, mask, pose


def unit_scores(fx):
    """The set with scores None (all 1): make_set's scores are drawn independently of the planted mask, and at 10 % planted they are
    enough to send the objective to another minimum (seed 6 with them: RRE 154.7 degrees; without: 0.095)."""
    return fx[0], fx[1], None, fx[3], fx[4]


def two_used_set():
    src, tgt, w, mask, pose = CU.make_set(33, 10, 1.0)
    w = np.zeros_like(w)
    w[[2, 7]] = 1.0
    return src, tgt, w, mask, pose


# name -> (builder, keyword arguments of the call).  Rows per pair 3, 4, around the block (256) and around the staging capacity (1536),
# and 20 000 (the global path); iterations at the edges of mu_every = 4; tuples around the wave (64) and at 4096 (16 blocks).
CASES = {}
for _n in (3, 4, 255, 256, 257, LDS_ROWS - 1, LDS_ROWS, LDS_ROWS + 1):
    CASES[f"n_{_n}"] = (lambda n=_n: CU.make_set(40 + n, n, 1.0 if n < 255 else 0.5, noise=0.003 if n < 255 else 0.005), dict(iterations=32))
CASES["n_20000"] = (lambda: CU.make_set(41, 20000, 0.5), dict(iterations=16))
for _k in (1, 3, 4, 5):
    CASES[f"it_{_k}"] = (lambda: CU.make_set(42, 300, 0.5), dict(iterations=_k))
CASES["it_128"] = (lambda: CU.make_set(5, 400, 0.30), {})
for _t in (1, 63, 64, 65, 4096):
    CASES[f"tuples_{_t}"] = (lambda: CU.make_set(43, 120, 0.8), dict(tuples=_t, iterations=16, key=7, seed=11))
CASES["ratio_10"] = (lambda: unit_scores(CU.make_set(6, 600, 0.10)), {})      # scores None: the NULL pointer of the operator
CASES["m_1000"] = (lambda: unit_scores(CU.make_set(3, 1000, 0.10)), {})
CASES["no_tuples"] = (stretched_set, dict(tuples=256, iterations=8, key=3, seed=5))
CASES["zero_scores"] = (zero_score_set, dict(iterations=32))
CASES["two_used"] = (two_used_set, dict(iterations=8))
CASES["line"] = (line_set, dict(iterations=8))
CASES["other_params"] = (lambda: CU.make_set(44, 500, 0.4), dict(iterations=48, mu_every=3, division_factor=2.0, max_dist=0.05, radius=0.05))
GPU_CASES = sorted(CASES)
# The tuple count at which the restatement, under the project's stream (key 0, seed 0, unit scores), recovers the pose of the 5 % set:
# the first of 65 536, 131 072, ... that does (tests/test_fgr_cpu.py repeats the search; scripts/bench_fgr.py runs the same count).
# Measured: 65 536 drawn, 39 accepted: RRE 160.6 degrees (fails); 131 072 drawn, 84 accepted: RRE 0.064 degrees, RTE 0.0019 m.
TUPLES_05 = 131072

_cache = {}


def fixture(name):
    """(src, tgt, scores, mask, pose), kw"""
    if name not in _cache:
        build, kw = CASES[name]
        _cache[name] = (build(), dict(kw))
    return _cache[name]


def reference(name):
    """fgr_ref of a fixture, computed once per process and never changed."""
    key = ("ref", name)
    if key not in _cache:
        (src, tgt, w, _, _), kw = fixture(name)
        _cache[key] = fgr_ref(src, tgt, w, **kw)
    return _cache[key]
