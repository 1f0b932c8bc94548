"""float64 numpy restatement of roitr_gicp_batch (include/roitr_pointops.h) and the seeded fixtures its tests share.

Evaluation, loop and convergence rule are icp_util's (the operator shares them with roitr_icp_batch).  The update is restated
independently of the kernel's form: M^-1 by np.linalg.inv per point (the kernel: six cofactors over the determinant), the sums by
einsum over the full 3 x 6 Jacobians (the kernel: the block structure of J).  The fixtures are icp_util.make_fixture's recipe, seeds
and sizes, kept with the source surface normals rotated into the source frame.

DECIDED is icp_util's notion: no near tie, no near-radius match, no near convergence decision, cond(A) < 1e6 at every evaluated step.
"""
import numpy as np

import icp_util as U
import pairgt_util as P
from icp_util import CONVERGED, EMPTY, NONFINITE, SINGULAR, TOO_FEW, as_state, evaluate, ldl_solve, surface, ulp_perturb, vector_to_matrix  # noqa: F401

EPSILON = 1e-3
MAX_DIST, ITERATIONS, REL = U.MAX_DIST, U.ITERATIONS, U.REL


# ---------------------------------------------------------------------------------------------------- restatement
def unit(n):
    """n / |n| in float64 on the fp32 values; rows of squared length exactly 0 stay 0."""
    n = np.asarray(n, np.float32).astype(np.float64).reshape(-1, 3)
    l2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    out = np.zeros_like(n)
    ok = l2 != 0
    out[ok] = n[ok] / np.sqrt(l2[ok])[:, None]
    return out


def cofactor_inverse(M):
    """The header's formula for the inverse of symmetric 3 x 3 matrices M (k,3,3), from the upper triangle."""
    m00, m01, m02, m11, m12, m22 = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]
    c00, c01, c02 = m11 * m22 - m12 * m12, m12 * m02 - m01 * m22, m01 * m12 - m11 * m02
    c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
    det = (m00 * c00 + m01 * c01) + m02 * c02
    W = np.stack([np.stack([c00, c01, c02], 1), np.stack([c01, c11, c12], 1), np.stack([c02, c12, c22], 1)], 1)
    return W / det[:, None, None]


def plane_metric(a, b, eps):
    """M = 2I - (1 - eps)(a a^T + b b^T) for unit (or zero) rows a, b: (k,3,3)."""
    return 2 * np.eye(3)[None] - (1 - eps) * (a[:, :, None] * a[:, None, :] + b[:, :, None] * b[:, None, :])


def gicp_system(T, src, tgt, src_normals, tgt_normals, nn, eps=EPSILON, exact_state=False):
    """(A (6,6), g (6), objective = sum d^T M^-1 d / n_corr) of the step under T on the matches nn.  exact_state: T is taken as the
    float64 matrix it is, not rounded to the fp32 state of the operator (for convergence studies below the fp32 floor)."""
    hit = nn >= 0
    if exact_state:
        T = np.asarray(T, np.float64).reshape(-1, 4)[:3]
        pm = np.asarray(src, np.float32).astype(np.float64)[hit] @ T[:, :3].T + T[:, 3]
    else:
        T = as_state(T)
        pm = P.move(np.asarray(src, np.float32)[hit], T[:, :3], T[:, 3])
    q = np.asarray(tgt, np.float32).astype(np.float64)[nn[hit]]
    a = unit(src_normals)[hit] @ T[:, :3].T
    b = unit(tgt_normals)[nn[hit]]
    d = pm - q
    Mi = np.linalg.inv(plane_metric(a, b, eps)) if len(pm) else np.zeros((0, 3, 3))
    J = np.zeros((len(pm), 3, 6))
    J[:, 0, 1], J[:, 0, 2] = pm[:, 2], -pm[:, 1]
    J[:, 1, 0], J[:, 1, 2] = -pm[:, 2], pm[:, 0]
    J[:, 2, 0], J[:, 2, 1] = pm[:, 1], -pm[:, 0]
    J[:, :, 3:] = np.eye(3)
    A = np.einsum("kia,kij,kjb->ab", J, Mi, J)
    g = np.einsum("kia,kij,kj->a", J, Mi, d)
    obj = float(np.einsum("ki,kij,kj->", d, Mi, d)) / len(pm) if len(pm) else 0.0
    return A, g, obj


def step_gicp(T, src, tgt, src_normals, tgt_normals, nn, eps=EPSILON, exact_state=False):
    """(T_next, status bits): one Gauss-Newton step, T_next = fp32(dT T); with exact_state, dT T in float64, unrounded."""
    state = (lambda M: np.asarray(M, np.float64).reshape(-1, 4)[:3].copy()) if exact_state else as_state
    if (nn >= 0).sum() < 6:
        return state(T), TOO_FEW
    A, g, _ = gicp_system(T, src, tgt, src_normals, tgt_normals, nn, eps, exact_state)
    x = ldl_solve(A, -g)
    if x is None:
        return state(T), SINGULAR
    T4 = np.eye(4)
    T4[:3] = state(T)
    return state((vector_to_matrix(x) @ T4)[:3]), 0


def pair_status(src, tgt, T0, src_normals, tgt_normals):
    s = U.pair_status(src, tgt, T0, tgt_normals)
    if not np.isfinite(src_normals).all():
        s |= NONFINITE
    return s


def gicp_ref(src, tgt, T0, src_normals, tgt_normals, eps=EPSILON, max_dist=MAX_DIST, iterations=ITERATIONS, rel_fitness=REL,
             rel_rmse=REL, report=False, perturb=None):
    """One pair.  icp_util.icp_ref's dict plus `objective`; trace_stat rows are (fitness, rmse, objective).  With report, `decided` and
    the four counts behind it.  perturb(T, s): replaces every new state (the chain-stable check)."""
    T = as_state(T0)
    nan = float("nan")
    out = dict(T=np.eye(4), fitness=nan, rmse=nan, objective=nan, n_corr=0, steps=0, nn=np.full(len(src), -1, np.int32),
               status=pair_status(src, tgt, T0, src_normals, tgt_normals), trace_T=[], trace_stat=[], near_tie=0, near_radius=0,
               near_stop=0, cond=0.0)
    out["T"][:3] = T
    if out["status"]:
        out["trace_T"], out["trace_stat"] = [T] * (iterations + 1), [(nan, nan, nan)] * (iterations + 1)
        return out
    prev = None
    for s in range(iterations + 1):
        e = evaluate(T, src, tgt, max_dist, report)
        A, g, obj = gicp_system(T, src, tgt, src_normals, tgt_normals, e["nn"], eps)
        out["trace_T"].append(T)
        out["trace_stat"].append((e["fitness"], e["rmse"], obj))
        if report:
            out["near_tie"] += e["near_tie"]
            out["near_radius"] += e["near_radius"]
        bits, stop = 0, False
        if prev is not None:
            df, dr = abs(e["fitness"] - prev[0]), abs(e["rmse"] - prev[1])
            out["near_stop"] += int(abs(df - rel_fitness) < 1e-9 or abs(dr - rel_rmse) < 1e-9)
            if df < rel_fitness and dr < rel_rmse:
                bits, stop = CONVERGED, True
        if not stop and s == iterations:
            stop = True
        if not stop:
            Tn, bits = step_gicp(T, src, tgt, src_normals, tgt_normals, e["nn"], eps)
            if report and not bits:
                out["cond"] = max(out["cond"], float(np.linalg.cond(A)))
            stop = bits != 0
        if stop:
            out.update(fitness=e["fitness"], rmse=e["rmse"], objective=obj, n_corr=e["n_corr"], steps=s, nn=e["nn"],
                       status=out["status"] | bits)
            out["T"][:3] = T
            break
        prev = (e["fitness"], e["rmse"])
        T = Tn if perturb is None else perturb(Tn, s)
    while len(out["trace_T"]) < iterations + 1:
        out["trace_T"].append(out["trace_T"][-1])
        out["trace_stat"].append(out["trace_stat"][-1])
    out["decided"] = out["near_tie"] == 0 and out["near_radius"] == 0 and out["near_stop"] == 0 and out["cond"] < 1e6
    return out


def pose_error(T, T_gt):
    """(RRE degrees, RTE metres) of T against T_gt."""
    T, T_gt = np.asarray(T, np.float64).reshape(-1, 4)[:3], np.asarray(T_gt, np.float64).reshape(-1, 4)[:3]
    R = T[:, :3] @ T_gt[:, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))), float(np.linalg.norm(T[:, 3] - T_gt[:, 3]))


# ---------------------------------------------------------------------------------------------------- fixtures
def make_fixture(seed, n_src=700, n_tgt=650, noise=0.003, outliers=0.25, deg=3.0, shift=(0.03, -0.04, 0.05)):
    """icp_util.make_fixture with the same random stream (so src, tgt, T_gt and T0 are that fixture's, which the test of this module
    checks), and additionally src_normals: the source surface normals in the source frame, n_src = n_p R_gt."""
    rng = np.random.default_rng(seed)
    surface(rng, n_tgt)
    _, n_p = surface(rng, n_src)
    f = U.make_fixture(seed, n_src=n_src, n_tgt=n_tgt, noise=noise, outliers=outliers, deg=deg, shift=shift)
    return dict(src=f["src"], tgt=f["tgt"], src_normals=(n_p @ f["T_gt"][:3, :3]).astype(np.float32), tgt_normals=f["normals"],
                T_gt=f["T_gt"], T0=f["T0"])


FIXTURES = U.FIXTURES      # the same names, seeds and sizes
_CACHE, _REF = {}, {}


def fixture(name):
    if name not in _CACHE:
        seed, kw = FIXTURES[name]
        _CACHE[name] = make_fixture(seed, **kw)
    return _CACHE[name]


def reference(name, **kw):
    """gicp_ref of a fixture with the default parameters (computed once per session, shared, never modified)."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _REF:
        f = fixture(name)
        _REF[key] = gicp_ref(f["src"], f["tgt"], f["T0"], f["src_normals"], f["tgt_normals"], report=True, **kw)
    return _REF[key]
