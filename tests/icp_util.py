"""float64 numpy restatement of roitr_icp_batch (include/roitr_pointops.h) and the seeded fixtures its tests share.

The evaluation repeats the header's operations in the header's order on the fp32 inputs, brute force over all (i, j) (numpy evaluates
every ufunc on its own, nothing is fused), so matches and counts are compared exactly.  The point-to-point solve is SVD Kabsch with the
sign(det) fix, independent of the kernels' quaternion / Jacobi solver; the point-to-plane solve is a plain float64 L D L^T.  The state
is rounded to fp32 after every update, as the operator does.

A fixture is DECIDED when, at every evaluated step of its chain, no point has a best and second-best d2 closer than 1e-6 relative, no
best d2 lies within 1e-6 r^2 of r^2, neither convergence difference lies within 1e-9 of its tolerance, and (point-to-plane) the 6x6
system has a condition number below 1e6.  On such inputs the matches, counts and stop decisions are the same for any arithmetic that
keeps the state within a few fp32 ulp; tests/test_icp_cpu.py re-verifies every fixture the GPU tests use.
"""
import numpy as np

import pairgt_util as P

NONFINITE, EMPTY, TOO_FEW, SINGULAR, CONVERGED = 1, 2, 4, 8, 16
NEAR = 1e-6
MAX_DIST, ITERATIONS, REL = 0.1, 30, 1e-6


# ---------------------------------------------------------------------------------------------------- restatement
def as_state(T):
    """(3,4) float64 holding the fp32 values of the top three rows of T."""
    return np.asarray(T, np.float64).reshape(-1, 4)[:3].astype(np.float32).astype(np.float64)


def evaluate(T, src, tgt, max_dist, report=False, chunk=512):
    """E(T): dict(nn (n) int32 pair-local match or -1, d2 (n) float64 (inf: none), n_corr, fitness, rmse) and, with report, near_tie /
    near_radius counts (see the module text)."""
    T = as_state(T)
    src, tgt = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    r = np.float64(np.float32(max_dist))
    r2 = r * r
    pm = P.move(src, T[:, :3], T[:, 3])
    n = len(src)
    nn, best = np.full(n, -1, np.int32), np.full(n, np.inf)
    near_tie = near_radius = 0
    for a in range(0, n, chunk):
        d2 = P.sqdist(pm[a:a + chunk], tgt)
        j = np.argmin(d2, 1)                      # the first of equal minima: the lower j
        rows = np.arange(len(j))
        b = d2[rows, j]
        ok = b < r2
        nn[a:a + chunk] = np.where(ok, j, -1)
        best[a:a + chunk] = np.where(ok, b, np.inf)
        if report:
            near_radius += int((np.abs(b - r2) <= NEAR * r2).sum())
            if d2.shape[1] > 1:
                d2[rows, j] = np.inf
                near_tie += int(((b < r2 * (1 + NEAR)) & (d2.min(1) - b <= NEAR * b)).sum())
    hit = nn >= 0
    nc = int(hit.sum())
    out = dict(nn=nn, d2=best, n_corr=nc, fitness=nc / n if n else float("nan"),
               rmse=float(np.sqrt(best[hit].sum() / nc)) if nc else 0.0)
    if report:
        out["near_tie"], out["near_radius"] = near_tie, near_radius
    return out


def kabsch(p, q):
    """[R | t] (3,4) float64 minimising sum |R p + t - q|^2 over rotations: SVD with the sign(det) fix."""
    cs, ct = p.mean(0), q.mean(0)
    H = (p - cs).T @ (q - ct)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    return np.concatenate([R, (ct - R @ cs)[:, None]], 1)


def step_point(T, src, tgt, nn):
    """(T_next (3,4) fp32 values, status bits): the rigid solve of the matched pairs on the ORIGINAL source points."""
    hit = nn >= 0
    if hit.sum() < 3:
        return as_state(T), TOO_FEW
    p, q = np.asarray(src, np.float32).astype(np.float64)[hit], np.asarray(tgt, np.float32).astype(np.float64)[nn[hit]]
    return as_state(kabsch(p, q)), 0


def vector_to_matrix(x):
    """Open3D's TransformVector6dToMatrix4d: R = Rz(g) Ry(b) Rx(a), t = (tx, ty, tz) for x = (a, b, g, tx, ty, tz); (4,4)."""
    a, b, g = x[:3]
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = Rz @ Ry @ Rx, x[3:]
    return M


def ldl_solve(A, b):
    """x of A x = b by L D L^T without pivoting, or None on a non-positive or non-finite pivot."""
    n = len(b)
    L, d = np.eye(n), np.zeros(n)
    for j in range(n):
        d[j] = A[j, j] - (L[j, :j] ** 2 * d[:j]).sum()
        if not (d[j] > 0 and np.isfinite(d[j])):
            return None
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * d[:j]).sum()) / d[j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = b[i] - L[i, :i] @ y[:i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = y[i] / d[i] - L[i + 1:, i] @ x[i + 1:]
    return x


def plane_system(T, src, tgt, normals, nn):
    """(A (6,6), b (6), residuals r) of the point-to-plane step under T."""
    T = as_state(T)
    hit = nn >= 0
    pm = P.move(np.asarray(src, np.float32)[hit], T[:, :3], T[:, 3])
    q = np.asarray(tgt, np.float32).astype(np.float64)[nn[hit]]
    nv = np.asarray(normals, np.float32).astype(np.float64)[nn[hit]]
    r = ((pm - q) * nv).sum(1)
    J = np.concatenate([np.cross(pm, nv), nv], 1)
    return J.T @ J, -J.T @ r, r


def step_plane(T, src, tgt, normals, nn):
    """(T_next, status bits): one Gauss-Newton step on the point-to-plane residuals, T_next = fp32(dT T)."""
    if (nn >= 0).sum() < 6:
        return as_state(T), TOO_FEW
    A, b, _ = plane_system(T, src, tgt, normals, nn)
    x = ldl_solve(A, b)
    if x is None:
        return as_state(T), SINGULAR
    T4 = np.eye(4)
    T4[:3] = as_state(T)
    return as_state((vector_to_matrix(x) @ T4)[:3]), 0


def plane_objective(T, src, tgt, normals, nn):
    return float((plane_system(T, src, tgt, normals, nn)[2] ** 2).sum())


def pair_status(src, tgt, T0, normals=None):
    s = 0
    fin = np.isfinite(src).all() and np.isfinite(tgt).all() and np.isfinite(np.asarray(T0, np.float32).reshape(-1)[:12]).all()
    if normals is not None:
        fin = fin and np.isfinite(normals).all()
    if not fin:
        s |= NONFINITE
    if len(src) == 0 or len(tgt) == 0:
        s |= EMPTY
    return s


def icp_ref(src, tgt, T0, max_dist=MAX_DIST, iterations=ITERATIONS, rel_fitness=REL, rel_rmse=REL, normals=None, report=False,
            perturb=None):
    """One pair.  dict(T (4,4), fitness, rmse, n_corr, steps, status, nn, trace_T [(3,4)], trace_stat [(fitness, rmse)]) and, with
    report, `decided` plus the four counts behind it.  perturb(T, s): replaces every new state (the chain-stable check)."""
    T = as_state(T0)
    out = dict(T=np.eye(4), fitness=float("nan"), rmse=float("nan"), n_corr=0, steps=0, nn=np.full(len(src), -1, np.int32),
               status=pair_status(src, tgt, T0, normals), trace_T=[], trace_stat=[], near_tie=0, near_radius=0, near_stop=0, cond=0.0)
    out["T"][:3] = T
    if out["status"]:
        out["trace_T"], out["trace_stat"] = [T] * (iterations + 1), [(float("nan"), float("nan"))] * (iterations + 1)
        return out
    prev = None
    for s in range(iterations + 1):
        e = evaluate(T, src, tgt, max_dist, report)
        out["trace_T"].append(T)
        out["trace_stat"].append((e["fitness"], e["rmse"]))
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
            if normals is None:
                Tn, bits = step_point(T, src, tgt, e["nn"])
            else:
                Tn, bits = step_plane(T, src, tgt, normals, e["nn"])
                if report and not bits:
                    out["cond"] = max(out["cond"], float(np.linalg.cond(plane_system(T, src, tgt, normals, e["nn"])[0])))
            stop = bits != 0
        if stop:
            out.update(fitness=e["fitness"], rmse=e["rmse"], n_corr=e["n_corr"], steps=s, nn=e["nn"], status=out["status"] | bits)
            out["T"][:3] = T
            break
        prev = (e["fitness"], e["rmse"])
        T = Tn if perturb is None else perturb(Tn, s)
    while len(out["trace_T"]) < iterations + 1:
        out["trace_T"].append(out["trace_T"][-1])
        out["trace_stat"].append(out["trace_stat"][-1])
    out["decided"] = out["near_tie"] == 0 and out["near_radius"] == 0 and out["near_stop"] == 0 and out["cond"] < 1e6
    return out


def ulp_perturb(seed):
    """perturb(T, s) moving every entry of the state by -1, 0 or +1 fp32 ulp, seeded."""
    rng = np.random.default_rng(seed)

    def f(T, s):
        t32 = T.astype(np.float32)
        k = rng.integers(-1, 2, t32.shape)
        moved = np.where(k > 0, np.nextafter(t32, np.float32(np.inf)), np.where(k < 0, np.nextafter(t32, np.float32(-np.inf)), t32))
        return moved.astype(np.float64)
    return f


# ---------------------------------------------------------------------------------------------------- fixtures
def euler_pose(deg, shift):
    """(4,4) float64: rotation of `deg` degrees about the axis (1, 2, 3) / |.|, translation `shift`."""
    M = np.eye(4)
    M[:3, :3] = P.rodrigues(np.deg2rad(deg) * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0))
    M[:3, 3] = shift
    return M


def surface(rng, k):
    """k points on a room corner (the three unit squares at x = 0, y = 0, z = 0) and a sphere patch (centre (0.55, 0.55, 0.55),
    radius 0.3, the octant facing the corner), with their unit normals."""
    which = rng.integers(0, 4, k)
    u, v = rng.uniform(0.0, 1.0, k), rng.uniform(0.0, 1.0, k)
    pts, nrm = np.zeros((k, 3)), np.zeros((k, 3))
    for a in range(3):
        sel = which == a
        pts[sel, (a + 1) % 3], pts[sel, (a + 2) % 3] = u[sel], v[sel]
        nrm[sel, a] = 1.0
    sel = which == 3
    d = -np.abs(rng.normal(size=(int(sel.sum()), 3)))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts[sel], nrm[sel] = 0.55 + 0.3 * d, d
    return pts, nrm


def make_fixture(seed, n_src=700, n_tgt=650, noise=0.003, outliers=0.25, deg=3.0, shift=(0.03, -0.04, 0.05)):
    """dict(src, tgt, normals (fp32), T_gt, T0 (4,4 float64 of fp32 values)).  The source is an independent sample of the target's
    surface under the inverse of T_gt, with noise; the last `outliers` share of it is displaced far out of range.  T0 is T_gt with a
    rotation of `deg` degrees and `shift` metres in front of it."""
    rng = np.random.default_rng(seed)
    q, nq = surface(rng, n_tgt)
    p, _ = surface(rng, n_src)
    q = q + noise * rng.normal(size=q.shape)
    p = p + noise * rng.normal(size=p.shape)
    k = int(round(outliers * n_src))
    if k:
        p[n_src - k:] += 3.0 + rng.uniform(0.0, 1.0, (k, 3))
    T_gt = np.eye(4)
    R, t = P.random_rigid(rng, angle=0.7, shift=0.5)
    T_gt[:3, :3], T_gt[:3, 3] = R.astype(np.float64), t.astype(np.float64)
    src = ((p - T_gt[:3, 3]) @ T_gt[:3, :3]).astype(np.float32)      # R^T (p - t)
    T0 = euler_pose(deg, np.asarray(shift)) @ T_gt
    T0[:3] = as_state(T0)
    return dict(src=src, tgt=q.astype(np.float32), normals=nq.astype(np.float32), T_gt=T_gt, T0=T0)


# name -> (seed, keyword arguments): every one is re-verified as decided and chain-stable in both modes by tests/test_icp_cpu.py
FIXTURES = {"room_a": (1, {}), "room_b": (2, {}), "room_c": (3, {}),
            "n255": (4, dict(n_src=255, n_tgt=300)), "n256": (5, dict(n_src=256, n_tgt=300)), "n257": (6, dict(n_src=257, n_tgt=300))}
_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        seed, kw = FIXTURES[name]
        _CACHE[name] = make_fixture(seed, **kw)
    return _CACHE[name]


_REF = {}


def reference(name, plane, **kw):
    """icp_ref of a fixture with the default parameters (computed once per session, shared, never modified)."""
    key = (name, plane, tuple(sorted(kw.items())))
    if key not in _REF:
        f = fixture(name)
        _REF[key] = icp_ref(f["src"], f["tgt"], f["T0"], normals=f["normals"] if plane else None, report=True, **kw)
    return _REF[key]


def lattice_pair(k=12, keep=0.5, seed=0):
    """An exact case: the target is a k^3 lattice of spacing h = 2^-4 (every coordinate exact in fp32), the source a subset of it moved
    by a translation of whole lattice steps; T_gt is that translation."""
    h = 2.0 ** -4
    g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64) * h
    rng = np.random.default_rng(seed)
    sel = np.sort(rng.choice(len(g), int(keep * len(g)), replace=False))
    T_gt = np.eye(4)
    T_gt[:3, 3] = (2 * h, -h, 3 * h)
    src = (g[sel] - T_gt[:3, 3]).astype(np.float32)
    return dict(src=src, tgt=g.astype(np.float32), T_gt=T_gt, sel=sel, h=h)


def lattice_start(f):
    """T_gt with the translation off by (0.4, -0.3, 0.2) lattice steps: inside max_dist = 1.5 h and inside the basin of the true
    matches.  (A start a WHOLE step off maps the source onto lattice points again -- rmse 0 for every interior point, a fixed point of
    ICP that no implementation leaves -- so the offset is a fraction of a step.)"""
    T0 = f["T_gt"].copy()
    T0[:3, 3] += np.array([0.4, -0.3, 0.2]) * f["h"]
    T0[:3] = as_state(T0)
    return T0
