"""float64 numpy restatement of multiway registration (csrc/posegraph.hip; the rules are stated in include/roitr_engine.h above
roitr_edge_information), in the operator's own order: the same products and sums in the same sequence, the assembly in edge order,
the L D L^T column by column with every entry's sum in ascending k, the block sums as 256 strided lanes and the fixed butterfly.
numpy evaluates every ufunc on its own, so nothing here is fused.  `solver="numpy"` swaps the L D L^T for np.linalg.solve: the
independent path whose deviation from the first sizes the tolerances of the GPU tests.  Also the seeded graphs both test files use."""
import numpy as np

ONE_NODE, NO_EDGES, BAD_EDGE, SINGULAR, CONVERGED, BAD_COUNTS = 1, 2, 4, 8, 16, 32
LANES = 256


# ------------------------------------------------------------------------------------------------------------------ pieces
def block_sum(terms):
    """sum of `terms` as the kernels take it: lane t adds terms t, t + 256, ... in order, then the xor butterfly over each wave of 64
    and (w0 + w1) + (w2 + w3)."""
    lanes = np.zeros(LANES)
    for q, v in enumerate(np.asarray(terms, np.float64).reshape(-1)):
        lanes[q % LANES] += v
    idx = np.arange(64)
    waves = []
    for w in range(4):
        v = lanes[64 * w:64 * w + 64].copy()
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[idx ^ o]
        waves.append(v[0])
    return (waves[0] + waves[1]) + (waves[2] + waves[3])


def inverse(S):
    """[R^T | -R^T t] of (..., 12) states [R | t] (rows of 4)."""
    I = np.empty_like(S)
    for r in range(3):
        for c in range(3):
            I[..., 4 * r + c] = S[..., 4 * c + r]
        I[..., 4 * r + 3] = 0.0 - ((S[..., r] * S[..., 3] + S[..., 4 + r] * S[..., 7]) + S[..., 8 + r] * S[..., 11])
    return I


def mul(A, B, translate=True):
    C = np.empty(np.broadcast(A, B).shape)
    for r in range(3):
        for c in range(4):
            v = (A[..., 4 * r] * B[..., c] + A[..., 4 * r + 1] * B[..., 4 + c]) + A[..., 4 * r + 2] * B[..., 8 + c]
            C[..., 4 * r + c] = v + A[..., 4 * r + 3] if (c == 3 and translate) else v
    return C


def six(D):
    return np.stack([(D[..., 9] - D[..., 6]) / 2.0, (D[..., 2] - D[..., 8]) / 2.0, (D[..., 4] - D[..., 1]) / 2.0,
                     D[..., 3], D[..., 7], D[..., 11]], -1)


def states(poses):
    """(n, 4, 4) fp32 poses as (n, 12) float64 states."""
    return np.asarray(poses, np.float32).astype(np.float64).reshape(-1, 16)[:, :12].copy()


def residuals(X, g):
    """A = T_e^-1 X_j^-1, xi, Lambda xi and e = xi . (Lambda xi) of every edge under the states X (n, 12)."""
    Te = states(g["edge_T"])
    A = mul(inverse(Te), inverse(X[g["edge_j"]]))
    xi = six(mul(A, X[g["edge_i"]]))
    Lm = g["edge_info"]
    Lxi = np.zeros_like(xi)
    en = np.zeros(len(xi))
    for a in range(6):
        v = np.zeros(len(xi))
        for b in range(6):
            v = v + Lm[:, a, b] * xi[:, b]
        Lxi[:, a] = v
        en = en + xi[:, a] * v
    return A, xi, Lxi, en


def line(g, en, mu):
    """(l, the objective's terms) of every edge."""
    with np.errstate(all="ignore"):
        r = mu / (mu + en)
        l = r * r
        d = np.sqrt(l) - 1.0
        unc = g["edge_uncertain"] != 0
        return np.where(unc, l, 1.0), np.where(unc, l * en + mu * (d * d), en)


def objective(X, g, mu):
    _, _, _, en = residuals(X, g)
    l, terms = line(g, en, mu)
    return block_sum(terms), l


def compose(x, S):
    """compose_step_d of csrc/gauss_newton6.h on (k, 6) steps and (k, 12) states."""
    ca, sa, cb, sb, cg, sg = np.cos(x[:, 0]), np.sin(x[:, 0]), np.cos(x[:, 1]), np.sin(x[:, 1]), np.cos(x[:, 2]), np.sin(x[:, 2])
    R = [cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
         sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
         0.0 - sb, cb * sa, cb * ca]
    Sn = np.empty_like(S)
    for r in range(3):
        for c in range(4):
            v = R[3 * r] * S[:, c] + R[3 * r + 1] * S[:, 4 + c] + R[3 * r + 2] * S[:, 8 + c]
            Sn[:, 4 * r + c] = v + x[:, 3 + r] if c == 3 else v
    return Sn


def linearise(X, g, mu):
    """(F, l, H, b) at X, assembled in edge order; the gauge (node 0) has no rows."""
    n, m = len(X), len(g["edge_i"])
    u = 6 * (n - 1)
    A, xi, Lxi, en = residuals(X, g)
    l, terms = line(g, en, mu)
    Xi = X[g["edge_i"]]
    J = np.zeros((m, 6, 6))
    zero = np.zeros(m)
    for k in range(6):
        B = np.zeros((m, 12))
        for c in range(4):
            if k == 0:
                B[:, 4 + c], B[:, 8 + c] = 0.0 - Xi[:, 8 + c], Xi[:, 4 + c]
            if k == 1:
                B[:, c], B[:, 8 + c] = Xi[:, 8 + c], 0.0 - Xi[:, c]
            if k == 2:
                B[:, c], B[:, 4 + c] = 0.0 - Xi[:, 4 + c], Xi[:, c]
        if k >= 3:
            B[:, 4 * (k - 3) + 3] = 1.0
        J[:, :, k] = six(mul(A, B, translate=False))
    Lm = g["edge_info"]
    LJ = np.zeros((m, 6, 6))
    for a in range(6):
        for c in range(6):
            v = zero.copy()
            for b in range(6):
                v = v + Lm[:, a, b] * J[:, b, c]
            LJ[:, a, c] = v
    M = np.zeros((m, 6, 6))
    gv = np.zeros((m, 6))
    for r in range(6):
        for c in range(6):
            v = zero.copy()
            for a in range(6):
                v = v + J[:, a, r] * LJ[:, a, c]
            M[:, r, c] = l * v
    for c in range(6):
        v = zero.copy()
        for a in range(6):
            v = v + J[:, a, c] * Lxi[:, a]
        gv[:, c] = l * v
    H, b = np.zeros((u, u)), np.zeros(u)
    for e in range(m):
        i, j = int(g["edge_i"][e]), int(g["edge_j"][e])
        si, sj = slice(6 * (i - 1), 6 * i), slice(6 * (j - 1), 6 * j)
        if i > 0:
            H[si, si] += M[e]
            b[si] += gv[e]
        if j > 0:
            H[sj, sj] += M[e]
            b[sj] -= gv[e]
        if i > 0 and j > 0:
            H[si, sj] -= M[e]
            H[sj, si] -= M[e]
    return block_sum(terms), l, H, b


def ldl_solve(H, b, lam):
    """delta of (H + lam I) delta = -b by the operator's L D L^T (upper triangle of H; None: a bad pivot)."""
    u = len(b)
    V, w, d = H.copy(), np.zeros(u), np.zeros(u)
    for j in range(u):
        t = V[:j, j] / d[:j]
        v = V[j, j:].copy()
        v[0] = v[0] + lam
        rv = 0.0 - b[j]
        for k in range(j):
            v -= V[k, j:] * t[k]
            rv -= w[k] * t[k]
        V[j, j:], w[j], d[j] = v, rv, v[0]
        if not (d[j] > 0.0 and np.isfinite(d[j])):
            return None
    acc, x = w.copy(), np.zeros(u)
    for k in range(u - 1, -1, -1):
        x[k] = acc[k] / d[k]
        acc[:k] -= V[:k, k] * x[k]
    return x


def solve_once(X, g, mu, lam, tau=None, solver="ldl"):
    """One solve from the state X (n, 12): dict(F, lam (tau * max diag H when lam is None), delta (u) or None, maxd, den, Fn, rho)."""
    F, l, H, b = linearise(X, g, mu)
    if lam is None:
        lam = tau * np.max(np.diag(H))
    with np.errstate(all="ignore"):
        if solver == "ldl":
            delta = ldl_solve(H, b, lam)
        else:
            A = H + lam * np.eye(len(b))
            delta = np.linalg.solve(A, -b) if np.isfinite(A).all() and np.isfinite(b).all() else None
    out = dict(F=F, lam=lam, delta=delta, H=H, b=b)
    if delta is None:
        return out
    out["maxd"] = float(np.max(np.abs(delta)))
    out["den"] = block_sum(delta * (lam * delta - b))
    Xn = X.copy()
    Xn[1:] = compose(delta.reshape(-1, 6), X[1:])
    out["Xn"] = Xn
    out["Fn"], _ = objective(Xn, g, mu)
    out["rho"] = (F - out["Fn"]) / out["den"]
    return out


def damping_update(lam, nu, rho):
    """(lambda, nu, accepted) after a solve with gain rho."""
    if rho > 0.0:
        c = 2.0 * rho - 1.0
        return lam * max(1.0 / 3.0, 1.0 - c * c * c), 2.0, True
    return lam * nu, nu * 2.0, False


def optimise(g, mu, tau=1e-3, step_tol=1e-6, prune_threshold=0.25, iterations=100, solver="ldl"):
    """The whole loop on one scene g (a dict of arrays, see make_graph).  Returns dict(poses fp32, line_weight, pruned, steps, solves,
    objective, lam, status, trace: a list of dict(X, F, lam, rho, maxd, accepted, delta) per solve)."""
    n, m = len(g["init_poses"]), len(g["edge_i"])
    init = np.asarray(g["init_poses"], np.float32).reshape(-1, 4, 4)
    X = states(init)
    out = dict(poses=init.copy(), line_weight=np.ones(m), pruned=np.zeros(m, np.int32), steps=0, solves=0, objective=0.0, lam=0.0,
               status=0, trace=[])
    ei, ej = np.asarray(g["edge_i"]), np.asarray(g["edge_j"])
    st = ONE_NODE if n < 2 else NO_EDGES if m == 0 else 0
    if n >= 2 and m and ((ei < 0) | (ei >= n) | (ej < 0) | (ej >= n) | (ei == ej)).any():
        st = BAD_EDGE
    if st:
        out["status"] = st
        return out
    lam, nu = None, 2.0
    for _ in range(iterations):
        r = solve_once(X, g, mu, lam, tau, solver)
        lam = r["lam"]
        out["solves"] += 1
        row = dict(X=X.copy(), F=r["F"], lam=lam, rho=0.0, maxd=0.0, accepted=False, delta=r["delta"])
        out["trace"].append(row)
        if r["delta"] is None:
            st |= SINGULAR
            break
        row["maxd"] = r["maxd"]
        if r["maxd"] < step_tol:
            st |= CONVERGED
            break
        row["rho"] = r["rho"]
        lam, nu, row["accepted"] = damping_update(lam, nu, r["rho"])
        if row["accepted"]:
            X = r["Xn"]
            out["steps"] += 1
    F, l = objective(X, g, mu)
    if out["steps"]:
        out["poses"][1:, :3, :] = X[1:].reshape(-1, 3, 4).astype(np.float32)
        out["poses"][1:, 3, :] = (0, 0, 0, 1)
    out.update(line_weight=l, pruned=((g["edge_uncertain"] != 0) & (l < prune_threshold)).astype(np.int32), objective=F,
               lam=0.0 if lam is None else lam, status=st, X=X)
    return out


# ------------------------------------------------------------------------------------------------------------------ edge information
def fma32(a, b, c):
    """fp32 fused multiply-add of fp32 arrays, rounded ONCE.  The product of two fp32 values is exact in float64; the float64 sum with c
    need not be, so its rounding error e is recovered exactly (Knuth's two-sum) and consulted in the one case where rounding the
    float64 sum to fp32 could differ from rounding the exact sum: when the float64 sum lies exactly halfway between two fp32 values."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float32).astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                        # s + e = p + c exactly
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)                         # exact: both are float64 values within one fp32 spacing
    other = np.nextafter(r, np.where(d >= 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    with np.errstate(invalid="ignore", over="ignore"):
        tie = (d != 0) & (d == (other.astype(np.float64) - r.astype(np.float64)) / 2)
    # at a tie the float64 sum went to the even neighbour r; the exact sum lies on e's side of the midpoint
    return np.where(tie & (e != 0) & (np.sign(e) == np.sign(d)), other, r).astype(np.float32)


def edge_information(src, T, tgt, radius):
    """(info (6,6) float64, n_inlier) of one pair: the fp32 inlier test of rg_dist2 (fused multiply-adds, emulated exactly by fma32) and the operator's nine lane sums."""
    src, tgt = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    T = np.asarray(T, np.float32).reshape(4, 4)
    f32 = np.float32
    fma = fma32

    def axis(r):
        return fma(src[:, 2], T[r, 2], fma(src[:, 1], T[r, 1], fma(src[:, 0], T[r, 0], np.full(len(src), T[r, 3], f32))))
    dx, dy, dz = (axis(0) - tgt[:, 0]).astype(f32), (axis(1) - tgt[:, 1]).astype(f32), (axis(2) - tgt[:, 2]).astype(f32)
    d2 = fma(dz, dz, fma(dy, dy, (dx * dx).astype(f32)))
    thr2 = f32(radius) * f32(radius)
    inl = d2 < thr2
    x, y, z = (src[:, c].astype(np.float64) for c in range(3))
    terms = [y * y + z * z, x * y, x * z, x * x + z * z, y * z, x * x + y * y, x, y, z]
    a = []
    for t in terms:
        lanes_in = np.where(inl, t, 0.0)   # a skipped row adds nothing; adding +0.0 changes no bits of a lane sum that starts at +0.0
        a.append(block_sum(lanes_in))
    c, o = float(inl.sum()), 0.0
    info = np.array([[a[0], o - a[1], o - a[2], o, o - a[8], a[7]],
                     [o - a[1], a[3], o - a[4], a[8], o, o - a[6]],
                     [o - a[2], o - a[4], a[5], o - a[7], a[6], o],
                     [o, a[8], o - a[7], c, o, o],
                     [o - a[8], o, a[6], o, c, o],
                     [a[7], o - a[6], o, o, o, c]])
    return info, int(inl.sum())


def information_from_points(p):
    """sum G^T G over the rows of p (float64), G = [-[p]x | I3], by einsum: independent of the lane sums above."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    G = np.zeros((len(p), 3, 6))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    G[:, 0, 1], G[:, 0, 2] = z, -y       # -[p]x = [[0, z, -y], [-z, 0, x], [y, -x, 0]]
    G[:, 1, 0], G[:, 1, 2] = -z, x
    G[:, 2, 0], G[:, 2, 1] = y, -x
    G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
    return np.einsum("nki,nkj->ij", G, G)


def information_abs_terms(p):
    """per entry, the sum of the absolute values of the terms it adds up: the scale of its rounding error."""
    p = np.abs(np.asarray(p, np.float64).reshape(-1, 3))
    G = np.zeros((len(p), 3, 6))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    G[:, 0, 1], G[:, 0, 2] = z, y
    G[:, 1, 0], G[:, 1, 2] = z, x
    G[:, 2, 0], G[:, 2, 1] = y, x
    G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
    return np.einsum("nki,nkj->ij", G, G)


# ------------------------------------------------------------------------------------------------------------------ seeded graphs
def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def rigid(rng, angle, shift):
    T = np.eye(4)
    w = rng.normal(size=3)
    T[:3, :3] = rodrigues(w / np.linalg.norm(w) * angle)
    T[:3, 3] = rng.normal(size=3) * shift
    return T


def make_graph(n, seed, loops=None, wrong=0.2, noise=0.004, start="chain", points=200, max_dist=0.05, preference=1.0):
    """A seeded scene of n nodes: planted poses, the n - 1 odometry edges (k, k + 1) (certain) and `loops` loop closures between random
    node pairs (uncertain), a share `wrong` of them with a random transform; every measured transform carries a small rigid
    perturbation (`noise`: its angle in radians and its shift).  Each edge's information matrix is that of `points` points of a unit
    cube.  start: "chain" (the odometry edges chained from node 0), "identity" or "planted".  Returns the dict of arrays
    pose_graph_batch takes, plus planted (n,4,4), wrong (edges) bool and mu (Open3D's rule, line_process_weight)."""
    rng = np.random.default_rng(seed)
    loops = 2 * n if loops is None else loops
    planted = [np.eye(4)] + [rigid(rng, rng.uniform(0.2, 1.5), 1.0) for _ in range(n - 1)]
    ei, ej, unc, bad = [], [], [], []
    for k in range(n - 1):
        ei.append(k); ej.append(k + 1); unc.append(0); bad.append(False)
    made = 0
    while made < loops:
        i, j = (int(v) for v in rng.integers(0, n, size=2))
        if n == 2:
            i, j = made % 2, 1 - made % 2     # two nodes: repeats of the one pair, in both directions
        elif abs(i - j) < 2:
            continue
        ei.append(i); ej.append(j); unc.append(1); bad.append(False)
        made += 1
    n_wrong = int(round(wrong * made))
    for e in rng.permutation(np.arange(n - 1, n - 1 + made))[:n_wrong]:
        bad[e] = True
    Ts, infos = [], []
    for i, j, w in zip(ei, ej, bad):
        T = np.linalg.inv(planted[j]) @ planted[i]
        T = rigid(rng, 1.0, 0.5) @ T if w else (rigid(rng, noise, noise) @ T if noise > 0 else T)
        Ts.append(T)
        infos.append(information_from_points(rng.uniform(-0.5, 0.5, size=(points, 3))))
    edge_T = np.asarray(Ts, np.float64).reshape(-1, 4, 4).astype(np.float32)
    init = [np.eye(4)]
    for k in range(n - 1):
        step = np.linalg.inv(edge_T[k].astype(np.float64))   # X_i = X_j T_e
        init.append({"chain": init[-1] @ step, "identity": np.eye(4), "planted": planted[k + 1]}[start])
    g = dict(edge_i=np.asarray(ei, np.int32), edge_j=np.asarray(ej, np.int32), edge_T=edge_T,
             edge_info=np.asarray(infos, np.float64).reshape(-1, 6, 6), edge_uncertain=np.asarray(unc, np.int32),
             init_poses=np.asarray(init, np.float64).reshape(-1, 4, 4).astype(np.float32),
             planted=np.asarray(planted), wrong=np.asarray(bad, bool))
    u = g["edge_uncertain"] != 0
    g["mu"] = preference * max_dist ** 2 * (float(g["edge_info"][u, 5, 5].mean()) if u.any() else 1.0)
    return g


def batch(graphs):
    """The concatenated arrays and host starts of a list of scenes."""
    cat = lambda k, shape, dt: (np.concatenate([np.asarray(g[k]).reshape(shape) for g in graphs]) if graphs
                                else np.zeros(shape, dt)).astype(dt)
    return dict(node_starts=np.concatenate([[0], np.cumsum([len(g["init_poses"]) for g in graphs])]).astype(np.int32),
                edge_starts=np.concatenate([[0], np.cumsum([len(g["edge_i"]) for g in graphs])]).astype(np.int32),
                edge_i=cat("edge_i", (-1,), np.int32), edge_j=cat("edge_j", (-1,), np.int32), edge_T=cat("edge_T", (-1, 4, 4), np.float32),
                edge_info=cat("edge_info", (-1, 6, 6), np.float64), edge_uncertain=cat("edge_uncertain", (-1,), np.int32),
                init_poses=cat("init_poses", (-1, 4, 4), np.float32))


# The decided fixtures of both test files: name -> (make_graph arguments, optimiser arguments).  Each step_tol sits more than a factor
# 2 away from every max |delta| of the fixture's run (tests/test_posegraph_cpu.py asserts it).
FIXTURES = {
    "chain2": (dict(n=2, seed=2, loops=3, wrong=0.34), dict(iterations=20, step_tol=1e-6)),
    "chain5": (dict(n=5, seed=5, loops=8, wrong=0.25), dict(iterations=30, step_tol=3e-6)),
    "chain12": (dict(n=12, seed=12, loops=24, wrong=0.2), dict(iterations=30, step_tol=2.5e-6)),
    "chain33": (dict(n=33, seed=33, loops=66, wrong=0.15), dict(iterations=30, step_tol=1e-6)),
    "identity12": (dict(n=12, seed=112, loops=24, wrong=0.2, start="identity"), dict(iterations=60, step_tol=1e-6)),
    "clean12": (dict(n=12, seed=212, loops=24, wrong=0.2, noise=0.0), dict(iterations=30, step_tol=1.4e-6)),
}
EPS = 2.0 ** -52
_CACHE = {}


def fixture(name):
    """(graph, optimiser arguments, the restatement's run, the two-solver deviation) of a fixture, computed once per process."""
    if name not in _CACHE:
        ga, oa = FIXTURES[name]
        g = make_graph(**ga)
        _CACHE[name] = (g, oa, optimise(g, g["mu"], **oa), two_solver_deviation(g, g["mu"], **oa))
    return _CACHE[name]


def two_solver_deviation(g, mu, **oa):
    """How far the restatement's two solve paths (the operator's L D L^T, np.linalg.solve) drift apart over the whole run of a scene:
    per quantity the largest difference over the solves, dict(delta, F, rho: absolute; lam: relative).  Two values that agree to the
    last bit still carry the rounding of the quantity itself, so no deviation is taken finer than one unit in the last place of the
    quantity's largest magnitude in the run (2^-52 * max |q|; lam: 2^-52)."""
    a, b = optimise(g, mu, solver="ldl", **oa), optimise(g, mu, solver="numpy", **oa)
    assert [t["accepted"] for t in a["trace"]] == [t["accepted"] for t in b["trace"]] and a["status"] == b["status"]
    rows = [(s, t) for s, t in zip(a["trace"], b["trace"]) if s["delta"] is not None and t["delta"] is not None]
    big = lambda k: max(float(np.max(np.abs(s[k]))) for s, _ in rows)
    dev = {k: max(max(float(np.max(np.abs(s[k] - t[k]))) for s, t in rows), EPS * big(k)) for k in ("delta", "F", "rho")}
    dev["lam"] = max(max(abs(s["lam"] - t["lam"]) / s["lam"] for s, t in rows), EPS)
    return dev
