"""float64 numpy restatement of roitr_lgr_batch (include/roitr_engine.h) and the seeded sets its tests share.

The restatement follows the header's definition with an independent solver: SVD Kabsch with the sign(det) fix (as `kabsch` in
tests/test_registration_gpu.py) where the kernels use Horn's quaternion form.  T is rounded to fp32 after every solve, residuals are
float64 from that fp32 T.  For every hypothesis and every global step it also returns the number of NEAR rows,
|d^2 - r^2| < 1e-4 r^2: the boundary rule the RANSAC tests use for fp32 decisions (an fp32 residual can only fall on the other side
of r^2 for such a row).

A set is DECIDED when no row is near at any global step and no row is near for any hypothesis whose count could reach the maximum
(upper count >= the largest lower count).  On a decided set the winner, every later inlier set and the final count are the same
for any arithmetic that meets the fp32 bound, so the GPU tests compare them exactly.  SEEDS lists, per case of the GPU tests, a seed
picked on the CPU for which the case is decided (tests/test_lgr_cpu.py checks every one, none may be skipped).
"""
import numpy as np

RADIUS, MIN_ROWS, STEPS, EPS = 0.1, 3, 5, 1e-5
NEAR = 1e-4
NO_ROWS, NO_LOCAL, EMPTY_REFIT = 1, 2, 4


# ---------------------------------------------------------------------------------------------------- restatement
def moments(src, tgt, w):
    """Normalised weights, centroids and H of the header's Solve, float64."""
    s, t, w = src.astype(np.float64), tgt.astype(np.float64), w.astype(np.float64)
    wn = w / (w.sum() + EPS)
    cs, ct = wn @ s, wn @ t
    return cs, ct, ((s - cs) * wn[:, None]).T @ (t - ct)


def solve(src, tgt, w):
    """T (3,4) float64 holding fp32 values, or None when the weights sum to 0."""
    if w.astype(np.float64).sum() == 0.0:
        return None
    cs, ct, H = moments(src, tgt, w)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    return np.concatenate([R, (ct - R @ cs)[:, None]], 1).astype(np.float32).astype(np.float64)


def dist2(T, src, tgt):
    d = src.astype(np.float64) @ T[:, :3].T + T[:, 3] - tgt.astype(np.float64)
    return (d * d).sum(1)


def counts(T, src, tgt, radius):
    """(inliers, near rows, lower count, upper count, inlier mask)"""
    d2, r2 = dist2(T, src, tgt), radius * radius
    near = np.abs(d2 - r2) < NEAR * r2
    return int((d2 < r2).sum()), int(near.sum()), int((d2 < r2 * (1 - NEAR)).sum()), int((d2 < r2 * (1 + NEAR)).sum()), d2 < r2


def runs(patch, min_rows=MIN_ROWS):
    """[(first row, rows)] of the runs of at least min_rows rows, in row order."""
    n = len(patch)
    if n == 0:
        return []
    heads = np.flatnonzero(np.concatenate([[True], patch[1:] != patch[:-1]]))
    lens = np.diff(np.concatenate([heads, [n]]))
    return [(int(f), int(l)) for f, l in zip(heads, lens) if l >= min_rows]


def lgr_ref(src, tgt, scores, patch, radius=RADIUS, min_rows=MIN_ROWS, steps=STEPS):
    """One pair.  Returns a dict: T (4,4), inliers, mask, best, best_first_row, hypotheses, local_inliers, status, hyp_first_row,
    hyp_T (H,3,4), hyp_counts, hyp_near, step_near (near rows under the transform each global step and the final count used) and
    decided."""
    n = src.shape[0]
    scores = np.ones(n, np.float32) if scores is None else scores
    out = dict(T=np.eye(4), inliers=0, mask=np.zeros(n, bool), best=-1, best_first_row=-1, hypotheses=0, local_inliers=0, status=0,
               hyp_first_row=[], hyp_T=np.zeros((0, 3, 4)), hyp_counts=[], hyp_near=[], step_near=[], decided=True)
    if n == 0:
        out["status"] = NO_ROWS
        return out
    hyps = runs(patch, min_rows)
    out["hypotheses"] = len(hyps)
    out["hyp_first_row"] = [f for f, _ in hyps]
    T, alive = np.concatenate([np.eye(3), np.zeros((3, 1))], 1), True
    if hyps:
        Ts = [solve(src[f:f + l], tgt[f:f + l], scores[f:f + l]) for f, l in hyps]
        Ts = [np.concatenate([np.eye(3), np.zeros((3, 1))], 1) if t is None else t for t in Ts]
        c = [counts(t, src, tgt, radius) for t in Ts]
        out["hyp_T"], out["hyp_counts"], out["hyp_near"] = np.stack(Ts), [x[0] for x in c], [x[1] for x in c]
        best = int(np.argmax(out["hyp_counts"]))   # the first of equal counts
        top_lower = max(x[2] for x in c)
        out["decided"] = all(x[1] == 0 for x in c if x[3] >= top_lower)
        out["best"], out["best_first_row"], out["local_inliers"], T = best, hyps[best][0], out["hyp_counts"][best], Ts[best]
    else:
        out["status"] |= NO_LOCAL
        T0 = solve(src, tgt, scores)
        alive = T0 is not None
        if alive:
            T = T0
            out["local_inliers"] = counts(T, src, tgt, radius)[0]
    for _ in range(steps):
        if not alive:
            break
        c = counts(T, src, tgt, radius)
        out["step_near"].append(c[1])
        Tn = solve(src, tgt, scores * c[4])
        alive = Tn is not None
        T = Tn if alive else T
    if not alive:
        out["status"] |= EMPTY_REFIT
    c = counts(T, src, tgt, radius)
    out["step_near"].append(c[1])
    out["decided"] = out["decided"] and not any(out["step_near"])
    out["T"][:3] = T
    out["inliers"], out["mask"] = c[0], c[4]
    return out


def procrustes64(src, tgt, w):
    """Plain float64 weighted Procrustes (no fp32 rounding): (3,4)."""
    cs, ct, H = moments(src, tgt, w)
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
    return np.concatenate([R, (ct - R @ cs)[:, None]], 1)


# ---------------------------------------------------------------------------------------------------- generator
def random_pose(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return R, rng.uniform(-1, 1, 3)


def well_posed(src, tgt, w):
    """Horn's quaternion and the SVD form agree where the optimal rotation is well separated: s2 >= 1e-3 s1 and, where the sign fix
    flips the third axis, s2 - s3 >= 1e-3 s1 as well."""
    _, _, H = moments(src, tgt, w)
    U, S, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    return S[1] >= 1e-3 * S[0] and S[1] + d * S[2] >= 1e-3 * S[0]


def make_pair(seed, lengths, inlier, noise=0.003, extent=0.5, pose=None):
    """A pair with one patch per entry of `lengths` (rows) / `inlier` (bool): a planted pose, inlier patches tgt = R s + t + noise
    (sigma well below the radius), outlier patches tgt = R s + t + u with |u| in [0.5, 1.5] in a direction of the row's own.  A run of
    at least MIN_ROWS rows is redrawn until it is well_posed.  noise may be one sigma per patch.  Returns src, tgt (fp32), scores,
    row_patch, the planted inlier mask and the pose (R, t)."""
    rng = np.random.default_rng(seed)
    R, t = random_pose(rng) if pose is None else pose
    noise = np.broadcast_to(noise, (len(lengths),))
    S, G, W, P, M = [], [], [], [], []
    for k, (L, good) in enumerate(zip(lengths, inlier)):
        while True:
            s = (rng.uniform(-1.5, 1.5, 3) + extent * rng.normal(size=(L, 3))).astype(np.float32)
            g = s.astype(np.float64) @ R.T + t
            if good:
                g = g + noise[k] * rng.normal(size=(L, 3))
            else:
                u = rng.normal(size=(L, 3))
                g = g + u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.5, 1.5, (L, 1))
            g, w = g.astype(np.float32), rng.uniform(0.2, 1.0, L).astype(np.float32)
            if L < MIN_ROWS or well_posed(s, g, w):
                break
        S.append(s); G.append(g); W.append(w); P.append(np.full(L, k, np.int32)); M.append(np.full(L, bool(good)))
    cat = lambda xs, shape: np.concatenate(xs) if xs else np.zeros(shape, xs[0].dtype if xs else np.float32)
    return (cat(S, (0, 3)), cat(G, (0, 3)), cat(W, (0,)), cat(P, (0,)).astype(np.int32), cat(M, (0,)).astype(bool), (R, t))


def split_rows(rng, total, n_patches, low=MIN_ROWS):
    """n_patches ragged run lengths of at least `low` rows that sum to `total`."""
    extra = rng.multinomial(total - low * n_patches, np.ones(n_patches) / n_patches)
    return [int(low + e) for e in extra]


# The cases of tests/test_lgr_gpu.py.  name -> (lengths, inlier flags) builders; the seed of each is in SEEDS.
def case(name, seed):
    rng = np.random.default_rng(1000 + seed)
    if name == "mixed_runs":              # run lengths 1, 2, 3, 4, 63, 64, 65 and a few hundred, mixed in one pair
        lengths = [1, 3, 64, 2, 300, 4, 63, 1, 65, 5, 2, 17]
        inlier = [True, True, True, False, True, False, True, True, False, True, True, False]
    elif name.startswith("rows_"):        # rows per pair around the verification tile / chunk (512)
        lengths = split_rows(rng, int(name[5:]), 40)
        inlier = list(rng.uniform(size=40) < 0.5)
    elif name.startswith("hyps_"):        # hypotheses per pair around one workgroup's worth (256): every run has 3 or 4 rows
        h = int(name[5:])
        lengths = [int(x) for x in rng.integers(3, 5, h)]
        inlier = list(rng.uniform(size=h) < 0.4)
    elif name == "no_local":              # no run of 3 rows: the degenerate start on all rows
        lengths = [int(x) for x in rng.integers(1, 3, 30)]
        inlier = [True] * 30
    elif name == "empty_refit":           # outlier patches only: every count is 0, the first global solve has no weight
        lengths, inlier = [3, 4, 3, 5, 3], [False] * 5
    elif name in ("graded", "graded_tail"):   # a noise level per patch: the counts differ, the winner is one patch in the middle and the
        lengths = [int(x) for x in rng.integers(3, 9, 300)]   # inlier set changes from step to step (no planted mask to recover)
        inlier = list(rng.uniform(size=300) < 0.6)
        if name == "graded_tail":         # inlier patches behind number 270 only: the winner sits in a lane's second hypothesis
            inlier[:270] = [False] * 270
        return make_pair(seed, lengths, inlier, noise=rng.uniform(0.002, 0.03, 300))
    elif name == "tie":                   # built by tie_pair
        return tie_pair(seed)
    else:
        raise KeyError(name)
    return make_pair(seed, lengths, inlier)


def tie_pair(seed):
    """The winning patch twice, first and last, with outlier patches between: equal transforms, equal counts."""
    src, tgt, w, patch, mask, pose = make_pair(seed, [48, 5, 7, 3], [True, False, False, False], extent=0.8)
    k = 48
    return (np.concatenate([src, src[:k]]), np.concatenate([tgt, tgt[:k]]), np.concatenate([w, w[:k]]),
            np.concatenate([patch, np.full(k, 9, np.int32)]), np.concatenate([mask, mask[:k]]), pose)


SEEDS = {"mixed_runs": 0, "rows_511": 0, "rows_512": 0, "rows_513": 0, "hyps_255": 0, "hyps_256": 0, "hyps_257": 0,
         "no_local": 0, "empty_refit": 1, "tie": 0, "graded": 0, "graded_tail": 0}
# other parameter settings the GPU tests run, each decided on its fixture
PARAM_CASES = [("mixed_runs", dict(min_rows=5, steps=1)), ("rows_513", dict(min_rows=4, steps=2, radius=0.05)),
               ("hyps_257", dict(min_rows=4, steps=3)), ("rows_512", dict(min_rows=7, steps=1, radius=0.2))]
PLANTED = [n for n in SEEDS if not n.startswith("graded")]   # the sets whose noise is well below the radius


def fixture(name):
    return case(name, SEEDS[name])
