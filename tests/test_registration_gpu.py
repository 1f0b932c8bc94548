"""GPU: registration (csrc/registration.hip through roitr_amd/registration.py) against float64 restatements written here.

The random stream is restated in numpy uint64 and must match bit for bit.  The hypotheses are replayed in float64 from the same
triples (edge checker, degenerate test, SVD Kabsch with the determinant fix, distance checker, strict inlier count, RMSE); the GPU
decides in fp32, so decisions within 1e-4 thr^2 of the threshold are boundary cases and the comparisons carry them as a margin.
Selection (top-k ties, Efraimidis-Spirakis keys), the batch / chunk / run invariances, edge cases, weighted Procrustes
(lib/utils.py:159-212), engine batches and the Tester are covered as well.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
THR = 0.05
SIM = 0.9


# ---------------------------------------------------------------------------------------------------- restatements
def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def draws(seed, key, its, d, n):
    c = (np.uint64(key) << np.uint64(32)) | (np.asarray(its, dtype=np.uint64) << np.uint64(4)) | np.uint64(d)
    u = splitmix64(np.uint64(seed) ^ splitmix64(c)) >> np.uint64(32)
    return ((u * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def triples(seed, key, its, n):
    """(len(its), 3) int64, -1 rows for invalid iterations: draws 0..15, repeats skipped, first three distinct."""
    its = np.asarray(its)
    out = np.full((its.shape[0], 3), -1, np.int64)
    got = np.zeros(its.shape[0], np.int64)
    for d in range(16):
        x = draws(seed, key, its, d, n)
        new = got < 3
        for k in range(3):
            new &= ~((k < got) & (out[:, k] == x))
        rows = np.nonzero(new)[0]
        out[rows, got[rows]] = x[rows]
        got[rows] += 1
    out[got < 3] = -1
    return out


def select_uniform(seed, key, j):
    c = (np.uint64(key) << np.uint64(32)) | np.asarray(j, dtype=np.uint64)
    u = splitmix64(np.uint64(seed) ^ np.uint64(0xA0761D6478BD642F) ^ splitmix64(c)) >> np.uint64(32)
    return (u.astype(np.float64) + 0.5) / 2.0 ** 32


def kabsch(s, t):
    """(H,3,3) x2 -> R (H,3,3), t (H,3): SVD with the sign(det) fix (lib/utils.py:196-205 in float64)."""
    cs, ct = s.mean(1, keepdims=True), t.mean(1, keepdims=True)
    H = np.einsum("hna,hnb->hab", s - cs, t - ct)
    U, _, Vt = np.linalg.svd(H)
    V = np.transpose(Vt, (0, 2, 1))
    D = np.tile(np.eye(3), (s.shape[0], 1, 1))
    D[:, 2, 2] = np.sign(np.linalg.det(V @ np.transpose(U, (0, 2, 1))))
    R = V @ D @ np.transpose(U, (0, 2, 1))
    return R, ct[:, 0] - np.einsum("hab,hb->ha", R, cs[:, 0])


def oracle_hypotheses(src, tgt, seed, key, iterations, thr=THR, sim=SIM):
    """float64 replay of every iteration: dict of arrays over iterations (valid, near-boundary flag, count, M, sum d^2, R, t)."""
    n = src.shape[0]
    its = np.arange(iterations)
    tri = triples(seed, key, its, n)
    ok = tri[:, 0] >= 0
    s = src.astype(np.float64)[np.where(ok[:, None], tri, 0)]
    t = tgt.astype(np.float64)[np.where(ok[:, None], tri, 0)]
    edge_ok, edge_near = np.ones(iterations, bool), np.zeros(iterations, bool)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        ds, dt = np.linalg.norm(s[:, i] - s[:, j], axis=1), np.linalg.norm(t[:, i] - t[:, j], axis=1)
        edge_ok &= ~(ds < dt * sim) & ~(dt < ds * sim)
        edge_near |= (np.abs(ds - dt * sim) <= 1e-6 * (ds + dt)) | (np.abs(dt - ds * sim) <= 1e-6 * (ds + dt))

    def tri_ok(p):
        a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        c2 = (np.cross(a, b) ** 2).sum(1)
        ab = (a * a).sum(1) * (b * b).sum(1)
        return c2 > 1e-12 * ab, np.abs(c2 - 1e-12 * ab) <= 1e-3 * 1e-12 * ab
    so, sn = tri_ok(s)
    to, tn = tri_ok(t)
    cand = ok & edge_ok & so & to
    R, tt = np.tile(np.eye(3), (iterations, 1, 1)), np.zeros((iterations, 3))
    idx = np.nonzero(cand)[0]
    if idx.size:
        R[idx], tt[idx] = kabsch(s[idx], t[idx])
    d2s = ((np.einsum("hab,hkb->hka", R, s) + tt[:, None] - t) ** 2).sum(2)
    thr2 = thr * thr
    dist_ok = (d2s <= thr2).all(1)
    dist_near = (np.abs(d2s - thr2) < 1e-4 * thr2).any(1)
    valid = cand & dist_ok
    near = ok & (edge_near | sn | tn | (cand & dist_near))
    count, M, ssum = np.zeros(iterations, np.int64), np.zeros(iterations, np.int64), np.zeros(iterations)
    src64, tgt64 = src.astype(np.float64), tgt.astype(np.float64)
    vi = np.nonzero(valid | (cand & dist_near))[0]
    for c0 in range(0, vi.size, 64):
        h = vi[c0:c0 + 64]
        d2 = ((np.einsum("hab,nb->hna", R[h], src64) + tt[h][:, None] - tgt64[None]) ** 2).sum(2)
        inl = d2 < thr2
        count[h] = inl.sum(1)
        ssum[h] = np.where(inl, d2, 0).sum(1)
        M[h] = (np.abs(d2 - thr2) < 1e-4 * thr2).sum(1)
    return dict(valid=valid, near=near, count=count, M=M, ssum=ssum, R=R, t=tt)


def transform_of(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def make_set(n, inlier_frac, rng, sigma=0.005, extent=1.0):
    """n correspondences: src uniform in [-extent, extent]^3, the first round(inlier_frac n) mapped by (R, t) plus noise, the
    rest uniform in the target cloud's box.  Returns src, tgt (float32), R, t, per-row confidence in (0, 1]."""
    R, t = random_rotation(rng), rng.uniform(-1, 1, 3)
    src = rng.uniform(-extent, extent, (n, 3))
    tgt = src @ R.T + t + rng.normal(0, sigma, (n, 3))
    k = int(round(inlier_frac * n))
    if k < n:
        tgt[k:] = rng.uniform(tgt.min(0), tgt.max(0), (n - k, 3))
    conf = rng.uniform(0.05, 1.0, n)
    return src.astype(np.float32), tgt.astype(np.float32), R, t, conf.astype(np.float32)


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dt) if dt is not None else t).cuda()


def starts_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def run(sets, **kw):
    from roitr_amd.registration import ransac_batch
    src = np.concatenate([s[0] for s in sets]).reshape(-1, 3)
    tgt = np.concatenate([s[1] for s in sets]).reshape(-1, 3)
    sc = np.concatenate([s[2] for s in sets]) if all(len(s) > 2 and s[2] is not None for s in sets) else None
    st = starts_of([s[0].shape[0] for s in sets])
    r = ransac_batch(dev(st), dev(src), dev(tgt), None if sc is None else dev(sc), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}, st


def rre_rte(T, R, t):
    c = np.clip((np.trace(T[:3, :3].T.astype(np.float64) @ R) - 1) / 2, -1, 1)
    return np.degrees(np.arccos(c)), np.linalg.norm(T[:3, 3] - t)


# ---------------------------------------------------------------------------------------------------- 1. stream
@pytest.mark.parametrize("seed,key,n", [(0, 0, 3), (1, 5, 3), (0, 7, 4), (12345, 3, 1000), (2 ** 63 + 11, 2 ** 32 - 1, 20000),
                                        (99, 123456, 7)])
def test_stream_matches_restatement(seed, key, n):
    from roitr_amd.registration import ransac_samples
    for it0 in (0, (1 << 20) - 100, (1 << 27) + 5):
        got = ransac_samples([n], pair_keys=[key], seed=seed, it0=it0, count=2000)[0].cpu().numpy()
        ref = triples(seed, key, np.arange(it0, it0 + 2000), n)
        assert np.array_equal(got, ref), (seed, key, n, it0)
    if n == 3:   # the redraw path: permutations of {0, 1, 2}, or -1 rows where 16 draws did not give three distinct indices
        ok = got[:, 0] >= 0
        assert ok.mean() > 0.99 and np.all(np.sort(got[ok], 1) == [0, 1, 2]) and np.all(got[~ok] == -1)


def test_stream_batched_keys_and_small_n():
    from roitr_amd.registration import ransac_samples
    ns, keys = [0, 2, 3, 4, 50], [9, 8, 7, 6, 5]
    got = ransac_samples(ns, pair_keys=keys, seed=4, it0=10, count=300).cpu().numpy()
    for b, (n, k) in enumerate(zip(ns, keys)):
        ref = triples(4, k, np.arange(10, 310), n) if n >= 3 else np.full((300, 3), -1)
        assert np.array_equal(got[b], ref)


# ---------------------------------------------------------------------------------------------------- 2. hypothesis parity
def check_parity(src, tgt, r, b, seed, key, iterations, refined=False):
    o = oracle_hypotheses(src, tgt, seed, key, iterations)
    margin = int(o["near"].sum())
    assert abs(int(r["valid_hypotheses"][b]) - int(o["valid"].sum())) <= margin, (int(r["valid_hypotheses"][b]), int(o["valid"].sum()), margin)
    if not o["valid"].any() and margin == 0:
        assert int(r["valid_hypotheses"][b]) == 0 and int(r["best_iteration"][b]) == -1
        assert np.array_equal(r["T"][b], np.eye(4, dtype=np.float32))
        return o
    h = int(r["best_iteration"][b])
    assert 0 <= h < iterations
    lower = o["count"] - o["M"]
    assert o["count"][h] + o["M"][h] >= lower[o["valid"]].max(initial=0), (h, o["count"][h], lower.max())
    if not refined:
        assert np.abs(r["T"][b].astype(np.float64) - transform_of(o["R"][h], o["t"][h])).max() < 1e-5
        assert abs(int(r["inliers"][b]) - int(o["count"][h])) <= int(o["M"][h])
    return o


@pytest.mark.parametrize("n,frac,iters", [(3, 1.0, 2000), (4, 1.0, 2000), (64, 0.5, 3000), (1000, 0.3, 3000), (3000, 0.2, 2000),
                                          (20000, 0.3, 2000)])
def test_hypothesis_parity(n, frac, iters):
    rng = np.random.default_rng(n)
    src, tgt, R, t, conf = make_set(n, frac, rng)
    seed, key = 77, 5
    r, _ = run([(src, tgt, conf)], sample="all", iterations=iters, seed=seed, pair_keys=[key])
    assert int(r["n_used"][0]) == n
    check_parity(src, tgt, r, 0, seed, key, iters)


def test_hypothesis_parity_batch_of_sets():
    """Several pairs in one call, each replayed with its own key."""
    rng = np.random.default_rng(3)
    sets = [make_set(n, f, rng) for n, f in ((200, 0.4), (1500, 0.1), (5, 1.0), (700, 0.6))]
    keys = [11, 2 ** 31 + 3, 0, 42]
    r, _ = run([(s[0], s[1], s[4]) for s in sets], sample="all", iterations=2500, seed=9, pair_keys=keys)
    for b, s in enumerate(sets):
        check_parity(s[0], s[1], r, b, 9, keys[b], 2500)


# ---------------------------------------------------------------------------------------------------- 3. recovery at 50 000
@pytest.mark.parametrize("refine,rre_max,rte_max", [(0, 3.0, 0.05), (2, 0.5, 0.02)])
def test_recovery_full_iterations(refine, rre_max, rte_max):
    rng = np.random.default_rng(2024)
    sets, gts = [], []
    for frac in (0.05, 0.10, 0.30, 1.00):
        for _ in range(3):
            src, tgt, R, t, conf = make_set(1000, frac, rng)
            sets.append((src, tgt, conf))
            gts.append((R, t, frac))
    r, _ = run(sets, sample="weighted", n_points=1000, iterations=50000, refine_iters=refine, seed=1)
    for b, (R, t, frac) in enumerate(gts):
        rre, rte = rre_rte(r["T"][b], R, t)
        assert rre <= rre_max and rte <= rte_max, (b, frac, rre, rte)
        assert int(r["inliers"][b]) >= 0.9 * frac * 1000 and np.isfinite(r["T"][b]).all()


# ---------------------------------------------------------------------------------------------------- 4. selection
def test_topk_selection_with_ties():
    rng = np.random.default_rng(5)
    n, k = 3000, 1000
    conf = rng.integers(0, 40, n).astype(np.float32) / 8   # many exact ties, including at the cut
    src, tgt = rng.uniform(-1, 1, (n, 3)).astype(np.float32), rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    r, st = run([(src, tgt, conf), (src[:500], tgt[:500], conf[:500])], sample="topk", n_points=k, iterations=10)
    ref = np.sort(np.lexsort((np.arange(n), -conf))[:k])
    assert int(r["n_used"][0]) == k and np.array_equal(r["selected"][:k], ref)
    assert int(r["n_used"][1]) == 500 and np.array_equal(r["selected"][n:n + 500], np.arange(500))   # n_points >= n: all
    assert np.all(r["selected"][k:n] == -1)   # rows past n_used stay untouched


@pytest.mark.parametrize("n,k", [(3000, 1000), (10000, 5000), (1200, 1199)])
def test_weighted_selection_matches_keys(n, k):
    rng = np.random.default_rng(n + k)
    conf = rng.uniform(0, 1, n).astype(np.float32) ** 3
    conf[rng.choice(n, n // 10, replace=False)] = 0.0
    conf[:5] = -1.0
    src, tgt = rng.uniform(-1, 1, (n, 3)).astype(np.float32), rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    seed, key = 31, 17
    r, _ = run([(src, tgt, conf)], sample="weighted", n_points=k, iterations=10, seed=seed, pair_keys=[key])
    pos = conf > 0
    kk = min(k, int(pos.sum()))
    assert int(r["n_used"][0]) == kk
    got = r["selected"][:kk]
    assert np.all(np.diff(got) > 0) and np.all(conf[got] > 0)
    keys = np.full(n, -np.inf)
    keys[pos] = np.log(select_uniform(seed, key, np.nonzero(pos)[0])) / conf[pos].astype(np.float64)
    order = np.lexsort((np.arange(n), -keys))
    ref = np.sort(order[:kk])
    diff = np.setxor1d(got, ref)
    cut = keys[order[kk - 1]]
    assert np.all(np.abs(keys[diff] - cut) <= 1e-6 * abs(cut)), diff


def test_weighted_selection_takes_all_when_few_positive():
    rng = np.random.default_rng(8)
    n = 400
    conf = np.zeros(n, np.float32)
    conf[::7] = rng.uniform(0.1, 1, len(conf[::7]))
    src, tgt = rng.uniform(-1, 1, (n, 3)).astype(np.float32), rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    r, _ = run([(src, tgt, conf)], sample="weighted", n_points=1000, iterations=10)
    m = int(r["n_used"][0])
    assert m == len(conf[::7]) and np.array_equal(r["selected"][:m], np.arange(0, n, 7))


# ---------------------------------------------------------------------------------------------------- 5. invariance
def test_batch_run_and_chunk_invariance():
    rng = np.random.default_rng(64)
    sizes = rng.integers(0, 900, 64)
    sizes[:4] = (0, 2, 3, 1500)
    sets = [make_set(int(m), float(rng.uniform(0.1, 0.8)), rng) for m in sizes]
    sets = [(s[0], s[1], s[4]) for s in sets]
    keys = list(range(1000, 1064))
    kw = dict(sample="weighted", n_points=600, iterations=3000, refine_iters=1, seed=5)
    full, _ = run(sets, pair_keys=keys, **kw)
    again, _ = run(sets, pair_keys=keys, **kw)
    fields = ("T", "inliers", "best_iteration", "valid_hypotheses", "n_used")
    for f in fields:
        assert np.array_equal(full[f], again[f]), f
    for ch in (1, 3, 11):
        other, _ = run(sets, pair_keys=keys, chunks=ch, **kw)
        for f in fields:
            assert np.array_equal(full[f], other[f]), (f, ch)
    for b in range(64):
        alone, _ = run([sets[b]], pair_keys=[keys[b]], **kw)
        for f in fields:
            assert np.array_equal(full[f][b], alone[f][0]), (b, f)


# ---------------------------------------------------------------------------------------------------- 6. edge cases
def test_degenerate_pairs_give_identity():
    rng = np.random.default_rng(6)
    p = rng.uniform(-1, 1, (50, 3)).astype(np.float32)
    line = (np.linspace(0, 1, 50)[:, None] * np.array([1.0, 2.0, -0.5])).astype(np.float32)
    dup = np.repeat(p[:1], 50, 0)
    sets = [(p[:0], p[:0]), (p[:1], p[:1]), (p[:2], p[:2]),
            (dup, dup),                       # all-duplicate points
            (line, line + 0.3),               # all-collinear
            (p, p / 3.0)]                     # every triple fails the edge checker (|s| = 3 |t|)
    r, _ = run([(a, b, None) for a, b in sets], sample="all", iterations=4000)
    for b in range(len(sets)):
        assert np.array_equal(r["T"][b], np.eye(4, dtype=np.float32)), b
        assert int(r["inliers"][b]) == 0 and int(r["valid_hypotheses"][b]) == 0 and int(r["best_iteration"][b]) == -1, b
    assert np.isfinite(r["T"]).all()


def test_outputs_written_only_for_live_pairs():
    """The C entry point writes B entries of every output and nothing past them (NaN / -7 sentinels)."""
    from roitr_amd import _lib as L
    from roitr_amd import registration as G
    rng = np.random.default_rng(12)
    sets = [make_set(m, 0.5, rng) for m in (300, 40, 0)]
    src = dev(np.concatenate([s[0] for s in sets]))
    tgt = dev(np.concatenate([s[1] for s in sets]))
    st = dev(starts_of([s[0].shape[0] for s in sets]))
    B, rows = 3, int(src.shape[0])
    T = torch.full((B + 2, 4, 4), float("nan"), device="cuda")
    ints = [torch.full((B + 2,), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    sel = torch.full((rows + 5,), -7, dtype=torch.int32, device="cuda")
    keys = torch.arange(B, dtype=torch.int32, device="cuda")
    lib = L.lib()
    nb = int(lib.roitr_registration_workspace_bytes(B, rows, 2000, 0))
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    L.check(lib.roitr_ransac_correspondences(B, st.data_ptr(), rows, src.data_ptr(), tgt.data_ptr(), None, keys.data_ptr(), 2, 100, 3,
                                             0.05, 0.9, 2000, 1, 0, 0, 0, ws.data_ptr(), nb, T.data_ptr(), ints[0].data_ptr(),
                                             ints[1].data_ptr(), ints[2].data_ptr(), ints[3].data_ptr(), sel.data_ptr(),
                                             L.stream_ptr().value), "ransac")
    torch.cuda.synchronize()
    assert torch.isfinite(T[:B]).all() and torch.isnan(T[B:]).all()
    for a in ints:
        assert (a[B:] == -7).all() and (a[:B] != -7).all()
    sel = sel.cpu().numpy()
    assert np.all(sel[100:300] == -7) and np.all(sel[300 + 40:] == -7) and np.all(sel[:100] >= 0) and np.all(sel[300:340] >= 0)


# ---------------------------------------------------------------------------------------------------- 7. weighted Procrustes
def procrustes_ref(src, tgt, weights=None, weight_thresh=0., eps=1e-5):
    """lib/utils.py:159-212 in float64 numpy (batched)."""
    src, tgt = src.astype(np.float64), tgt.astype(np.float64)
    w = np.ones(src.shape[:2]) if weights is None else weights.astype(np.float64)
    w = np.where(w < weight_thresh, 0.0, w)
    wn = w / (w.sum(1, keepdims=True) + eps)
    cs, ct = (src * wn[..., None]).sum(1, keepdims=True), (tgt * wn[..., None]).sum(1, keepdims=True)
    H = np.einsum("bna,bn,bnc->bac", src - cs, w, tgt - ct)
    U, _, Vt = np.linalg.svd(H)
    V, Ut = np.transpose(Vt, (0, 2, 1)), np.transpose(U, (0, 2, 1))
    D = np.tile(np.eye(3), (src.shape[0], 1, 1))
    D[:, 2, 2] = np.sign(np.linalg.det(V @ Ut))
    R = V @ D @ Ut
    t = ct[:, 0] - np.einsum("bij,bj->bi", R, cs[:, 0])
    T = np.tile(np.eye(4), (src.shape[0], 1, 1))
    T[:, :3, :3], T[:, :3, 3] = R, t
    return R, t, T


def test_weighted_procrustes_matches_reference():
    from roitr_amd.registration import weighted_procrustes
    rng = np.random.default_rng(7)
    B, N = 5, 300
    src = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    Rs = np.stack([random_rotation(rng) for _ in range(B)])
    tgt = (np.einsum("bij,bnj->bni", Rs, src) + rng.uniform(-1, 1, (B, 1, 3)) + rng.normal(0, 0.05, (B, N, 3))).astype(np.float32)
    tgt[1] = src[1] * np.array([1, 1, -1], np.float32) + 0.2             # a reflection: det(V U^T) < 0
    w = rng.uniform(0, 1, (B, N)).astype(np.float32)
    for weights, thresh in ((None, 0.0), (w, 0.0), (w, 0.5)):
        R, t, T = procrustes_ref(src, tgt, weights, thresh)
        gR, gt = weighted_procrustes(dev(src), dev(tgt), None if weights is None else dev(weights), weight_thresh=thresh)
        gT = weighted_procrustes(dev(src), dev(tgt), None if weights is None else dev(weights), weight_thresh=thresh,
                                 return_transform=True)
        assert gR.shape == (B, 3, 3) and gt.shape == (B, 3) and gT.shape == (B, 4, 4)
        assert np.abs(gR.cpu().numpy() - R).max() < 1e-5 and np.abs(gt.cpu().numpy() - t).max() < 1e-5
        assert np.abs(gT.cpu().numpy() - T).max() < 1e-5
    assert np.linalg.det(R[1]) > 0.99
    # 2-D input: squeezed outputs
    R, t, T = procrustes_ref(src[2:3], tgt[2:3], w[2:3])
    gR, gt = weighted_procrustes(dev(src[2]), dev(tgt[2]), dev(w[2]))
    gT = weighted_procrustes(dev(src[2]), dev(tgt[2]), dev(w[2]), return_transform=True)
    assert gR.shape == (3, 3) and gt.shape == (3,) and gT.shape == (4, 4)
    assert np.abs(gR.cpu().numpy() - R[0]).max() < 1e-5 and np.abs(gt.cpu().numpy() - t[0]).max() < 1e-5
    assert np.abs(gT.cpu().numpy() - T[0]).max() < 1e-5


# ---------------------------------------------------------------------------------------------------- 8. engine end to end
def test_register_handle_equals_ransac_batch_per_pair():
    from roitr_amd.registration import ransac_batch, register_handle
    from roitr_amd.synthetic import make_pair
    from tests.gpu_util import build_model, pair_to_device
    model = build_model("3DMatch", weights="selective")
    pairs = [pair_to_device(make_pair(2048, config=1, pair_index=i, normals="field")) for i in range(8)]
    keys = [100 + 3 * i for i in range(8)]
    kw = dict(iterations=5000, n_points=1000, refine_iters=1, seed=3)
    with torch.no_grad():
        h = model.launch_batch(pairs, want_gt=True)
        res = model.finish_batch(h)
        reg = {k: v.cpu().numpy() for k, v in register_handle(h, pair_keys=keys, **kw).items()}
    assert sum(int(r["corr_scores"].shape[0]) for r in res) > 0
    for b, r in enumerate(res):
        n = int(r["corr_scores"].shape[0])
        st = torch.tensor([0, n], dtype=torch.int32, device="cuda")
        one = ransac_batch(st, r["src_corr_points"].contiguous(), r["tgt_corr_points"].contiguous(), r["corr_scores"].contiguous(),
                           pair_keys=[keys[b]], **kw)
        for f in ("T", "inliers", "best_iteration", "valid_hypotheses", "n_used"):
            assert np.array_equal(reg[f][b], one[f][0].cpu().numpy()), (b, f)


def test_golden_pair_parity():
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "pair_sel_n1024.npz"))
    src, tgt, conf = g["out.src_corr_points"], g["out.tgt_corr_points"], g["out.corr_scores"]
    assert src.shape[0] == 4740
    r, _ = run([(src, tgt, conf)], sample="all", iterations=3000, seed=0, pair_keys=[0])
    check_parity(src, tgt, r, 0, 0, 0, 3000)     # parity only: the closed-form weights do not promise a recoverable pose


# ---------------------------------------------------------------------------------------------------- 9. Tester
def test_tester_register_is_independent_of_batching(tmp_path):
    from roitr_amd.config import test_config
    from roitr_amd.tester import SyntheticPairs, Tester
    from tests.gpu_util import build_model
    model = build_model("3DMatch", weights="selective")
    data = SyntheticPairs(4, 1024, config=1)
    poses = []
    for ppf in (1, 3):
        d = tmp_path / str(ppf)
        t = Tester(test_config("3DMatch"), model, data, str(d), pairs_per_forward=ppf, evaluate=True, register=True,
                   ransac=dict(iterations=4000))
        t.test()
        assert sorted(t.registration) == [0, 1, 2, 3]
        files = [torch.load(d / "3DMatch" / f"{i}.pth") for i in range(4)]
        assert all(f["est_transform"].shape == (4, 4) for f in files)
        poses.append(np.stack([f["est_transform"].numpy() for f in files]))
    assert np.array_equal(poses[0], poses[1])


# ---------------------------------------------------------------------------------------------------- 10. refusals
@pytest.mark.parametrize("kw,msg", [(dict(ransac_n=4), "ransac_n"), (dict(iterations=0), "iterations"),
                                    (dict(distance_threshold=-0.05), "distance_threshold"),
                                    (dict(distance_threshold=float("nan")), "distance_threshold"),
                                    (dict(edge_similarity=1.5), "edge_similarity"), (dict(edge_similarity=0.0), "edge_similarity")])
def test_refusals(kw, msg):
    from roitr_amd._lib import RoitrError
    rng = np.random.default_rng(1)
    src, tgt, _, _, conf = make_set(100, 0.5, rng)
    with pytest.raises(RoitrError, match=msg):
        run([(src, tgt, conf)], **kw)
