"""float64 restatement of the ground-truth side outputs (reference lib/utils.py:474-614: get_node_occlusion_score and
get_node_correspondences) and the seeded inputs the CPU and GPU tests of csrc/gt.hip share.

The kernels decide `d2 < r^2` and `sqrt(d2) < thr` in fp32, so the restatement returns INTERVALS: a point pair whose float64 squared
distance lies within `band` of the threshold is undecided, and every count / ratio / score carries a lower bound (undecided pairs
out) and an upper bound (undecided pairs in).  band = 16 fp32 ulps of the largest squared norm that enters a distance (points of
both clouds, the transformed source points, the pad rows, the threshold itself): square_distance accumulates
-2 s.t + |s|^2 + |t|^2 with about 4 roundings of terms of that size, the transform adds a few ulps of the coordinates times a
distance below the radius, which is far smaller.  On inputs that satisfy the lattice conditions (is_exact) nothing is rounded and
the band is 0: the expectations are then exact.

The enclosing-sphere prune (l.577-586) is not restated: by the triangle inequality it removes only node pairs without any point pair
inside the radius, i.e. pairs whose overlap is 0 anyway, so the final list is all the reference defines.

Layout of a pair (dict of numpy arrays): {tgt,src}_points (n,3) f32, {tgt,src}_nodes (m,3) f32, {tgt,src}_knn_idx (m,64) int32 with
the pad index n for empty slots (the zero row of RIGA_v2.py:86-87), {tgt,src}_knn_mask (m,64) bool, {tgt,src}_node_mask (m,) bool,
rot (3,3) f32, trans (3,) f32.  ref = tgt everywhere, as at model/RIGA_v2.py:91-111.
"""
import numpy as np

LIMIT = 64
POS_RADIUS = 0.05
OCC_THR = 0.0375
ULPS = 16
# fp32 rounding of the final value: two quotients <= 1 (2^-25 each), their sum <= 2 (2^-24), halved exactly -> 2^-24; the
# occlusion score is one quotient (2^-25) and fp32 drops the 1e-10 of the denominator (relative 1e-10): below 2^-24 too
EPS_VALUE = 2.0 ** -24
SHAPES = [(40, 37), (33, 64), (5, 70)]   # (n_t, n_s) nodes: > 1024 matrix entries, > 1 prune workgroup per pair, n_s != max_nodes
STEP = 2.0 ** -8


def f64(a):
    return np.asarray(a, dtype=np.float64)


def on_lattice(a, bound=4.0):
    a = f64(a)
    return bool(np.array_equal(np.round(a / STEP) * STEP, a) and np.abs(a).max() <= bound)


def is_exact(p):
    """The lattice conditions: coordinates (the transformed source and trans included) are multiples of 2^-8 of magnitude <= 4
    and rot is a signed permutation.  Then the products of transform3 / square_distance3 are multiples of 2^-16 below 16 and all
    their sums and the -2 s.t term stay below 256, which fp32 holds exactly: the kernels compute every squared distance without
    rounding.  Squared distances are then multiples of 2^-16, and r^2 = 0.0025 (163.84 steps) and thr^2 = 0.00140625 (92.16 steps) lie
    0.16 steps = 2.4e-6 from the nearest one, far more than the rounding of the fp32 thresholds or of sqrtf."""
    rot, trans = f64(p["rot"]), f64(p["trans"]).reshape(3)
    perm = np.array_equal(np.abs(rot).sum(0), np.ones(3)) and np.array_equal(np.abs(rot).sum(1), np.ones(3)) and set(np.unique(np.abs(rot))) <= {0.0, 1.0}
    return bool(perm and all(on_lattice(a) for a in (p["tgt_points"], p["src_points"], trans, f64(p["src_points"]) @ rot.T + trans)))


def band_of(p, *thresholds2):
    """16 fp32 ulps of the largest squared norm among the pair's clouds (source before and after the transform, pad rows = 0 and
    trans) and the squared thresholds; 0 when the inputs satisfy the lattice conditions (nothing is rounded)."""
    if is_exact(p):
        return 0.0
    rot, trans = f64(p["rot"]), f64(p["trans"]).reshape(3)
    src_w = f64(p["src_points"]) @ rot.T + trans
    m = max([float((f64(a) ** 2).sum(-1).max()) for a in (p["tgt_points"], p["src_points"], src_w, trans[None])] + list(thresholds2))
    return ULPS * float(np.spacing(np.float32(m)))


def partition(points, nodes, limit=LIMIT):
    """lib/utils.py:428-471 in float64 -> (node_mask (m,) bool, knn_idx (m,limit) int32 with pad index n, knn_mask bool)."""
    P, N = f64(points), f64(nodes)
    n, m = P.shape[0], N.shape[0]
    d2 = ((N[:, None, :] - P[None, :, :]) ** 2).sum(-1)
    p2n = d2.argmin(0)
    node_mask = np.zeros(m, bool)
    node_mask[p2n] = True
    own = np.where(p2n[None, :] == np.arange(m)[:, None], d2, np.inf)
    if n < limit:
        own = np.concatenate([own, np.full((m, limit - n), np.inf)], 1)
    order = np.argsort(own, axis=1, kind="stable")[:, :limit]
    mask = np.isfinite(np.take_along_axis(own, order, 1))
    return node_mask, np.where(mask, order, n).astype(np.int32), mask


def _patches(points, idx):
    return np.concatenate([f64(points), np.zeros((1, 3))], 0)[idx]


def corr_intervals(p, pos_radius=POS_RADIUS):
    """Per node pair (i of tgt, j of src): hit counts and the overlap interval.  lo > 0: must be listed; hi == 0: must not."""
    rot, trans = f64(p["rot"]), f64(p["trans"]).reshape(3)
    r2 = float(pos_radius) ** 2
    band = band_of(p, r2)
    R = _patches(p["tgt_points"], p["tgt_knn_idx"])
    S = _patches(p["src_points"], p["src_knn_idx"]) @ rot.T + trans     # pad slots are transformed too; they are masked
    rmask, smask = np.asarray(p["tgt_knn_mask"], bool), np.asarray(p["src_knn_mask"], bool)
    nt, ns = R.shape[0], S.shape[0]
    cnt = {k: np.zeros((nt, ns)) for k in ("rc_lo", "rc_hi", "sc_lo", "sc_hi")}
    n_und = 0
    for i in range(nt):
        d2 = ((R[i][None, :, None, :] - S[:, None, :, :]) ** 2).sum(-1)           # (ns, L, L): [j, p, q]
        valid = rmask[i][None, :, None] & smask[:, None, :]
        cin = valid & (d2 < r2 - band)
        und = valid & ~cin & (d2 <= r2 + band)
        n_und += int(und.sum())
        cnt["rc_lo"][i], cnt["rc_hi"][i] = cin.any(2).sum(1), (cin | und).any(2).sum(1)
        cnt["sc_lo"][i], cnt["sc_hi"][i] = cin.any(1).sum(1), (cin | und).any(1).sum(1)
    live = np.asarray(p["tgt_node_mask"], bool)[:, None] & np.asarray(p["src_node_mask"], bool)[None, :]
    rm, sm = rmask.sum(1).astype(np.float64), smask.sum(1).astype(np.float64)
    live &= (rm[:, None] > 0) & (sm[None, :] > 0)     # 0 / 0 is NaN in the reference, and NaN > 0 is false: never listed
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = np.where(live, (cnt["rc_lo"] / rm[:, None] + cnt["sc_lo"] / sm[None, :]) / 2, 0.0)
        hi = np.where(live, (cnt["rc_hi"] / rm[:, None] + cnt["sc_hi"] / sm[None, :]) / 2, 0.0)
    out = {k: np.where(live, v, 0.0) for k, v in cnt.items()}
    out.update(lo=lo, hi=hi, rm=rm, sm=sm, band=band, live=live, undecided_point_pairs=n_und)
    return out


def _nearest_d2(q, ref, chunk=512):
    out = np.empty(q.shape[0])
    for a in range(0, q.shape[0], chunk):
        out[a:a + chunk] = ((q[a:a + chunk, None, :] - ref[None, :, :]) ** 2).sum(-1).min(1)
    return out


def occ_intervals(p, thr=OCC_THR):
    """Per node the interval of the occlusion score; *_d2 is the float64 squared nearest distance of every PADDED point (n + 1 rows:
    the pad row last) to the padded partner cloud, the source side transformed."""
    rot, trans = f64(p["rot"]), f64(p["trans"]).reshape(3)
    thr2 = float(thr) ** 2
    band = band_of(p, thr2)
    tgt = np.concatenate([f64(p["tgt_points"]), np.zeros((1, 3))], 0)
    src = np.concatenate([f64(p["src_points"]), np.zeros((1, 3))], 0) @ rot.T + trans
    out = dict(band=band)
    for side, q, ref in (("tgt", tgt, src), ("src", src, tgt)):
        d2 = _nearest_d2(q, ref)
        idx, mask = p[side + "_knn_idx"], np.asarray(p[side + "_knn_mask"], np.float64)
        nm = np.asarray(p[side + "_node_mask"], np.float64)
        in_lo, in_hi = (d2 < thr2 - band).astype(np.float64), (d2 <= thr2 + band).astype(np.float64)
        den = mask.sum(1) + 1e-10
        out[side + "_d2"] = d2
        out[side + "_s_lo"], out[side + "_s_hi"], out[side + "_m"] = (in_lo[idx] * mask).sum(1), (in_hi[idx] * mask).sum(1), mask.sum(1)
        out[side + "_lo"], out[side + "_hi"] = out[side + "_s_lo"] / den * nm, out[side + "_s_hi"] / den * nm
    return out


def undecided_counts(civ, oiv):
    """(undecided node pairs, listed node pairs, undecided scores, nodes) of one pair.  A node pair is undecided when it may or may
    not be listed, or is listed with an interval of positive width."""
    must = int((civ["lo"] > 0).sum())
    may = int(((civ["lo"] == 0) & (civ["hi"] > 0)).sum()) + int(((civ["lo"] > 0) & (civ["hi"] > civ["lo"])).sum())
    n_nodes = oiv["tgt_lo"].shape[0] + oiv["src_lo"].shape[0]
    und = int((oiv["tgt_hi"] > oiv["tgt_lo"]).sum() + (oiv["src_hi"] > oiv["src_lo"]).sum())
    return may, must, und, n_nodes


def undecided_shares(civ, oiv):
    """(undecided node pairs / listed node pairs, undecided scores / nodes) of one pair."""
    may, must, und, n_nodes = undecided_counts(civ, oiv)
    return may / max(must, 1), und / n_nodes


def check_corr(idx, ov, civ, what=""):
    """idx (C,2) [tgt, src], ov (C,): row-major order, must / must-not, every overlap inside its interval."""
    idx, ov = np.asarray(idx, np.int64).reshape(-1, 2), np.asarray(ov, np.float64).reshape(-1)
    nt, ns = civ["lo"].shape
    assert idx.shape[0] == ov.shape[0], what
    assert idx.size == 0 or (idx.min() >= 0 and idx[:, 0].max() < nt and idx[:, 1].max() < ns), (what, "index out of range")
    flat = idx[:, 0] * ns + idx[:, 1]
    assert np.all(np.diff(flat) > 0), (what, "not in row-major (i, j) order")
    listed = np.zeros((nt, ns), bool)
    listed[idx[:, 0], idx[:, 1]] = True
    missing, extra = np.argwhere((civ["lo"] > 0) & ~listed), np.argwhere((civ["hi"] == 0) & listed)
    assert missing.shape[0] == 0, (what, "node pairs with a positive lower bound are not listed", missing[:8].tolist())
    assert extra.shape[0] == 0, (what, "node pairs with upper bound 0 are listed", extra[:8].tolist())
    lo, hi = civ["lo"][idx[:, 0], idx[:, 1]], civ["hi"][idx[:, 0], idx[:, 1]]
    bad = np.nonzero(~((ov > 0) & (ov >= lo - EPS_VALUE) & (ov <= hi + EPS_VALUE)))[0]
    assert bad.size == 0, (what, "overlaps outside their interval", [(idx[b].tolist(), ov[b], lo[b], hi[b]) for b in bad[:8]])


def check_occ(score, oiv, side, what=""):
    score = np.asarray(score, np.float64).reshape(-1)
    lo, hi = oiv[side + "_lo"], oiv[side + "_hi"]
    assert score.shape == lo.shape, (what, side)
    bad = np.nonzero(~((score >= lo - EPS_VALUE) & (score <= hi + EPS_VALUE)))[0]
    assert bad.size == 0, (what, side, "scores outside their interval", [(int(b), score[b], lo[b], hi[b]) for b in bad[:8]])


def exact_overlaps(civ, idx):
    """fp32 value of (rc / rm + sc / sm) / 2 in that order, for decided node pairs."""
    f = np.float32
    i, j = idx[:, 0], idx[:, 1]
    return (civ["rc_lo"][i, j].astype(f) / civ["rm"][i].astype(f) + civ["sc_lo"][i, j].astype(f) / civ["sm"][j].astype(f)) / f(2.0)


def exact_scores(oiv, p, side):
    """fp32 value of s / (m + 1e-10f) * node_mask for decided scores."""
    f = np.float32
    return oiv[side + "_s_lo"].astype(f) / (oiv[side + "_m"].astype(f) + f(1e-10)) * np.asarray(p[side + "_node_mask"], f)


# ------------------------------------------------------------------------------------------------ seeded inputs
def signed_permutation(rng):
    m = np.zeros((3, 3))
    m[np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3)
    return m


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _finish(tgt_w, src_w, rot, trans, nt, ns, rng):
    """World-frame clouds -> a pair: the source is carried back through (rot, trans), nodes are random picks, the partition float64."""
    src = (f64(src_w) - trans) @ rot            # rows R^T (w - t)
    p = dict(tgt_points=np.ascontiguousarray(tgt_w, np.float32), src_points=np.ascontiguousarray(src, np.float32),
             rot=np.ascontiguousarray(rot, np.float32), trans=np.ascontiguousarray(trans, np.float32))
    for side, n_nodes in (("tgt", nt), ("src", ns)):
        pts = p[side + "_points"]
        p[side + "_nodes"] = pts[rng.choice(pts.shape[0], n_nodes, replace=False)].copy()
        p[side + "_node_mask"], p[side + "_knn_idx"], p[side + "_knn_mask"] = partition(pts, p[side + "_nodes"])
    return p


def _boxes(nt, ns, per_node, density):
    """Edge lengths of the two boxes (same density) and the target box's shift along x: partial overlap."""
    a_t, a_s = (nt * per_node / density) ** (1 / 3), (ns * per_node / density) ** (1 / 3)
    return a_t, a_s, 0.35 * min(a_t, a_s)


def lattice_pair(seed, nt, ns, per_node=50, density=12000.0, src_shift=0.0, pad_row_hits=False):
    """Coordinates are multiples of 2^-8, rot a signed permutation, trans on the lattice: every product and sum of the kernels'
    square_distance3 / transform3 is exact in fp32 (magnitudes < 4 at step 2^-8: squares and their sums below 256 at step 2^-16),
    and no squared distance can equal r^2 = 0.0025 or thr^2, which are no lattice values.  src_shift moves the source cloud along x
    in the world frame (exactness is then not claimed).  pad_row_hits: trans sits inside the target-only part of the scene, so the
    source pad row lands next to target points after the transform, where no source point is."""
    rng = np.random.default_rng(seed)
    a_t, a_s, shift = _boxes(nt, ns, per_node, density)
    c0 = 1.0 + np.round(rng.random(3) * 0.5 / STEP) * STEP
    lat = lambda x: np.round(x / STEP) * STEP   # noqa: E731
    src_w = c0 + lat(rng.random((ns * per_node, 3)) * a_s)
    tgt_w = c0 + lat(rng.random((nt * per_node, 3)) * a_t)
    tgt_w[:, 0] -= lat(shift)                     # part of the target box lies outside the source box
    src_w[:, 0] += src_shift
    if pad_row_hits:
        rot = np.eye(3)[rng.permutation(3)]
        lonely = tgt_w[np.argmin(tgt_w[:, 0])]    # the target point farthest outside the source box
        trans = lonely + STEP * np.array([1.0, -1.0, 1.0])
    else:
        rot = signed_permutation(rng)
        u_sign = np.sign((np.ones(3) @ rot))       # sign of R^T w per source axis (w > 0)
        s0 = np.where(u_sign > 0, lat(rng.random(3) * 0.5), 4.0 - lat(rng.random(3) * 0.5))
        trans = -(rot @ s0)                        # src = R^T w + s0 stays inside [0, 4)
    return _finish(tgt_w, src_w, rot, trans, nt, ns, rng)


def random_pair(seed, nt, ns, per_node=50, density=12000.0):
    """synthetic.make_pair-like: uniform clouds of one scene, partial overlap, full-range random rotation.  The scene is centred at the
    origin and trans is small, so that |p|^2 < 1 and the band stays below 0.1 % of thr^2."""
    rng = np.random.default_rng(seed)
    a_t, a_s, shift = _boxes(nt, ns, per_node, density)
    src_w = (rng.random((ns * per_node, 3)) - 0.5) * a_s
    tgt_w = (rng.random((nt * per_node, 3)) - 0.5) * a_t
    tgt_w[:, 0] -= shift
    return _finish(tgt_w, src_w, random_rotation(rng), rng.uniform(-0.2, 0.2, 3), nt, ns, rng)


def ball_pair(seed, n_nodes=70, n_points=700, steps=6):
    """Target = source (identity transform): distinct lattice points inside a ball of radius `steps` lattice steps.  steps = 6:
    radius 0.0234 < 0.5 pos_radius, every point pair is closer than 0.0469 and every node pair has overlap exactly 1.  steps = 9:
    diameter 0.070 > pos_radius, the overlaps differ from one node pair to the next."""
    rng = np.random.default_rng(seed)
    g = np.arange(-steps, steps + 1)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    cells = cells[(cells ** 2).sum(1) <= steps * steps]
    w = 2.0 + STEP * cells[rng.choice(cells.shape[0], n_points, replace=False)]
    p = _finish(w, w, np.eye(3), np.zeros(3), n_nodes, n_nodes, rng)
    for k in ("points", "nodes", "node_mask", "knn_idx", "knn_mask"):
        p["src_" + k] = p["tgt_" + k].copy()
    return p


def lattice_batch(seed=11):
    return [lattice_pair(seed + b, nt, ns) for b, (nt, ns) in enumerate(SHAPES)]


def random_batch(seed=23):
    return [random_pair(seed + b, nt, ns) for b, (nt, ns) in enumerate(SHAPES)]


BALL_STEPS = (6, 6, 9, 9)


def ball_batch(seed=31):
    """Four (70, 70) pairs: two whose overlaps are all exactly 1, two with wider balls whose overlaps vary, so that a triple computed
    from another triple's records shows."""
    return [ball_pair(seed + b, steps=st) for b, st in enumerate(BALL_STEPS)]


def _shorten(p, side, node, keep):
    n = p[side + "_points"].shape[0]
    valid = np.nonzero(p[side + "_knn_mask"][node])[0]
    assert valid.size >= keep, (side, node, valid.size, keep)
    p[side + "_knn_mask"][node, valid[keep:]] = False
    p[side + "_knn_idx"][node, valid[keep:]] = n


def shorten_patches(p, keeps=(1, 17, 63)):
    """On both sides the first len(keeps) full patches keep only that many valid points; the other slots get the pad index."""
    for side in ("tgt", "src"):
        full = np.nonzero(p[side + "_knn_mask"].sum(1) == LIMIT)[0]
        assert full.size >= len(keeps), (side, full.size)
        for node, keep in zip(full[:len(keeps)], keeps):
            _shorten(p, side, node, keep)
    return p


EDGES = ("node_masks", "short_patches", "pad_row", "far_pair", "sphere_zero", "single")


def edge_batch(name):
    """-> (pairs, exact): exact[b] tells whether pair b satisfies the lattice conditions (bit-exact expectations)."""
    if name == "node_masks":        # live-looking nodes (full patches, real overlaps) switched off on both sides
        p = lattice_pair(101, 12, 11)
        p["tgt_node_mask"][[0, 5, 11]] = False
        p["src_node_mask"][[2, 10]] = False
        return [p], [True]
    if name == "short_patches":     # 1, 17 and 63 valid points, the other slots hold the pad index
        p = lattice_pair(102, 12, 11, per_node=110)
        shorten_patches(p)
        return [p], [True]
    if name == "pad_row":
        return [lattice_pair(103, 12, 11, pad_row_hits=True)], [True]
    if name == "far_pair":          # the middle pair's clouds are 10 m apart
        return [lattice_pair(104, 12, 11), lattice_pair(105, 9, 14, src_shift=10.0), lattice_pair(106, 7, 13)], [True, False, True]
    if name == "sphere_zero":
        return [lattice_pair(107, 12, 11)], [True]
    if name == "single":
        return [lattice_pair(108, 40, 37)], [True]
    raise KeyError(name)


def sphere_pass(p, pos_radius=POS_RADIUS, margin=1e-4):
    """Node pairs that pass the enclosing-sphere test of l.577-586 in float64 by at least `margin` (far above fp32 rounding)."""
    rot, trans = f64(p["rot"]), f64(p["trans"]).reshape(3)
    rn, sn = f64(p["tgt_nodes"]), f64(p["src_nodes"]) @ rot.T + trans
    R = _patches(p["tgt_points"], p["tgt_knn_idx"])
    S = _patches(p["src_points"], p["src_knn_idx"]) @ rot.T + trans
    rmax = (np.linalg.norm(R - rn[:, None], axis=-1) * p["tgt_knn_mask"]).max(1)
    smax = (np.linalg.norm(S - sn[:, None], axis=-1) * p["src_knn_mask"]).max(1)
    nd = np.linalg.norm(rn[:, None] - sn[None], axis=-1)
    live = np.asarray(p["tgt_node_mask"], bool)[:, None] & np.asarray(p["src_node_mask"], bool)[None, :]
    return (rmax[:, None] + smax[None, :] + pos_radius - nd > margin) & live


def sphere_pass_zero_overlap(p, civ, pos_radius=POS_RADIUS, margin=1e-4):
    """Node pairs that pass the enclosing-sphere test although no point pair can be inside the radius."""
    return sphere_pass(p, pos_radius, margin) & civ["live"] & (civ["hi"] == 0)


def pack(pairs):
    """The kernels' batched layout: clouds [src_0..src_{B-1}, tgt_0..tgt_{B-1}], cumulative offsets, rot (B,3,3), trans (B,3)."""
    B = len(pairs)
    order = [(p, "src") for p in pairs] + [(p, "tgt") for p in pairs]
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([p[s + "_" + k] for p, s in order], 0).astype(dt))   # noqa: E731
    n_nodes = [p[s + "_nodes"].shape[0] for p, s in order]
    return dict(pairs=B, points=cat("points", np.float32), nodes=cat("nodes", np.float32), knn_idx=cat("knn_idx", np.int32),
                knn_mask=cat("knn_mask", np.int32), node_masks=cat("node_mask", np.int32),
                pt_offset=np.cumsum([p[s + "_points"].shape[0] for p, s in order]).astype(np.int32),
                node_offset=np.cumsum(n_nodes).astype(np.int32), max_nodes=max(n_nodes),
                cloud_of_node=np.repeat(np.arange(2 * B), n_nodes).astype(np.int32),
                rot=np.stack([p["rot"] for p in pairs]).astype(np.float32),
                trans=np.stack([np.asarray(p["trans"]).reshape(3) for p in pairs]).astype(np.float32))
