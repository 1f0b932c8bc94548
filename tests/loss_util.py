"""Helpers of the validation-loss tests (tests/test_loss_cpu.py, tests/test_loss_gpu.py, tests/golden/make_loss_golden.py): a seeded
case generator and float64 restatements of lib/loss.py:8-143 (weighted_circle_loss, CoarseMatchingLoss, FineMatchingLoss).

Everything the generator computes is elementwise +, -, * on seeded uniform numbers (no matmul, no transcendental function), so the
float32 inputs are the same bits on every host and the checksums in tests/golden/loss_ref.npz hold.

DECIDED CASES.  The reference measures patch distances as |a|^2 + |b|^2 - 2ab in fp32.  With coordinates bounded by M (after the
transform), each of the three terms is a sum of three products bounded by 3 M^2 and carries at most 3 roundings of the running sum
plus one per product: <= 6 u 3 M^2 = 18 u M^2 for 2ab (doubling is exact), 9 u M^2 for each square norm with the roundings of the
smaller partial sums, and the two additions round values <= 9 M^2 and <= 6 M^2: 15 u M^2; together <= 51 u M^2 with u = 2^-24.
fine_error_bound() returns E = 64 u M^2 (the transform of the source points in fp32 adds < 1 u M^2 at d = 5 cm).  The generator
masks out every source point that has, in float64, a valid target point of its patch with |d^2 - r^2| <= E; every label is then the
same in the reference's form, in the kernel's difference form (whose error is far smaller) and in float64.  At most MAX_MASKED of a
case's source points may go that way (asserted).

FP32 BOUND.  REF_DEVIATION is the largest relative deviation |reference fp32 - float64 restatement| / |float64| over c_loss and
f_loss of the six golden cases, as tests/golden/make_loss_golden.py measured it on the CPU (it prints the figures);
F32_BOUND = 8 x that: the factor covers another summation order and FMA contraction on the GPU.
"""
import hashlib

import numpy as np

RADIUS = 0.05
CIRCLE = dict(positive_margin=0.1, negative_margin=1.4, positive_optimal=0.1, negative_optimal=1.4, log_scale=24.0, positive_overlap=0.1)
MAX_MASKED = 0.02
REF_DEVIATION = 1.28e-7   # measured: 1.277e-07 (c_loss of case 1), rounded up in the third digit
F32_BOUND = 8 * REF_DEVIATION   # 1.024e-06, relative
KEYS = ("tgt_feats", "src_feats", "gt_idx", "gt_overlaps", "tgt_pts", "src_pts", "tgt_masks", "src_masks", "scores", "rot", "trans")


def _rotation(rng):
    q = rng.uniform(-1.0, 1.0, 4)
    while not 0.1 < float(np.sum(q * q)) <= 1.0:
        q = rng.uniform(-1.0, 1.0, 4)
    w, x, y, z = q
    s = 1.0 / (w * w + x * x + y * y + z * z)   # the rotation of a non-unit quaternion: no square root
    return np.array([[1 - 2 * s * (y * y + z * z), 2 * s * (x * y - z * w), 2 * s * (x * z + y * w)],
                     [2 * s * (x * y + z * w), 1 - 2 * s * (x * x + z * z), 2 * s * (y * z - x * w)],
                     [2 * s * (x * z - y * w), 2 * s * (y * z + x * w), 1 - 2 * s * (x * x + y * y)]])


def apply(rot, trans, p):
    """p @ rot.T + trans over the last axis, written out (a BLAS matmul may contract differently from host to host)."""
    return np.stack([p[..., 0] * rot[i, 0] + p[..., 1] * rot[i, 1] + p[..., 2] * rot[i, 2] + trans[i] for i in range(3)], -1)


def fine_error_bound(case):
    """E of the module docstring at the case's coordinate magnitude."""
    f = {k: np.asarray(case[k], np.float64) for k in ("tgt_pts", "src_pts", "rot", "trans")}
    sw = apply(f["rot"], f["trans"], f["src_pts"])
    m = max(float(np.abs(f["tgt_pts"]).max(initial=0.0)), float(np.abs(sw).max(initial=0.0)))
    return 64.0 * 2.0 ** -24 * m * m


def sqdist_f64(case):
    """(patches, L, L) float64 squared distances tgt_i - (src_j rot^T + trans)."""
    f = {k: np.asarray(case[k], np.float64) for k in ("tgt_pts", "src_pts", "rot", "trans")}
    sw = apply(f["rot"], f["trans"], f["src_pts"])
    return ((f["tgt_pts"][:, :, None, :] - sw[:, None, :, :]) ** 2).sum(-1)


def ambiguous_entries(case, radius=RADIUS):
    """(patches, L, L) bool: entries between valid points whose label the reference's fp32 form may decide either way."""
    d2 = sqdist_f64(case)
    live = np.asarray(case["tgt_masks"], bool)[:, :, None] & np.asarray(case["src_masks"], bool)[:, None, :]
    return (np.abs(d2 - radius * radius) <= fine_error_bound(case)) & live


def make_case(seed, L=64, patches=12, n_t=78, n_s=125, D=256, n_gt=300, decided=True):
    """One pair.  Coarse side: n_t / n_s descriptors of norm ~1 (uniform components), n_gt distinct ground-truth node pairs in
    torch.nonzero order with overlaps in (0, 1] -- a fifth of them in (0, 0.1], neither positive nor negative -- the source
    descriptor of a listed pair a noisy copy of its target's.  Fine side: `patches` patches of L points inside a 0.6 m cube around
    the origin (small coordinates keep E, and with it the masked share, small), half of the source points noisy copies of target
    points (some within the 5 cm radius, some not), half uniform in the patch; ~85 % of the points valid; scores uniform in
    (-12, -0.05); a seeded rigid motion.  decided: apply the module docstring's masking."""
    rng = np.random.default_rng(91000 + seed)
    f32 = np.float32
    amp = (3.0 / D) ** 0.5
    tgt_feats = rng.uniform(-1.0, 1.0, (n_t, D)) * amp
    src_feats = rng.uniform(-1.0, 1.0, (n_s, D)) * amp
    flat = np.unique(rng.integers(0, n_t * n_s, n_gt)) if n_t * n_s > 0 else np.zeros(0, np.int64)
    gt_idx = np.stack([flat // max(n_s, 1), flat % max(n_s, 1)], 1).astype(np.int64)
    gt_overlaps = rng.uniform(0.1, 1.0, len(flat))
    low = rng.uniform(0.0, 1.0, len(flat)) < 0.2
    gt_overlaps[low] = rng.uniform(0.001, 0.1, int(low.sum()))
    for k in np.nonzero(~low)[0][::2]:   # every other positive pair: similar descriptors
        src_feats[gt_idx[k, 1]] = tgt_feats[gt_idx[k, 0]] + rng.uniform(-1.0, 1.0, D) * (0.3 * amp)
    rot = _rotation(rng)
    trans = rng.uniform(-0.1, 0.1, 3)
    centre = rng.uniform(-0.2, 0.2, (patches, 1, 3))
    tgt = centre + rng.uniform(-0.08, 0.08, (patches, L, 3))
    perm = rng.permuted(np.tile(np.arange(L), (patches, 1)), axis=1)
    world = np.take_along_axis(tgt, perm[:, :, None], axis=1) + rng.uniform(-0.03, 0.03, (patches, L, 3))
    world[:, L // 2:] = centre + rng.uniform(-0.08, 0.08, (patches, L - L // 2, 3))
    src = apply(rot.T, np.zeros(3), world - trans)   # rot^T (world - trans)
    case = dict(tgt_feats=tgt_feats.astype(f32), src_feats=src_feats.astype(f32), gt_idx=gt_idx, gt_overlaps=gt_overlaps.astype(f32),
                tgt_pts=tgt.astype(f32), src_pts=src.astype(f32), tgt_masks=rng.uniform(0, 1, (patches, L)) < 0.85,
                src_masks=rng.uniform(0, 1, (patches, L)) < 0.85, scores=rng.uniform(-12.0, -0.05, (patches, L + 1, L + 1)).astype(f32),
                rot=rot.astype(f32), trans=trans.astype(f32))
    if decided:
        decide(case)
    return case


def decide(case, radius=RADIUS):
    """Mask out the source points with an undecided label (module docstring); returns the masked share, asserted <= MAX_MASKED."""
    hit = ambiguous_entries(case, radius).any(1)
    share = float(hit.sum()) / max(hit.size, 1)
    assert share <= MAX_MASKED, share
    case["src_masks"] = np.asarray(case["src_masks"], bool) & ~hit
    return share


GOLDEN_SIZES = ((64, 12, 78, 125), (64, 12, 78, 125), (64, 7, 125, 78), (37, 9, 33, 61), (64, 5, 130, 63), (16, 20, 16, 16))   # L, patches, n_t, n_s


def golden_cases():
    """The six cases of tests/golden/loss_ref.npz: the working sizes, then smaller and odd ones."""
    return [make_case(s, *size) for s, size in enumerate(GOLDEN_SIZES)]


def checksum(case):
    h = hashlib.sha256()
    for k in KEYS:
        h.update(np.ascontiguousarray(case[k]).tobytes())
    return h.hexdigest()[:16]


def fine_labels_f64(case, radius=RADIUS):
    """(patches, L+1, L+1) bool labels of lib/loss.py:131-139 from float64 distances."""
    tm, sm = np.asarray(case["tgt_masks"], bool), np.asarray(case["src_masks"], bool)
    gt = (sqdist_f64(case) < radius * radius) & tm[:, :, None] & sm[:, None, :]
    P, L = tm.shape
    labels = np.zeros((P, L + 1, L + 1), bool)
    labels[:, :-1, :-1] = gt
    labels[:, :-1, -1] = (gt.sum(2) == 0) & tm
    labels[:, -1, :-1] = (gt.sum(1) == 0) & sm
    return labels


def fine_f64(case, radius=RADIUS):
    """dict(sum, count, loss): FineMatchingLoss.forward in float64 on the case's float32 inputs; loss is nan without labels."""
    labels = fine_labels_f64(case, radius)
    total = float(np.asarray(case["scores"], np.float64)[labels].sum())
    n = int(labels.sum())
    return dict(sum=total, count=n, loss=-total / n if n else float("nan"), labels=labels)


def fine_interval(case, radius=RADIUS):
    """(lowest, highest, n_ambiguous): the span of the fine loss when every ambiguous entry may take either label.  An ambiguous
    entry (i, j) can also switch the slack labels of its row and column; every other label is fixed.  The loss is the mean of
    -score over the labels: with the fixed ones always in and any subset of the m affected ones, it lies between the smallest mean
    obtained by adding the k smallest affected values and the largest by adding the k largest, over k = 0..m."""
    amb = ambiguous_entries(case, radius)
    P, L = np.asarray(case["tgt_masks"]).shape
    affected = np.zeros((P, L + 1, L + 1), bool)
    affected[:, :-1, :-1] = amb
    affected[:, :-1, -1] = amb.any(2)
    affected[:, -1, :-1] = amb.any(1)
    labels = fine_labels_f64(case, radius)
    v = -np.asarray(case["scores"], np.float64)
    fixed = labels & ~affected
    s0, n0 = float(v[fixed].sum()), int(fixed.sum())
    free = np.sort(v[affected])
    def span(order):
        c = np.concatenate([[0.0], np.cumsum(order)])
        k = np.arange(len(c))
        with np.errstate(invalid="ignore", divide="ignore"):
            return (s0 + c) / (n0 + k)
    lo, hi = span(free), span(free[::-1])
    return float(np.nanmin(lo)), float(np.nanmax(hi)), int(amb.sum())


def _logsumexp(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.exp(x - m).sum(axis=axis))


def coarse_f64(case, positive_margin=0.1, negative_margin=1.4, positive_optimal=0.1, negative_optimal=1.4, log_scale=24.0,
               positive_overlap=0.1):
    """dict(loss, rows, cols): CoarseMatchingLoss.forward in float64 on the case's float32 inputs (square_distance's order of
    operations); loss is nan when no row or no column has both a positive and a negative."""
    t, s = np.asarray(case["tgt_feats"], np.float64), np.asarray(case["src_feats"], np.float64)
    d2 = (-2.0 * (t @ s.T) + (t ** 2).sum(1)[:, None]) + (s ** 2).sum(1)[None, :]
    d = np.sqrt(np.maximum(d2, 1e-12))
    ov = np.zeros_like(d)
    gi = np.asarray(case["gt_idx"], np.int64).reshape(-1, 2)
    ov[gi[:, 0], gi[:, 1]] = np.asarray(case["gt_overlaps"], np.float64)   # the last entry of a repeated pair wins
    pos, neg = ov > float(np.float32(positive_overlap)), ov == 0
    pw = np.maximum(0.0, d - 1e5 * ~pos - positive_optimal) * np.sqrt(ov * pos)
    nw = np.maximum(0.0, negative_optimal - (d + 1e5 * ~neg))
    pt, nt = log_scale * (d - positive_margin) * pw, log_scale * (negative_margin - d) * nw
    out = {}
    for name, axis in (("rows", 1), ("cols", 0)):
        if d.shape[axis] == 0 or d.shape[1 - axis] == 0:
            out[name] = np.zeros(0)
            continue
        keep = (pos.sum(axis) > 0) & (neg.sum(axis) > 0)
        out[name] = (np.logaddexp(0.0, _logsumexp(pt, axis) + _logsumexp(nt, axis)) / log_scale)[keep]
    ok = len(out["rows"]) > 0 and len(out["cols"]) > 0
    out["loss"] = (out["rows"].mean() + out["cols"].mean()) / 2 if ok else float("nan")
    return out


def rel(a, b):
    """|a - b| / |b| (b the float64 value)."""
    return abs(float(a) - float(b)) / abs(float(b))
