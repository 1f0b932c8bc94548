"""GPU: the matching-tail kernels of csrc/matching.hip called directly, against float64 / integer restatements written here.

Optimal transport (ot_kernel, ot_log_kernel) against the log-domain iteration of model/modules.py:10-72 in float64, on both sides
of the OT_FAST_SPREAD dispatch (roitr_ot_stats tells which kernel served a patch).  Fine matching (fine_flag / fine_scan /
fine_emit) against FineMatching.compute_correspondence_matrix on arbitrary score matrices, both top-k paths (k <= 4 in registers,
k > 4 by wave maxima), with bit-identical ties across the k boundary.  Both patch layouts (strided with dead slots, compacted by
roitr_patch_offsets with and without a cut) through the C structs, against the same patches run alone, with NaN / -7 sentinels
where the kernels must not write.  roitr_patch_gather in both layouts.  point_to_node_partition on clouds whose coordinates are
multiples of 1/64, so that every squared distance is exact in fp32 and float64 alike and the restatement must agree bit for bit,
ties included; nodes owning 64, 65, 2048 and 2049 points (the last one takes the arg-min fallback) and none.  Coarse and adaptive
matching at the branches the stage tests do not reach.

Inputs with a discrete answer are built with margins far above fp32 expf error (fine-matching log scores on a 0.01 grid), or
with exact ties on purpose.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OTN = 65


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def i32(a):
    return dev(np.asarray(a, dtype=np.int32))


def _lib():
    from roitr_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------ optimal transport
def ot_ref(scores, rm, cm, alpha, num_iter):
    """model/modules.py:28-68 in float64: (B, 64, 64) -> (B, 65, 65)."""
    B = scores.shape[0]
    S = np.full((B, OTN, OTN), float(alpha))
    S[:, :64, :64] = scores
    prm = np.zeros((B, OTN), bool)
    prm[:, :64] = ~rm
    pcm = np.zeros((B, OTN), bool)
    pcm[:, :64] = ~cm
    S[prm[:, :, None] | pcm[:, None, :]] = -1e6
    nvr, nvc = rm.sum(1).astype(np.float64), cm.sum(1).astype(np.float64)
    norm = -np.log(nvr + nvc)
    lmu = np.repeat(norm[:, None], OTN, 1)
    lmu[:, 64] = np.log(nvc) + norm
    lmu[prm] = -1e6
    lnu = np.repeat(norm[:, None], OTN, 1)
    lnu[:, 64] = np.log(nvr) + norm
    lnu[pcm] = -1e6

    def lse(x, axis):
        m = x.max(axis=axis, keepdims=True)
        return (m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True))).squeeze(axis)

    u, v = np.zeros_like(lmu), np.zeros_like(lnu)
    for _ in range(num_iter):
        u = lmu - lse(S + v[:, None, :], 2)
        v = lnu - lse(S + u[:, :, None], 1)
    return S + u[:, :, None] + v[:, None, :] - norm[:, None, None]


def ot_valid(rm, cm):
    B = rm.shape[0]
    prm = np.concatenate([rm, np.ones((B, 1), bool)], 1)
    pcm = np.concatenate([cm, np.ones((B, 1), bool)], 1)
    return prm[:, :, None] & pcm[:, None, :]


def ot_stats(enable):
    out = (ctypes.c_ulonglong * 3)()
    L = _lib()
    L.check(L.lib().roitr_ot_stats(ctypes.c_int(enable), out), "ot_stats")
    return [int(x) for x in out]


def ot_raw(scores, rm, cm, alpha, num_iter=100, n_corr=None, num_corr=None, pair_off=None, slots=0, pairs=1):
    """roitr_optimal_transport through the C struct.  scores / masks are slot arrays (patches, 64, 64) / (patches, 64); the output
    starts as NaN everywhere."""
    from roitr_amd import ops
    L = _lib()
    P = scores.shape[0]
    out = torch.full((P, OTN, OTN), float("nan"), dtype=torch.float32, device="cuda")
    sc, r, c = dev(scores.astype(np.float32)), i32(rm), i32(cm)
    al = torch.tensor([alpha], dtype=torch.float32, device="cuda")
    nc = i32(n_corr if n_corr is not None else [P])
    a = ops._OT(pairs, P if num_corr is None else num_corr, 64, int(num_iter), L.ptr(nc), L.ptr(sc), L.ptr(r), L.ptr(c), L.ptr(al),
                L.ptr(out), L.ptr(pair_off), int(slots))
    L.check(L.lib().roitr_optimal_transport(ctypes.byref(a), L.stream_ptr()), "optimal_transport")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def ot_err(got, ref, valid):
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref)))[valid].max())


def mask_set():
    """The seven row / column mask patterns (name, rows, cols)."""
    ar = np.arange(64)
    one = lambda i: ar == i
    full = np.ones(64, bool)
    return [("all", full, full), ("one_row", one(17), full), ("one_col", full, one(40)), ("lane0", one(0), one(0)),
            ("lane63", one(63), one(63)), ("alternating", ar % 2 == 0, ar % 2 == 1), ("64x1", full, one(63))]


OT_TOL = 1e-4


@pytest.mark.parametrize("sigma", [0.1, 1.0, 5.0])
@pytest.mark.parametrize("alpha", [-2.0, 0.0, 1.0, 5.0])
def test_optimal_transport_against_float64(sigma, alpha):
    """Every mask pattern at once (one patch each), 1 / 2 / 7 / 100 iterations: valid entries, dustbin row and column included,
    within 1e-4 relative above magnitude 1; masked entries below -1e5."""
    rng = np.random.default_rng(int(sigma * 10) * 31 + int(alpha) + 7)
    ms = mask_set()
    B = len(ms)
    scores = (sigma * rng.standard_normal((B, 64, 64))).astype(np.float32)
    rm = np.stack([m[1] for m in ms])
    cm = np.stack([m[2] for m in ms])
    valid = ot_valid(rm, cm)
    worst = 0.0
    for it in (1, 2, 7, 100):
        got = ot_raw(scores, rm, cm, alpha, it)
        ref = ot_ref(scores.astype(np.float64), rm, cm, alpha, it)
        assert np.isfinite(got[valid]).all()
        for b in range(B):
            e = ot_err(got[b], ref[b], valid[b])
            worst = max(worst, e)
            assert e <= OT_TOL, (ms[b][0], it, e)
        assert (got[~valid] < -1e5).all()
    print(f"OT sigma={sigma} alpha={alpha}: max relative error {worst:.2e}")


def spread_patch(rng, half, alpha=0.0, rows_at=None):
    """Scores in [alpha - half, alpha + half] with both ends present in every row listed (default: all rows): row range 2 * half,
    the dustbin score alpha inside it."""
    s = rng.uniform(alpha - 0.9 * half, alpha + 0.9 * half, (64, 64)).astype(np.float32)
    for r in (range(64) if rows_at is None else rows_at):
        s[r, r % 64] = alpha - half
        s[r, (r + 7) % 64] = alpha + half
    return s


def test_optimal_transport_dispatch_boundary():
    """OT_FAST_SPREAD = 30: a row range of 29.5 stays on ot_kernel, 30.5 in ONE row sends the patch to ot_log_kernel, and so do far
    wider ranges; values of masked rows / columns do not count.  roitr_ot_stats must show exactly the log-served patches, and every
    patch must match float64 either way."""
    rng = np.random.default_rng(5)
    full = np.ones(64, bool)
    cases = []   # (scores, rows, cols, on the log path)
    cases.append((spread_patch(rng, 14.75), full, full, False))
    s = spread_patch(rng, 14.75)
    s[9] = spread_patch(rng, 15.25)[9]
    cases.append((s, full, full, True))
    s = spread_patch(rng, 14.75)
    cm = full.copy()
    cm[[3, 50]] = False
    s[:, 3], s[:, 50] = 400.0, -400.0    # masked columns far outside the range
    rmk = full.copy()
    rmk[20] = False
    s[20] = 1000.0 * rng.standard_normal(64)
    cases.append((s, rmk, cm, False))
    cases.append((spread_patch(rng, 14.75, alpha=0.5), full, full, False))   # shifted by 0.5, alpha = 0 still inside: 29.5
    cases.append((spread_patch(rng, 100.0), full, full, True))
    s = rng.standard_normal((64, 64)).astype(np.float32)
    s[np.arange(64), rng.permutation(64)] = 150.0
    cases.append((s, full, full, True))
    cases.append((spread_patch(rng, 14.0, alpha=-1.0), full, full, False))
    scores = np.stack([c[0] for c in cases])
    rm = np.stack([c[1] for c in cases])
    cm = np.stack([c[2] for c in cases])
    alphas = [0.0] * len(cases)
    alphas[6] = -1.0   # the dustbin score is shared by a launch: the last case was built around alpha = -1
    want_log = 0
    for alpha in sorted(set(alphas)):
        sel = [i for i, a in enumerate(alphas) if a == alpha]
        ot_stats(1)
        got = ot_raw(scores[sel], rm[sel], cm[sel], alpha)
        st = ot_stats(0)
        ref = ot_ref(scores[sel].astype(np.float64), rm[sel], cm[sel], alpha, 100)
        valid = ot_valid(rm[sel], cm[sel])
        for j, i in enumerate(sel):
            e = ot_err(got[j], ref[j], valid[j])
            assert e <= OT_TOL, (i, e)
        assert (got[~valid] < -1e5).all()
        want = sum(1 for i in sel if cases[i][3])
        want_log += want
        assert st[0] == len(sel) - want and st[2] == want, (alpha, st, want)
    assert want_log >= 3 and want_log < len(cases)


def test_optimal_transport_dispatch_counts_rows_with_the_dustbin():
    """A row whose scores span 29 but sit 1.5 above alpha: range 30.5 with the dustbin -> ot_log_kernel; the same row 0.5 above
    alpha: 29.5 -> ot_kernel."""
    rng = np.random.default_rng(11)
    full = np.ones(64, bool)
    base = rng.uniform(-2.0, 2.0, (2, 64, 64)).astype(np.float32)
    base[0, 5, :] = np.linspace(1.5, 30.5, 64, dtype=np.float32)   # min 1.5 above alpha = 0 -> 30.5
    base[1, 5, :] = np.linspace(-28.5, 0.5, 64, dtype=np.float32)  # max 0.5 above alpha, min 28.5 below -> 29.0 (alpha inside)
    base[1, 6, :] = np.linspace(0.5, 29.5, 64, dtype=np.float32)   # alpha = 0 below the row: range 29.5
    for b, logp in ((0, 1), (1, 0)):
        ot_stats(1)
        got = ot_raw(base[b:b + 1], full[None], full[None], 0.0)
        st = ot_stats(0)
        assert st[2] == logp and st[0] == 1 - logp, (b, st)
        ref = ot_ref(base[b:b + 1].astype(np.float64), full[None], full[None], 0.0, 100)
        assert ot_err(got[0], ref[0], ot_valid(full[None], full[None])[0]) <= OT_TOL


def _ot_layout_inputs(rng, P):
    scores = (2.0 * rng.standard_normal((P, 64, 64))).astype(np.float32)
    scores[1] = spread_patch(rng, 40.0)             # one patch on the log path
    rm = rng.random((P, 64)) > 0.2
    cm = rng.random((P, 64)) > 0.3
    rm[:, 0] = cm[:, 0] = True
    return scores, rm, cm


def test_optimal_transport_strided_layout_with_dead_slots():
    rng = np.random.default_rng(21)
    pairs, num_corr, n_corr = 3, 4, [4, 2, 0]
    P = pairs * num_corr
    scores, rm, cm = _ot_layout_inputs(rng, P)
    live = [b * num_corr + p for b in range(pairs) for p in range(n_corr[b])]
    dead = [s for s in range(P) if s not in live]
    scores[dead] = np.nan                            # never read
    got = ot_raw(scores, rm, cm, 1.0, n_corr=n_corr, num_corr=num_corr, pairs=pairs)
    assert np.isnan(got[dead]).all()
    for s in live:
        alone = ot_raw(scores[s:s + 1], rm[s:s + 1], cm[s:s + 1], 1.0)
        assert np.array_equal(got[s].view(np.uint32), alone[0].view(np.uint32)), s
    ref = ot_ref(scores[live].astype(np.float64), rm[live], cm[live], 1.0, 100)
    valid = ot_valid(rm[live], cm[live])
    for j, s in enumerate(live):
        assert ot_err(got[s], ref[j], valid[j]) <= OT_TOL, s


def patch_offsets(n_corr, slots):
    L = _lib()
    po = torch.full((len(n_corr) + 1,), -7, dtype=torch.int32, device="cuda")
    L.check(L.lib().roitr_patch_offsets(len(n_corr), L.ptr(i32(n_corr)), int(slots), L.ptr(po), L.stream_ptr()), "patch_offsets")
    torch.cuda.synchronize()
    return po


def host_pair_off(n_corr, slots):
    return np.minimum(np.concatenate([[0], np.cumsum(n_corr)]), slots).astype(np.int32)


@pytest.mark.parametrize("n_corr,slots", [([3, 0, 2], 8), ([3, 0, 4], 5), ([0, 0, 1], 1), ([2, 1, 0, 0, 3], 6)])
def test_optimal_transport_compacted_layout(n_corr, slots):
    """pair_off from roitr_patch_offsets (a cut when the counts add up to more than the slots); slots past pair_off[pairs] keep
    their NaN, live slots equal the patch run alone."""
    rng = np.random.default_rng(31 + slots)
    po = patch_offsets(n_corr, slots)
    assert np.array_equal(po.cpu().numpy(), host_pair_off(n_corr, slots))
    live = int(host_pair_off(n_corr, slots)[-1])
    scores, rm, cm = _ot_layout_inputs(rng, slots + 1)
    scores, rm, cm = scores[:slots], rm[:slots], cm[:slots]
    scores[live:] = np.nan
    got = ot_raw(scores, rm, cm, -0.5, n_corr=n_corr, num_corr=10, pair_off=po, slots=slots, pairs=len(n_corr))
    assert np.isnan(got[live:]).all()
    for s in range(live):
        alone = ot_raw(scores[s:s + 1], rm[s:s + 1], cm[s:s + 1], -0.5)
        assert np.array_equal(got[s].view(np.uint32), alone[0].view(np.uint32)), s


# ------------------------------------------------------------------------------------------------ fine matching
def fine_ref_flags(x, rm, cm, k, mutual, conf):
    """FineMatching.compute_correspondence_matrix (modules.py:228-266) on exp(x[:, :64, :64]) in float64; ties rank the lower index
    first (the kernel's documented order)."""
    E = np.exp(x[:, :64, :64].astype(np.float64))
    B = E.shape[0]
    out = np.zeros((B, 64, 64), bool)
    for b in range(B):
        e = E[b]
        rsel = np.zeros((64, 64), bool)
        csel = np.zeros((64, 64), bool)
        ro = np.argsort(-e, axis=1, kind="stable")[:, :k]
        rsel[np.arange(64)[:, None], ro] = True
        co = np.argsort(-e, axis=0, kind="stable")[:k, :]
        csel[co, np.arange(64)[None, :]] = True
        rc, cc = rsel & (e > conf), csel & (e > conf)
        f = (rc & cc) if mutual else (rc | cc)
        out[b] = f & rm[b][:, None] & cm[b][None, :]
    return out


def fine_scores(rng, B):
    """(B, 65, 65) log scores on a 0.01 grid in [-6, 0): unequal values differ by far more than expf error, equal ones are the
    same bits.  On top, bit-identical duplicate rows / columns and ties planted at the k boundary for every k in use."""
    x = np.empty((B, OTN, OTN), np.float32)
    for b in range(B):
        x[b] = (-0.01 * (1 + rng.permutation(600 * 8)[:OTN * OTN] % 600)).reshape(OTN, OTN)
        x[b, 64, :] = x[b, :, 64] = 5.0                  # the dustbin row / column: dropped, must not matter
        x[b, 11] = x[b, 40]                              # duplicate rows (tie in every column)
        x[b, :, 52] = x[b, :, 7]                         # duplicate columns (tie in every row)
        for r, kk in ((3, 1), (5, 2), (8, 3), (13, 4), (21, 5), (34, 8), (44, 3), (50, 5)):
            order = np.argsort(-x[b, r, :64], kind="stable")
            c_in, c_out = order[kk - 1], order[kk + 3]   # the k-th best and one below the boundary
            x[b, r, c_out] = x[b, r, c_in]               # equal bits: the lower column index takes the place
        for c, kk in ((2, 2), (30, 4), (61, 8)):
            order = np.argsort(-x[b, :64, c], kind="stable")
            x[b, order[kk + 2], c] = x[b, order[kk - 1], c]
    return x


def fine_raw(x, rp, cp, rm, cm, k, mutual, conf, gs=None, pairs=1, num_corr=None, n_corr=None, pair_off=None, slots=0,
             out_cap=None, pair_starts=False):
    """roitr_fine_matching through the C struct; output rows past what is written keep their sentinels (NaN points / scores,
    -7 patch numbers)."""
    from roitr_amd import ops
    L = _lib()
    P = x.shape[0]
    cap = P * 64 * 64 if out_cap is None else out_cap
    room = P * 64 * 64 + 8
    flags = torch.zeros(P * 64 * 64, dtype=torch.uint8, device="cuda")
    counts = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    offs = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    n_out = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    o_r = torch.full((room, 3), float("nan"), device="cuda")
    o_c = torch.full((room, 3), float("nan"), device="cuda")
    o_s = torch.full((room,), float("nan"), device="cuda")
    o_p = torch.full((room,), -7, dtype=torch.int32, device="cuda")
    ps = torch.full((pairs + 1,), -7, dtype=torch.int32, device="cuda") if pair_starts else None
    t = [dev(x.astype(np.float32)), i32(rm), i32(cm), dev(rp.astype(np.float32)), dev(cp.astype(np.float32)),
         dev(gs.astype(np.float32)) if gs is not None else None, i32(n_corr if n_corr is not None else [P])]
    a = ops._Fine(pairs, P if num_corr is None else num_corr, 64, int(k), int(mutual), float(conf), L.ptr(t[6]), L.ptr(t[0]),
                  L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), L.ptr(t[4]), L.ptr(t[5]), L.ptr(flags), L.ptr(counts), L.ptr(offs),
                  L.ptr(n_out), L.ptr(o_r), L.ptr(o_c), L.ptr(o_s), L.ptr(o_p), int(cap), L.ptr(pair_off), int(slots), L.ptr(ps))
    L.check(L.lib().roitr_fine_matching(ctypes.byref(a), L.stream_ptr()), "fine_matching")
    torch.cuda.synchronize()
    h = lambda z: None if z is None else z.cpu().numpy()
    return dict(flags=h(flags).reshape(P, 64, 64).astype(bool), counts=h(counts), offsets=h(offs), n_out=int(n_out.item()),
                row=h(o_r), col=h(o_c), score=h(o_s), patch=h(o_p), pair_starts=h(ps))


def fine_expect(x, rp, cp, rm, cm, k, mutual, conf, g, patches):
    """The emitted list of `patches` in order: (row point, col point, float64 score, patch) in torch.nonzero order."""
    f = fine_ref_flags(x[patches], rm[patches], cm[patches], k, mutual, conf)
    rows, cols, scs, pat = [], [], [], []
    for j, s in enumerate(patches):
        ii, jj = np.nonzero(f[j])
        rows.append(rp[s][ii])
        cols.append(cp[s][jj])
        scs.append(np.exp(x[s, ii, jj].astype(np.float64)) * (1.0 if g is None else float(g[j])))
        pat.append(np.full(len(ii), s))
    cat = lambda z, w: np.concatenate(z) if z else np.zeros((0,) + w)
    return f, cat(rows, (3,)), cat(cols, (3,)), cat(scs, ()), cat(pat, ())


def fine_inputs(rng, P, dead_cols=True):
    x = fine_scores(rng, P)
    rp = rng.standard_normal((P, 64, 3)).astype(np.float32)
    cp = rng.standard_normal((P, 64, 3)).astype(np.float32)
    rm = rng.random((P, 64)) > 0.15
    cm = rng.random((P, 64)) > 0.15
    if dead_cols:
        for b in range(P):                              # a masked column that wins the top place of every other row
            cm[b, 9] = False
            x[b, 0:64:2, 9] = -0.001
    return x, rp, cp, rm, cm


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("mutual", [True, False])
def test_fine_matching_against_float64(k, mutual):
    """Flags, the emitted list (rows, order, points) exactly; scores exp(x) * g within 1e-6 relative; for conf 0 / 0.05 / 0.5, with
    and without global scores."""
    rng = np.random.default_rng(100 + k * 2 + int(mutual))
    P = 5
    x, rp, cp, rm, cm = fine_inputs(rng, P)
    g = rng.uniform(0.2, 1.0, P).astype(np.float32)
    emitted = 0
    for conf in (0.0, 0.05, 0.5):
        for gs in (None, g):
            got = fine_raw(x, rp, cp, rm, cm, k, mutual, conf, gs=gs)
            f, er, ec, es, ep = fine_expect(x, rp, cp, rm, cm, k, mutual, conf, gs, list(range(P)))
            assert np.array_equal(got["flags"], f), (conf, np.argwhere(got["flags"] != f)[:5])
            assert np.array_equal(got["counts"], f.reshape(P, -1).sum(1))
            n = got["n_out"]
            assert n == len(es), (n, len(es))
            assert np.array_equal(got["row"][:n], er) and np.array_equal(got["col"][:n], ec)
            assert np.array_equal(got["patch"][:n], ep)
            assert np.abs(got["score"][:n] / es - 1.0).max(initial=0.0) <= 1e-6
            assert np.isnan(got["score"][n:]).all() and (got["patch"][n:] == -7).all()
            emitted += n
    assert emitted > 0


def test_fine_matching_ties_take_the_lower_index():
    """Fully tied rows / columns (one value everywhere): the k lowest indices win, for both top-k paths."""
    P = 1
    x = np.full((P, OTN, OTN), -1.0, np.float32)
    x[0, 64, :] = x[0, :, 64] = -20.0
    rp = np.arange(P * 64 * 3, dtype=np.float32).reshape(P, 64, 3)
    cp = -rp
    m = np.ones((P, 64), bool)
    for k in (1, 4, 5, 8):
        for mutual in (True, False):
            got = fine_raw(x, rp, cp, m, m, k, mutual, 0.05)
            f = fine_ref_flags(x, m, m, k, mutual, 0.05)
            assert np.array_equal(got["flags"], f), (k, mutual)
            want = np.zeros((64, 64), bool)
            want[:, :k] = True
            want_c = want.T
            assert np.array_equal(f[0], (want & want_c) if mutual else (want | want_c))


def test_fine_matching_tie_behind_a_displaced_entry():
    """Equal entries at indices 3 and 5, a larger one at 7 arriving later: the top 2 are 7 and 3.  Row 20 and column 20 both carry
    the pattern (the register top-k of k <= 4 once kept 5: the entry 7 pushed 3 down, and 3 did not pass the equal 5)."""
    x = np.full((1, OTN, OTN), -3.0, np.float32)
    for idx, v in ((3, -1.0), (5, -1.0), (7, -0.5)):
        x[0, 20, idx] = v
        x[0, idx, 20] = v
    rp = np.zeros((1, 64, 3), np.float32)
    m = np.ones((1, 64), bool)
    for k in (2, 3, 5):
        f = fine_ref_flags(x, m, m, k, True, 0.01)
        assert f[0, 20, 3] and f[0, 3, 20] and (k > 2) == bool(f[0, 20, 5]) == bool(f[0, 5, 20])
        for mutual in (True, False):
            got = fine_raw(x, rp, rp, m, m, k, mutual, 0.01)
            assert np.array_equal(got["flags"], fine_ref_flags(x, m, m, k, mutual, 0.01)), (k, mutual)


def _fine_layout_inputs(seed, P, pairs, num_corr):
    rng = np.random.default_rng(seed)
    x, rp, cp, rm, cm = fine_inputs(rng, P)
    g = rng.uniform(0.2, 1.0, (pairs, num_corr)).astype(np.float32)
    return x, rp, cp, rm, cm, g


def _alone(x, rp, cp, rm, cm, s, k, mutual, conf, g):
    return fine_raw(x[s:s + 1], rp[s:s + 1], cp[s:s + 1], rm[s:s + 1], cm[s:s + 1], k, mutual, conf, gs=np.array([g], np.float32))


@pytest.mark.parametrize("k,mutual", [(3, True), (5, False)])
def test_fine_matching_strided_layout(k, mutual):
    """B = 3 pairs, num_corr = 4, n_corr = (4, 1, 0): dead slots emit nothing; every live patch's rows equal the patch run alone;
    offsets and pair_starts equal the host prefix sums; then out_cap cuts the list: n_out = min(total, out_cap), the rows are the
    first out_cap of the uncut list, nothing past them is written, offsets and pair_starts clamped the same way."""
    pairs, num_corr, n_corr, conf = 3, 4, [4, 1, 0], 0.05
    P = pairs * num_corr
    x, rp, cp, rm, cm, g = _fine_layout_inputs(40 + k, P, pairs, num_corr)
    live = [b * num_corr + p for b in range(pairs) for p in range(n_corr[b])]
    x[[s for s in range(P) if s not in live]] = np.nan
    full = fine_raw(x, rp, cp, rm, cm, k, mutual, conf, gs=g, pairs=pairs, num_corr=num_corr, n_corr=n_corr, pair_starts=True)
    cnt = np.zeros(P, np.int64)
    rows = []
    for s in live:
        b, p = divmod(s, num_corr)
        al = _alone(x, rp, cp, rm, cm, s, k, mutual, conf, g[b, p])
        cnt[s] = al["n_out"]
        o = int(full["offsets"][s])
        for key in ("row", "col", "score"):
            assert np.array_equal(full[key][o:o + al["n_out"]], al[key][:al["n_out"]]), (s, key)
        assert (full["patch"][o:o + al["n_out"]] == s).all()
        rows.append(al["row"][:al["n_out"]])
        _, er, _, es, _ = fine_expect(x, rp, cp, rm, cm, k, mutual, conf, [g[b, p]], [s])
        assert np.array_equal(al["row"][:al["n_out"]], er) and np.abs(al["score"][:al["n_out"]] / es - 1).max(initial=0) <= 1e-6
    assert np.array_equal(full["counts"], cnt)
    excl = np.concatenate([[0], np.cumsum(cnt)])
    total = int(excl[-1])
    assert full["n_out"] == total and total > 0
    assert np.array_equal(full["offsets"], excl[:-1])
    assert np.array_equal(full["pair_starts"], [excl[b * num_corr] for b in range(pairs)] + [total])
    assert np.isnan(full["score"][total:]).all()
    for cap in (1, int(excl[2]) + 3, total - 1, total, total + 5):
        cut = fine_raw(x, rp, cp, rm, cm, k, mutual, conf, gs=g, pairs=pairs, num_corr=num_corr, n_corr=n_corr, out_cap=cap,
                       pair_starts=True)
        n = min(total, cap)
        assert cut["n_out"] == n, (cap, cut["n_out"])
        for key in ("row", "col", "score", "patch"):
            assert np.array_equal(cut[key][:n], full[key][:n]), (cap, key)
        assert np.isnan(cut["score"][n:]).all() and np.isnan(cut["row"][n:]).all() and (cut["patch"][n:] == -7).all(), cap
        assert np.array_equal(cut["offsets"], np.minimum(excl[:-1], cap)), cap
        assert np.array_equal(cut["pair_starts"], np.minimum(full["pair_starts"], cap)), cap


@pytest.mark.parametrize("n_corr,slots", [([3, 0, 2], 7), ([2, 3, 4], 6)])
def test_fine_matching_compacted_layout(n_corr, slots):
    """pair_off from roitr_patch_offsets, with spare slots and with a cut: out_patch holds slot numbers, global scores are read
    at (pair, p) of the strided coarse list, pair_starts at the pairs' first slots, dead slots emit nothing."""
    pairs, num_corr, k, mutual, conf = len(n_corr), 5, 4, True, 0.0
    po_h = host_pair_off(n_corr, slots)
    live = int(po_h[-1])
    x, rp, cp, rm, cm, g = _fine_layout_inputs(60 + slots, slots, pairs, num_corr)
    x[live:] = np.nan
    po = patch_offsets(n_corr, slots)
    got = fine_raw(x, rp, cp, rm, cm, k, mutual, conf, gs=g, pairs=pairs, num_corr=num_corr, n_corr=n_corr, pair_off=po,
                   slots=slots, pair_starts=True)
    cnt = np.zeros(slots, np.int64)
    for s in range(live):
        b = int(np.searchsorted(po_h[1:], s, side="right"))
        p = s - int(po_h[b])
        al = _alone(x, rp, cp, rm, cm, s, k, mutual, conf, g[b, p])
        cnt[s] = al["n_out"]
        o = int(got["offsets"][s])
        for key in ("row", "col", "score"):
            assert np.array_equal(got[key][o:o + al["n_out"]], al[key][:al["n_out"]]), (s, key)
        assert (got["patch"][o:o + al["n_out"]] == s).all()
    assert np.array_equal(got["counts"], cnt)
    excl = np.concatenate([[0], np.cumsum(cnt)])
    assert got["n_out"] == excl[-1] > 0
    assert np.array_equal(got["offsets"], excl[:-1])
    assert np.array_equal(got["pair_starts"], [excl[po_h[b]] if po_h[b] < slots else excl[-1] for b in range(pairs)] + [excl[-1]])
    assert np.isnan(got["score"][int(excl[-1]):]).all()


# ------------------------------------------------------------------------------------------------ patch gather
@pytest.mark.parametrize("compacted", [False, True])
def test_patch_gather_layouts(compacted):
    """Two pairs of different sizes: per slot and knn position the global row (-1 for the pad index n_c), the mask and the point,
    both sides, against a host restatement; dead strided slots give row -1, mask 0, point 0; dead compacted slots are untouched."""
    L = _lib()
    rng = np.random.default_rng(77 + int(compacted))
    pairs, num_corr, lim = 2, 4, 64
    npts = [300, 170, 260, 90]          # clouds [src0, src1, tgt0, tgt1]
    nnod = [5, 3, 4, 2]
    pt_end, nd_end = np.cumsum(npts), np.cumsum(nnod)
    pts = rng.standard_normal((int(pt_end[-1]), 3)).astype(np.float32)
    knn = np.zeros((int(nd_end[-1]), lim), np.int32)
    kmask = np.zeros_like(knn)
    for c in range(4):
        for nd in range(nd_end[c] - nnod[c], nd_end[c]):
            own = rng.integers(1, lim + 1)
            knn[nd, :own] = rng.choice(npts[c], own, replace=False)
            knn[nd, own:] = npts[c]
            kmask[nd, :own] = 1
    n_corr = [3, 2]
    tc = np.zeros((pairs, num_corr), np.int32)
    sc = np.zeros((pairs, num_corr), np.int32)
    for b in range(pairs):
        tc[b] = rng.integers(0, nnod[pairs + b], num_corr)
        sc[b] = rng.integers(0, nnod[b], num_corr)
    if compacted:
        slots = 7
        po = patch_offsets(n_corr, slots)
        po_h = host_pair_off(n_corr, slots)
        slot_of = [(int(np.searchsorted(po_h[1:], s, side="right")), s - int(po_h[np.searchsorted(po_h[1:], s, side="right")]))
                   if s < po_h[-1] else None for s in range(slots)]
    else:
        slots, po = pairs * num_corr, None
        slot_of = [(s // num_corr, s % num_corr) if s % num_corr < n_corr[s // num_corr] else None for s in range(slots)]
    tot = slots * lim
    outs = [torch.full((tot,), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    opts = [torch.full((tot, 3), float("nan"), device="cuda") for _ in range(2)]
    keep = [i32(n_corr), i32(tc), i32(sc), i32(nd_end), i32(pt_end), i32(knn), i32(kmask), dev(pts)]
    a = L.struct("RoitrPatch")(pairs, num_corr, lim, *[L.ptr(t) for t in keep], *[L.ptr(t) for t in outs], *[L.ptr(t) for t in opts], L.ptr(po),
               slots if compacted else 0)
    L.check(L.lib().roitr_patch_gather(ctypes.byref(a), L.stream_ptr()), "patch_gather")
    torch.cuda.synchronize()
    rows = [outs[0].cpu().numpy(), outs[1].cpu().numpy()]
    masks = [outs[2].cpu().numpy(), outs[3].cpu().numpy()]
    ptsg = [opts[0].cpu().numpy(), opts[1].cpu().numpy()]
    pad_seen = 0
    for s in range(slots):
        sl = slice(s * lim, (s + 1) * lim)
        if slot_of[s] is None:
            for side in range(2):
                if compacted:
                    assert (rows[side][sl] == -7).all() and (masks[side][sl] == -7).all() and np.isnan(ptsg[side][sl]).all()
                else:
                    assert (rows[side][sl] == -1).all() and (masks[side][sl] == 0).all() and (ptsg[side][sl] == 0).all()
            continue
        b, p = slot_of[s]
        for side, cloud, corr in ((0, pairs + b, tc), (1, b, sc)):
            node = nd_end[cloud] - nnod[cloud] + corr[b, p]
            p0 = pt_end[cloud] - npts[cloud]
            li = knn[node]
            pad = li == npts[cloud]
            pad_seen += int(pad.sum())
            want_rows = np.where(pad, -1, p0 + li)
            assert np.array_equal(rows[side][sl], want_rows), (s, side)
            assert np.array_equal(masks[side][sl], kmask[node]), (s, side)
            want_pts = np.where(pad[:, None], 0.0, pts[np.minimum(p0 + li, len(pts) - 1)])
            assert np.array_equal(ptsg[side][sl], want_pts.astype(np.float32)), (s, side)
    assert pad_seen > 0


# ------------------------------------------------------------------------------------------------ point-to-node partition
Q = 1.0 / 64   # coordinate quantum: squared distances of these clouds are exact in fp32


def quantized_cloud(rng, counts, extra_nodes=0, dup=0, lattice=False):
    """Nodes 8 apart on a line (every point within 1.5 of its own node, so ownership is known), `counts[j]` points around node j,
    `extra_nodes` nodes far from every point (they own nothing); `dup` exact duplicates of random points; `lattice`: points on
    the mid-plane between nodes 0 and 1 (equidistant: the first node wins)."""
    n = len(counts)
    nodes = np.zeros((n + extra_nodes, 3))
    nodes[:n, 0] = 8.0 * np.arange(n)
    nodes[n:, 1] = 64.0 + 8.0 * np.arange(extra_nodes)
    pts = [nodes[j] + np.round(rng.uniform(-1.5, 1.5, (c, 3)) / Q) * Q for j, c in enumerate(counts)]
    pts = np.concatenate(pts) if pts else np.zeros((0, 3))
    if lattice:
        g = np.stack(np.meshgrid(np.arange(-2, 3), np.arange(-2, 3), indexing="ij"), -1).reshape(-1, 2) * 0.25
        mid = np.concatenate([np.full((len(g), 1), 4.0), g], 1)
        pts = np.concatenate([pts, mid, mid[:5]])
    if dup:
        pts = np.concatenate([pts, pts[rng.integers(0, len(pts), dup)]])
    pts = pts[rng.permutation(len(pts))]
    perm = rng.permutation(len(nodes))
    return pts.astype(np.float32), nodes[perm].astype(np.float32)


def p2n_ref(pts, nodes, limit):
    """float64 restatement: first nearest node; per node its owned points by (distance, index), padded with n_c."""
    d = ((nodes[:, None, :].astype(np.float64) - pts[None, :, :].astype(np.float64)) ** 2).sum(-1)
    p2n = d.argmin(0)
    M, N = len(nodes), len(pts)
    masks = np.zeros(M, bool)
    masks[p2n] = True
    knn = np.full((M, limit), N, np.int64)
    km = np.zeros((M, limit), bool)
    for j in range(M):
        own = np.nonzero(p2n == j)[0]
        own = own[np.argsort(d[j, own], kind="stable")][:limit]
        knn[j, :len(own)] = own
        km[j, :len(own)] = True
    return p2n, masks, knn, km


def _check_partition(got, ref):
    for a, b, name in zip(got, ref, ("point_to_node", "node_masks", "knn_indices", "knn_masks")):
        assert np.array_equal(a, b), (name, np.argwhere(a != b)[:5])


@pytest.mark.parametrize("counts,extra,dup,lattice", [
    ([64, 65, 3, 40], 1, 0, False),
    ([2048, 2049, 64, 65], 1, 0, False),
    ([10, 30, 5], 2, 12, True),
])
def test_point_to_node_partition_against_float64_and_the_oracle(counts, extra, dup, lattice):
    from oracle import roitr_ref as R
    from roitr_amd import ops
    rng = np.random.default_rng(sum(counts) + extra)
    pts, nodes = quantized_cloud(rng, counts, extra, dup, lattice)
    got = [t.cpu().numpy() for t in ops.point_to_node_partition(dev(pts), dev(nodes), 64)]
    ref = p2n_ref(pts, nodes, 64)
    _check_partition(got, ref)
    _check_partition(got, R.point_to_node_partition(pts, nodes, 64))
    owned = np.bincount(ref[0], minlength=len(nodes))
    if not dup and not lattice:
        assert sorted(owned[owned > 0].tolist()) == sorted(counts)
    assert (~ref[1]).sum() == extra
    if lattice:
        assert np.isclose(((pts - nodes[ref[0]]) ** 2).sum(1), ((pts[:, None] - nodes[None]) ** 2).sum(-1).min(1)).all()


def test_point_to_node_partition_fallback_returns_the_nearest_in_order():
    """A node owning 2049 points takes the repeated arg-min path: the 64 nearest, ascending, ties by index, no repeats; with many
    exact duplicates among them."""
    from roitr_amd import ops
    rng = np.random.default_rng(3)
    pts, nodes = quantized_cloud(rng, [2049, 1], 0, 0)
    big = int(np.argmax(np.bincount(p2n_ref(pts, nodes, 64)[0])))
    near = np.argsort(((pts - nodes[big]) ** 2).sum(1), kind="stable")[:4]
    pts = np.concatenate([pts, np.repeat(pts[near], 20, 0)])   # 80 more points, 20 copies each of the four nearest
    got = [t.cpu().numpy() for t in ops.point_to_node_partition(dev(pts), dev(nodes), 64)]
    ref = p2n_ref(pts, nodes, 64)
    assert np.bincount(ref[0])[big] > 2048
    _check_partition(got, ref)
    assert len(set(got[2][big].tolist())) == 64


def test_point_to_node_partition_three_clouds_in_one_launch():
    """b = 3 clouds of different sizes (one with a node owning 2049 points and one with an empty node) through one
    roitr_point_to_node_partition: every cloud equal to its single-cloud call bitwise, and to float64."""
    from roitr_amd import ops
    L = _lib()
    rng = np.random.default_rng(9)
    clouds = [quantized_cloud(rng, [64, 65, 20], 1, 5), quantized_cloud(rng, [2049, 7], 0, 0), quantized_cloud(rng, [3, 2048], 2, 0, True)]
    pts = np.concatenate([c[0] for c in clouds])
    nodes = np.concatenate([c[1] for c in clouds])
    pe = np.cumsum([len(c[0]) for c in clouds])
    ne = np.cumsum([len(c[1]) for c in clouds])
    con = np.repeat(np.arange(3), [len(c[1]) for c in clouds])
    N, M, lim = len(pts), len(nodes), 64
    p2n = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    p2nd = torch.zeros(N, dtype=torch.float32, device="cuda")
    nm = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    kidx = torch.full((M, lim), -7, dtype=torch.int32, device="cuda")
    km = torch.full((M, lim), -7, dtype=torch.int32, device="cuda")
    keep = [dev(pts), i32(pe), dev(nodes), i32(ne), i32(con)]
    L.check(L.lib().roitr_point_to_node_partition(3, N, M, L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(keep[2]), L.ptr(keep[3]),
                                                  L.ptr(keep[4]), lim, L.ptr(p2n), L.ptr(p2nd), L.ptr(nm), L.ptr(kidx), L.ptr(km),
                                                  L.stream_ptr()), "point_to_node_partition")
    torch.cuda.synchronize()
    p2n, nm, kidx, km = (t.cpu().numpy() for t in (p2n, nm, kidx, km))
    for c, (cp, cn) in enumerate(clouds):
        ps, ns = (pe[c - 1] if c else 0), (ne[c - 1] if c else 0)
        part = (p2n[ps:pe[c]], nm[ns:ne[c]].astype(bool), kidx[ns:ne[c]], km[ns:ne[c]].astype(bool))
        single = [t.cpu().numpy() for t in ops.point_to_node_partition(dev(cp), dev(cn), lim)]
        _check_partition([part[0], part[1], part[2], part[3]], single)
        _check_partition(part, p2n_ref(cp, cn, lim))


# ------------------------------------------------------------------------------------------------ coarse / adaptive matching
def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def _coarse_inputs(rng, nr, ns, C=64):
    ref_f = _unit(rng.normal(size=(nr, C)))
    src_f = _unit(rng.normal(size=(ns, C)))
    m = min(nr, ns)
    src_f[:m] = _unit(ref_f[rng.permutation(nr)[:m]] + 0.3 * rng.normal(size=(m, C)))
    return ref_f, src_f


@pytest.mark.parametrize("dual", [True, False])
@pytest.mark.parametrize("shape", ["num_over_valid", "one_ref", "one_src"])
def test_coarse_matching_edges(dual, shape):
    """num above the number of valid pairs (every valid pair comes back, sorted by score), a side with one valid node, with and
    without dual normalisation, against the oracle: same set, scores within 2e-4, order by score."""
    from oracle import roitr_ref as R
    from roitr_amd import ops
    rng = np.random.default_rng(len(shape) + 2 * int(dual))
    nr, ns = 23, 31
    ref_f, src_f = _coarse_inputs(rng, nr, ns)
    ref_m, src_m = rng.random(nr) > 0.3, rng.random(ns) > 0.3
    if shape == "one_ref":
        ref_m[:] = False
        ref_m[7] = True
    if shape == "one_src":
        src_m[:] = False
        src_m[30] = True
    nvalid = int(ref_m.sum() * src_m.sum())
    num = nvalid + 50 if shape == "num_over_valid" else 256
    ri, si, sc = (t.cpu().numpy() for t in ops.coarse_matching(dev(ref_f), dev(src_f), dev(ref_m), dev(src_m), num, dual))
    eri, esi, esc = R.coarse_matching(ref_f, src_f, ref_m, src_m, num, dual)
    assert len(sc) == len(esc) == min(num, nvalid)
    assert set(zip(ri.tolist(), si.tolist())) == set(zip(eri.tolist(), esi.tolist()))
    np.testing.assert_allclose(sc, esc, rtol=2e-4, atol=1e-12)
    assert (np.diff(sc) <= 0).all()
    assert ref_m[ri].all() and src_m[si].all()


def _coarse_multi(ref_fs, src_fs, ref_ms, src_ms, num, dual, adaptive=None):
    """One roitr_coarse_matching / roitr_adaptive_matching launch over several pairs (cloud order [src.., tgt..]); -> per pair lists."""
    from roitr_amd import ops
    L = _lib()
    lib = L.lib()
    lib.roitr_coarse_scratch_floats.restype = ctypes.c_size_t
    B = len(ref_fs)
    feats = np.concatenate(list(src_fs) + list(ref_fs))
    masks = np.concatenate(list(src_ms) + list(ref_ms)).astype(np.int32)
    off = np.cumsum([len(f) for f in list(src_fs) + list(ref_fs)])
    max_r, max_s = max(len(f) for f in ref_fs), max(len(f) for f in src_fs)
    stride = int(lib.roitr_coarse_scratch_floats(max_r, max_s))
    scratch = torch.empty(stride * B, dtype=torch.float32, device="cuda")
    P = num
    tc = torch.full((B * P,), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((B * P,), -7, dtype=torch.int32, device="cuda")
    cs = torch.full((B * P,), float("nan"), device="cuda")
    nc = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    keep = [dev(feats), i32(off), i32(masks)]
    xy_t, xy_stride, xy_ld = None, 0, 0
    if adaptive is not None:
        xy = np.zeros((B, max_r, max_s), np.float32)
        for b in range(B):   # the same GEMM the ops front uses, one pair at a time
            xy[b, :len(ref_fs[b]), :len(src_fs[b])] = ops.linear(dev(ref_fs[b]), dev(src_fs[b])).cpu().numpy()
        xy_t, xy_stride, xy_ld = dev(xy), max_r * max_s, max_s
    a = ops._Coarse(B, feats.shape[1], P, int(dual), max_r, max_s, L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(keep[2]), L.ptr(scratch),
                    stride, L.ptr(tc), L.ptr(sc), L.ptr(cs), L.ptr(nc), L.ptr(xy_t), xy_stride, xy_ld)
    if adaptive is None:
        L.check(lib.roitr_coarse_matching(ctypes.byref(a), L.stream_ptr()), "coarse_matching")
    else:
        L.check(lib.roitr_adaptive_matching(ctypes.byref(a), int(adaptive[0]), ctypes.c_float(adaptive[1]), L.stream_ptr()), "adaptive")
    torch.cuda.synchronize()
    n = nc.cpu().numpy()
    tc, sc, cs = tc.cpu().numpy().reshape(B, P), sc.cpu().numpy().reshape(B, P), cs.cpu().numpy().reshape(B, P)
    return [(tc[b, :n[b]], sc[b, :n[b]], cs[b, :n[b]]) for b in range(B)], (tc, sc, cs, n)


@pytest.mark.parametrize("dual", [True, False])
def test_coarse_matching_several_pairs_in_one_launch(dual):
    """Three pairs of different sizes in one launch (one of them past the 16384-key LDS sort): each pair bitwise equal to the
    ops front's single-pair launch; slots past n_corr hold -1 / 0."""
    from roitr_amd import ops
    rng = np.random.default_rng(50 + int(dual))
    shapes = [(40, 57), (130, 129), (9, 4)]
    ins = [_coarse_inputs(rng, nr, ns) for nr, ns in shapes]
    ms = [(rng.random(nr) > 0.1, rng.random(ns) > 0.1) for nr, ns in shapes]
    num = 300
    per, (tc, sc, cs, n) = _coarse_multi([i[0] for i in ins], [i[1] for i in ins], [m[0] for m in ms], [m[1] for m in ms], num, dual)
    for b in range(3):
        one = [t.cpu().numpy() for t in ops.coarse_matching(dev(ins[b][0]), dev(ins[b][1]), dev(ms[b][0]), dev(ms[b][1]), num, dual)]
        assert np.array_equal(per[b][0], one[0]) and np.array_equal(per[b][1], one[1]), b
        assert np.array_equal(per[b][2].view(np.uint32), one[2].view(np.uint32)), b
        assert (tc[b, n[b]:] == -1).all() and (sc[b, n[b]:] == -1).all() and (cs[b, n[b]:] == 0).all()
    assert n[2] == int(ms[2][0].sum() * ms[2][1].sum()) < num


def _adaptive_inputs(rng, na, nb, planted, C=64):
    """Unit features with entries +-1/8: every dot product is a multiple of 1/32 and exact in fp32, so the distances
    sqrt(2 - 2 xy) are the oracle's bit for bit and ties are exact.  The first `planted` rows of b are rows of a with 0..8 signs
    flipped (distance sqrt(flips) / 4 <= 0.75); other pairs sit near sqrt(2)."""
    a = (rng.choice([-1.0, 1.0], (na, C)) / 8.0).astype(np.float32)
    b = (rng.choice([-1.0, 1.0], (nb, C)) / 8.0).astype(np.float32)
    src = rng.permutation(na)[:planted]
    for i, r in enumerate(src):
        b[i] = a[r]
        b[i, rng.permutation(C)[:rng.integers(0, 9)]] *= -1.0
    return a, b


def test_adaptive_matching_threshold_from_both_sides():
    """min_num valid pairs at or under the threshold: all of them in row-major order; one fewer: the min_num smallest, ascending;
    min_num above the number of valid pairs: every valid pair, ascending.  Against the oracle exactly."""
    from oracle import roitr_ref as R
    from roitr_amd import ops
    rng = np.random.default_rng(8)
    na, nb, mn = 20, 26, 40
    a, b = _adaptive_inputs(rng, na, nb, 12)
    am, bm = rng.random(na) > 0.15, rng.random(nb) > 0.15
    sim = np.sqrt(R.square_distance(a[am], b[bm], normalized=True)).astype(np.float32)
    d = np.unique(sim.reshape(-1))
    cum = np.array([(sim <= v).sum() for v in d])
    j = int(np.nonzero(cum >= mn)[0][0])            # the smallest distance level with >= mn pairs at or under it
    thr_hi = float(d[j])                            # >= mn under: the all-under branch
    thr_lo = float((d[j - 1] + d[j]) / 2)           # cum[j - 1] < mn under: the top-mn branch
    assert cum[j - 1] < mn <= cum[j]
    nvalid = int(am.sum() * bm.sum())
    for thr, k in ((thr_hi, mn), (thr_lo, mn), (thr_hi, nvalid + 7)):
        ia, ib, sc = (t.cpu().numpy() for t in ops.adaptive_superpoint_matching(dev(a), dev(b), dev(am), dev(bm), k, thr))
        ea, eb, es = R.adaptive_matching(a, b, am, bm, k, thr)
        assert np.array_equal(ia, ea) and np.array_equal(ib, eb), (thr, k)
        np.testing.assert_allclose(sc, es, rtol=1e-6)
        if thr == thr_hi and k == mn:
            assert len(ia) == cum[j] and (np.diff(ia * nb + ib) > 0).all()
        else:
            assert len(ia) == min(k, nvalid)


def test_adaptive_matching_several_pairs_in_one_launch():
    """Three pairs, one per branch, in one roitr_adaptive_matching launch: each equals the oracle exactly."""
    from oracle import roitr_ref as R
    rng = np.random.default_rng(12)
    shapes = [(20, 26), (33, 17), (5, 6)]
    ins = [_adaptive_inputs(rng, na, nb, p) for (na, nb), p in zip(shapes, (16, 15, 2))]
    ms = [(rng.random(na) > 0.1, rng.random(nb) > 0.1) for na, nb in shapes]
    mn, thr = 10, 0.9
    cap = max(na * nb for na, nb in shapes)
    # engine convention: the ref (row) side is the adaptive matching's FIRST argument
    per, _ = _coarse_multi([i[0] for i in ins], [i[1] for i in ins], [m[0] for m in ms], [m[1] for m in ms], cap, 0, adaptive=(mn, thr))
    branches = set()
    for bi in range(3):
        ea, eb, es = R.adaptive_matching(ins[bi][0], ins[bi][1], ms[bi][0], ms[bi][1], mn, thr)
        assert np.array_equal(per[bi][0], ea) and np.array_equal(per[bi][1], eb), bi
        np.testing.assert_allclose(per[bi][2], es, rtol=1e-6)
        sim = np.sqrt(R.square_distance(ins[bi][0][ms[bi][0]], ins[bi][1][ms[bi][1]], normalized=True)).astype(np.float32)
        branches.add(bool((sim <= np.float32(thr)).sum() >= min(mn, sim.size)))
    assert branches == {True, False}
