"""GPU: the global geometric transformer kernels of csrc/geo_attn.hip called directly (ops.multi_head_attention / ops.geo_indices),
against float64 restatements, at every dispatch threshold of roitr_mha from both sides.

roitr_mha dispatches on C, heads, E, partner, e_bf16 and nk_max to ten kernel forms (ROITR_MHA_*, include/roitr_engine.h: ten
instantiations of four kernels); the forwards reach some of them at about N / 64 superpoints per cloud only.  Each case below names
the form it is meant to reach, and every launch first asserts that roitr_mha_form -- the rule roitr_mha dispatches through -- gives
that form to the very struct it launches (tests/test_mha_form_cpu.py holds the same table without a GPU).  The data is built to make
index errors visible: scores spread over several units (the softmax is far from uniform), a different gain per head for q and a
different mean per head for v (a head mix-up shows), ragged clouds under one nk_max bound, launch windows that start at an odd
row and end short of a multiple of 4 (XCD remap, the four-row blocks of mha_plain_kernel straddling clouds), q | k | v as the
column blocks of one (T, 3C) buffer like the engine's, and in some cases a diagonal key that dominates through qt . E_ii, so that
the softmax a and the diagonal-masked a' differ by O(1) and a wrong diagonal index cannot pass.
"""
import numpy as np
import pytest
import torch

import mha_util

pytestmark = pytest.mark.gpu

GAIN = (0.7, 1.4, 2.1, 2.8)   # per-head gain of q (8 heads: each used twice, with a different v mean)


class Setup:
    """Clouds `sizes` (cross: src sizes then tgt sizes, partner of cloud c = (c + B) mod 2B) with random q / k / v, and for self
    attention with E: E (fp32 or bf16), qt = Wp_h^T q_h from a random Wp (as the engine's batched GEMM forms it), bp, Wvp, bvp."""

    def __init__(self, C, heads, sizes, cross=False, e=None, diag=False, packed=True, seed=0, nk_max=None):
        dev = "cuda"
        self.C, self.heads, self.sizes, self.cross, self.e = C, heads, list(sizes), cross, e
        n = len(sizes)
        self.T = T = int(sum(sizes))
        self.nk_max = max(sizes) if nk_max is None else nk_max
        ends = np.cumsum(sizes)
        self.starts = np.concatenate([[0], ends[:-1]]).astype(np.int64)
        self.cl = np.repeat(np.arange(n), sizes)
        self.partner = np.array([(c + n // 2) % n for c in range(n)]) if cross else np.arange(n)
        self.offset = torch.tensor(ends, dtype=torch.int32, device=dev)
        self.cloud_of_row = torch.tensor(self.cl, dtype=torch.int32, device=dev)
        self.partner_t = torch.tensor(self.partner, dtype=torch.int32, device=dev) if cross else None
        g = torch.Generator(device=dev).manual_seed(1000 + seed)
        c = C // heads
        head_of = (torch.arange(C, device=dev) // c).clamp(max=heads - 1)   # C % heads != 0 only in the refusal test
        gain = torch.tensor([GAIN[h % 4] for h in range(heads)], device=dev)[head_of]
        vmean = torch.tensor([0.5 * h - 0.25 * heads for h in range(heads)], device=dev)[head_of]
        qkv = torch.randn((T, 3 * C), generator=g, device=dev)
        qkv[:, :C] *= gain
        qkv[:, 2 * C:] += vmean
        if packed:
            self.q, self.k, self.v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        else:
            self.q, self.k, self.v = (qkv[:, i * C:(i + 1) * C].contiguous() for i in range(3))
        self.E = None
        if e is not None:
            blocks = np.array(sizes, dtype=np.int64) ** 2
            self.eoff_h = np.concatenate([[0], np.cumsum(blocks)[:-1]])
            self.eoff = torch.tensor(self.eoff_h, dtype=torch.int64, device=dev)
            self.Wp = torch.randn((C, C), generator=g, device=dev) * (0.5 / c ** 0.5)
            self.bp = torch.randn((C,), generator=g, device=dev) * 0.5
            self.Wvp = torch.randn((C, C), generator=g, device=dev) / C ** 0.5
            self.bvp = torch.randn((C,), generator=g, device=dev) * 0.1
            self.qt = torch.einsum("thk,hki->thi", self.q.reshape(T, heads, c), self.Wp.reshape(heads, c, C)).contiguous()
            E = torch.randn((int(blocks.sum()), C), generator=g, device=dev)
            if diag:   # E_ii along every head's qt: scale * qt_h . E_ii is +10 or more, the diagonal key dominates a
                u = (self.qt / self.qt.norm(dim=2, keepdim=True)).sum(1)
                qi = np.arange(T) - self.starts[self.cl]
                ii = torch.tensor(self.eoff_h[self.cl] + qi * np.array(sizes)[self.cl] + qi, device=dev)
                E[ii] = 15.0 * u
            self.E = E.to(torch.bfloat16) if e == "bf16" else E

    def launch(self, form, q_row0=0, q_rows=None, out=None, ebar=None):
        """The launch, after the assertion that roitr_mha gives its struct the form `form`."""
        if out is None:
            out = torch.full((self.T, self.C), float("nan"), device="cuda")
        if ebar is None and self.E is not None:
            ebar = torch.full((self.T, self.heads, self.C), float("nan"), device="cuda")
        kw = dict(E=self.E, eoff=self.eoff, qt=self.qt, bp=self.bp) if self.E is not None else {}
        return mha_util.launch(form, self.q, self.k, self.v, self.offset, self.cloud_of_row, self.nk_max, heads=self.heads,
                               partner=self.partner_t, q_row0=q_row0, q_rows=q_rows, out=out, ebar=ebar, **kw)

    def key_range(self, r):
        kc = self.partner[self.cl[r]]
        return int(self.starts[kc]), int(self.sizes[kc])

    def E_rows(self, r):
        """E[i, :, :] of query row r, as float64 (the values the kernel reads: bf16-rounded in the bf16 case)."""
        c = self.cl[r]
        n, qi = self.sizes[c], r - self.starts[c]
        s = int(self.eoff_h[c] + qi * n)
        return self.E[s:s + n].double().cpu().numpy()

    def reference(self, rows):
        """Float64 restatement of geoattention.py:87-136 in the folded form (26-66 without E) for query rows `rows`:
        s_hj = scale (q_h . k_jh + qt_h . E_ij + q_h . bp_h), a = softmax_j s, a' = softmax_{j != qi} s,
        out[h-slice] = sum_j a_hj v_j[h-slice], ebar_h = sum_j a'_hj E_ij.  Returns (out, ebar, a, a')."""
        C, H = self.C, self.heads
        c = C // H
        scale = 1.0 / np.sqrt(c)
        q = self.q.double().cpu().numpy()
        k = self.k.double().cpu().numpy()
        v = self.v.double().cpu().numpy()
        qt = self.qt.double().cpu().numpy() if self.E is not None else None
        bp = self.bp.double().cpu().numpy() if self.E is not None else None
        outs, ebars, As, A2s = [], [], [], []
        for r in rows:
            ks, nk = self.key_range(r)
            qh = q[r].reshape(H, c)
            s = np.einsum("hc,jhc->hj", qh, k[ks:ks + nk].reshape(nk, H, c))
            if self.E is not None:
                Ei = self.E_rows(r)
                s = s + qt[r] @ Ei.T + (qh * bp.reshape(H, c)).sum(1)[:, None]
            s *= scale
            a = np.exp(s - s.max(1, keepdims=True))
            a /= a.sum(1, keepdims=True)
            outs.append(np.einsum("hj,jhc->hc", a, v[ks:ks + nk].reshape(nk, H, c)).reshape(C))
            As.append(a)
            if self.E is not None:
                qi = r - self.starts[self.cl[r]]
                s2 = s.copy()
                s2[:, qi] = -np.inf
                a2 = np.exp(s2 - s2.max(1, keepdims=True))
                a2 /= a2.sum(1, keepdims=True)
                ebars.append(a2 @ Ei)
                A2s.append(a2)
        return np.array(outs), (np.array(ebars) if ebars else None), As, A2s

    def check_rows(self, q_row0, q_rows, rng, extra=16):
        """Rows to compare: window edges, first / last row of every cloud inside it, some random ones (all rows without E)."""
        lo, hi = q_row0, q_row0 + q_rows
        if self.E is None or q_rows <= 48:
            return list(range(lo, hi))
        rows = {lo, lo + 1, lo + 2, hi - 3, hi - 2, hi - 1}
        for s, n in zip(self.starts, self.sizes):
            rows.update(r for r in (s, s + 1, s + n - 2, s + n - 1) if lo <= r < hi)
        rows.update(rng.integers(lo, hi, extra).tolist())
        return sorted(rows)


def window(T):
    """An odd first row and a row count that is not a multiple of 4: rows 0-2 and the last one or two stay untouched."""
    q_row0 = 3 if T > 8 else 1
    q_rows = T - q_row0 - 1
    return q_row0, q_rows - 1 if q_rows % 4 == 0 else q_rows


# (id, form (ROITR_MHA_*) the case is meant to reach, C, heads, cloud sizes, cross, E storage, dominant diagonal)
CASES = [
    ("geo20-nk4", "GEO20", 256, 4, (4, 3, 4, 2), False, "f32", False),
    ("geo20-nk79", "GEO20", 256, 4, (79, 40, 17, 63), False, "f32", False),
    ("geo20-nk80", "GEO20", 256, 4, (80, 80, 33, 7), False, "f32", True),
    ("geo32-nk81", "GEO32", 256, 4, (81, 5, 60), False, "f32", False),
    ("geo32-nk127", "GEO32", 256, 4, (127, 90, 30), False, "f32", True),
    ("geo32-nk128", "GEO32", 256, 4, (128, 128, 77), False, "f32", False),
    ("stream-nk129", "GEO_STREAM", 256, 4, (129, 100, 3), False, "f32", False),
    ("stream-nk511", "GEO_STREAM", 256, 4, (511, 200), False, "f32", True),
    ("stream-nk512", "GEO_STREAM", 256, 4, (512, 64, 129), False, "f32", False),
    ("stream-nk513", "GEO_STREAM", 256, 4, (513, 47), False, "f32", False),
    ("stream-nk1024", "GEO_STREAM", 256, 4, (1024, 300, 5), False, "f32", True),
    ("wide1h-nk4", "GEO_WIDE_H", 256, 4, (4, 2, 3), False, "bf16", False),
    ("wide1h-nk80", "GEO_WIDE_H", 256, 4, (80, 31), False, "bf16", True),
    ("wide1h-nk129", "GEO_WIDE_H", 256, 4, (129, 7, 64), False, "bf16", False),
    ("wide1h-nk511", "GEO_WIDE_H", 256, 4, (511, 90), False, "bf16", False),
    ("wide1h-nk512", "GEO_WIDE_H", 256, 4, (512, 200), False, "bf16", True),
    ("wide2-nk79", "GEO_WIDE2", 512, 4, (79, 50, 2), False, "f32", False),
    ("wide2-nk128", "GEO_WIDE2", 512, 4, (128, 33), False, "f32", True),
    ("wide2-nk512", "GEO_WIDE2", 512, 4, (512, 100), False, "f32", False),
    ("wide2h-nk81", "GEO_WIDE2_H", 512, 4, (81, 12), False, "bf16", True),
    ("wide2h-nk511", "GEO_WIDE2_H", 512, 4, (511, 67), False, "bf16", False),
    ("plain128-nk4", "PLAIN128", 256, 4, (4, 2, 3, 4), True, None, False),
    ("plain128-nk80", "PLAIN128", 256, 4, (80, 13, 77, 9), True, None, False),
    ("plain128-nk128", "PLAIN128", 256, 4, (128, 50, 97, 128), True, None, False),
    ("plain1024-nk129", "PLAIN1024", 256, 4, (129, 40, 100, 66), True, None, False),
    ("plain1024-nk513", "PLAIN1024", 256, 4, (513, 2, 300, 129), True, None, False),
    ("plain1024-nk1024", "PLAIN1024", 256, 4, (1024, 77, 600, 5), True, None, False),
    ("plainwide-nk4", "PLAIN_WIDE2", 512, 4, (4, 3, 2, 4), True, None, False),
    ("plainwide-nk128", "PLAIN_WIDE2", 512, 4, (128, 21, 61, 127), True, None, False),
    ("plainwide-nk512", "PLAIN_WIDE2", 512, 4, (300, 512, 511, 17), True, None, False),
    ("generic-c512-self-nk513", "GENERIC", 512, 4, (513, 40), False, "f32", True),
    ("generic-c512-cross-nk513", "GENERIC", 512, 4, (513, 20, 100, 7), True, None, False),
    ("generic-h8-self", "GENERIC", 256, 8, (100, 37, 9), False, "f32", True),
    ("generic-h8-cross", "GENERIC", 256, 8, (50, 20, 33, 60), True, None, False),
]


def measure(case_id, seed=0):
    """Launch the case on its window and return (max |out - ref|, max |ebar - ref| or None, setup, launch results)."""
    _, form, C, heads, sizes, cross, e, diag = next(c for c in CASES if c[0] == case_id)
    S = Setup(C, heads, sizes, cross, e, diag, packed=(seed % 2 == 0), seed=seed)
    q_row0, q_rows = window(S.T)
    out, ebar = S.launch(form, q_row0, q_rows)
    rows = S.check_rows(q_row0, q_rows, np.random.default_rng(seed))
    ro, re_, a, a2 = S.reference(rows)
    err_o = float(np.abs(out[rows].double().cpu().numpy() - ro).max())
    err_e = float(np.abs(ebar[rows].double().cpu().numpy() - re_).max()) if ebar is not None else None
    return err_o, err_e, S, (q_row0, q_rows, out, ebar, rows, a, a2)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_mha_against_float64(case):
    """Every roitr_mha instantiation against the float64 restatement on a partial launch window.  Rows outside the window stay
    NaN, launched rows are finite.  Bound 2e-5 absolute on out and ebar (O(1) inputs, fp32 dot products of up to 512 terms and
    sums over up to 1024 keys; bf16-stored E is read back rounded, so the bound is the same).  Measured on an MI355X: at most
    6.4e-6 on out and 7.2e-6 on ebar (mha_kernel at C = 512), 5.5e-6 / 1.9e-6 on the register and wide kernels."""
    case_id, kernel, C, heads, sizes, cross, e, diag = case
    err_o, err_e, S, (q_row0, q_rows, out, ebar, rows, a, a2) = measure(case_id, seed=CASES.index(case))
    lo, hi = q_row0, q_row0 + q_rows
    o = out.cpu()
    assert torch.isnan(o[:lo]).all() and torch.isnan(o[hi:]).all(), (kernel, "a row outside the launch window was written")
    assert torch.isfinite(o[lo:hi]).all(), (kernel, "a launched row was left unwritten")
    if ebar is not None:
        eb = ebar.cpu()
        assert torch.isnan(eb[:lo]).all() and torch.isnan(eb[hi:]).all(), (kernel, "ebar outside the launch window")
        assert torch.isfinite(eb[lo:hi]).all(), (kernel, "ebar of a launched row left unwritten")
    # the data does what it is meant to: a peaked softmax, and with a dominant diagonal a and a' far apart
    assert max(float(x.max()) for x in a) > 0.25
    if diag:
        d = max(float(np.abs(x - y).max()) for x, y in zip(a, a2))
        assert d > 0.5, d
    assert err_o < 2e-5, (kernel, err_o)
    if ebar is not None:
        assert err_e < 2e-5, (kernel, err_e)


FOLD_FORM = {(256, "f32"): "GEO_STREAM", (256, "bf16"): "GEO_WIDE_H", (512, "f32"): "GEO_WIDE2", (512, "bf16"): "GEO_WIDE2_H"}   # 150 keys


@pytest.mark.parametrize("C,e", [(256, "f32"), (256, "bf16"), (512, "f32"), (512, "bf16")])
def test_rpe_fold_matches_the_unfolded_reference(C, e):
    """geoattention.py:102-136 as written -- p = proj_p(E), vp = proj_vp(E), scores q . k + q . p, pos_states = sum_j a'_j vp_j --
    against the kernel's folded form finished the way the engine finishes it: pos = Wvp_h ebar_h + bvp_h (and out unchanged).
    Pins the fold identity itself (qt = Wp_h^T q_h, bp riding in the scores, ebar on the diagonal-masked softmax)."""
    S = Setup(C, 4, (90, 150, 37), e=e, diag=False, seed=7 + C)
    out, ebar = S.launch(FOLD_FORM[C, e])
    H, c = 4, C // 4
    q, k, v = (t.double().cpu().numpy() for t in (S.q, S.k, S.v))
    Wp, bp, Wvp, bvp = (t.double().cpu().numpy() for t in (S.Wp, S.bp, S.Wvp, S.bvp))
    rows = [0, 89, 90, 91, 170, 239, 240, 276]
    eb = ebar[rows].double().cpu().numpy()
    ob = out[rows].double().cpu().numpy()
    err_pos = err_out = 0.0
    for m, r in enumerate(rows):
        ks, n = S.key_range(r)
        qi = r - ks
        Ei = S.E_rows(r)
        p = (Ei @ Wp.T + bp).reshape(n, H, c)
        vp = (Ei @ Wvp.T + bvp).reshape(n, H, c)
        qh = q[r].reshape(H, c)
        s = (np.einsum("hc,jhc->hj", qh, k[ks:ks + n].reshape(n, H, c)) + np.einsum("hc,jhc->hj", qh, p)) / np.sqrt(c)
        a = np.exp(s - s.max(1, keepdims=True)); a /= a.sum(1, keepdims=True)
        s2 = s.copy(); s2[:, qi] = -np.inf
        a2 = np.exp(s2 - s2.max(1, keepdims=True)); a2 /= a2.sum(1, keepdims=True)
        hid = np.einsum("hj,jhc->hc", a, v[ks:ks + n].reshape(n, H, c)).reshape(C)
        pos = np.einsum("hj,jhc->hc", a2, vp).reshape(C)
        pos_k = np.concatenate([Wvp[h * c:(h + 1) * c] @ eb[m, h] + bvp[h * c:(h + 1) * c] for h in range(H)])
        err_pos = max(err_pos, float(np.abs(pos_k - pos).max()))
        err_out = max(err_out, float(np.abs(ob[m] - hid).max()))
    assert err_out < 2e-5 and err_pos < 2e-5, (err_out, err_pos)


# one case per form (GENERIC: with and without E) for the bitwise invariants
BITWISE = ["geo20-nk79", "geo32-nk127", "stream-nk513", "wide1h-nk129", "wide2-nk79", "wide2h-nk81", "plain128-nk80",
           "plain1024-nk129", "plainwide-nk128", "generic-h8-self", "generic-c512-cross-nk513"]


def _slices(S):
    """Cuts of [0, T) at odd rows, inside clouds and across cloud boundaries."""
    T = S.T
    cuts = {0, T, 1, 6, 11}
    for s in S.starts[1:]:
        cuts.update(x for x in (int(s) - 3, int(s) + 2) if 0 < x < T)
    cuts = sorted(x for x in cuts if 0 <= x <= T)
    return list(zip(cuts[:-1], cuts[1:]))


@pytest.mark.parametrize("case_id", BITWISE)
def test_mha_bits_do_not_depend_on_the_launch(case_id):
    """A pair's bits never depend on the batch: (1) the rows of a full launch equal the same rows launched as several q_row0 /
    q_rows slices (odd starts, slices straddling cloud boundaries); (2) a cloud's rows are the same launched alone (cloud index 0,
    offsets 0) as among the others (same nk_max bound, so the same kernel); (3) two identical launches give identical bits."""
    _, kernel, C, heads, sizes, cross, e, diag = next(c for c in CASES if c[0] == case_id)
    S = Setup(C, heads, sizes, cross, e, diag, seed=50 + BITWISE.index(case_id))
    full, ebar_full = S.launch(kernel)
    again, ebar_again = S.launch(kernel)
    assert torch.equal(full, again) and (ebar_full is None or torch.equal(ebar_full, ebar_again)), (kernel, "not deterministic")
    out = torch.full_like(full, float("nan"))
    eb = torch.full_like(ebar_full, float("nan")) if ebar_full is not None else None
    for lo, hi in _slices(S):
        S.launch(kernel, lo, hi - lo, out=out, ebar=eb)
    assert torch.equal(out, full), (kernel, "sliced launches differ from the full launch")
    assert eb is None or torch.equal(eb, ebar_full), (kernel, "ebar of sliced launches differs")
    # (2) cloud 1 alone: its own rows (and, cross, its partner's) in a layout of its own
    c = 1
    clouds = [c, S.partner[c]] if cross else [c]
    rows = np.concatenate([np.arange(S.starts[x], S.starts[x] + S.sizes[x]) for x in clouds])
    ri = torch.tensor(rows, device="cuda")
    A = Setup.__new__(Setup)
    A.C, A.heads, A.cross, A.e, A.nk_max = C, heads, cross, e, S.nk_max
    A.sizes = [S.sizes[x] for x in clouds]
    A.T = len(rows)
    A.starts = np.concatenate([[0], np.cumsum(A.sizes)[:-1]]).astype(np.int64)
    A.cl = np.repeat(np.arange(len(clouds)), A.sizes)
    A.partner = np.array([1, 0]) if cross else np.array([0])
    A.offset = torch.tensor(np.cumsum(A.sizes), dtype=torch.int32, device="cuda")
    A.cloud_of_row = torch.tensor(A.cl, dtype=torch.int32, device="cuda")
    A.partner_t = torch.tensor(A.partner, dtype=torch.int32, device="cuda") if cross else None
    A.q, A.k, A.v = S.q[ri], S.k[ri], S.v[ri]
    A.E = None
    if S.E is not None:
        n = S.sizes[c]
        A.E = S.E[int(S.eoff_h[c]):int(S.eoff_h[c]) + n * n]
        A.eoff_h = np.array([0])
        A.eoff = torch.zeros(1, dtype=torch.int64, device="cuda")
        A.qt, A.bp = S.qt[ri].contiguous(), S.bp
    alone, ebar_alone = A.launch(kernel, 0, S.sizes[c])
    n = S.sizes[c]
    s = int(S.starts[c])
    assert torch.equal(alone[:n], full[s:s + n]), (kernel, "a cloud's rows depend on the other clouds of the launch")
    assert ebar_alone is None or torch.equal(ebar_alone[:n], ebar_full[s:s + n]), (kernel, "ebar depends on the other clouds")


def test_mha_unsupported_shapes_name_themselves():
    """roitr_mha refuses what no instantiation covers with ROITR_ERR_UNSUPPORTED and a message naming the limit, and launches
    nothing: the preset output stays NaN."""
    from roitr_amd import _lib as L
    sizes = (6, 5)

    def refused(match, C=256, heads=4, e=None, nk_max=None, cross=False):
        S = Setup(C, heads, sizes, cross=cross, e=e, nk_max=nk_max, seed=3)
        out = torch.full((S.T, C), float("nan"), device="cuda")
        ebar = torch.full((S.T, heads, C), float("nan"), device="cuda") if e else None
        from roitr_amd import ops
        kw = dict(E=S.E, eoff=S.eoff, qt=S.qt, bp=S.bp) if e else {}
        with pytest.raises(L.RoitrError, match=match):
            ops.multi_head_attention(S.q, S.k, S.v, S.offset, S.cloud_of_row, S.nk_max, heads=heads, partner=S.partner_t, out=out,
                                     ebar=ebar, scale=0.125, **kw)
        torch.cuda.synchronize()
        assert torch.isnan(out).all() and (ebar is None or torch.isnan(ebar).all())

    # bf16 E outside C = 256 / 512, 4 heads, <= 512 keys
    refused("bf16 E", C=256, heads=8, e="bf16")
    refused("bf16 E", C=384, heads=4, e="bf16")
    refused("bf16 E", C=512, heads=4, e="bf16", nk_max=513)
    refused("bf16 E", C=256, heads=4, e="bf16", nk_max=1024)
    # heads, C % heads, (C / heads) % 4
    refused("1 to 8 heads", C=288, heads=9)
    refused("multiple of heads", C=250, heads=4)
    refused("multiple of 4", C=24, heads=4)
    # the generic kernel's LDS bound: C + heads C + 2 heads nk_max floats with E, C + heads nk_max without
    refused("LDS bound", C=256, heads=4, e="f32", nk_max=4700)
    refused("LDS bound", C=256, heads=8, nk_max=4800, cross=True)


# ------------------------------------------------------------------------------------------------ geo_indices
def _lattice(rng, shape, step=0.25):
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3) * step + 0.5
    return g[rng.permutation(len(g))].astype(np.float32)


def _pairwise_f32(p):
    """positional_encoding.py:9-34 pairwise_distance(p, p), sqrt, in float32 with the operation order the kernel pins (csrc/geo_attn.hip
    pair_sqdist): squared norms ((x0^2 + x1^2) + x2^2), xy = fma(x2, y2, fma(x1, y1, x0 y0)), (x2 - 2 xy) + y2, clamped at 0.
    (An fma is restated as the float64 product -- exact for float32 operands -- plus the addend, rounded to float32.)"""
    f32 = np.float32
    x, y = p[:, None, :], p[None, :, :]
    sq = lambda v: ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]).astype(f32) + v[..., 2] * v[..., 2]).astype(f32)
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
    xy = fma(x[..., 2], y[..., 2], fma(x[..., 1], y[..., 1], (x[..., 0] * y[..., 0]).astype(f32)))
    return np.sqrt(np.maximum(((sq(x) - f32(2) * xy).astype(f32) + sq(y)).astype(f32), f32(0)))


def _check_geo_indices(clouds, sigma_d=0.2, sigma_a=15.0, k=3):
    """d_idx bitwise equal to the float32 matmul form of pairwise_distance in the kernel's operation order (its diagonal is the
    rounding noise of that form, sqrt of ~1e-7), and off the diagonal within the rounding of that form of float64; on the diagonal
    also bitwise equal to torch-CPU float32 for clouds of 64 nodes and more (torch's own CPU matmul takes another path for tiny
    matrices: at n = 4 its diagonal noise differs between machines).  The k nearest neighbours are the k + 1 smallest distances of a
    row, lowest index first on ties (the stable argsort), the first dropped; a_idx against float64 on those neighbours within 2e-5
    (float32 vectors and atan2f: a few ulps of an angle of up to pi, times 180 / (sigma_a pi)); and the oracle's restatement
    (oracle/roitr_ref.py geo_embedding_indices, numpy matmul) within its own rounding."""
    from oracle import roitr_ref as R
    from roitr_amd import ops
    pts = np.concatenate(clouds)
    d_idx, a_idx = ops.geo_indices(torch.from_numpy(pts).cuda(), [len(c) for c in clouds], sigma_d, sigma_a, k)
    d_idx, a_idx = d_idx.cpu().numpy(), a_idx.cpu().numpy()
    e0 = 0
    u = 2.0 ** -24
    for p in clouds:
        n = len(p)
        d = d_idx[e0:e0 + n * n].reshape(n, n)
        a = a_idx[e0:e0 + n * n].reshape(n, n, k)
        e0 += n * n
        dist = _pairwise_f32(p)
        assert np.array_equal(d, dist / np.float32(sigma_d)), (n, float((d != dist / np.float32(sigma_d)).mean()))
        P = p.astype(np.float64)
        x2 = (P ** 2).sum(1)
        xy = P @ P.T
        d64 = np.sqrt(np.maximum(x2[:, None] - 2 * xy + x2[None, :], 0))
        off = ~np.eye(n, dtype=bool)
        # |error of d^2| <= ~8 u (x2 + y2 + 2 |xy|) in the matmul form, |error of d| = that / 2d, plus the sqrt and the division
        bound = (8 * u * (x2[:, None] + x2[None, :] + 2 * np.abs(xy)) / (2 * np.maximum(d64, 1e-30)) + 4 * u * d64) / sigma_d
        assert np.all(np.abs(d - d64 / sigma_d)[off] <= bound[off]), float((np.abs(d - d64 / sigma_d) / bound)[off].max())
        if n >= 64:
            t = torch.from_numpy(p)
            dt = torch.sqrt((((t ** 2).sum(-1)[:, None] - 2 * (t @ t.T)) + (t ** 2).sum(-1)[None, :]).clamp(min=0.0)) / sigma_d
            assert np.array_equal(np.diag(d), np.diag(dt.numpy())), "diagonal differs from torch-CPU pairwise_distance"
        # the neighbours: k + 1 smallest of the row, lowest index first, the first dropped (topk(largest=False), l.124)
        knn = np.argsort(dist, axis=1, kind="stable")[:, 1:k + 1]
        ref = P[knn] - P[:, None, :]                      # (n, k, 3)
        anc = P[None, :, :] - P[:, None, :]               # (n, n, 3)
        cr = np.cross(ref[:, None, :, :], anc[:, :, None, :])
        cs = (ref[:, None, :, :] * anc[:, :, None, :]).sum(-1)
        a64 = np.arctan2(np.linalg.norm(cr, axis=-1), cs) * (180.0 / (sigma_a * np.pi))
        err_a = float(np.abs(a - a64).max())
        assert err_a < 2e-5, err_a
        od, oa = R.geo_embedding_indices(p, sigma_d, sigma_a, k)
        np.testing.assert_allclose(d[off], od[off], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(a, oa, rtol=0, atol=2e-4)


def test_geo_indices_ragged_clouds_against_float64_and_the_oracle():
    rng = np.random.default_rng(5)
    sizes = (257, 4, 1024, 64, 5, 468, 255, 256)
    _check_geo_indices([(rng.random((n, 3)) * 2).astype(np.float32) for n in sizes])


def test_geo_indices_tied_neighbours_on_lattices():
    """Lattice clouds (shuffled): every interior node has six neighbours at exactly the same distance; the kernel takes the lowest
    index first, like the stable argsort (and topk on the reference's float32 distances)."""
    rng = np.random.default_rng(6)
    _check_geo_indices([_lattice(rng, (4, 4, 4)), _lattice(rng, (8, 8, 4)), _lattice(rng, (5, 1, 1))])


def test_geo_indices_refuses_what_it_cannot_hold():
    from roitr_amd import _lib as L
    from roitr_amd import ops
    pts = torch.rand((1025, 3), device="cuda")
    with pytest.raises(L.RoitrError, match="at most 1024 nodes"):
        ops.geo_indices(pts, [1025])
    with pytest.raises(L.RoitrError, match="at most 6 angle neighbours"):
        ops.geo_indices(pts[:64], [64], angle_k=7)
