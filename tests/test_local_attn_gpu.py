"""GPU: roitr_local_attention (csrc/local_attn.hip), every dispatch branch, against the float64 restatement of the unfolded attention
(tests/local_attn_util.py attention_unfolded64, tied to the oracle by tests/test_local_attn_cpu.py), and roitr_build_pfold.

The branch a call takes follows from H, the storage type, wpe and the alignment alone; the parametrisation ids name it:

    quad-...      local_attn_quad_kernel<K>: H = 64, fp32 rows, wpe / bpe given, every ld a multiple of 4, 16-byte bases
    wave1x2-...   local_attn_kernel<K, 1, HALF, 2> (H = 64, two nodes per wave): a = extra q columns (wpe NULL, ldq = H + 20), b = bf16 rows
                  with wpe, c = bf16 rows with extra columns, d = fp32 rows with wpe and an odd ldk = ldv = 2H + 1 (falls through the quad test)
    wave2 / wave4 / wave8-...   local_attn_kernel<K, H / 64, HALF, 1> at H = 128 / 256 / 512, fp32 and bf16, wpe given or extra columns

Layouts: "packed" = q | k | v are the column blocks of one 3H-wide buffer (M == N_in), "split" = an H-wide (or H + 20-wide) q and a 2H-wide
k | v buffer of N_in = 300 rows.  Per case: the value bound, guard columns and rows around the output (ldo = H + 8, three rows past M), a
permuted visiting order (same bits), a row range computed in a call of its own (same bits), and two planted nodes (all K neighbours one
row; one neighbour whose key leads every head's softmax by about 50).

Value metric max |got - ref| / mean |ref|, fp32 rows: bound 2e-5 (the bound of local_attention_fold for the same formulas).  bf16 rows:
elementwise |got - ref| <= 2^-8 |ref| + 2e-5 mean |ref| (the output is rounded to bf16), the reference reads the rounded rows; where the
rounded rows carry the extra columns (c and the bf16 extra-column cases) the positional score term can only come from those stored columns,
so the reference is attention_folded64 of the stored values, which the CPU test holds to attention_unfolded64 at 1e-12.

Measured on an MI355X (maximum over the cases of a branch; bf16: the largest |got - ref| / (2^-8 |ref| + 2e-5 mean |ref|), bound 1):
    quad (K 8 / 16, both layouts)                 1.1e-6  (bound 2e-5)     wave1x2 a, fp32 extra columns      8.5e-7
    wave1x2 d, fp32 odd ldk = ldv                 1.0e-6                   wave2 fp32, wpe / extra columns    1.1e-6 / 1.1e-6
    wave4 fp32, wpe / extra columns               1.3e-6 / 1.2e-6          wave8 fp32, wpe / extra columns    1.6e-6 / 1.4e-6
    bf16 rows, ratio to the elementwise bound:    wave1x2 b 0.99, c 0.98; wave2 0.98 / 0.98; wave4 0.99 / 0.96; wave8 0.99 / 0.97 (wpe / extra)
    quad against wave at H = 64, same operands:   9.4e-7 (K = 8), 1.2e-6 (K = 16) of mean |ref| apart
(the bf16 figures sit just below 1 by construction: half a bf16 ulp IS 2^-8 of the bottom of its binade, the fp32 arithmetic adds 1e-6.)"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import local_attn_util as U  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12288.0            # exact in bf16 and fp32
FP32_BOUND = 2e-5
N_SPLIT = 300


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Case:
    """One set of stored operands on the device, and the float64 reference of exactly those stored values."""

    def __init__(self, H, K, M, layout="split", bf16=False, extra=False, odd=False, seed=0):
        self.H, self.K, self.M, self.bf16, self.extra = H, K, M, bf16, extra
        dt = self.dt = torch.bfloat16 if bf16 else torch.float32
        c = H // 4
        rng = np.random.default_rng(1000 * H + 10 * K + M + seed)
        N_in = M if layout == "packed" else N_SPLIT
        stored = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
        q, k, v = (stored(rng.standard_normal(s)) for s in ((M, H), (N_in, H), (N_in, H)))
        wpe, bpe, wvpe, bvpe = (f32(rng.standard_normal(s)) for s in ((H, 4), (H,), (H, 4), (H,)))
        ppf = f32(rng.random((M, K, 4)) * 3.0)
        grp = rng.integers(0, N_in, (M, K)).astype(np.int32)
        self.planted = M >= 5
        if self.planted:
            grp[1, :] = grp[1, 0]                                     # node 1: all K neighbours are one row
            # node 2: the key of one neighbour is 50 / (scale |q_h|^2) q_h per head -- its score leads by about 50
            qh = q[2].double().numpy().reshape(4, c)
            r = int(grp[2, 3])
            k[r] = stored((50.0 * np.sqrt(c) / (qh ** 2).sum(1, keepdims=True) * qh).reshape(H))
        q64, k64, v64 = q.double().numpy(), k.double().numpy(), v.double().numpy()
        w64 = [t.double().numpy() for t in (wpe, bpe, wvpe, bvpe)]
        ppf64 = ppf.double().numpy()
        self.grp_np, self.ppf64, self.q64, self.v64, self.w64 = grp, ppf64, q64, v64, w64
        cols = None
        if extra:
            cols = stored(U.qp_columns64(q64, w64[0], w64[1]))      # the extra columns as the q rows store them
        if extra and bf16:
            self.ref = U.attention_folded64(q64, cols.double().numpy(), k64, v64, grp, ppf64, w64[2], w64[3])
        else:
            self.ref = U.attention_unfolded64(q64, k64, v64, grp, ppf64, *w64)
        dev = "cuda"
        if layout == "packed":
            buf = torch.cat([q, k, v], 1).to(dev)
            self.q, self.k, self.v = buf[:, :H], buf[:, H:2 * H], buf[:, 2 * H:]
        else:
            self.q = (torch.cat([q, cols], 1) if extra else q).to(dev)
            kv = torch.zeros((N_in, 2 * H + (1 if odd else 0)), dtype=dt, device=dev)
            kv[:, :H], kv[:, H:2 * H] = k.to(dev), v.to(dev)
            self.k, self.v = kv[:, :H], kv[:, H:2 * H]
        self.grp, self.ppf = torch.from_numpy(grp).to(dev), ppf.to(dev)
        self.wpe, self.bpe, self.wvpe, self.bvpe = (None if extra else wpe.to(dev)), (None if extra else bpe.to(dev)), wvpe.to(dev), bvpe.to(dev)

    def run(self, lo=0, hi=None, node_order=None):
        """Rows [lo, hi) in one call into a sentinel-filled (hi - lo + 3, H + 8) output (ldo = H + 8)."""
        from roitr_amd import ops
        hi = self.M if hi is None else hi
        out = torch.full((hi - lo + 3, self.H + 8), SENTINEL, dtype=self.dt, device="cuda")
        ops.local_attention(self.q[lo:hi], self.k, self.v, self.grp[lo:hi], self.ppf[lo:hi], self.wvpe, self.bvpe, wpe=self.wpe, bpe=self.bpe,
                            bf16=self.bf16, node_order=node_order, out=out)
        return out

    def error(self, got):
        """(figure, bound) of got (M, H) against the reference: fp32 rows max |d| / mean |ref| with 2e-5; bf16 rows the largest elementwise
        |d| / (2^-8 |ref| + 2e-5 mean |ref|) with 1."""
        got = got.double().cpu().numpy()
        assert np.isfinite(got).all()
        scale = np.abs(self.ref).mean()
        d = np.abs(got - self.ref)
        if self.bf16:
            return float((d / (2.0 ** -8 * np.abs(self.ref) + 2e-5 * scale)).max()), 1.0
        return float(d.max() / scale), FP32_BOUND


def _cases():
    cases = {}
    for K in (8, 16):
        for M in (1, 17, 131):
            for layout in ("packed", "split"):
                cases[f"quad-H64-K{K}-M{M}-{layout}"] = dict(H=64, K=K, M=M, layout=layout)
        for M in (1, 9, 131):
            cases[f"wave1x2-a_f32_extra-H64-K{K}-M{M}"] = dict(H=64, K=K, M=M, extra=True)
            cases[f"wave1x2-b_bf16_wpe-H64-K{K}-M{M}"] = dict(H=64, K=K, M=M, bf16=True)
            cases[f"wave1x2-c_bf16_extra-H64-K{K}-M{M}"] = dict(H=64, K=K, M=M, bf16=True, extra=True)
            cases[f"wave1x2-d_f32_oddld-H64-K{K}-M{M}"] = dict(H=64, K=K, M=M, odd=True)
    for H, K in ((128, 16), (128, 8), (256, 16), (512, 16)):
        for M in (1, 5, 131):
            for bf16 in (False, True):
                ty = "bf16" if bf16 else "f32"
                cases[f"wave{H // 64}-H{H}-K{K}-M{M}-{ty}-wpe-split"] = dict(H=H, K=K, M=M, bf16=bf16)
                if H == 256:
                    cases[f"wave{H // 64}-H{H}-K{K}-M{M}-{ty}-wpe-packed"] = dict(H=H, K=K, M=M, bf16=bf16, layout="packed")
    for H in (128, 256, 512):
        cases[f"wave{H // 64}-H{H}-K16-M131-f32-extra-split"] = dict(H=H, K=16, M=131, extra=True)
        cases[f"wave{H // 64}-H{H}-K16-M5-bf16-extra-split"] = dict(H=H, K=16, M=5, bf16=True, extra=True)
    return cases


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_local_attention_against_float64(name):
    c = Case(**CASES[name])
    H, M = c.H, c.M
    out = c.run()
    torch.cuda.synchronize()
    # 1. value
    err, bound = c.error(out[:M, :H])
    print(f"local_attention {name}: {'bf16 ratio' if c.bf16 else 'max|d|/mean|ref|'} = {err:.3e} (bound {bound:g})")
    assert err < bound, (name, err)
    # 2. guard columns and rows keep the sentinel, bit for bit
    guard = torch.full_like(out, SENTINEL)
    assert torch.equal(_bits(out[:M, H:]), _bits(guard[:M, H:])), "a lane wrote past its channels"
    assert torch.equal(_bits(out[M:]), _bits(guard[M:])), "a dead slot stored"
    # 3. a permuted visiting order gives the same bits
    perm = np.random.default_rng(M).permutation(M).astype(np.int32)
    order = np.zeros((M, 4), np.float32)
    order[:, 3] = perm.view(np.float32)
    assert torch.equal(_bits(c.run(node_order=torch.from_numpy(order).cuda())), _bits(out)), "the visiting order changed a result"
    # 4. a row range computed in a call of its own gives the bits of the full call (selection by shape only, never by M)
    if M > 4:
        lo, hi = (36, 101) if M > 101 else (4, M)
        part = c.run(lo, hi)
        assert torch.equal(_bits(part[:hi - lo, :H]), _bits(out[lo:hi, :H])), "a node's result depends on the call it is in"
        assert torch.equal(_bits(part[hi - lo:]), _bits(guard[:3])) and torch.equal(_bits(part[:, H:]), _bits(guard[:hi - lo + 3, H:]))
    # planted nodes
    if c.planted:
        got = out[:M, :H].double().cpu().numpy()
        wpe, bpe, wvpe, bvpe = c.w64
        # node 1, all neighbours one row r: v[r] + Wvpe pbar + bvpe with the softmax over the PPF term alone
        r = int(c.grp_np[1, 0])
        cols = U.qp_columns64(c.q64[1:2], wpe, bpe).reshape(4, 5)
        a = U.softmax64((c.ppf64[1] @ cols[:, :4].T) / np.sqrt(H // 4), 0)                      # (K, heads)
        pbar = a.T @ c.ppf64[1]                                                              # (heads, 4)
        want = c.v64[r] + np.einsum("hct,ht->hc", wvpe.reshape(4, H // 4, 4), pbar).reshape(H) + bvpe
        scale = np.abs(c.ref).mean()
        if not (c.bf16 and c.extra):                                 # (the stored columns of that mode are not Wpe^T q exactly)
            assert np.abs(want - c.ref[1]).max() < 1e-11 * scale
        for node in (1, 2):
            d = np.abs(got[node] - c.ref[node])
            tol = 2.0 ** -8 * np.abs(c.ref[node]) + 2e-5 * scale if c.bf16 else FP32_BOUND * scale
            assert np.isfinite(got[node]).all() and (d <= tol).all(), (name, node, float(d.max() / scale))


@pytest.mark.parametrize("K", [8, 16])
def test_quad_and_wave_kernels_agree_at_h64(K):
    """The same stored values through the quad kernel and (odd ldk = ldv: the fall-through) through the wave kernel: both within the bound
    of float64; their summation orders differ, so equal bits are not required."""
    quad, wave = Case(64, K, 131, seed=7), Case(64, K, 131, odd=True, seed=7)
    assert np.array_equal(quad.ref, wave.ref)
    a, b = quad.run()[:131, :64], wave.run()[:131, :64]
    ea, eb = quad.error(a)[0], wave.error(b)[0]
    diff = float((a - b).abs().max() / np.abs(quad.ref).mean())
    print(f"local_attention quad vs wave H=64 K={K}: quad {ea:.3e} wave {eb:.3e} quad-wave {diff:.3e}")
    assert ea < FP32_BOUND and eb < FP32_BOUND and diff < 2 * FP32_BOUND


def _reject_args(H=64, K=8, bf16=False, pad=0):
    dt = torch.bfloat16 if bf16 else torch.float32
    M, N = 4, 12
    z = lambda *s: torch.zeros(s, device="cuda")
    kv = torch.zeros((N, 2 * H + pad), dtype=dt, device="cuda")
    return dict(q=torch.zeros((M, H), dtype=dt, device="cuda"), k=kv[:, :H], v=kv[:, H:2 * H], group_idx=torch.zeros((M, K), dtype=torch.int32, device="cuda"),
                ppf=z(M, K, 4), wvpe=z(H, 4), bvpe=z(H), wpe=z(H, 4), bpe=z(H))


@pytest.mark.parametrize("what,args,kw,text", [
    ("heads=2", dict(), dict(heads=2), "local_attention: heads must be 4"),
    ("K=12", dict(K=12), dict(), "local_attention: heads must be 4, K 8 or 16"),
    ("H=96", dict(H=96), dict(), "H 64, 128, 256 or 512"),
    ("H=1024", dict(H=1024), dict(), "H 64, 128, 256 or 512"),
    ("bf16=1", dict(bf16=True), dict(bf16=1), "local_attention: bf16 must be 0"),
    ("H=256 ldk=2H+2", dict(H=256, pad=2), dict(), "local_attention: fp32 rows of H > 64 need"),
])
def test_local_attention_host_side_rejections(what, args, kw, text):
    """The conditions roitr_local_attention tests on the host before any launch: each is refused with a message of its own."""
    from roitr_amd import _lib, ops
    a = _reject_args(**args)
    with pytest.raises(_lib.RoitrError) as e:
        ops.local_attention(a["q"], a["k"], a["v"], a["group_idx"], a["ppf"], a["wvpe"], a["bvpe"], wpe=a["wpe"], bpe=a["bpe"], **kw)
    assert "local_attention" in str(e.value) and text in str(e.value), str(e.value)


def test_local_attention_of_no_nodes_is_ok():
    from roitr_amd import ops
    a = _reject_args()
    out = ops.local_attention(a["q"][:0], a["k"], a["v"], a["group_idx"][:0], a["ppf"][:0], a["wvpe"], a["bvpe"], wpe=a["wpe"], bpe=a["bpe"])
    assert out.shape == (0, 64)


@pytest.mark.parametrize("H", [64, 256])
def test_build_pfold_is_the_scatter_of_wpe_and_bpe(H):
    """Pfold (20, H): row 5 h + j holds Wpe[:, j] (j < 4) / bpe (j = 4) on the channels of head h, zero elsewhere -- exactly; and
    q @ Pfold^T (the fp32 GEMM the engine uses) are the extra columns of qp_columns64 to fp32 rounding: at most c = H / 4 products per
    entry, |error| <= c 2^-23 sum |q_i w_i|."""
    from roitr_amd import ops
    rng = np.random.default_rng(H)
    c = H // 4
    wpe, bpe = rng.standard_normal((H, 4)).astype(np.float32), rng.standard_normal(H).astype(np.float32)
    want = np.zeros((20, H), np.float32)
    for h in range(4):
        want[5 * h:5 * h + 4, h * c:(h + 1) * c] = wpe[h * c:(h + 1) * c].T
        want[5 * h + 4, h * c:(h + 1) * c] = bpe[h * c:(h + 1) * c]
    pf = ops.build_pfold(torch.from_numpy(wpe).cuda(), torch.from_numpy(bpe).cuda())
    assert pf.shape == (20, H) and np.array_equal(pf.cpu().numpy(), want)
    q = rng.standard_normal((37, H)).astype(np.float32)
    cols = ops.linear(torch.from_numpy(q).cuda(), pf).double().cpu().numpy()
    ref = U.qp_columns64(q, wpe, bpe)
    slack = c * 2.0 ** -23 * (np.abs(q).astype(np.float64) @ np.abs(want).astype(np.float64).T)
    assert (np.abs(cols - ref) <= slack).all(), float((np.abs(cols - ref) / slack).max())
