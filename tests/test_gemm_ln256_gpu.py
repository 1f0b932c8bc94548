"""The 32 x 256 LayerNorm GEMM (csrc/gemm_ln256.hip): nn.Linear -> (+ residual) -> LayerNorm (+ post) (ReLU) (+ interpolation) over
256-wide rows in one launch.  It must give the bytes of the two-launch form (roitr_gemm, then roitr_add_layernorm /
roitr_add_layernorm_interp) for every option, row count and K, also in place, independent of the row count of the launch; and an
engine that sends its 256-wide layers through it must return the bytes of one that does not."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 256
MS = (1, 31, 32, 33, 64, 65, 97)
KS = (32, 256, 512, 384)          # 384 = [x (256) | x_cat (128)]
IL_MIN_TILES = 1024               # gemm_ln256.hip: LN256_IL_MIN_TILES (tiles of 32 rows)
OPTIONS = ("plain", "res", "res_idx", "post_relu", "addend", "interp", "all")


def _inputs(M, K, option, seed=11):
    """Operands of one call; every tensor is made whatever the option, so that a row's data does not depend on it."""
    g = torch.Generator().manual_seed(seed + K)
    k_x = 256 if K == 384 else K
    t = {"x": torch.randn(M, k_x, generator=g), "x_cat": torch.randn(M + 5, K - k_x, generator=g) if K == 384 else None,
         "w": torch.randn(N, K, generator=g) / K ** 0.5, "b": torch.randn(N, generator=g), "gam": torch.randn(N, generator=g),
         "bet": torch.randn(N, generator=g), "res": torch.randn(M + 13, N, generator=g), "idx": torch.randint(0, M + 13, (M,), generator=g),
         "post": torch.randn(M, N, generator=g), "add": torch.randn(M, k_x, generator=g), "feat": torch.randn(M + 7, N, generator=g),
         "ip_idx": torch.randint(0, M + 7, (M, 3), generator=g), "ip_d2": torch.rand(M, 3, generator=g) + 0.01,
         "cat_idx": torch.randint(0, M + 5, (M,), generator=g)}
    t = {k: (v.cuda() if v is not None else None) for k, v in t.items()}
    use = {"plain": (), "res": ("res",), "res_idx": ("res", "idx"), "post_relu": ("post", "relu"), "addend": ("add",),
           "interp": ("interp", "relu"), "all": ("res", "idx", "post", "relu", "add", "cat_idx")}[option]
    return t, use


def _fused(t, use):
    from roitr_amd import ops
    return ops.linear_layernorm(t["x"], t["w"], t["b"], t["gam"], t["bet"], res=t["res"] if "res" in use else None,
                                res_idx=t["idx"] if "idx" in use else None, post=t["post"] if "post" in use else None, relu="relu" in use,
                                x_cat=t["x_cat"], x_cat_idx=t["cat_idx"] if ("cat_idx" in use and t["x_cat"] is not None) else None,
                                addend=t["add"] if "add" in use else None,
                                interp=(t["feat"], t["ip_idx"], t["ip_d2"]) if "interp" in use else None)


def _two_launches(t, use):
    from roitr_amd import ops
    M = t["x"].shape[0]
    xc = t["x_cat"]
    cat_idx = t["cat_idx"] if ("cat_idx" in use and xc is not None) else None
    if xc is not None and cat_idx is None:
        xc = xc[:M]
    y = ops.linear(t["x"], t["w"], t["b"], x_cat=xc, x_cat_idx=cat_idx, addend=t["add"] if "add" in use else None)
    res = t["res"] if "res" in use else None
    idx = t["idx"] if "idx" in use else None
    if res is not None and idx is None:
        res = res[:M]
    if "interp" in use:
        return ops.add_layernorm_interp(y, t["gam"], t["bet"], t["feat"], t["ip_idx"], t["ip_d2"], res=res, res_idx=idx, relu="relu" in use)
    return ops.add_layernorm(y, t["gam"], t["bet"], res=res, res_idx=idx, post=t["post"] if "post" in use else None, relu="relu" in use)


def _float64(t, use):
    M = t["x"].shape[0]
    x = t["x"].double()
    if "add" in use:
        x = (t["x"] + t["add"]).double()          # the addend is summed in fp32 while the operand is staged
    if t["x_cat"] is not None:
        xc = t["x_cat"][t["cat_idx"].long()] if "cat_idx" in use else t["x_cat"][:M]
        x = torch.cat([x, xc.double()], 1)
    y = x @ t["w"].double().T + t["b"].double()
    if "res" in use:
        y = y + (t["res"][t["idx"].long()] if "idx" in use else t["res"][:M]).double()
    y = torch.nn.functional.layer_norm(y, (N,), t["gam"].double(), t["bet"].double(), 1e-5)
    if "post" in use:
        y = y + t["post"].double()
    if "relu" in use:
        y = y.clamp_min(0)
    if "interp" in use:
        w = 1.0 / (t["ip_d2"].double().sqrt() + 1e-8)
        w = w / w.sum(1, keepdim=True)
        y = y + (t["feat"].double()[t["ip_idx"].long()] * w[:, :, None]).sum(1)
    return y


def _fused_call(t, use):
    """linear_layernorm of the fused path, with the x_cat rows cut to M when they are not gathered (the kernel reads row r)."""
    if t["x_cat"] is not None and "cat_idx" not in use:
        t = dict(t, x_cat=t["x_cat"][:t["x"].shape[0]])
    if "res" in use and "idx" not in use:
        t = dict(t, res=t["res"][:t["x"].shape[0]])
    return _fused(t, use)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("option", OPTIONS)
def test_fused_equals_two_launches_bitwise_and_float64(option, K):
    for M in MS:
        t, use = _inputs(M, K, option)
        got = _fused_call(t, use)
        two = _two_launches(t, use)
        assert torch.equal(got, two), (M, K, option, float((got - two).abs().max()))
        ref = _float64(t, use)
        # the tolerance of test_linear_layernorm_fused_epilogue
        assert torch.allclose(got.double(), ref, atol=2e-5, rtol=2e-5), (M, K, option, float((got.double() - ref).abs().max()))


def _gemm_into(out, x, w, b, gam, bet, res=None):
    """roitr_gemm with the LayerNorm epilogue, writing into `out` (which may be x or res)."""
    from roitr_amd import _lib as L
    from roitr_amd import ops
    M, K = x.shape
    g = ops._Gemm(M, N, K, L.ptr(x), L.ptr(None), K, L.ptr(None), 0, L.ptr(w), K, L.ptr(None), 0, L.ptr(b), 1.0, 0,
                  L.ptr(out), N, 1, 0, 0, 0, 0, 0, 0, L.ptr(None), 0, 0, L.ptr(gam), L.ptr(bet), L.ptr(res), L.ptr(None), L.ptr(None), 0, 1e-5)
    L.check(L.lib().roitr_gemm(ctypes.byref(g), L.stream_ptr()), "gemm+layernorm in place")
    torch.cuda.synchronize()


@pytest.mark.parametrize("M", (33, 97, 4099))
def test_in_place_output_is_the_operand_or_the_residual(M):
    """The engine's global transformer normalises into the buffer the GEMM reads (K = 256), the FFN into its residual: a block reads
    all its A and residual rows before it stores."""
    from roitr_amd import ops
    t, _ = _inputs(M, 256, "res")
    x, res = t["x"].contiguous(), t["res"][:M].contiguous()
    want = ops.linear_layernorm(x, t["w"], t["b"], t["gam"], t["bet"], res=res)
    a = x.clone()
    _gemm_into(a, a, t["w"], t["b"], t["gam"], t["bet"], res=res)
    assert torch.equal(a, want)
    r = res.clone()
    _gemm_into(r, x, t["w"], t["b"], t["gam"], t["bet"], res=r)
    assert torch.equal(r, want)
    both = x.clone()                                   # out = A = residual
    want_both = ops.linear_layernorm(x, t["w"], t["b"], t["gam"], t["bet"], res=x)
    _gemm_into(both, both, t["w"], t["b"], t["gam"], t["bet"], res=both)
    assert torch.equal(both, want_both)


def test_rows_do_not_depend_on_the_row_count():
    """97 rows alone (four tiles: staging loads in a burst) and as the last rows of a launch of 32 x the interleave threshold + 32 rows
    (staging loads between the MFMAs); with and without the addend, which has kernels of its own."""
    from roitr_amd import ops
    M_big, K = 32 * IL_MIN_TILES + 32, 32
    for option in ("all", "res"):
        t, use = _inputs(M_big, K, option, seed=3)
        big = _fused_call(t, use)
        lo = M_big - 97
        cut = {k: (v[lo:].contiguous() if (v is not None and v.shape[0] == M_big) else v) for k, v in t.items()}
        if "idx" not in use:
            cut["res"] = t["res"][lo:M_big].contiguous()
        small = _fused_call(cut, use)
        assert torch.equal(big[lo:], small), option
        two = _two_launches(t, use)
        assert torch.equal(big, two), option


def test_tile_switch_reaches_both_kernels():
    """roitr_gemm_set_ln256_tile(64) sends the same launch to the 64 x 256 instantiation of the general kernel: same bytes."""
    from roitr_amd import _lib as L
    t, use = _inputs(97, 256, "all")
    a = _fused_call(t, use)
    try:
        L.lib().roitr_gemm_set_ln256_tile(64)
        b = _fused_call(t, use)
    finally:
        L.lib().roitr_gemm_set_ln256_tile(32)
    assert torch.equal(a, b)


# ---------------------------------------------------------------- engine
TAPS = ("enc3.1", "enc4.2", "geo.layer5", "geo.out", "dec4.1", "dec3.1")
_MODEL = []


def _model():
    from tests.gpu_util import build_model
    if not _MODEL:
        _MODEL.append(build_model("3DMatch", weights="selective"))
    return _MODEL[0]


def _pairs(sizes):
    from roitr_amd.synthetic import make_pair
    from tests.gpu_util import pair_to_device
    out = []
    for i, s in enumerate(sizes):
        n_src, n_tgt = s if isinstance(s, tuple) else (s, s)
        out.append(pair_to_device(make_pair(n_src, n_tgt, config=2, pair_index=80 + i, normals="field")))
    torch.cuda.synchronize()
    return out


def _run(model, pairs, min_rows):
    n3 = sum(int(p[k].shape[0]) // 4 // 4 for p in pairs for k in ("src_pcd", "tgt_pcd"))
    n4 = sum(int(p[k].shape[0]) // 4 // 4 // 4 for p in pairs for k in ("src_pcd", "tgt_pcd"))
    rows = {"enc3.1": n3, "enc4.2": n4, "geo.layer5": n4, "geo.out": n4, "dec4.1": n4, "dec3.1": n3}
    bufs = {}
    for name in TAPS:
        bufs[name] = torch.full((rows[name], 256), float("nan"), device="cuda")
        model.set_tap(name, bufs[name])
    model.set_ln256_min_rows(min_rows)
    try:
        with torch.no_grad():
            res = model.forward_batch(pairs)
        torch.cuda.synchronize()
    finally:
        model.set_ln256_min_rows(-1)
        for name in TAPS:
            model.set_tap(name, None)
    for name, t in bufs.items():
        assert not torch.isnan(t).any(), name     # the tap was written
    return res, bufs


def _assert_same(a, b, what):
    (ra, ta), (rb, tb) = a, b
    assert len(ra) == len(rb), what
    for j, (x, y) in enumerate(zip(ra, rb)):
        assert set(x.keys()) == set(y.keys()), (what, j)
        for k in x.keys():
            if x[k] is None or y[k] is None:
                assert x[k] is None and y[k] is None, (what, j, k)
                continue
            assert x[k].shape == y[k].shape and torch.equal(x[k], y[k]), (what, j, k)
    for name in TAPS:
        assert torch.equal(ta[name], tb[name]), (what, name)


@pytest.mark.parametrize("sizes", ([1024, 1024], [(700, 1100), (1500, 900), (1300, 760)]), ids=("2x1024", "ragged"))
def test_engine_same_bytes_fused_and_two_launches(sizes):
    """Every 256-wide Linear + LayerNorm of the forward through the 32 x 256 kernel (threshold 1 row) against none of them (off): every
    output array and the tapped stages, and each form against itself from run to run."""
    model = _model()
    pairs = _pairs(sizes)
    off = _run(model, pairs, 0)
    assert sum(int(r["corr_scores"].shape[0]) for r in off[0]) > 0
    on = _run(model, pairs, 1)
    _assert_same(on, off, "fused vs two launches")
    _assert_same(_run(model, pairs, 1), on, "fused, run to run")
    _assert_same(_run(model, pairs, 0), off, "two launches, run to run")
