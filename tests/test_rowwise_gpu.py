"""GPU: the row-wise layers of csrc/nn_ops.hip that the engine calls, each against float64 or exactly: roitr_add_layernorm (every
values-per-lane instantiation with a ragged and a full last lane group), roitr_l2_normalize, roitr_segment_mean, roitr_interp3_add,
roitr_gather_rows, roitr_compose_idx, roitr_transpose, roitr_add_vectors.  Row counts 1, 5 (one workgroup, dead waves) and 131 (more than
one workgroup, the last not full).  Every index handed to a kernel is in range (or one of the values the gather defines as a zero row)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 131)
SENTINEL = -12288.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ln64(t, g, b, eps=1e-5):
    mu = t.mean(1, keepdims=True)
    return (t - mu) / np.sqrt(((t - mu) ** 2).mean(1, keepdims=True) + eps) * g + b


# res: None / "rows" (res (M, C)) / "idx" (res (M + 13, C) gathered by res_idx, the engine's cloud_of_node form)
LN_VARIANTS = {"plain": (None, False, False), "res": ("rows", False, False), "res_idx": ("idx", False, False),
               "res-post-relu": ("rows", True, True), "res_idx-relu": ("idx", False, True), "post-relu": (None, True, True)}


@pytest.mark.parametrize("variant", list(LN_VARIANTS))
@pytest.mark.parametrize("C", [40, 64, 65, 128, 200, 256, 257, 512, 1000, 1024])
def test_add_layernorm_against_float64(C, variant):
    from roitr_amd import ops
    res_kind, with_post, relu = LN_VARIANTS[variant]
    for M in ROWS:
        rng = np.random.default_rng(C * 7 + M)
        f32 = np.float32
        x = rng.standard_normal((M, C)).astype(f32)
        g, b = (1 + 0.1 * rng.standard_normal(C)).astype(f32), (0.1 * rng.standard_normal(C)).astype(f32)
        res = res_idx = post = None
        t = x.astype(np.float64)
        if res_kind == "rows":
            res = rng.standard_normal((M, C)).astype(f32)
            t = t + res
        elif res_kind == "idx":
            res = rng.standard_normal((M + 13, C)).astype(f32)
            res_idx = rng.integers(0, M + 13, M).astype(np.int32)
            t = t + res[res_idx]
        ref = _ln64(t, g.astype(np.float64), b.astype(np.float64))
        if with_post:
            post = rng.standard_normal((M, C)).astype(f32)
            ref = ref + post
        if relu:
            ref = np.maximum(ref, 0.0)
        got = ops.add_layernorm(dev(x), dev(g), dev(b), res=None if res is None else dev(res), res_idx=None if res_idx is None else dev(res_idx),
                                post=None if post is None else dev(post), relu=relu)
        got = got.double().cpu().numpy()
        assert got.shape == (M, C)
        assert np.allclose(got, ref, atol=2e-5, rtol=2e-5), (M, float(np.abs(got - ref).max()))


@pytest.mark.parametrize("C", [40, 65, 257, 1000])
def test_add_layernorm_of_a_zero_row_is_beta(C):
    """A row of zeros with no residual: (0 - 0) * rstd * gamma + beta (+ post), ReLU applied -- exactly."""
    from roitr_amd import ops
    rng = np.random.default_rng(C)
    M = 5
    x = rng.standard_normal((M, C)).astype(np.float32)
    x[2] = 0.0
    g, b = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    post = rng.standard_normal((M, C)).astype(np.float32)
    assert np.array_equal(ops.add_layernorm(dev(x), dev(g), dev(b)).cpu().numpy()[2], b)
    assert np.array_equal(ops.add_layernorm(dev(x), dev(g), dev(b), relu=True).cpu().numpy()[2], np.maximum(b, 0))
    assert np.array_equal(ops.add_layernorm(dev(x), dev(g), dev(b), post=dev(post), relu=True).cpu().numpy()[2], np.maximum(b + post[2], 0))


def test_add_layernorm_refuses_rows_wider_than_1024():
    from roitr_amd import _lib, ops
    z = torch.zeros((3, 1025), device="cuda")
    with pytest.raises(_lib.RoitrError):
        ops.add_layernorm(z, z[0], z[0])


@pytest.mark.parametrize("C", [64, 200, 256, 257, 512, 1024])
def test_l2_normalize_against_float64(C):
    """Elementwise relative error <= 2e-6: all elements of a row share one factor 1 / ||x||, formed by at most 16 + 6 additions, a square
    root and a division (below 1.3e-6 in the worst case), times one multiplication."""
    from roitr_amd import ops
    for M in ROWS:
        rng = np.random.default_rng(C + M)
        x = rng.standard_normal((M, C)).astype(np.float32)
        ref = x.astype(np.float64) / np.maximum(np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True)), 1e-12)
        got = ops.l2_normalize(dev(x)).double().cpu().numpy()
        assert (np.abs(got - ref) <= 2e-6 * np.abs(ref)).all(), (M, float((np.abs(got - ref) / np.abs(ref)).max()))
    # a zero row: zeros, no NaN; a row below the 1e-12 clamp (its squares are still normal fp32 numbers): x * 1e12
    x = rng.standard_normal((5, C)).astype(np.float32)
    x[1] = 0.0
    x[3] = 1e-14
    got = ops.l2_normalize(dev(x)).double().cpu().numpy()
    assert np.isfinite(got).all() and not got[1].any()
    want = x[3].astype(np.float64) * 1e12
    assert (np.abs(got[3] - want) <= 2e-6 * np.abs(want)).all(), got[3][:4]


@pytest.mark.parametrize("C", [64, 256, 300, 512])
def test_segment_mean_against_float64(C):
    """Clouds of 1, 2, 255, 256, 257 and 1000 rows in one call, C beyond 256 for the channel loop.  Bound per entry 2^-23 sum_r |x[r, c]| / n.
    The kernel adds the rows of a cloud one after the other; as a plain fp32 running sum it measured 1.03 - 1.04 x this bound at the 255-row
    cloud (C = 64, 300, 512; 0.94 at C = 256) -- such a sum is only good to (n - 1) 2^-24 sum |x| -- so the sum is compensated now: 0.46 - 0.50 x
    the bound, which is the rounding of the final sum and of the division."""
    from roitr_amd import ops
    sizes = np.array([1, 2, 255, 256, 257, 1000])
    rng = np.random.default_rng(C)
    x = rng.standard_normal((int(sizes.sum()), C)).astype(np.float32)
    off = np.cumsum(sizes).astype(np.int32)
    got = ops.segment_mean(dev(x), dev(off)).double().cpu().numpy()
    assert got.shape == (len(sizes), C)
    worst = 0.0
    for b, (e, n) in enumerate(zip(off, sizes)):
        seg = x[e - n:e].astype(np.float64)
        bound = 2.0 ** -23 * np.abs(seg).sum(0) / n
        d = np.abs(got[b] - seg.mean(0))
        worst = max(worst, float((d / bound).max()))
        assert (d <= bound).all(), (int(n), float((d / bound).max()))
    print(f"segment_mean C={C}: largest |d| / bound = {worst:.3f}")


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("C", [64, 100, 256])
def test_interp3_add_against_float64(C, with_base):
    """TransitionUp's interpolation (+ base): atol = rtol = 3e-5 against float64, and the interpolation term of roitr_add_layernorm_interp
    (a zero row through a LayerNorm with beta = 0 is exactly zero, so that call returns its interpolation term alone) within 2e-6."""
    from roitr_amd import ops
    R = 40
    for M in ROWS:
        rng = np.random.default_rng(C + M)
        feat = rng.standard_normal((R, C)).astype(np.float32)
        idx = rng.integers(0, R, (M, 3)).astype(np.int32)
        d2 = (rng.random((M, 3)) * 0.3).astype(np.float32)
        if M >= 5:
            d2[3, 0] = 0.0                                        # a query on top of a coarse point: weight 1e8 before normalisation
        base = rng.standard_normal((M, C)).astype(np.float32) if with_base else None
        w = 1.0 / (np.sqrt(d2.astype(np.float64)) + 1e-8)
        w = w / w.sum(1, keepdims=True)
        ref = (feat.astype(np.float64)[idx] * w[..., None]).sum(1) + (base if with_base else 0.0)
        got = ops.interp3_add(dev(feat), dev(idx), dev(d2), None if base is None else dev(base))
        assert got.shape == (M, C)
        assert np.allclose(got.double().cpu().numpy(), ref, atol=3e-5, rtol=3e-5), (M, float(np.abs(got.double().cpu().numpy() - ref).max()))
        if not with_base:
            zero = torch.zeros((M, C), device="cuda")
            term = ops.add_layernorm_interp(zero, torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"), dev(feat), dev(idx), dev(d2))
            assert (got - term).abs().max().item() <= 2e-6 * max(1.0, term.abs().max().item())


@pytest.mark.parametrize("C", [3, 64, 100])
def test_gather_rows_is_exact(C):
    from roitr_amd import ops
    R = 50
    for M in ROWS:
        rng = np.random.default_rng(C + M)
        x = rng.standard_normal((R, C)).astype(np.float32)
        # limit = R: -1 and indices >= R give zero rows
        idx = rng.integers(-1, R + 8, M).astype(np.int32)
        if M >= 5:
            idx[:4] = (-1, R, R + 7, R - 1)
        want = np.where(((idx >= 0) & (idx < R))[:, None], x[np.clip(idx, 0, R - 1)], np.float32(0))
        assert np.array_equal(ops.gather_rows(dev(x), dev(idx), limit=R).cpu().numpy(), want), M
        # limit = 0: no upper test, so only rows of x and -1
        idx = rng.integers(-1, R, M).astype(np.int32)
        if M >= 5:
            idx[:3] = (-1, 0, R - 1)
        want = np.where((idx >= 0)[:, None], x[np.clip(idx, 0, R - 1)], np.float32(0))
        assert np.array_equal(ops.gather_rows(dev(x), dev(idx), limit=0).cpu().numpy(), want), M


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_compose_idx_and_add_vectors_are_exact(n):
    from roitr_amd import ops
    rng = np.random.default_rng(n)
    outer = rng.integers(0, 10 ** 6, 77).astype(np.int32)
    inner = rng.integers(0, 77, n).astype(np.int32)
    assert np.array_equal(ops.compose_idx(dev(outer), dev(inner)).cpu().numpy(), outer[inner])
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    assert np.array_equal(ops.add_vectors(dev(a), dev(b)).cpu().numpy(), a + b)


@pytest.mark.parametrize("rows,cols", [(64, 4), (4, 64), (33, 65), (128, 100)])
def test_transpose_with_leading_dimensions_is_exact(rows, cols):
    """ld_in = cols + 3, ld_out = rows + 5: the block is transposed exactly and the padding of `out` keeps its sentinel."""
    from roitr_amd import ops
    rng = np.random.default_rng(rows + cols)
    src = dev(rng.standard_normal((rows, cols + 3)).astype(np.float32))
    dst = torch.full((cols, rows + 5), SENTINEL, device="cuda")
    got = ops.transpose(src[:, :cols], out=dst[:, :rows])
    assert got.stride(0) == rows + 5 and src[:, :cols].stride(0) == cols + 3
    assert torch.equal(dst[:, :rows], src[:, :cols].t())
    assert torch.equal(dst[:, rows:].contiguous().view(torch.int32), torch.full((cols, 5), SENTINEL, device="cuda").view(torch.int32))
    assert torch.equal(ops.transpose(src[:, :cols]), src[:, :cols].t())
