"""GPU: the bf16 operand mode (BASELINE.json configs[3]: 4DMatch, ~8000 pts/cloud, bf16).

Kernel level: csrc/gemm_bf16.hip against a float64 product of the SAME bf16-rounded operands -- with identical inputs the only
difference is the fp32 accumulation order, so the bound is fp32-rounding tight (2e-5 relative to the row's |a|.|w| mass) and a
wrong lane / k mapping cannot hide.  Engine level: the 4DMatch forward at N = 8000 in bf16 mode against the fp32 CPU oracle:
everything that does not pass through a dense layer (FPS nodes, point-to-node partition) is bit-identical, descriptors are
within the STATED bf16 tolerance, coarse correspondences overlap.

Stated tolerances (bf16 has 8 mantissa bits: 2^-9 = 2e-3 relative rounding per operand; the network is ~40 layers deep with
LayerNorm re-normalising every block).  Round 3: the pair and the weights are the 'selective' ones (roitr_amd/weights.py: x8 / x4
gains on the geometry inputs and the point head, centred heads), whose coarse matching actually selects (1 033 of 15 625 node
pairs for this pair) -- a harder case for bf16 than the plain weights: the centred descriptors are the small difference of two
bf16-rounded quantities.  Measured on this N = 8000 pair (scripts/bf16_report.py, profiles/r03_bf16_error.json): L2-normalised
node descriptors (entries ~0.035): max abs error 3.3e-3, cosine >= 0.99978; point descriptors (|x| ~ 0.30): max abs error 7.7e-2,
mean 1.2e-2; coarse matching: 1 023 of the oracle's 1 033 node pairs found, 68 extra ones just over the 0.75 threshold; the fp32
engine on the same pair: 8e-7 / 1.4e-5 and identical sets.  The tests allow ~3x the measured error: node descriptors max abs
1e-2 and cosine >= 0.9993 per node; point descriptors max abs 0.25, mean 3.5e-2; coarse matching: >= 90 % of the fp32 oracle's
node correspondences selected and at most 15 % more than it selects.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gemm_util import _gemm_abi  # noqa: E402
from gpu_util import build_model, pair_to_device  # noqa: E402

CORES = len(os.sched_getaffinity(0))


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float64).numpy()


def ref_linear(x, w, b=None, relu=False, alpha=1.0, x_is_bf16=False):
    y = alpha * (bf16_round(x) @ bf16_round(w).T)
    if b is not None:
        y = y + b.astype(np.float64)
    return np.maximum(y, 0) if relu else y


def mass(x, w):
    return np.abs(bf16_round(x)) @ np.abs(bf16_round(w)).T + 1e-6


@pytest.mark.parametrize("M,N,K", [(64, 64, 64), (1000, 404, 128), (257, 128, 256), (4096, 512, 512), (130, 1024, 512), (77, 65, 1024), (1, 512, 64)])
@pytest.mark.parametrize("relu", [False, True])
def test_gemm_bf16_matches_bf16_rounded_float64(M, N, K, relu):
    from roitr_amd import ops
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    xd, wd, bd = (torch.from_numpy(t).cuda() for t in (x, w, b))
    ref = ref_linear(x, w, b, relu, 0.75)
    tol = 4e-5 * 0.75 * mass(x, w) + 1e-6
    got = ops.linear(xd, wd, bd, relu=relu, alpha=0.75, bf16=True).cpu().numpy()
    assert (np.abs(got - ref) <= tol).all(), float((np.abs(got - ref) / tol).max())
    # stored-bf16 activation in, stored-bf16 result out (the GEMM -> GEMM intermediates of the engine)
    got_h = ops.linear(xd.to(torch.bfloat16), wd, bd, relu=relu, alpha=0.75, bf16=True, out_bf16=True)
    assert got_h.dtype == torch.bfloat16
    gh = got_h.float().cpu().numpy()
    assert (np.abs(gh - ref) <= tol + 2.0 ** -8 * np.abs(ref)).all()      # + one bf16 rounding of the result


@pytest.mark.parametrize("M,N,K,a_h", [(333, 192, 128, False), (70001, 512, 128, False), (517, 256, 64, True)])
def test_gemm_bf16_gather_zero_rows_and_addend(M, N, K, a_h):
    """The operand options of the bf16 kernel that the engine uses but ops.linear does not reach: row gather on A with negative and past-the-limit
    rows (zero rows), the fp32 addend on A (summed in fp32, then rounded), ragged last tiles, 64-, and (70001 rows) 256-column tiles.
    Same reference and bound as test_gemm_bf16_matches_bf16_rounded_float64."""
    rng = np.random.default_rng(M + N + K)
    R = M + 50
    a = rng.standard_normal((R, K)).astype(np.float32)
    a2 = None if a_h else rng.standard_normal((R, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    idx = rng.integers(-5, R + 20, M).astype(np.int32)   # < 0 or >= R: zero rows
    ad, wd = torch.from_numpy(a).cuda(), torch.from_numpy(w).cuda().to(torch.bfloat16)
    if a_h:
        ad = ad.to(torch.bfloat16)
    a2d = None if a2 is None else torch.from_numpy(a2).cuda()
    out = torch.full((M, N), float("nan"), device="cuda")
    _gemm_abi(M=M, N=N, K=K, A=ad, lda=K, a_idx=torch.from_numpy(idx).cuda(), a_limit=R, W=wd, ldw=K, bias=torch.from_numpy(b).cuda(), alpha=0.75,
              relu=1, C=out, ldc=N, batch=1, bf16=1 | (2 if a_h else 0), **({} if a2d is None else {"A2": a2d}))
    rows = (a if a2 is None else a + a2)[np.clip(idx, 0, R - 1)] * ((idx >= 0) & (idx < R))[:, None]
    ref = ref_linear(rows, w, b, True, 0.75)
    tol = 4e-5 * 0.75 * mass(rows, w) + 1e-6
    got = out.cpu().numpy()
    assert (np.abs(got - ref) <= tol).all(), float((np.abs(got - ref) / tol).max())


def test_gemm_bf16_gathered_batch_list_with_a_live_count():
    """The matching-score contraction of the bf16 engine (engine.cpp: a batch of 64 x 64 products of gathered rows of ONE stored-bf16
    matrix, both operands gathered with out-of-range rows, a device-side live batch count): the live batches against float64, the
    batches past the live count untouched."""
    rng = np.random.default_rng(11)
    T1, K, LIM, NB, live = 5000, 256, 64, 40, 29
    f = rng.standard_normal((T1, K)).astype(np.float32)
    ia = rng.integers(-3, T1 + 40, (NB, LIM)).astype(np.int32)
    iw = rng.integers(-3, T1 + 40, (NB, LIM)).astype(np.int32)
    fd = torch.from_numpy(f).cuda().to(torch.bfloat16)
    out = torch.full((NB, LIM, LIM), -7.0, device="cuda")
    _gemm_abi(M=LIM, N=LIM, K=K, A=fd, lda=K, a_idx=torch.from_numpy(ia).cuda(), a_limit=T1, W=fd, ldw=K, w_idx=torch.from_numpy(iw).cuda(), w_limit=T1,
              alpha=1.0 / 16.0, C=out, ldc=LIM, batch=NB, sC=LIM * LIM, sAidx=LIM, sWidx=LIM, batch_live=torch.tensor([live], dtype=torch.int32).cuda(),
              bf16=1 | 2)
    got = out.cpu().numpy()
    assert (got[live:] == -7.0).all()
    row = lambda ix: f[np.clip(ix, 0, T1 - 1)] * ((ix >= 0) & (ix < T1))[:, None]
    for b in range(live):
        x, w = row(ia[b]), row(iw[b])
        ref = ref_linear(x, w, None, False, 1.0 / 16.0)
        tol = 4e-5 / 16.0 * mass(x, w) + 1e-6
        assert (np.abs(got[b] - ref) <= tol).all(), (b, float((np.abs(got[b] - ref) / tol).max()))


def test_gemm_bf16_ragged_batch():
    """RoitrGemm::seg_off through the bf16 kernel: batch b multiplies row segment B + b of A by row segment b of W (the layout of the
    coarse node products, engine.cpp), every batch with its own row and column count; entries outside a batch's product untouched."""
    rng = np.random.default_rng(12)
    K, B = 128, 3
    lens = [70, 129, 33, 200, 64, 5]   # W segments 0..2, A segments 3..5
    off = np.cumsum(lens).astype(np.int32)
    f = rng.standard_normal((int(off[-1]), K)).astype(np.float32)
    nmax = max(lens)
    out = torch.full((B, nmax, nmax), -7.0, device="cuda")
    fd = torch.from_numpy(f).cuda()
    _gemm_abi(M=nmax, N=nmax, K=K, A=fd, lda=K, W=fd.to(torch.bfloat16), ldw=K, alpha=0.75, C=out, ldc=nmax, batch=B, sC=nmax * nmax,
              seg_off=torch.from_numpy(off).cuda(), seg_a0=B, seg_w0=0, bf16=1)
    got = out.cpu().numpy()
    start = np.concatenate([[0], off[:-1]])
    for b in range(B):
        x, w = f[start[B + b]:off[B + b]], f[start[b]:off[b]]
        ref = ref_linear(x, w, None, False, 0.75)
        tol = 4e-5 * 0.75 * mass(x, w) + 1e-6
        blk = got[b, :x.shape[0], :w.shape[0]]
        assert (np.abs(blk - ref) <= tol).all(), (b, float((np.abs(blk - ref) / tol).max()))
        assert (got[b, x.shape[0]:] == -7.0).all() and (got[b, :, w.shape[0]:] == -7.0).all()


@pytest.mark.parametrize("N", [64, 128, 256])
def test_gemm_bf16_layernorm_epilogue(N):
    from roitr_amd import ops
    rng = np.random.default_rng(N)
    M, K = 333, 2 * N
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b, gm, bt = (rng.standard_normal(N).astype(np.float32) for _ in range(3))
    res = rng.standard_normal((500, N)).astype(np.float32)
    ridx = rng.integers(0, 500, M).astype(np.int32)
    post = rng.standard_normal((M, N)).astype(np.float32)
    t = ref_linear(x, w, b) + res[ridx]
    mu = t.mean(1, keepdims=True)
    ref = np.maximum((t - mu) / np.sqrt(((t - mu) ** 2).mean(1, keepdims=True) + 1e-5) * gm + bt + post, 0)
    d = lambda a: torch.from_numpy(a).cuda()
    got = ops.linear_layernorm(d(x), d(w), d(b), d(gm), d(bt), res=d(res), res_idx=d(ridx), post=d(post), relu=True, bf16=True)
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=0, atol=2e-4)
    got_h = ops.linear_layernorm(d(x).to(torch.bfloat16), d(w), d(b), d(gm), d(bt), res=d(res), res_idx=d(ridx), post=d(post), relu=True,
                                 bf16=True, out_bf16=True)
    np.testing.assert_allclose(got_h.float().cpu().numpy(), ref, rtol=2.0 ** -8, atol=2e-4)


def test_gemm_bf16_rejects_unsupported_shapes():
    from roitr_amd import _lib as L
    from roitr_amd import ops
    x = torch.randn(10, 48, device="cuda")
    w = torch.randn(16, 48, device="cuda")
    with pytest.raises(L.RoitrError):
        ops.linear(x, w, bf16=True)          # K % 64 != 0: no silent fp32 fallback behind the operator


def test_geo_embed_bf16_against_float64():
    from roitr_amd import ops
    rng = np.random.default_rng(9)
    rows, C, k = 3000, 512, 3
    d_idx = (rng.random(rows) * 15).astype(np.float32)
    a_idx = (rng.random((rows, k)) * 12).astype(np.float32)
    div = np.exp(np.arange(0, C, 2, dtype=np.float32) * np.float32(-np.log(10000.0) / C)).astype(np.float32)
    wd, wa = ((rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32) for _ in range(2))
    bd, ba = (rng.standard_normal(C).astype(np.float32) for _ in range(2))

    def emb(v):
        om = v.astype(np.float64)[..., None] * div.astype(np.float64)
        return np.stack([np.sin(om), np.cos(om)], -1).reshape(*v.shape, C)

    ref = emb(d_idx) @ wd.T.astype(np.float64) + bd + (emb(a_idx) @ wa.T.astype(np.float64) + ba).max(1)
    d = lambda a: torch.from_numpy(a).cuda()
    got = ops.geo_embed(d(d_idx), d(a_idx), d(div), d(wd), d(bd), d(wa), d(ba), bf16=True).cpu().numpy()
    err = np.abs(got - ref)
    # bf16 operands: 2^-9 relative per factor, ~sqrt(C) accumulation of independent roundings on O(1) outputs
    assert err.max() < 2e-2 and err.mean() < 3e-3, (err.max(), err.mean())


@pytest.fixture(scope="module")
def fd8000():
    from conftest import oracle_forward
    pair, ref = oracle_forward("4DMatch", 8000, 4, 2)      # selective weights, field normals (shared with test_correspondences_gpu)
    model = build_model("4DMatch", operand_dtype="bf16", weights="selective")
    with torch.no_grad():
        out = model.forward(**pair_to_device(pair))
    return out, ref


def test_bf16_forward_indices_identical_to_fp32_oracle(fd8000):
    out, ref = fd8000
    for k in ("src_nodes", "tgt_nodes"):                     # FPS chain: fp32, untouched by the operand dtype
        assert np.array_equal(out[k].cpu().numpy(), ref[k]), k
    for side in ("src", "tgt"):                              # partition: fp32 geometry only
        assert np.array_equal(out[f"_{side}_node_knn_indices"].cpu().numpy(), ref[f"_{side}_node_knn_indices"])
        assert np.array_equal(out[f"_{side}_node_masks"].cpu().numpy(), ref[f"_{side}_node_masks"])


def test_bf16_forward_descriptors_within_stated_tolerance(fd8000):
    out, ref = fd8000
    for k in ("src_node_feats", "tgt_node_feats"):
        a, b = out[k].cpu().numpy(), ref[k]
        assert np.abs(a - b).max() < 1e-2, (k, float(np.abs(a - b).max()))
        cos = (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        assert cos.min() > 0.9993, (k, float(cos.min()))
    for k in ("src_point_feats", "tgt_point_feats"):
        e = np.abs(out[k].cpu().numpy() - ref[k])
        assert e.max() < 0.25 and e.mean() < 3.5e-2, (k, float(e.max()), float(e.mean()))


def test_bf16_forward_coarse_overlap(fd8000):
    out, ref = fd8000
    got = set(zip(out["tgt_node_corr_indices"].tolist(), out["src_node_corr_indices"].tolist()))
    want = set(zip(ref["tgt_node_corr_indices"].tolist(), ref["src_node_corr_indices"].tolist()))
    assert 128 < len(want) < 0.5 * 125 * 125                 # the threshold branch, and not every node pair: this check can fail
    assert len(got & want) >= 0.9 * len(want), (len(got & want), len(want), len(got))
    assert len(got) <= 1.15 * len(want), (len(got), len(want))
    sc = out["corr_scores"].cpu().numpy()
    assert (sc > 0.05).all()
