"""GPU: the fp32 GEMM (csrc/gemm.hip) directly -- every kernel form roitr_gemm can give a struct, with every operand option of
RoitrGemm the engine relies on, against the float64 restatement of the struct's contract in tests/gemm_util.py.

Every launch first asserts that roitr_gemm_form (the rule roitr_gemm dispatches through) names the form the case was written for;
tests/test_gemm_form_cpu.py pins the same table without a GPU.  The output buffer is filled with a sentinel before each launch and
compared WHOLE: padding columns, rows past M, gaps between batches, batches past the live count and everything outside a ragged
batch's block must still hold it.  Operand kinds and bounds: gemm_util's docstring (exact integers: `==`; standard normal at
K <= 512: 2e-6 of the |a| . |w| mass).  Shapes are the smallest that reach each form."""
import functools

import numpy as np
import pytest
import torch

from gemm_util import (ERR_UNSUPPORTED, PAST, Offset, SENTINEL, assert_gemm, gather_indices, gemm_form, gemm_reference, gemm_status, operands,
                       run_gemm, _gemm_abi)

pytestmark = pytest.mark.gpu

ROWS = ((100, "SMALL"), (8327, "TILE"), (16647, "TILE_IL"))   # N = 250: 4 x 2 | 4 x 131 = 524 | 4 x 261 = 1044 tiles of 64 x 64
N, LDC = 250, 260   # three vector-stored column tiles, a partial scalar one, ten padding columns to keep
OPTIONS = ("plain", "a_idx", "A2", "a_idx+A2", "w_idx", "A_cat", "A_cat+a_cat_idx+A2", "no_bias", "relu_alpha", "ldc251")
KINDS = ("exact", "normal")
TAIL = 3   # rows of sentinel behind the last row of a launch


def option_fields(opt, K, exact, rng, mmax):
    """The operands of one option for launches of up to mmax rows (a launch of fewer rows reads a prefix of the gathers)."""
    R = mmax + 50
    f = dict(N=N, K=K, ldc=LDC, batch=1, alpha=1.0)
    ka = K
    if opt.startswith("A_cat"):   # k_cat = 32: [A (32) | A_cat (K - 32)], at K = 32 [A (32) | A_cat (32)]
        f["K"], ka = max(K, 64), 32
    K = f["K"]
    f.update(A=operands(rng, (R + PAST, ka), exact), lda=ka, W=operands(rng, (N + 50 + PAST, K), exact, K ** -0.5), ldw=K)
    if opt != "no_bias":
        f["bias"] = operands(rng, N, exact)
    if "A2" in opt:
        f["A2"] = operands(rng, (R + PAST, ka), exact)
    if "a_idx" in opt.split("+"):
        f.update(a_idx=gather_indices(rng, mmax, R), a_limit=R)
    if opt == "w_idx":
        f.update(w_idx=gather_indices(rng, N, N + 50), w_limit=N + 50)
    if opt.startswith("A_cat"):
        f.update(A_cat=operands(rng, (2 * R, K - ka), exact), lda_cat=K - ka, k_cat=ka)
    if "a_cat_idx" in opt:
        f["a_cat_idx"] = rng.integers(0, 2 * R, mmax).astype(np.int32)
    if opt == "relu_alpha":
        f.update(relu=1, alpha=0.5 if exact else 0.75)
    if opt == "ldc251":
        f["ldc"] = 251   # every store scalar
    return f


def first_rows(full, M, ldc):
    """gemm_reference of the M-row launch from the one of a longer launch of the same operands: its first M rows, then sentinel."""
    size = (M + TAIL) * ldc
    exp, mass, written = np.full(size, SENTINEL, dtype=np.float64), np.zeros(size), np.zeros(size, dtype=bool)
    exp[:M * ldc], mass[:M * ldc], written[:M * ldc] = full[0][:M * ldc], full[1][:M * ldc], full[2][:M * ldc]
    return exp, mass, written


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("opt", OPTIONS)
@pytest.mark.parametrize("K", [32, 64, 256])
def test_forms_and_options(K, opt, kind):
    """Fast path: SMALL, TILE and TILE_IL, each with every operand option.  One operand set per case; the float64 product of the
    longest launch serves the shorter ones (their rows are its first rows)."""
    exact = kind == "exact"
    f = option_fields(opt, K, exact, np.random.default_rng([K, OPTIONS.index(opt), exact]), ROWS[-1][0])
    ldc, device = f["ldc"], {}
    full = gemm_reference((ROWS[-1][0] + TAIL) * ldc, M=ROWS[-1][0], **f)
    for M, form in ROWS:
        got, _ = run_gemm((M + TAIL) * ldc, form, device, reference=False, M=M, **f)
        assert_gemm(got, first_rows(full, M, ldc), exact, (M, form))


@pytest.mark.parametrize("opt", ["plain", "A2", "a_idx", "w_idx", "A_cat+a_cat_idx+A2"])
def test_same_bytes_whatever_the_form(opt):
    """A row's result does not depend on which of SMALL, TILE and TILE_IL its launch was given (gemm_small_kernel's comment; what keeps
    a one-pair forward identical to the same pair inside a batch).  GENERIC differs by design (its k order inside a slab)."""
    rows = ((156, "SMALL"), (8327, "TILE"), (16647, "TILE_IL"))
    f = option_fields(opt, 256, False, np.random.default_rng([7, OPTIONS.index(opt)]), rows[-1][0])
    device, got = {}, []
    for M, form in rows:
        got.append(run_gemm((M + TAIL) * LDC, form, device, reference=False, M=M, **f)[0][:156 * LDC])
    assert (got[0] != SENTINEL).sum() == 156 * N
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


@pytest.mark.parametrize("a2", [False, True])
def test_last_k_of_the_fast_path(a2):
    """K = 2048: the resident zero row that stands in for gathered rows that do not exist is read to its last element."""
    rng = np.random.default_rng(2048)
    M = Nn = 70
    R = 90
    f = dict(M=M, N=Nn, K=2048, A=operands(rng, (R + PAST, 2048), True), lda=2048, a_idx=gather_indices(rng, M, R), a_limit=R,
             W=operands(rng, (R + PAST, 2048), True), ldw=2048, w_idx=gather_indices(rng, Nn, R), w_limit=R, bias=operands(rng, Nn, True), alpha=0.5,
             ldc=72, batch=1)
    if a2:
        f["A2"] = operands(rng, (R + PAST, 2048), True)
    got, ref = run_gemm((M + TAIL) * 72, "SMALL", **f)
    assert_gemm(got, ref, True)


GENERIC = [(1, 0, 0), (31, 0, 0), (33, 0, 0), (100, 0, 0), (64, 3, 0), (64, 0, 1), (2080, 0, 0)]   # K, lda - K, floats the A pointer is offset by


@pytest.mark.parametrize("K,pad,skip,kind", [(*g, kind) for g in GENERIC for kind in KINDS if g[0] <= 512 or kind == "exact"])
def test_generic_kernel(K, pad, skip, kind):
    """Everything off the fast path: K no multiple of 32 (scalar tails, K = 1), rows that are not 16-byte aligned by their pitch or
    by their base, K > 2048 (aligned: vector loads with a scalar tail; exact operands only, the fp32 bound is established for
    K <= 512).  Each with zero rows on both operands, the addend and ReLU."""
    exact = kind == "exact"
    rng = np.random.default_rng([K, pad, skip, exact])
    M, Nn, R, lda = 130, 70, 150, K + pad
    a = operands(rng, (R + PAST) * lda + skip, exact)
    f = dict(M=M, N=Nn, K=K, A=Offset(a, skip) if skip else a, lda=lda, A2=operands(rng, (R + PAST) * lda, exact), a_idx=gather_indices(rng, M, R), a_limit=R,
             W=operands(rng, (R + PAST, K), exact, K ** -0.5), ldw=K, w_idx=gather_indices(rng, Nn, R), w_limit=R, bias=operands(rng, Nn, exact),
             alpha=0.5 if exact else 0.75, relu=1, ldc=72, batch=1)
    got, ref = run_gemm((M + TAIL) * 72, "GENERIC", **f)
    assert_gemm(got, ref, exact)


BATCH_SHAPES = ((70, 70, "SMALL"), (5500, 128, "TILE"), (11000, 128, "TILE_IL"))   # x 3 batches: 12 | 86 x 2 x 3 = 516 | 172 x 2 x 3 = 1032 tiles


def batch_fields(layout, M, Nn, exact, rng):
    K, R, ldc, B = 64, M + 9, Nn + 4, 3
    f = dict(M=M, N=Nn, K=K, lda=K, ldw=K, ldc=ldc, batch=B, alpha=0.5 if exact else 0.75, relu=1)
    f.update({"padded": dict(sA=R * K + 8, sW=Nn * K + 12, sC=M * ldc + 20, sBias=Nn + 2),        # gaps behind every operand of a batch
              "shared": dict(sA=0, sW=0, sC=M * ldc + 20, sBias=Nn + 2),                            # one A, one W, a bias per batch
              "sA_odd": dict(sA=R * K + 1, sW=Nn * K, sC=M * ldc, sBias=Nn),                        # alignment of A and A2 differs per batch
              "sC_odd": dict(sA=R * K, sW=Nn * K, sC=M * ldc + 21, sBias=Nn)}[layout])             # vector and scalar stores alternate by batch
    f.update(A=operands(rng, (B - 1) * f["sA"] + R * K, exact), A2=operands(rng, (B - 1) * f["sA"] + R * K, exact),
             W=operands(rng, (B - 1) * f["sW"] + Nn * K, exact, K ** -0.5), bias=operands(rng, (B - 1) * f["sBias"] + Nn, exact))
    return f, (B - 1) * f["sC"] + (M + TAIL) * ldc


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout,M,Nn,form", [(lay, *shape) for lay in ("padded", "shared", "sC_odd") for shape in BATCH_SHAPES] + [("sA_odd", 70, 70, "GENERIC")])
def test_batch_and_strides(layout, M, Nn, form, kind):
    exact = kind == "exact"
    f, size = batch_fields(layout, M, Nn, exact, np.random.default_rng([M, Nn, exact, len(layout)]))
    got, ref = run_gemm(size, form, **f)
    assert_gemm(got, ref, exact)


# ------------------------------------------------------------------------------------------------ the engine's two fp32 score launches
PATCH_NB = ((40, "SMALL"), (600, "TILE"), (1100, "TILE_IL"))
LIM, T1 = 64, 3000


@functools.lru_cache(maxsize=None)
def patch_case(kind):
    """Patch scores (engine.cpp, heads_and_matching): a batch list of 64 x 64 products of gathered rows of ONE matrix, both operands
    gathered with out-of-range rows.  Operands for the longest list; a shorter list is its first batches."""
    rng = np.random.default_rng(31 + (kind == "exact"))
    nb = PATCH_NB[-1][0]
    feat = operands(rng, (T1 + PAST, 64), kind == "exact")
    ia = np.stack([gather_indices(rng, LIM, T1) for _ in range(nb)])
    iw = np.stack([gather_indices(rng, LIM, T1) for _ in range(nb)])
    f = dict(M=LIM, N=LIM, K=64, A=feat, lda=64, a_idx=ia, a_limit=T1, W=feat, ldw=64, w_idx=iw, w_limit=T1, alpha=0.125, ldc=LIM,
             sC=LIM * LIM, sAidx=LIM, sWidx=LIM)
    return f, gemm_reference((nb + 1) * LIM * LIM, batch=nb, **f), {}


def live_batches(full, live, NB):
    size, n = (NB + 1) * LIM * LIM, live * LIM * LIM
    exp, mass, written = np.full(size, SENTINEL, dtype=np.float64), np.zeros(size), np.zeros(size, dtype=bool)
    exp[:n], mass[:n], written[:n] = full[0][:n], full[1][:n], full[2][:n]
    return exp, mass, written


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("live", [0, 1, -11, None], ids=["live0", "live1", "liveNB-11", "liveNB"])
@pytest.mark.parametrize("NB,form", PATCH_NB)
def test_patch_scores_with_a_live_count(NB, form, live, kind):
    """The live batches against float64; the batches past the device-side count keep the sentinel."""
    f, full, device = patch_case(kind)
    live = NB if live is None else NB + live if live < 0 else live
    got, _ = run_gemm((NB + 1) * LIM * LIM, form, device, reference=False, batch=NB, batch_live=live, **f)
    assert_gemm(got, live_batches(full, live, NB), kind == "exact")


def test_patch_scores_same_bytes_whatever_the_list_length():
    f, _, device = patch_case("normal")
    got = [run_gemm((NB + 1) * LIM * LIM, form, device, reference=False, batch=NB, **f)[0] for NB, form in PATCH_NB]
    n = PATCH_NB[0][0] * LIM * LIM
    assert (got[0][:n] != SENTINEL).all()
    assert np.array_equal(got[0][:n], got[1][:n]) and np.array_equal(got[0][:n], got[2][:n])


COARSE = {3: (200, "SMALL", [70, 129, 33, 200, 64, 5]), 40: (260, "TILE", None), 48: (260, "TILE_IL", None)}   # 4 x 4 x 3 = 48 | 5 x 5 x 40 = 1000 | 5 x 5 x 48 = 1200 tiles


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,seg_a0,seg_w0", [(B, B, 0) for B in sorted(COARSE)] + [(B, 0, B) for B in sorted(COARSE)], ids=lambda v: str(v))
def test_coarse_scores_ragged_batch(B, seg_a0, seg_w0, kind):
    """Coarse scores (engine.cpp, coarse_front): batch b multiplies row segment B + b of one matrix by its row segment b, every batch
    with its own row and column count; each block against float64, everything outside each block against the sentinel.  Once with
    the engine's seg_a0 = B, seg_w0 = 0, once with the roles of the two segment lists exchanged (seg_w0 != 0)."""
    exact = kind == "exact"
    rng = np.random.default_rng([B, exact])
    nmax, form, lens = COARSE[B]
    if lens is None:
        lens = rng.integers(1, nmax + 1, 2 * B)
        plant = [1, 4, 5, 33, 64, 129, 200, nmax]
        lens[rng.permutation(B)[:8]] = plant            # W segments
        lens[B + rng.permutation(B)[:8]] = plant[::-1]  # A segments
    off = np.cumsum(lens).astype(np.int32)
    feat = operands(rng, (int(off[-1]), 32), exact)
    f = dict(M=nmax, N=nmax, K=32, A=feat, lda=32, W=feat, ldw=32, alpha=0.5 if exact else 0.75, ldc=nmax, batch=B, sC=nmax * nmax,
             seg_off=off, seg_a0=seg_a0, seg_w0=seg_w0)
    got, ref = run_gemm((B + 1) * nmax * nmax, form, **f)
    assert int(ref[2].sum()) == int(sum(int(lens[B + b]) * int(lens[b]) for b in range(B)))   # every block whole, none overlapping
    assert_gemm(got, ref, exact)


# ------------------------------------------------------------------------------------------------ LayerNorm epilogue behind a gather
@pytest.mark.parametrize("Nn,form", [(64, "LN_TILE64"), (128, "LN_TILE128"), (256, "LN_TILE256")])
def test_layernorm_epilogue_with_a_gather_on_a(Nn, form):
    """The LayerNorm launches gemm_ln256 declines (and the two narrower widths) with zero rows in the gather: against float64 at the
    tolerance of test_linear_layernorm_fused_epilogue, and bitwise against the gathered GEMM followed by roitr_add_layernorm."""
    from roitr_amd import ops
    rng = np.random.default_rng(Nn)
    M, K, R, RR = 130, 64, 150, 143
    f = dict(M=M, N=Nn, K=K, A=operands(rng, (R + PAST, K), False), lda=K, a_idx=gather_indices(rng, M, R), a_limit=R, W=operands(rng, (Nn, K), False, K ** -0.5),
             ldw=K, bias=operands(rng, Nn, False), alpha=1.0, ldc=Nn, batch=1)
    ln = dict(ln_gamma=operands(rng, Nn, False), ln_beta=operands(rng, Nn, False), ln_res=operands(rng, (RR, Nn), False),
              ln_res_idx=rng.integers(0, RR, M).astype(np.int32), ln_post=operands(rng, (M, Nn), False), ln_relu=1, ln_eps=1e-5)
    device = {}
    got, (exp, _, written) = run_gemm((M + TAIL) * Nn, form, device, **f, **ln)
    assert (got[~written] == SENTINEL).all() and int(written.sum()) == M * Nn
    err = np.abs(got - exp)[written]
    assert (err <= 2e-5 + 2e-5 * np.abs(exp[written])).all(), float(err.max())
    plain, _ = run_gemm(M * Nn, "SMALL", device, reference=False, **f)
    d = lambda k: device[id(ln[k])][0]
    two = ops.add_layernorm(torch.from_numpy(plain).cuda().view(M, Nn), d("ln_gamma"), d("ln_beta"), res=d("ln_res").view(RR, Nn), res_idx=d("ln_res_idx"),
                            post=d("ln_post").view(M, Nn), relu=True, eps=1e-5)
    assert np.array_equal(two.cpu().numpy().reshape(-1), got[:M * Nn])


# ------------------------------------------------------------------------------------------------ refusals and empty launches
def dev(*shape):
    return torch.full(shape, 0.5, device="cuda")


def refused_cases():
    """Refusals that return before any launch, with real, correctly sized buffers: (fields, what the message must say)."""
    c = lambda *shape: torch.full(shape, SENTINEL, device="cuda")
    ln = lambda n: dict(ln_gamma=dev(n), ln_beta=dev(n), ln_eps=1e-5)
    return {"layernorm_batch2": (dict(M=64, N=64, K=64, A=dev(2, 64, 64), lda=64, W=dev(2, 64, 64), ldw=64, C=c(2, 64, 64), ldc=64, batch=2, sA=4096, sW=4096,
                                      sC=4096, alpha=1.0, **ln(64)), "LayerNorm epilogue shape"),
            "layernorm_n192": (dict(M=64, N=192, K=64, A=dev(64, 64), lda=64, W=dev(192, 64), ldw=64, C=c(64, 192), ldc=192, batch=1, alpha=1.0, **ln(192)),
                               "LayerNorm epilogue shape"),
            "a_cat_batch2": (dict(M=64, N=64, K=96, A=dev(2, 64, 64), lda=64, A_cat=dev(64, 32), lda_cat=32, k_cat=64, W=dev(2, 64, 96), ldw=96, C=c(2, 64, 64),
                                  ldc=64, batch=2, sA=4096, sW=64 * 96, sC=4096, alpha=1.0), "K-concatenated A")}


@pytest.mark.parametrize("case", ["layernorm_batch2", "layernorm_n192", "a_cat_batch2"])
def test_refusals_name_themselves_and_write_nothing(case):
    fields, says = refused_cases()[case]
    assert gemm_form(**fields) == -ERR_UNSUPPORTED
    status, stale = gemm_status(M=8, N=64, K=64, A=None, lda=64, W=dev(64, 64), ldw=64, C=dev(8, 64), ldc=64, batch=1)   # leaves ITS message behind
    assert status != 0 and "null operand" in stale
    status, text = gemm_status(**fields)
    assert status == ERR_UNSUPPORTED
    assert says in text and "null operand" not in text, text
    assert (fields["C"] == SENTINEL).all()


@pytest.mark.parametrize("empty", ["M", "N", "batch"])
def test_empty_launches_return_ok_and_write_nothing(empty):
    out = torch.full((64, 64), SENTINEL, device="cuda")
    fields = dict(M=64, N=64, K=64, A=dev(64, 64), lda=64, W=dev(64, 64), ldw=64, bias=dev(64), C=out, ldc=64, batch=1, alpha=1.0)
    fields[empty] = 0
    assert gemm_form(**fields) == "NOTHING"
    _gemm_abi(**fields)
    assert (out == SENTINEL).all()
