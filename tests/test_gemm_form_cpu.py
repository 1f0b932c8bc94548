"""roitr_gemm_form (include/roitr_engine.h): the kernel form roitr_gemm gives a RoitrGemm, or the status it refuses it with.  The
launcher dispatches through the same function, so what is pinned here is what runs.  Pure host code that follows no pointer: needs
the built library, no GPU; fake aligned integers serve as pointers.

The table is the one of DESIGN.md ("Forms of the fp32 GEMM").  CASES lists the form of every launch of tests/test_gemm_fp32_gpu.py by
its shape, so a later change of a threshold cannot silently move one of its cases to another kernel."""
import os
import re

import pytest

from gemm_util import ERR_ARG, ERR_UNSUPPORTED, FORM, ROOT, gemm_form

P = 0x7f0000000000   # a 16-byte aligned "pointer"; the operands get addresses 1 MiB apart


def form(**over):
    """Form of a dense fast-path launch (M = N = 64, K = 64) with `over` laid over it."""
    f = dict(M=64, N=64, K=64, A=P, lda=64, W=P + (1 << 20), ldw=64, C=P + (2 << 20), ldc=64, batch=1, alpha=1.0)
    f.update(over)
    for k in ("lda", "ldw", "ldc"):
        if k not in over:
            f[k] = f["N"] if k == "ldc" else f["K"]
    return gemm_form(**f)


PTR = lambda i: P + (i << 20)
LN = dict(ln_gamma=PTR(3), ln_beta=PTR(4))


def test_form_names():
    assert FORM == {"NOTHING": 0, "SMALL": 1, "TILE": 2, "TILE_IL": 3, "GENERIC": 4, "LN_GENERIC": 5, "LN_TILE64": 6, "LN_TILE128": 7,
                    "LN_TILE256": 8, "LN256": 9, "BF16": 10, "X3": 11}


def test_design_table_lists_every_form():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = text[text.index("**Forms of the fp32 GEMM.**"):]
    table = table[:table.index("\n\n", table.index("| form |"))]
    assert re.findall(r"^\| (\w+) \| (\d+) \|", table, re.M) == [(name, str(value)) for name, value in sorted(FORM.items(), key=lambda kv: kv[1])]


# the launches of tests/test_gemm_fp32_gpu.py: (form, fields over the dense 64 x 64 x 64 launch)
CASES = [
    # forms x options: N = 250, three row counts, three K
    *[(f, dict(M=M, N=250, K=K, ldc=260)) for M, f in ((100, "SMALL"), (8327, "TILE"), (16647, "TILE_IL")) for K in (32, 64, 256)],
    *[(f, dict(M=M, N=250, K=64, ldc=251)) for M, f in ((100, "SMALL"), (8327, "TILE"), (16647, "TILE_IL"))],
    *[(f, dict(M=M, N=250, K=64, ldc=260, A2=PTR(5), a_idx=PTR(6), a_limit=M + 50)) for M, f in ((100, "SMALL"), (8327, "TILE"), (16647, "TILE_IL"))],
    *[(f, dict(M=M, N=250, K=96, ldc=260, lda=64, A2=PTR(5), A_cat=PTR(7), lda_cat=32, k_cat=64, a_cat_idx=PTR(8)))
      for M, f in ((100, "SMALL"), (8327, "TILE"), (16647, "TILE_IL"))],
    ("SMALL", dict(M=156, N=250, K=256, ldc=260)),
    # K = 2048: the last K of the fast path
    ("SMALL", dict(M=70, N=70, K=2048, ldc=72, a_idx=PTR(6), a_limit=90, w_idx=PTR(9), w_limit=90)),
    # generic
    *[("GENERIC", dict(M=130, N=70, K=K, relu=1)) for K in (1, 31, 33, 100, 2080)],
    ("GENERIC", dict(M=130, N=70, K=64, lda=67)),
    ("GENERIC", dict(M=130, N=70, K=64, A=P + 4)),
    # batch and strides
    *[(f, dict(M=M, N=N, K=64, ldc=N + 4, batch=3, sA=(M + 9) * 64 + 8, sW=N * 64 + 12, sC=M * (N + 4) + 20, sBias=N + 2))
      for M, N, f in ((70, 70, "SMALL"), (5500, 128, "TILE"), (11000, 128, "TILE_IL"))],
    *[(f, dict(M=M, N=N, K=64, ldc=N + 4, batch=3, sA=0, sW=0, sC=M * (N + 4) + 20, sBias=N + 2))
      for M, N, f in ((70, 70, "SMALL"), (5500, 128, "TILE"), (11000, 128, "TILE_IL"))],
    ("GENERIC", dict(M=70, N=70, K=64, ldc=72, batch=3, sA=79 * 64 + 1, sW=70 * 64, sC=70 * 72)),
    *[(f, dict(M=M, N=N, K=64, ldc=N + 4, batch=3, sA=(M + 9) * 64, sW=N * 64, sC=M * (N + 4) + 21))
      for M, N, f in ((70, 70, "SMALL"), (5500, 128, "TILE"), (11000, 128, "TILE_IL"))],
    # patch scores
    *[(f, dict(M=64, N=64, K=64, a_idx=PTR(6), a_limit=3000, w_idx=PTR(9), w_limit=3000, batch=NB, sC=4096, sAidx=64, sWidx=64, alpha=0.125,
               batch_live=PTR(10))) for NB, f in ((40, "SMALL"), (600, "TILE"), (1100, "TILE_IL"))],
    # coarse scores
    *[(f, dict(M=nmax, N=nmax, K=32, ldc=nmax, batch=B, sC=nmax * nmax, seg_off=PTR(11), seg_a0=a0, seg_w0=B - a0))
      for B, nmax, f in ((3, 200, "SMALL"), (40, 260, "TILE"), (48, 260, "TILE_IL")) for a0 in (B, 0)],
    # LayerNorm with a gather on A
    *[(f, dict(M=130, N=N, K=64, a_idx=PTR(6), a_limit=150, ln_res=PTR(12), ln_res_idx=PTR(13), ln_post=PTR(14), ln_relu=1, **LN))
      for N, f in ((64, "LN_TILE64"), (128, "LN_TILE128"), (256, "LN_TILE256"))],
    # ... and its two-launch twin's first launch
    *[("SMALL", dict(M=130, N=N, K=64, a_idx=PTR(6), a_limit=150)) for N in (64, 128, 256)],
    # nothing to do
    ("NOTHING", dict(M=0)), ("NOTHING", dict(N=0)), ("NOTHING", dict(batch=0)),
]


@pytest.mark.parametrize("want,fields", CASES, ids=[f"{i}-{c[0]}" for i, c in enumerate(CASES)])
def test_form_of_every_gpu_case(want, fields):
    assert form(**fields) == want


def test_other_forms():
    assert form(M=130, K=40, **LN) == "LN_GENERIC"
    assert form(M=130, N=256, **LN) == "LN256"
    assert form(M=130, N=256, w_idx=PTR(9), **LN) == "LN_TILE256"
    assert form(M=130, N=128, **LN) == "LN_TILE128"
    assert form(M=64 * 2000, N=64, **LN) == "LN_TILE64"          # the LayerNorm forms do not switch to SMALL or by the grid
    assert form(W=PTR(1), ldw=64, bf16=1) == "BF16"
    assert form(W=PTR(1), ldw=64, bf16=8, w_piece=64 * 64) == "X3"
    assert form(W=PTR(1), ldw=64, bf16=8, w_piece=64 * 64 - 8) == -ERR_UNSUPPORTED
    assert form(K=48, bf16=1) == -ERR_UNSUPPORTED


@pytest.mark.parametrize("batch", [1, 3])
def test_switch_points(batch):
    """511 / 512 / 1023 / 1024 tiles of 64 x 64, times batch."""
    for rows, want in ((511, "SMALL"), (512, "TILE"), (1023, "TILE"), (1024, "TILE_IL")):
        if batch == 1:
            shapes = [dict(M=64 * rows), dict(M=64 * rows - 63), dict(M=64, N=64 * rows - 63, ldc=64 * rows)]
        elif rows % 3 == 0:
            shapes = [dict(M=64 * (rows // 3), batch=3, sC=64 * 64 * rows)]
        else:   # rows = 7 * 73, 512 = 2 * 256, 1024 = 4 * 256
            d = 7 if rows == 511 else 4
            shapes = [dict(M=64 * (rows // d), batch=d, sC=64 * 64 * rows)]
            assert (rows // d) * d == rows
        for s in shapes:
            assert form(**s) == want, (s, want)
    # the count is of 64 x 64 tiles, whatever the kernel's own tile is
    assert form(M=64 * 511 + 1) == "TILE" and form(M=64 * 1023 + 1) == "TILE_IL"


def test_each_fast_path_condition_broken_alone_gives_the_generic_kernel():
    assert form(M=640, N=640) == "SMALL"
    for broken in (dict(K=2080), dict(K=33), dict(lda=65), dict(ldw=65), dict(A=P + 4), dict(W=PTR(1) + 4), dict(batch=2, sA=4097, sW=4096, sC=4096),
                   dict(batch=2, sA=4096, sW=4098, sC=4096), dict(A2=PTR(5) + 8)):
        assert form(M=640, N=640, **broken) == "GENERIC", broken
        assert form(M=64 * 2000, N=640, **broken) == "GENERIC", broken      # at any grid
    assert form(M=640, N=640, K=2048) == "SMALL"
    assert form(M=640, N=640, A2=PTR(5), batch=2, sA=4096, sW=4096, sC=640 * 640) == "SMALL"
    # the output's layout does not choose the kernel (the store path is the kernel's own decision)
    assert form(M=640, N=640, ldc=641, C=PTR(2) + 4) == "SMALL"


REFUSALS = [
    ("LayerNorm with batch 2", dict(batch=2, sA=4096, sW=4096, sC=4096, **LN), ERR_UNSUPPORTED),
    ("LayerNorm with N = 192", dict(N=192, **LN), ERR_UNSUPPORTED),
    ("LayerNorm with N = 512", dict(N=512, **LN), ERR_UNSUPPORTED),
    ("LayerNorm with N = 100", dict(N=100, **LN), ERR_UNSUPPORTED),
    ("LayerNorm with relu", dict(relu=1, **LN), ERR_UNSUPPORTED),
    ("LayerNorm without beta", dict(ln_gamma=PTR(3)), ERR_UNSUPPORTED),
    ("LayerNorm with seg_off", dict(seg_off=PTR(11), **LN), ERR_UNSUPPORTED),
    ("non-fast LayerNorm with N = 128", dict(N=128, K=40, **LN), ERR_UNSUPPORTED),
    ("A_cat with batch 2", dict(K=96, lda=64, A_cat=PTR(7), lda_cat=32, k_cat=64, batch=2, sA=4096, sW=8192, sC=4096), ERR_UNSUPPORTED),
    ("A_cat with seg_off", dict(K=96, lda=64, A_cat=PTR(7), lda_cat=32, k_cat=64, seg_off=PTR(11)), ERR_UNSUPPORTED),
    ("A_cat with k_cat 16", dict(K=96, lda=16, A_cat=PTR(7), lda_cat=80, k_cat=16), ERR_UNSUPPORTED),
    ("A_cat with k_cat = K", dict(K=64, lda=64, A_cat=PTR(7), lda_cat=32, k_cat=64), ERR_UNSUPPORTED),
    ("A_cat off the fast path", dict(K=100, lda=64, A_cat=PTR(7), lda_cat=36, k_cat=64), ERR_UNSUPPORTED),
    ("A_cat misaligned", dict(K=96, lda=64, A_cat=PTR(7) + 4, lda_cat=32, k_cat=64), ERR_UNSUPPORTED),
    ("a_cat_idx without A_cat", dict(a_cat_idx=PTR(8)), ERR_ARG),
    ("ip_feat without LayerNorm", dict(ip_feat=PTR(15), ip_idx=PTR(16), ip_dist2=PTR(17)), ERR_UNSUPPORTED),
    ("ip_feat without its indices", dict(ip_feat=PTR(15), **LN), ERR_UNSUPPORTED),
    ("more than 0x7ffffff0 tiles", dict(M=0x7fffffff, N=64 * 64, ldc=64 * 64), ERR_UNSUPPORTED),
    ("more than 0x7ffffff0 tiles by the batch", dict(M=64 * 32768, N=64 * 256, ldc=64 * 256, batch=256, sC=1 << 40), ERR_UNSUPPORTED),
    ("more than 0x7ffffff0 tiles, bf16", dict(M=0x7fffffff, N=64 * 300, ldc=64 * 300, bf16=1, w_idx=PTR(9)), ERR_UNSUPPORTED),
    ("more than 0x7ffffff0 tiles, x3", dict(M=0x7fffffff, N=64 * 300 + 1, ldc=64 * 304, bf16=8, w_piece=(64 * 300 + 1) * 64), ERR_UNSUPPORTED),
    ("K = 0", dict(K=0), ERR_ARG),
    ("no A", dict(A=0), ERR_ARG),
    ("no W", dict(W=0), ERR_ARG),
    ("no C", dict(C=0), ERR_ARG),
]


@pytest.mark.parametrize("what,fields,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, fields, status):
    assert form(**fields) == -status


def test_the_largest_grid_that_is_taken():
    assert form(M=64 * 32768, N=64 * 256, ldc=64 * 256, batch=255, sC=1 << 40) == "TILE_IL"     # 0x7f800000 tiles
    assert form(M=64 * 32768, N=64 * 256, ldc=64 * 256, batch=256, sC=1 << 40) == -ERR_UNSUPPORTED  # 0x80000000
