"""roitr_mha_form (include/roitr_engine.h): the kernel form roitr_mha gives a RoitrMha, or the status it refuses it with.  The launcher
dispatches through the same host function (mha_plan, csrc/geo_attn.hip), so what is pinned here is what runs.  Host code that
follows no pointer: needs the built library, no GPU; fake aligned integers serve as pointers.

The table is the one of DESIGN.md ("Forms of the global attention").  test_form_of_every_gpu_case takes the cases of
tests/test_geo_attn_gpu.py from that module's own table, so a later change of a threshold cannot silently move one of them to
another kernel."""
import os
import re

import pytest

import test_geo_attn_gpu as G
from mha_util import ERR_UNSUPPORTED, FORM, PTR, ROOT, mha_form, shape


def form(**kw):
    return mha_form(**shape(**kw))


def test_form_names():
    assert FORM == {"NOTHING": 0, "GEO20": 1, "GEO32": 2, "GEO_STREAM": 3, "GEO_WIDE_H": 4, "GEO_WIDE2": 5, "GEO_WIDE2_H": 6, "PLAIN128": 7,
                    "PLAIN1024": 8, "PLAIN_WIDE2": 9, "GENERIC": 10}


def test_design_table_lists_every_form():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = text[text.index("**Forms of the global attention.**"):]
    table = table[:table.index("\n\n", table.index("| form |"))]
    assert re.findall(r"^\| (\w+) \| (\d+) \|", table, re.M) == [(name, str(value)) for name, value in sorted(FORM.items(), key=lambda kv: kv[1])]


@pytest.mark.parametrize("case", G.CASES, ids=[c[0] for c in G.CASES])   # importing the GPU module starts nothing on a GPU
def test_form_of_every_gpu_case(case):
    _, want, C, heads, sizes, cross, e, _ = case
    T = sum(sizes)
    for q_rows in (T, G.window(T)[1]):
        for packed in (True, False):   # the engine's leading dimensions and dense ones
            assert form(C=C, heads=heads, nk_max=max(sizes), cross=cross, e=e, packed=packed, q_rows=q_rows) == want, (packed, q_rows)


def test_bitwise_and_fold_cases_cover_every_form():
    forms = {c[1] for c in G.CASES}
    assert forms == set(FORM) - {"NOTHING"}
    assert {c[1] for c in G.CASES if c[0] in G.BITWISE} == forms
    for (C, e), want in G.FOLD_FORM.items():
        assert form(C=C, nk_max=150, e=e) == want


# nk_max -> form at every switch point, from both sides
SELF_F32_256 = {80: "GEO20", 81: "GEO32", 128: "GEO32", 129: "GEO_STREAM", 512: "GEO_STREAM", 513: "GEO_STREAM", 1024: "GEO_STREAM", 1025: "GENERIC"}
SELF_F32_512 = {80: "GEO_WIDE2", 81: "GEO_WIDE2", 128: "GEO_WIDE2", 129: "GEO_WIDE2", 512: "GEO_WIDE2", 513: "GENERIC", 1024: "GENERIC", 1025: "GENERIC"}
SELF_BF16 = {80: 0, 81: 0, 128: 0, 129: 0, 512: 0, 513: -ERR_UNSUPPORTED, 1024: -ERR_UNSUPPORTED, 1025: -ERR_UNSUPPORTED}   # 0: the width's form
CROSS_256 = {80: "PLAIN128", 81: "PLAIN128", 128: "PLAIN128", 129: "PLAIN1024", 512: "PLAIN1024", 513: "PLAIN1024", 1024: "PLAIN1024", 1025: "GENERIC"}
CROSS_512 = {80: "PLAIN_WIDE2", 81: "PLAIN_WIDE2", 128: "PLAIN_WIDE2", 129: "PLAIN_WIDE2", 512: "PLAIN_WIDE2", 513: "GENERIC", 1024: "GENERIC", 1025: "GENERIC"}


@pytest.mark.parametrize("nk", [80, 81, 128, 129, 512, 513, 1024, 1025])
@pytest.mark.parametrize("packed", [True, False])
def test_nk_max_switch_points(nk, packed):
    kw = dict(nk_max=nk, packed=packed)
    assert form(C=256, e="f32", **kw) == SELF_F32_256[nk]
    assert form(C=512, e="f32", **kw) == SELF_F32_512[nk]
    assert form(C=256, e="bf16", **kw) == (SELF_BF16[nk] or "GEO_WIDE_H")
    assert form(C=512, e="bf16", **kw) == (SELF_BF16[nk] or "GEO_WIDE2_H")
    assert form(C=256, cross=True, **kw) == CROSS_256[nk]
    assert form(C=512, cross=True, **kw) == CROSS_512[nk]
    # self attention without E is plain attention over the own cloud
    assert form(C=256, **kw) == CROSS_256[nk] and form(C=512, **kw) == CROSS_512[nk]


@pytest.mark.parametrize("cross,e", [(False, "f32"), (True, None)])
def test_off_layout_calls_take_the_generic_kernel(cross, e):
    kw = dict(cross=cross, e=e)
    for C in (256, 512):
        assert form(C=C, **kw) != "GENERIC"
        assert form(C=C, heads=8, **kw) == "GENERIC"
        assert form(C=C, packed=False, ldq=C + 2, **kw) == "GENERIC"       # ldq % 4 != 0
        assert form(C=C, packed=False, ldv=C + 2, **kw) != "GENERIC"       # ldv chooses nothing
    assert form(C=384, **kw) == "GENERIC"
    assert form(C=128, heads=2, **kw) == "GENERIC"


def test_partner_with_e_takes_the_generic_kernel():
    for C in (256, 512):
        for nk in (78, 468):
            assert form(C=C, nk_max=nk, e="f32", partner=PTR(6)) == "GENERIC"
            assert form(C=C, nk_max=nk, e="bf16", partner=PTR(6)) == -ERR_UNSUPPORTED


def test_nothing_to_do():
    for q_rows in (0, -1):
        assert form(q_rows=q_rows) == "NOTHING"
        assert form(q_rows=q_rows, heads=9, C=250, e="bf16") == "NOTHING"   # as the launcher: before any refusal


def test_the_engines_calls():
    """csrc/engine.cpp run_geo: a self layer (q | k | v in one (T, 3C) buffer, E, no partner) and the two halves of a cross layer (dense
    rows, a partner list, a window of the rows), with nk_max = the largest superpoint count of the call."""
    for nk, C, e, self_form, cross_form in ((78, 256, "f32", "GEO20", "PLAIN128"),          # 5000-point clouds
                                            (125, 512, "bf16", "GEO_WIDE2_H", "PLAIN_WIDE2"),   # factor 2 with bf16 operands: config 4
                                            (468, 256, "f32", "GEO_STREAM", "PLAIN1024")):      # 30000-point clouds
        assert form(C=C, nk_max=nk, e=e, q_rows=16 * nk) == self_form
        for q_row0 in (0, 8 * nk):
            assert form(C=C, nk_max=nk, cross=True, q_row0=q_row0, q_rows=8 * nk) == cross_form


# the refusals of test_geo_attn_gpu.test_mha_unsupported_shapes_name_themselves (clouds of 6 and 5 nodes, nk_max 6 unless given)
REFUSALS = [
    ("bf16 E with 8 heads", dict(C=256, heads=8, e="bf16", nk_max=6)),
    ("bf16 E at C = 384", dict(C=384, heads=4, e="bf16", nk_max=6)),
    ("bf16 E at C = 512 with 513 keys", dict(C=512, heads=4, e="bf16", nk_max=513)),
    ("bf16 E at C = 256 with 1024 keys", dict(C=256, heads=4, e="bf16", nk_max=1024)),
    ("9 heads", dict(C=288, heads=9, nk_max=6)),
    ("C % heads", dict(C=250, heads=4, nk_max=6)),
    ("(C / heads) % 4", dict(C=24, heads=4, nk_max=6)),
    ("LDS bound with E", dict(C=256, heads=4, e="f32", nk_max=4700)),
    ("LDS bound without E", dict(C=256, heads=8, nk_max=4800, cross=True)),
    ("ldk % 4", dict(C=256, packed=False, ldk=258)),
    ("0 heads", dict(C=256, heads=0)),
]


@pytest.mark.parametrize("what,fields", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, fields):
    assert form(**fields) == -ERR_UNSUPPORTED


def test_the_generic_kernels_lds_bound():
    """C + heads C + 2 heads nk_max + 8 floats with E, C + heads nk_max + 8 without, against 150 KB = 38400 floats; no other form has it
    (each has nk_max <= 1024)."""
    assert form(C=256, heads=4, e="f32", nk_max=(38400 - 5 * 256 - 8) // 8) == "GENERIC"
    assert form(C=256, heads=4, e="f32", nk_max=(38400 - 5 * 256 - 8) // 8 + 1) == -ERR_UNSUPPORTED
    assert form(C=256, heads=8, cross=True, nk_max=(38400 - 256 - 8) // 8) == "GENERIC"
    assert form(C=256, heads=8, cross=True, nk_max=(38400 - 256 - 8) // 8 + 1) == -ERR_UNSUPPORTED
