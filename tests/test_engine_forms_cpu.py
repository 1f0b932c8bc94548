"""roitr_local_form (include/roitr_engine.h): the form the engine runs every local transformer in, for every layer of both
configurations in all three operand modes.  Pure host code: needs the built library, no GPU.

The table is the one of DESIGN.md ("Forms of the local transformer"); the launch counts of profiles/engine_layers_refactor.txt hold
it against the forward before the forms had a name."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSAMPLE = (8, 16, 16, 16)
NBLOCKS = (2, 3, 3, 3)
FP32, BF16, F32X3 = 0, 1, 2


def _forms():
    text = open(os.path.join(ROOT, "include", "roitr_engine.h")).read()
    return {name: int(value) for name, value in re.findall(r"#define ROITR_LOCAL_(\w+) (\d+)", text)}


FORM = _forms()


@pytest.fixture(scope="module")
def local_form():
    from roitr_amd import _lib
    lib = _lib.lib()
    lib.roitr_local_form.restype = ctypes.c_int
    lib.roitr_local_form.argtypes = [ctypes.c_int] * 6
    names = {v: k for k, v in FORM.items()}
    return lambda *args: names[lib.roitr_local_form(*args)]


def layers(factor):
    """(name, in_dim, H, out_dim, K, transition_down) of every local transformer of the backbone (model/model.py:146-184)."""
    planes = (64 * factor, 128 * factor, 256 * factor, 256 * factor)
    out, in_planes = [], 1
    for l, pl in enumerate(planes):
        hid = min(pl, 256 * factor)
        out.append((f"enc{l + 1}.0", in_planes, hid, pl, NSAMPLE[l], 1))
        for b in range(1, NBLOCKS[l]):
            out.append((f"enc{l + 1}.{b}", pl, hid, pl, NSAMPLE[l], 0))
        out.append((f"dec{l + 1}.1", pl, hid, pl, NSAMPLE[l], 0))
        in_planes = pl
    return out


def expected(name, column):
    """column: (factor, bf16).  Rows as in the table: encN.0 by name, every other layer as "the blocks of level N"."""
    level = int(name[3])
    if name.endswith(".0") and name.startswith("enc"):
        return {"enc1.0": {(1, False): "FIRST"},
                "enc2.0": {(1, False): "FUSED_TD", (2, False): "TD_FOLD"},
                "enc3.0": {(1, False): "TD_FOLD"},
                "enc4.0": {(1, False): "TD_FOLD"}}[name].get(column, "SEQUENCE")
    if level == 1 or (level == 2 and column[0] == 1):
        return "FUSED_BLOCK"
    return "SEQUENCE"


def test_form_names():
    assert FORM == {"FIRST": 0, "FUSED_BLOCK": 1, "FUSED_TD": 2, "TD_FOLD": 3, "SEQUENCE": 4}


@pytest.mark.parametrize("factor", [1, 2], ids=["3DMatch", "4DMatch"])
@pytest.mark.parametrize("dtype", [FP32, BF16, F32X3], ids=["fp32", "bf16", "f32x3"])
def test_form_table(local_form, factor, dtype):
    ls = layers(factor)
    assert len(ls) == 15
    got = {name: local_form(i, h, o, k, td, dtype) for name, i, h, o, k, td in ls}
    want = {name: expected(name, (factor, dtype == BF16)) for name, *_ in ls}
    assert got == want


def test_unsupported_neighbour_count_is_the_sequence(local_form):
    for k in (4, 12, 32):
        assert local_form(1, 64, 64, k, 1, FP32) == "SEQUENCE"     # enc1.0: not FIRST
        assert local_form(64, 64, 64, k, 0, FP32) == "SEQUENCE"    # level-1 blocks: not FUSED_BLOCK


def test_transition_down_of_equal_widths_in_bf16_is_the_sequence(local_form):
    for width in (64, 128, 256, 512):
        assert local_form(width, width, width, 16, 1, BF16) == "SEQUENCE"
