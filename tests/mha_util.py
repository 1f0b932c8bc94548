"""RoitrMha (include/roitr_engine.h) for the tests: the struct by field name, roitr_mha_form -- the rule roitr_mha dispatches through --
through the C ABI, and a launch that asserts the form first.  mha_struct / mha_form need the built library and no GPU (host code that
follows no pointer); launch needs one."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_UNSUPPORTED = 3
P = 0x7f0000000000   # a 16-byte aligned "pointer"; PTR(i): addresses 1 MiB apart
PTR = lambda i: P + (i << 20)


def _forms():
    text = open(os.path.join(ROOT, "include", "roitr_engine.h")).read()
    return {name: int(value) for name, value in re.findall(r"#define ROITR_MHA_(\w+) (\d+)", text)}


FORM = _forms()
FORM_NAME = {v: k for k, v in FORM.items()}


def mha_struct(**fields):
    """RoitrMha with the fields given by name, everything else zero (a pointer field takes a fake address)."""
    from roitr_amd import _lib as L
    a = L.struct("RoitrMha")()
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def mha_form(a=None, **fields):
    """Name of the form roitr_mha gives the struct `a` (or the one of `fields`), or the negative status as an int."""
    from roitr_amd import ops
    form = ops._lib().roitr_mha_form(ctypes.byref(mha_struct(**fields) if a is None else a))
    return FORM_NAME[form] if form >= 0 else form


def shape(C=256, heads=4, nk_max=78, cross=False, e=None, packed=True, **over):
    """Fields of a call with the engine's leading dimensions (csrc/engine.cpp): self attention (e = "f32" / "bf16": with E) on
    q | k | v as the column blocks of one (T, 3C) buffer, cross attention (a partner list) on three dense buffers; not packed: dense
    rows for both.  `over` is laid over it."""
    ld = C if cross or not packed else 3 * C
    f = dict(q_row0=0, q_rows=100, C=C, heads=heads, q=PTR(1), ldq=ld, k=PTR(2), ldk=ld, v=PTR(3), ldv=ld, offset=PTR(4), cloud_of_row=PTR(5),
             partner=PTR(6) if cross else 0, scale=0.125, nk_max=nk_max, out=PTR(7), ldo=C)
    if e:
        f.update(E=PTR(8), eoff=PTR(9), qt=PTR(10), bp=PTR(11), ebar=PTR(12), e_bf16=int(e == "bf16"))
    f.update(over)
    return f


def launch(expect_form, *args, **kw):
    """ops.multi_head_attention(*args, **kw) that first asserts roitr_mha_form on the very struct it launches."""
    from roitr_amd import _lib as L
    from roitr_amd import ops
    a, out, ebar = ops.mha_args(*args, **kw)
    form = mha_form(a)
    assert form == expect_form, (form, expect_form)
    L.check(ops._lib().roitr_mha(ctypes.byref(a), L.stream_ptr()), "mha")
    return out, ebar
