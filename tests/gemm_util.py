"""RoitrGemm (include/roitr_engine.h) for the tests: the struct by field name, roitr_gemm / roitr_gemm_form through the C ABI, and ONE
float64 restatement of what the header's comment promises -- written from that comment, not from the kernels.

The restatement works on the HOST copies of the flat buffers exactly as the device sees them (element offsets from the pointer
that is passed) and returns the expected C buffer together with the mask of the elements the call may write: every other element
of the output must keep the sentinel it was filled with (padding columns N..ldc, rows >= M, gaps between batches, batches past
the live count, everything outside a segment's M_b x N_b block).

Two kinds of operands:
  exact   A, A2, A_cat, W and bias are integers with |v| <= 4, alpha a power of two, K <= 2080: every partial sum is an integer
          below 8 * 4 * 2080 < 2^24, so fp32 is exact in ANY summation order and the assertion is `==` against float64.
  normal  standard normal A (W scaled by 1 / sqrt(K)): |got - ref| / mass < 2e-6 with mass = |alpha| (|a| @ |w|^T) + |bias|, the
          bound of tests/test_stages_gpu.py::test_gemm_wide_shapes_against_float64, used at K <= 512 only.
"""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = float(np.float32(-1234.5678))   # no multiple of 1/2: never the result of exact operands
REL_BOUND = 2e-6
ERR_ARG, ERR_UNSUPPORTED = 1, 3


def _forms():
    text = open(os.path.join(ROOT, "include", "roitr_engine.h")).read()
    return {name: int(value) for name, value in re.findall(r"#define ROITR_GEMM_(\w+) (\d+)", text)}


FORM = _forms()
FORM_NAME = {v: k for k, v in FORM.items()}


def gemm_struct(**fields):
    """RoitrGemm with the fields given by name, everything else zero.  Tensors become device pointers; integers stay what they
    are (a pointer field takes a fake address: roitr_gemm_form follows none)."""
    from roitr_amd import _lib as L
    g = L.struct("RoitrGemm")()
    for k, v in fields.items():
        setattr(g, k, L.ptr(v) if hasattr(v, "data_ptr") else v)
    return g


def gemm_form(**fields):
    """Name of the form roitr_gemm gives the struct, or the negative status as an int."""
    from roitr_amd import _lib as L
    lib = L.lib()
    lib.roitr_gemm_form.restype = ctypes.c_int
    lib.roitr_gemm_form.argtypes = [ctypes.c_void_p]
    form = lib.roitr_gemm_form(ctypes.byref(gemm_struct(**fields)))
    return FORM_NAME[form] if form >= 0 else form


def gemm_status(**fields):
    """roitr_gemm through the C ABI; returns (status, text of roitr_last_error())."""
    import torch
    from roitr_amd import _lib as L
    status = L.lib().roitr_gemm(ctypes.byref(gemm_struct(**fields)), L.stream_ptr())
    torch.cuda.synchronize()
    return status, L.lib().roitr_last_error().decode()


def _gemm_abi(**fields):
    """roitr_gemm through the C ABI: RoitrGemm fields by name (tensors as device pointers), everything else zero."""
    import torch
    from roitr_amd import _lib as L
    L.check(L.lib().roitr_gemm(ctypes.byref(gemm_struct(**fields)), L.stream_ptr()), "gemm")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ operands
def operands(rng, shape, exact, scale=1.0):
    """float32 operand of the given kind (module docstring)."""
    if exact:
        return rng.integers(-4, 5, shape).astype(np.float32)
    return (rng.standard_normal(shape) * scale).astype(np.float32)


PAST = 20   # rows a gathered operand holds behind its limit


def gather_indices(rng, count, rows):
    """int32 row gather with the limit `rows`, drawn from [-5, rows + PAST) with out-of-range entries (zero rows) planted at both
    ends, at the tile edges and every 37th place, whatever `rows` is.  The operand itself should hold rows + PAST rows of data: a
    row past the limit is then a zero row because of the LIMIT, and a kernel that forgot the limit reads other numbers, not
    past the buffer."""
    idx = rng.integers(-5, rows + PAST, count).astype(np.int32)
    bad = np.array([-1, rows, -5, rows + PAST - 1], dtype=np.int32)
    for j, p in enumerate(sorted({0, count - 1, count // 2, *range(31, count, 37), *[q for q in (63, 64) if q < count]})):
        idx[p] = bad[j % 4]
    idx[min(1, count - 1)] = rows - 1   # the last row that exists
    return idx


# ------------------------------------------------------------------------------------------------ the contract, in float64
def _rows(buf, ld, idx, limit, width, base):
    """(len(idx), width) float64: row idx[i] of the row-major operand at buf[base:], leading dimension ld; an index < 0 or >= limit
    (when limit > 0) is a zero row."""
    ok = (idx >= 0) & ((idx < limit) if limit > 0 else True)
    safe = np.where(ok, idx, 0).astype(np.int64)
    out = buf[base + safe[:, None] * ld + np.arange(width)[None, :]].astype(np.float64)
    return out * ok[:, None], ok


def gemm_reference(c_size, *, M, N, K, A, lda, W, ldw, ldc, A2=None, a_idx=None, a_limit=0, w_idx=None, w_limit=0, bias=None, alpha=1.0,
                   relu=0, batch=1, sA=0, sW=0, sC=0, sBias=0, sAidx=0, sWidx=0, seg_off=None, seg_a0=0, seg_w0=0, ln_gamma=None,
                   ln_beta=None, ln_res=None, ln_res_idx=None, ln_post=None, ln_relu=0, ln_eps=0.0, A_cat=None, lda_cat=0, k_cat=0,
                   a_cat_idx=None, batch_live=None, sentinel=SENTINEL):
    """What roitr_gemm leaves in a C buffer of c_size floats that was filled with `sentinel`: (expected, mass, written), flat
    float64 / float64 / bool.  All operands are flat host arrays as seen from the pointer the call passes; batch_live is the int
    the device-side count holds.  mass is |alpha| (|a| @ |w|^T) + |bias| of the written elements (the scale of the fp32 bound)."""
    flat = lambda v: None if v is None else v.array.reshape(-1)[v.skip:] if isinstance(v, Offset) else np.asarray(v).reshape(-1)
    A, A2, W, bias, a_idx, w_idx, seg_off, A_cat, a_cat_idx = (flat(v) for v in (A, A2, W, bias, a_idx, w_idx, seg_off, A_cat, a_cat_idx))
    ln_gamma, ln_beta, ln_res, ln_res_idx, ln_post = (flat(v) for v in (ln_gamma, ln_beta, ln_res, ln_res_idx, ln_post))
    exp = np.full(c_size, float(np.float32(sentinel)), dtype=np.float64)
    mass = np.zeros(c_size, dtype=np.float64)
    written = np.zeros(c_size, dtype=bool)
    if M <= 0 or N <= 0 or batch <= 0:
        return exp, mass, written
    live = batch if batch_live is None else min(batch, int(batch_live))
    ka = k_cat if A_cat is not None else K
    for b in range(live):
        a_base, w_base, mb, nb = b * sA, b * sW, M, N
        if seg_off is not None:   # batch b: row segment seg_a0 + b of A times row segment seg_w0 + b of W; M / N only bound the grid
            assert a_idx is None and w_idx is None
            start = lambda i: 0 if i == 0 else int(seg_off[i - 1])
            ia, iw = seg_a0 + b, seg_w0 + b
            mb, nb = int(seg_off[ia]) - start(ia), int(seg_off[iw]) - start(iw)
            assert mb <= M and nb <= N
            a_base += start(ia) * lda
            w_base += start(iw) * ldw
        ai = np.arange(mb) if a_idx is None else a_idx[b * sAidx:b * sAidx + mb].astype(np.int64)
        wi = np.arange(nb) if w_idx is None else w_idx[b * sWidx:b * sWidx + nb].astype(np.int64)
        x, ok = _rows(A, lda, ai, a_limit, ka, a_base)
        if A2 is not None:   # with A_cat the addend covers the A part only
            x = x + _rows(A2, lda, ai, a_limit, ka, a_base)[0]
        if A_cat is not None:   # columns k >= k_cat: A_cat, by the A row's index or by its own gather
            assert a_cat_idx is None or a_idx is None
            ci = ai if a_cat_idx is None else a_cat_idx[:mb].astype(np.int64)
            x = np.concatenate([x, _rows(A_cat, lda_cat, ci, 0, K - k_cat, 0)[0] * ok[:, None]], axis=1)
        w, _ = _rows(W, ldw, wi, w_limit, K, w_base)
        bv = np.zeros(nb) if bias is None else bias[b * sBias:b * sBias + nb].astype(np.float64)
        y = float(alpha) * (x @ w.T) + bv
        ms = abs(float(alpha)) * (np.abs(x) @ np.abs(w).T) + np.abs(bv)
        if relu:
            y = np.maximum(y, 0.0)
        if ln_gamma is not None:   # the GEMM followed by roitr_add_layernorm: rows of N floats, dense
            if ln_res is not None:
                ri = np.arange(mb) if ln_res_idx is None else ln_res_idx[:mb].astype(np.int64)
                y = y + ln_res.astype(np.float64).reshape(-1, nb)[ri]
            mu = y.mean(1, keepdims=True)
            y = (y - mu) / np.sqrt(((y - mu) ** 2).mean(1, keepdims=True) + float(np.float32(ln_eps)))
            y = y * ln_gamma.astype(np.float64) + ln_beta.astype(np.float64)
            if ln_post is not None:
                y = y + ln_post.astype(np.float64).reshape(-1, nb)[:mb]
            if ln_relu:
                y = np.maximum(y, 0.0)
        at = b * sC + np.arange(mb)[:, None] * ldc + np.arange(nb)[None, :]
        assert not written[at].any(), "the batches of the case overlap in C"
        exp[at], mass[at], written[at] = y, ms, True
    return exp, mass, written


def assert_gemm(got, ref, exact, what=""):
    """got: the flat C buffer after the call (float32); ref: gemm_reference's triple."""
    exp, mass, written = ref
    got = np.asarray(got, dtype=np.float64)
    stray = np.flatnonzero(~written & (got != exp))
    assert stray.size == 0, (what, "written outside the result", stray[:8].tolist(), int(stray.size))
    if exact:
        bad = np.flatnonzero(written & (got != exp))
        assert bad.size == 0, (what, "not the exact product", bad[:8].tolist(), int(bad.size), got[bad[:4]].tolist(), exp[bad[:4]].tolist())
    else:
        err = np.abs(got - exp)[written] / (mass[written] + 1e-30)
        worst = float(err.max()) if err.size else 0.0
        assert worst < REL_BOUND, (what, worst)


# ------------------------------------------------------------------------------------------------ a call from host arrays
HOST_ARRAYS = ("A", "A2", "W", "bias", "a_idx", "w_idx", "seg_off", "A_cat", "a_cat_idx", "ln_gamma", "ln_beta", "ln_res", "ln_res_idx", "ln_post")


class Offset:
    """A host array passed by a pointer `skip` elements behind the start of its allocation."""
    def __init__(self, array, skip):
        self.array, self.skip = array, skip


def run_gemm(c_size, expect_form, device=None, reference=True, **fields):
    """Uploads the host arrays of `fields`, fills a C buffer of c_size floats with the sentinel, asserts the form, launches.
    Returns (C as a flat float32 numpy array, gemm_reference of the same fields -- None with reference=False, for a caller that
    has it already).  `device`: uploaded tensors to reuse, by id()."""
    import torch
    device = {} if device is None else device

    def up(v):
        base = v.array if isinstance(v, Offset) else v
        if id(base) not in device:
            device[id(base)] = (torch.from_numpy(np.ascontiguousarray(base).reshape(-1)).cuda(), base)   # the host array is kept alive: its id stays its own
        t = device[id(base)][0]
        return t[v.skip:] if isinstance(v, Offset) else t

    dev = {k: up(v) for k, v in fields.items() if k in HOST_ARRAYS}
    host = {k: v for k, v in fields.items() if k in HOST_ARRAYS}
    scalars = {k: v for k, v in fields.items() if k not in HOST_ARRAYS}
    live = scalars.pop("batch_live", None)
    if live is not None:
        dev["batch_live"] = torch.tensor([live], dtype=torch.int32).cuda()
    out = torch.full((c_size,), SENTINEL, device="cuda")
    call = dict(scalars, C=out, **dev)
    form = gemm_form(**call)
    assert form == expect_form, (form, expect_form)
    _gemm_abi(**call)
    return out.cpu().numpy(), gemm_reference(c_size, **scalars, **host, batch_live=live) if reference else None
