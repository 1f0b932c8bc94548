"""CPU: roitr_local_weights_reorder_host, the index permutation behind the fragment-ordered weight copies of csrc/local_block.hip,
against its definition (include/roitr_engine.h): for every 32-row region and every 32-k slab one block of four groups (c, n) =
(0,0), (0,1), (1,0), (1,1) of 64 float4; entry 16 g + i of a group holds W[32 region + 16 n + i][32 slab + 16 c + 4 g .. + 3]."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _fragment_order(W):
    """The definition as one numpy transpose: out[region, slab, c, n, g, i, e] = W[32 region + 16 n + i, 32 slab + 16 c + 4 g + e]."""
    rows, k = W.shape
    t = W.reshape(rows // 32, 2, 16, k // 32, 2, 4, 4)          # region, n, i, slab, c, g, e
    return np.ascontiguousarray(t.transpose(0, 3, 4, 1, 5, 2, 6)).reshape(-1)


def _weight(rows, k, ldw):
    """(rows, k) host view with row stride ldw over distinct values (every element identifies its place)."""
    full = torch.arange(rows * ldw, dtype=torch.float32).reshape(rows, ldw)
    off = ldw - k                                                # the view starts inside the row, like wcat's second K half
    return full[:, off:off + k]


@pytest.mark.parametrize("rows,k,ldw", [(64, 64, 64), (64, 128, 128), (128, 64, 64), (128, 256, 256), (128, 64, 192), (64, 64, 128)])
def test_reorder_host_is_the_stated_permutation(rows, k, ldw):
    from roitr_amd import ops
    w = _weight(rows, k, ldw)
    assert w.stride(0) == ldw and w.shape == (rows, k)
    got = ops.local_weights_reorder_host(w).numpy()
    want = _fragment_order(w.numpy())
    assert got.shape == want.shape == (rows * k,)
    assert np.array_equal(got, want)
    # every source element exactly once (the values are distinct)
    assert np.array_equal(np.sort(got), np.sort(w.numpy().reshape(-1)))
    # the address expression of gemm_phase, spelled out for a few lanes: float4 (((region * nslab + slab) * 4 + q) * 64 + lane)
    nslab = k // 32
    for region, slab, q, lane in ((0, 0, 0, 0), (rows // 32 - 1, nslab - 1, 3, 63), (1, nslab - 1, 2, 37), (0, 1 % nslab, 1, 16)):
        c, n, i, g = q >> 1, q & 1, lane & 15, lane >> 4
        d = ((region * nslab + slab) * 4 + q) * 64 + lane
        src = w[32 * region + 16 * n + i, 32 * slab + 16 * c + 4 * g:32 * slab + 16 * c + 4 * g + 4].numpy()
        assert np.array_equal(got[4 * d:4 * d + 4], src), (region, slab, q, lane)


@pytest.mark.parametrize("rows,k", [(48, 64), (64, 40), (0, 64), (64, 0)])
def test_reorder_host_rejects_shapes_that_are_not_whole_blocks(rows, k):
    import ctypes
    from roitr_amd import _lib
    lib = _lib.lib()
    src = torch.zeros(max(rows, 1) * max(k, 1) + 64)
    dst = torch.full((max(rows, 1) * max(k, 1) + 64,), -1.0)
    status = lib.roitr_local_weights_reorder_host(ctypes.c_void_p(src.data_ptr()), rows, k, max(k, 4), ctypes.c_void_p(dst.data_ptr()))
    assert status == 1                                           # ROITR_ERR_ARG
    assert bool((dst == -1.0).all())                             # nothing written


def test_reorder_host_rejects_a_leading_dimension_below_k():
    import ctypes
    from roitr_amd import _lib
    lib = _lib.lib()
    src, dst = torch.zeros(64 * 64), torch.full((64 * 64,), -1.0)
    assert lib.roitr_local_weights_reorder_host(ctypes.c_void_p(src.data_ptr()), 64, 64, 32, ctypes.c_void_p(dst.data_ptr())) == 1
    assert bool((dst == -1.0).all())


def test_abi_version_is_unchanged():
    from roitr_amd import _lib
    assert _lib.lib().roitr_abi_version() == 4                   # functions added, no struct changed
