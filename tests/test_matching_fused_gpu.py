"""GPU: roitr_matching_tail (the transport kernels set the fine-matching flags of their patch) against the two calls it replaces,
roitr_optimal_transport followed by roitr_fine_matching, on the same inputs: every output buffer must hold the same BYTES --
the transport tiles, flags, counts, offsets, the emitted correspondences (points, scores, patch numbers), the total and the
per-pair starts.  Buffers start from the same sentinels on both sides, so what a kernel must not write is compared too.

Both sides run the same selection (patch_flags in matching.hip: roitr_fine_matching's flag kernel calls it on the tile it reads back),
so this file proves the epilogue inside the transport kernels -- tile from the stored values, masks from registers, dead slots --
and not the selection itself: that is pinned to a float64 restatement in tests/test_matching_tail_gpu.py.

Patches: random scores with masked rows and columns, a patch with every row and one with every column masked, one with all of
both masked, a patch whose score spread sends it to the log-domain kernel (roitr_ot_stats confirms it went there), constant
scores and scores on a coarse grid (ties in every row and column: the lower index wins), k = 1 / 2 / 3 / 4 / 5 (registers and wave
maxima) and k = 0 (nothing selected) with and without `mutual`, a confidence threshold of 0 and one that cuts.  Layouts: one pair, strided with dead slots,
compacted with dead slots past the live count.  The score matrices are generated here; the score product itself is not part of
the fused launch.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OTN = 65


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _inputs(seed):
    """12 patches: (scores, row masks, col masks, row points, col points)."""
    rng = np.random.default_rng(seed)
    P = 12
    sc = rng.standard_normal((P, 64, 64)).astype(np.float32)
    rm = rng.random((P, 64)) > 0.2
    cm = rng.random((P, 64)) > 0.2
    rm[1] = True; cm[1] = True                       # nothing masked
    rm[2] = False                                    # every row masked
    cm[3] = False                                    # every column masked
    rm[4] = False; cm[4] = False                     # all masked
    sc[5] = (40.0 * rng.standard_normal((64, 64))).astype(np.float32)   # spread far above OT_FAST_SPREAD: log-domain kernel
    sc[6] = 0.25                                     # all equal
    sc[7] = np.round(sc[7] * 2.0) / 2.0              # coarse grid: many exact ties
    sc[8] = np.round(sc[8])
    rm[8] = True; cm[8] = True
    sc[9, 10] = sc[9, 20]                            # duplicate rows and columns
    sc[9, :, 33] = sc[9, :, 5]
    sc[10] *= 5.0
    rp = rng.standard_normal((P, 64, 3)).astype(np.float32)
    cp = rng.standard_normal((P, 64, 3)).astype(np.float32)
    return sc, rm, cm, rp, cp


LAYOUTS = {
    # name: (pairs, num_corr, n_corr, pair_off, slots)
    "one_pair": (1, 12, [12], None, 0),
    "strided": (3, 4, [4, 2, 0], None, 0),
    "compacted": (3, 4, [3, 1, 2], [0, 3, 4, 6], 9),
}


def _run(fused, inp, layout, k, mutual, conf, alpha, with_stats=False):
    from roitr_amd import _lib as L, ops
    sc, rm, cm, rp, cp = inp
    pairs, num_corr, n_corr, pair_off, slots = LAYOUTS[layout]
    P = slots if pair_off is not None else pairs * num_corr
    i32 = lambda a: _dev(np.asarray(a, dtype=np.int32))
    t_sc, t_rm, t_cm, t_rp, t_cp = _dev(sc[:P]), i32(rm[:P]), i32(cm[:P]), _dev(rp[:P]), _dev(cp[:P])
    t_nc = i32(n_corr)
    t_po = i32(pair_off) if pair_off is not None else None
    t_al = torch.tensor([alpha], dtype=torch.float32, device="cuda")
    t_gs = _dev((0.5 + np.arange(pairs * num_corr) / 16.0).astype(np.float32))
    room = P * 64 * 64 + 8
    out = torch.full((P, OTN, OTN), float("nan"), dtype=torch.float32, device="cuda")
    flags = torch.full((P * 64 * 64,), 7, dtype=torch.uint8, device="cuda")
    counts = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    offs = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    n_out = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    o_r = torch.full((room, 3), float("nan"), device="cuda")
    o_c = torch.full((room, 3), float("nan"), device="cuda")
    o_s = torch.full((room,), float("nan"), device="cuda")
    o_p = torch.full((room,), -7, dtype=torch.int32, device="cuda")
    ps = torch.full((pairs + 1,), -7, dtype=torch.int32, device="cuda")
    o = ops._OT(pairs, num_corr, 64, 100, L.ptr(t_nc), L.ptr(t_sc), L.ptr(t_rm), L.ptr(t_cm), L.ptr(t_al), L.ptr(out), L.ptr(t_po),
                int(slots))
    f = ops._Fine(pairs, num_corr, 64, int(k), int(mutual), float(conf), L.ptr(t_nc), L.ptr(out), L.ptr(t_rm), L.ptr(t_cm), L.ptr(t_rp),
                  L.ptr(t_cp), L.ptr(t_gs), L.ptr(flags), L.ptr(counts), L.ptr(offs), L.ptr(n_out), L.ptr(o_r), L.ptr(o_c), L.ptr(o_s),
                  L.ptr(o_p), int(P * 64 * 64), L.ptr(t_po), int(slots), L.ptr(ps))
    stats = (ctypes.c_ulonglong * 3)()
    if with_stats:
        L.check(L.lib().roitr_ot_stats(ctypes.c_int(1), None), "ot_stats")
    if fused:
        L.check(L.lib().roitr_matching_tail(ctypes.byref(o), ctypes.byref(f), L.stream_ptr()), "matching_tail")
    else:
        L.check(L.lib().roitr_optimal_transport(ctypes.byref(o), L.stream_ptr()), "optimal_transport")
        L.check(L.lib().roitr_fine_matching(ctypes.byref(f), L.stream_ptr()), "fine_matching")
    torch.cuda.synchronize()
    if with_stats:
        L.check(L.lib().roitr_ot_stats(ctypes.c_int(0), stats), "ot_stats")
    res = dict(ot=out, flags=flags, counts=counts, offsets=offs, n_out=n_out, row=o_r, col=o_c, score=o_s, patch=o_p, pair_starts=ps)
    return {n: t.cpu().numpy() for n, t in res.items()}, [int(x) for x in stats]


def _same_bytes(a, b, what):
    for name in a:
        x, y = a[name], b[name]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name)
        if x.tobytes() != y.tobytes():
            bad = np.flatnonzero(x.reshape(-1).view(np.uint8 if x.itemsize == 1 else np.uint32)
                                 != y.reshape(-1).view(np.uint8 if y.itemsize == 1 else np.uint32))
            raise AssertionError(f"{what}: {name} differs at {len(bad)} entries, first flat index {int(bad[0])}")


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("mutual", [True, False])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_fused_tail_is_bitwise_the_two_calls(k, mutual, layout):
    inp = _inputs(1234 + k)
    total = 0
    for conf in (0.0, 0.004):
        for alpha in (1.0, -0.5):
            old, _ = _run(False, inp, layout, k, mutual, conf, alpha)
            new, _ = _run(True, inp, layout, k, mutual, conf, alpha)
            _same_bytes(old, new, f"k={k} mutual={mutual} {layout} conf={conf} alpha={alpha}")
            assert old["n_out"][0] >= 0
            total += int(old["n_out"][0])
    assert total > 0   # the comparison is not of empty lists


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_fused_tail_with_k_zero_emits_nothing_like_the_two_calls(layout):
    """k = 0 selects nothing: both forms leave the same bytes (transport tiles, zero flags and counts of the live patches, sentinels
    elsewhere), an empty list and pair starts of 0."""
    inp = _inputs(77)
    for mutual in (True, False):
        old, _ = _run(False, inp, layout, 0, mutual, 0.0, 1.0)
        new, _ = _run(True, inp, layout, 0, mutual, 0.0, 1.0)
        _same_bytes(old, new, f"k=0 mutual={mutual} {layout}")
        for r in (old, new):
            assert r["n_out"][0] == 0 and not r["pair_starts"].any()
            assert (r["counts"] == 0).all() and not (r["flags"] == 1).any()
            assert np.isnan(r["score"]).all() and (r["patch"] == -7).all()   # nothing emitted


def test_fused_tail_serves_the_log_domain_patch_and_keeps_the_counters():
    """Patch 5 goes to ot_log_kernel in both forms (its flags then come from that kernel's epilogue); the roitr_ot_stats counters
    read the same either way."""
    inp = _inputs(99)
    old, s_old = _run(False, inp, "one_pair", 3, True, 0.0, 1.0, with_stats=True)
    new, s_new = _run(True, inp, "one_pair", 3, True, 0.0, 1.0, with_stats=True)
    _same_bytes(old, new, "stats run")
    assert s_old == s_new
    assert s_new[0] >= 1 and s_new[2] >= 1
    assert new["counts"][5] > 0   # the log-domain patch produced flags


def test_fused_tail_rejects_structs_of_different_patch_lists():
    from roitr_amd import _lib as L, ops
    z = torch.zeros(4, dtype=torch.int32, device="cuda")
    o = ops._OT(1, 1, 64, 100, L.ptr(z), L.ptr(None), L.ptr(z), L.ptr(z), L.ptr(None), L.ptr(None), L.ptr(None), 0)
    f = ops._Fine(1, 2, 64, 3, 1, 0.05, L.ptr(z), L.ptr(None), L.ptr(z), L.ptr(z), L.ptr(None), L.ptr(None), L.ptr(None), L.ptr(None),
                  L.ptr(None), L.ptr(None), L.ptr(None), L.ptr(None), L.ptr(None), L.ptr(None), L.ptr(None), 0, L.ptr(None), 0, L.ptr(None))
    assert L.lib().roitr_matching_tail(ctypes.byref(o), ctypes.byref(f), L.stream_ptr()) != 0
