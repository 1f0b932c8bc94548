"""CPU: the float64 restatement of the local-to-global registration (tests/lgr_util.py) on planted sets and hand-built cases, the
fixtures of the GPU tests (every seed is decided), and the header's prototypes."""
import numpy as np
import pytest

import lgr_util as U


@pytest.mark.parametrize("name", sorted(U.SEEDS))
def test_fixture_is_decided_and_recovers_the_planted_set(name):
    src, tgt, w, patch, mask, (R, t) = U.fixture(name)
    r = U.lgr_ref(src, tgt, w, patch)
    assert r["decided"], (name, r["step_near"], r["hyp_near"])
    if name not in U.PLANTED:      # graded noise, up to a third of the radius per axis: there is no planted set to recover exactly,
        c = np.array(r["hyp_counts"])   # these sets are there for counts that differ and a winner away from the front
        assert r["status"] == 0 and len(set(c.tolist())) > 10 and r["best"] == int(np.flatnonzero(c == c.max())[0]) >= 20
        assert (name != "graded_tail" or r["best"] >= 256) and np.abs(r["T"][:3, :3] - R).max() < 5e-3
        return
    assert np.array_equal(r["mask"], mask) and r["inliers"] == int(mask.sum())
    if name == "empty_refit":
        assert r["status"] == U.EMPTY_REFIT and r["best"] == 0 and r["local_inliers"] == 0 and max(r["hyp_counts"]) == 0
        assert np.array_equal(r["T"][:3], r["hyp_T"][0])          # the previous transform is kept
        return
    assert r["status"] == (U.NO_LOCAL if name == "no_local" else 0)
    # the final transform is weighted Procrustes on the planted inliers (fp32 rounding of T: half an ulp of values below 8)
    want = U.procrustes64(src, tgt, w * mask)
    assert np.abs(r["T"][:3] - want).max() <= 2.0 ** -22
    assert np.abs(r["T"][:3, :3] - R).max() < 5e-3 and np.abs(r["T"][:3, 3] - t).max() < 5e-3
    if name == "tie":
        assert r["hyp_counts"][0] == r["hyp_counts"][-1] == max(r["hyp_counts"]) and r["best"] == 0


@pytest.mark.parametrize("name,kw", U.PARAM_CASES)
def test_fixture_is_decided_under_other_parameters(name, kw):
    src, tgt, w, patch, mask, _ = U.fixture(name)
    r = U.lgr_ref(src, tgt, w, patch, **kw)
    assert r["decided"] and r["status"] == 0 and r["hypotheses"] == len(U.runs(patch, kw["min_rows"])) <= len(U.runs(patch))
    assert np.array_equal(r["mask"], mask) and len(r["step_near"]) == kw["steps"] + 1


def test_fixture_without_scores_is_decided():
    src, tgt, _, patch, mask, _ = U.fixture("rows_513")
    r = U.lgr_ref(src, tgt, None, patch)
    assert r["decided"] and np.array_equal(r["mask"], mask)


def test_fixture_shapes_cover_the_kernel_borders():
    for n in (511, 512, 513):
        assert U.fixture(f"rows_{n}")[0].shape[0] == n
    for h in (255, 256, 257):
        assert len(U.runs(U.fixture(f"hyps_{h}")[3])) == h
    lens = sorted(l for _, l in U.runs(U.fixture("mixed_runs")[3], 1))
    assert {1, 2, 3, 4, 63, 64, 65, 300} <= set(lens)
    assert U.runs(U.fixture("no_local")[3]) == []


def test_run_heads():
    patch = np.array([7, 7, 7, 2, 2, 7, 7, 7, 7, -1, -1, -1], np.int32)
    assert U.runs(patch) == [(0, 3), (5, 4), (9, 3)]           # a value that returns after another one starts a new run
    assert U.runs(patch, 4) == [(5, 4)]
    assert U.runs(patch + 100) == U.runs(patch) == U.runs(patch * 5)
    assert U.runs(np.zeros(0, np.int32)) == [] and U.runs(np.array([1, 2, 3], np.int32)) == []


def test_tie_goes_to_the_lower_number():
    src, tgt, w, patch, _, _ = U.fixture("tie")
    r = U.lgr_ref(src, tgt, w, patch)
    assert r["best"] == 0 and r["best_first_row"] == 0 and np.array_equal(r["hyp_T"][0], r["hyp_T"][-1])
    # the same rows with the duplicate in front of everything else: still the first of the two
    order = np.concatenate([np.arange(63, 111), np.arange(63)])
    r2 = U.lgr_ref(src[order], tgt[order], w[order], patch[order])
    assert r2["best"] == 0 and r2["hyp_counts"][0] == r2["hyp_counts"][1]


def test_degenerate_branch_and_empty_pair():
    src, tgt, w, patch, mask, _ = U.fixture("no_local")
    r = U.lgr_ref(src, tgt, w, patch)
    assert r["hypotheses"] == 0 and r["best"] == -1 and r["best_first_row"] == -1 and r["status"] == U.NO_LOCAL
    assert r["local_inliers"] == U.counts(U.solve(src, tgt, w), src, tgt, U.RADIUS)[0] and len(r["step_near"]) == U.STEPS + 1
    e = U.lgr_ref(src[:0], tgt[:0], w[:0], patch[:0])
    assert e["status"] == U.NO_ROWS and np.array_equal(e["T"], np.eye(4)) and e["inliers"] == 0 and e["best"] == -1
    # all scores 0: the first solve has no weight -> identity kept, both bits
    z = U.lgr_ref(src, tgt, np.zeros_like(w), patch)
    assert z["status"] == U.NO_LOCAL | U.EMPTY_REFIT and np.array_equal(z["T"], np.eye(4))


def test_empty_refit_keeps_the_previous_transform():
    src, tgt, w, patch, _, _ = U.fixture("mixed_runs")
    # a shift of the row's own breaks every patch: no row fits any hypothesis at a small radius, so every count is 0, hypothesis 0
    # wins, the first global solve has no weight and the winner's transform stays
    shift = (50.0 * (np.arange(len(w)) % 7))[:, None].astype(np.float32)
    far = U.lgr_ref(src, tgt + shift, w, patch, radius=1e-3)
    assert max(far["hyp_counts"]) == 0 and far["best"] == 0 and far["status"] == U.EMPTY_REFIT and far["inliers"] == 0
    assert np.array_equal(far["T"][:3], far["hyp_T"][0]) and len(far["step_near"]) == 2   # the loop ended at its first solve


def test_header_prototypes_and_workspace_size():
    import ctypes
    from roitr_amd import _lib
    protos = _lib.header_prototypes()
    assert protos["roitr_lgr_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
    res, args = protos["roitr_lgr_batch"]
    assert res is ctypes.c_int and len(args) == 24 and args[7] is ctypes.c_float and args[11] is ctypes.c_size_t
    assert "roitr_lgr_batch" not in _lib.BOUND
    lib = ctypes.CDLL(_lib.LIB_PATH)     # host-only: no device is touched
    f = lib.roitr_lgr_workspace_bytes
    f.restype, f.argtypes = protos["roitr_lgr_workspace_bytes"]
    assert f(0, 100) == 0 and f(1, -1) == 0
    sizes = [f(1, n) for n in (0, 1, 2, 3, 511, 512, 513, 10000, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert f(1, 5000) <= f(2, 5000) <= f(512, 5000)
