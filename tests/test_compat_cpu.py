"""CPU: the float64 restatement of the spatial-compatibility registration (tests/compat_util.py) on planted sets and hand-built cases,
the fixtures of the GPU tests (every one is decided and inside the well-posedness cap), and the header's prototypes."""
import numpy as np
import pytest

import compat_util as U
import lgr_util as LU


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_fixture_is_decided_and_within_the_cap(name):
    (src, tgt, w, mask, pose), kw = U.fixture(name)
    r = U.reference(name)
    assert U.decided(r, w, kw.get("max_rows"), ties=name.startswith("lattice")), (name, r["margin"], r["step_near"], r["hyp_near"])
    assert U.within_cap(r), (name, U.excluded(r), r["hypotheses"])
    assert r["margin"] >= 1e-9
    if name in U.PLANTED:
        R, t = pose
        assert r["status"] == (U.TRUNCATED if name.startswith("trunc_") else 0), name
        assert np.array_equal(r["mask"], mask) and r["inliers"] == int(mask.sum()), name
        assert np.abs(r["T"][:3, :3] - R).max() < 5e-3 and np.abs(r["T"][:3, 3] - t).max() < 1e-2, name


@pytest.mark.parametrize("name", ["ratio_30", "ratio_10", "ratio_05"])
def test_planted_pose_is_recovered(name):
    (src, tgt, w, mask, (R, t)), _ = U.fixture(name)
    r = U.reference(name)
    assert r["best"] >= 0 and mask[r["best_seed_row"]] and r["local_inliers"] >= 0.9 * mask.sum()
    rre = np.degrees(np.arccos(np.clip((np.trace(r["T"][:3, :3].T @ R) - 1) / 2, -1, 1)))
    assert rre < 0.5 and np.linalg.norm(r["T"][:3, 3] - t) < 0.02
    # the final transform is weighted Procrustes on the planted inliers
    assert np.abs(r["T"][:3] - LU.procrustes64(src, tgt, w * mask)).max() <= 2.0 ** -21


@pytest.mark.parametrize("name", ["lattice", "lattice_k5"])
def test_ties_go_to_the_lower_index(name):
    (src, tgt, w, mask, _), kw = U.fixture(name)
    r = U.reference(name)
    deg, seeds, k = r["deg"], r["seeds"], kw.get("k", U.K)
    # many exact zeros: the planted rows are pairwise compatible, so their degrees tie in large groups
    assert (r["C"][np.ix_(mask, mask)].sum(1) == mask.sum() - 1).all()
    vals, counts = np.unique(deg[seeds], return_counts=True)
    assert counts.max() >= 4
    for i in range(len(seeds) - 1):      # rank order: degree descending, index ascending inside a tie
        a, b = seeds[i], seeds[i + 1]
        assert deg[a] > deg[b] or (deg[a] == deg[b] and a < b)
    left = np.setdiff1d(np.arange(len(deg)), seeds)
    last = seeds[-1]
    assert all(deg[a] < deg[last] or (deg[a] == deg[last] and a > last) for a in left)
    cut = 0
    for i, s in enumerate(seeds):        # members: c descending, index ascending inside a tie at the cut
        if r["hyp_counts"][i] < 0:
            continue
        c = r["c"][i]
        mem = np.array([a for a in r["members"][i] if a != r["sel"][s]])
        out = np.setdiff1d(np.flatnonzero(c > 0), mem)
        assert len(mem) == min(k - 1, int((c > 0).sum())) and (c[mem] > 0).all()
        if len(out):
            low = c[mem].min()
            assert c[out].max() <= low
            tied_out, tied_in = out[c[out] == low], mem[c[mem] == low]
            if len(tied_out):
                cut += 1
                assert tied_in.max() < tied_out.min()
    assert cut > 0                       # the tie at the cut does occur on this fixture


def test_truncation_rule():
    n, M = 20, 8
    rng = np.random.default_rng(0)
    w = rng.permutation(n).astype(np.float32)
    assert U.select(n, w, M).tolist() == sorted(np.argsort(-w)[:M].tolist())
    assert U.select(n, None, M).tolist() == list(range(M)) and U.select(5, w[:5], M).tolist() == list(range(5))
    w = np.array([1, 3, 2, 2, 2, 3, 2, 0], np.float32)      # two 3s, then the first 2s in row order
    assert U.select(8, w, 4).tolist() == [1, 2, 3, 5] and U.select(8, w, 3).tolist() == [1, 2, 5]
    assert U.select(8, np.ones(8, np.float32), 5).tolist() == [0, 1, 2, 3, 4]
    (src, tgt, s, mask, _), kw = U.fixture("trunc_2049")
    r = U.reference("trunc_2049")
    assert len(r["sel"]) == 2048 and np.setdiff1d(np.arange(2049), r["sel"]).tolist() == [int(np.argmin(s))] and r["status"] & U.TRUNCATED
    tie = U.compat_ref(src[:300], tgt[:300], np.ones(300, np.float32), max_rows=200)
    assert tie["sel"].tolist() == list(range(200)) and tie["status"] & U.TRUNCATED


def test_common_neighbours_equal_a_triple_loop():
    (src, tgt, w, _, _), _ = U.fixture("m_63")
    C, _ = U.graph(src[:12], tgt[:12], 0.5)
    seeds = np.array([3, 0, 11, 7])
    c = U.common_neighbours(C, seeds)
    for i, s in enumerate(seeds):
        for b in range(12):
            want = sum(int(C[s, x]) * int(C[b, x]) for x in range(12)) * int(C[s, b])
            assert c[i, b] == want
    assert C.any() and not C.all() and not C.diagonal().any() and np.array_equal(C, C.T)


def test_graph_rows_equal_the_full_graph():
    (src, tgt, _, _, _), _ = U.fixture("m_257")
    C, margin = U.graph(src, tgt, U.COMPAT_DIST)
    rows = [0, 5, 128, 129, 256]
    Cr, mr = U.graph_rows(src, tgt, rows, U.COMPAT_DIST, chunk=2)
    assert np.array_equal(Cr, C[rows]) and mr >= margin


def test_degenerate_branch_empty_pair_and_two_rows():
    (src, tgt, w, _, _), _ = U.fixture("incompatible")
    r = U.reference("incompatible")
    assert not r["C"].any() and r["hypotheses"] == 0 and r["best"] == -1 and r["best_seed_row"] == -1
    assert r["status"] & U.NO_HYPOTHESIS and all(c == -1 for c in r["hyp_counts"]) and len(r["hyp_counts"]) == 12
    assert all(len(x) == 1 for x in r["members"]) and LU.well_posed(src, tgt, w)
    assert r["local_inliers"] == LU.counts(LU.solve(src, tgt, w), src, tgt, U.RADIUS)[0]
    e = U.compat_ref(src[:0], tgt[:0], w[:0])
    assert e["status"] == U.NO_ROWS and np.array_equal(e["T"], np.eye(4)) and e["inliers"] == 0 and e["best"] == -1
    two = U.reference("two_rows")
    assert two["status"] & U.NO_HYPOTHESIS and two["hypotheses"] == 0 and len(two["seeds"]) == 2 and two["deg"].tolist() == [1, 1]
    z = U.compat_ref(src, tgt, np.zeros_like(w))
    assert z["status"] == U.NO_HYPOTHESIS | U.EMPTY_REFIT and np.array_equal(z["T"], np.eye(4))


def test_fixture_shapes_cover_the_kernel_borders():
    for m in (3, 4, 63, 64, 65, 127, 128, 129, 257, 1000):
        assert len(U.reference(f"m_{m}")["sel"]) == m
    assert U.fixture("trunc_2049")[0][0].shape[0] == 2049
    over = U.reference("k_over")
    assert 3 <= max(len(x) for x in over["members"]) < 64
    assert len(U.reference("seeds_over")["seeds"]) == 100 and len(U.reference("seeds_1")["seeds"]) == 1
    assert len(U.reference("seeds_1024")["seeds"]) == 1024 and max(len(x) for x in U.reference("k_64")["members"]) == 64


def test_header_prototypes_and_workspace_size():
    import ctypes
    from roitr_amd import _lib
    protos = _lib.header_prototypes()
    assert protos["roitr_compat_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    res, args = protos["roitr_compat_batch"]
    assert res is ctypes.c_int and len(args) == 28 and args[6] is ctypes.c_float and args[7] is ctypes.c_float
    assert args[8] is ctypes.c_int and args[13] is ctypes.c_size_t
    assert "roitr_compat_batch" not in _lib.BOUND and len(_lib.BOUND) == 35
    lib = ctypes.CDLL(_lib.LIB_PATH)     # host-only: no device is touched
    f = lib.roitr_compat_workspace_bytes
    f.restype, f.argtypes = protos["roitr_compat_workspace_bytes"]
    assert f(0, 100, 64, 8, 20) == 0 and f(1, -1, 64, 8, 20) == 0
    assert f(1, 100, 8193, 8, 20) == 0 and f(1, 100, 2, 8, 20) == 0 and f(1, 100, 64, 1025, 20) == 0 and f(1, 100, 64, 8, 65) == 0
    sizes = [f(1, 10000, m, 64, 20) for m in (3, 63, 64, 65, 1000, 2048, 8192)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0] > 0
    # the bit matrix dominates: 8192 rows x 128 words x 8 bytes = 8 MiB per pair
    assert sizes[-1] >= 8192 * 128 * 8
    assert f(1, 5000, 1024, 64, 20) <= f(2, 5000, 1024, 64, 20) <= f(512, 5000, 1024, 64, 20)
    assert f(4, 5000, 1024, 1, 20) <= f(4, 5000, 1024, 64, 20) <= f(4, 5000, 1024, 1024, 20)
    assert f(4, 0, 1024, 64, 3) <= f(4, 5000, 1024, 64, 64)
