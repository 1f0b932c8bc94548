"""CPU: the float64 restatement of the FPFH operator (tests/fpfh_util.py) against closed forms, the fixtures of the GPU tests (every
one is decided), the header's prototypes and the new options of the command line."""
import numpy as np
import pytest

import fpfh_util as U


@pytest.mark.parametrize("name", U.DECIDED)
def test_fixture_is_decided(name):
    r = U.reference(name)
    assert U.is_decided(name), (name, r["radius_margin"], r["swap_margin"], r["bins_stable"])
    f = U.fixture(name)
    assert r["m"].max() <= f["max_nn"] - 1 and (r["counts"].reshape(-1, 3, 11).sum(2) == r["m"][:, None]).all()


def test_fixtures_reach_every_path():
    m = lambda name: U.reference(name)["m"]
    assert (m("nn2") == 1).all()
    assert m("nn16_cut").max() < 15 and m("nn16_cut").min() == 0                 # the radius cuts every row, some to nothing
    assert (m("nn16_full") == 15).all()                                          # the radius cuts none
    assert m("nn65").max() == 64 and m("nn65").min() < 64                        # both, with slots in the second lane round
    assert m("nn100").max() == 99 and m("nn100").min() < 99
    sizes = np.diff(np.concatenate([[0], U.fixture("sizes16")["offset"]])).tolist()
    assert sizes == [1, 2, 15, 0, 16, 17, 300]                                   # 1, 2, max_nn - 1, empty, max_nn, max_nn + 1
    assert m("sizes16")[0] == 0 and m("sizes16")[1:3].tolist() == [1, 1] and m("sizes16")[3:18].max() == 14
    assert np.diff(np.concatenate([[0], U.fixture("sizes100")["offset"]])).tolist() == [99, 0, 100, 101, 1]
    # the end-to-end cloud: the radius cuts every row, so K(i) does not depend on the order of the kNN row
    assert m("e2e").max() < 99 and m("e2e").min() > 0
    g = U.moved(U.fixture("e2e"))
    moved = U.fpfh_ref(**g)
    assert U.is_decided(g) and np.array_equal(moved["counts"], U.reference("e2e")["counts"])
    # the restatement's descriptors match the copy to the original: numpy argmin is the identity for nearly every point
    a, b = U.reference("e2e")["fpfh"], moved["fpfh"]
    d = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T
    assert (d.argmin(1) == np.arange(len(a))).mean() > 0.95 and (d.argmin(0) == np.arange(len(a))).mean() > 0.95


def test_planar_lattice_is_200_in_three_bins():
    f = U.lattice()
    r = U.fpfh_ref(**f)
    has = r["m"] > 0
    assert has[:-3].all() and not has[-3:].any() and r["m"].max() == 15   # 20 lattice points within the radius inside: the row caps them
    want = np.zeros(33)
    want[[5, 16, 27]] = 200.0
    assert np.abs(r["fpfh"][has] - want).max() < 1e-9 and np.array_equal(r["fpfh"][has].astype(np.float32), np.tile(want, (has.sum(), 1)).astype(np.float32))
    assert not r["fpfh"][~has].any() and not r["counts"][~has].any()
    assert (r["counts"][has][:, [5, 16, 27]] == r["m"][has][:, None]).all()


def two_points(p, q, n_p, n_q, radius=1.0):
    return U.fpfh_ref(np.array([p, q], np.float32), np.array([n_p, n_q], np.float32), np.array([2], np.int32), radius, 2)


def test_two_points_by_hand():
    # p = 0 with normal z, q = (0.5, 0, 0) with normal (0.6, 0, 0.8): from p, a1 = 0, a2 = 0.6 -> swap: n1 = n_q, n2 = n_p, dp = -x,
    # f2 = -0.6; v = dp x n1 = (-1, 0, 0) x (0.6, 0, 0.8) = (0, 0.8, 0) -> y; w = n1 x v = (-0.8, 0, 0.6); f1 = v . n2 = 0;
    # f0 = atan2(w . n2, n1 . n2) = atan2(0.6, 0.8)
    r = two_points([0, 0, 0], [0.5, 0, 0], [0, 0, 1], [0.6, 0, 0.8])
    f0 = np.arctan2(0.6, 0.8)
    bins = [int(np.floor(11 * (f0 + np.pi) / (2 * np.pi))), 11 + 5, 22 + int(np.floor(11 * 0.4 / 2))]
    assert bins == [6, 16, 24]
    for i in range(2):     # the pair feature is symmetric in (i, j): the swap rule picks the same source point from either side
        assert r["m"][i] == 1 and np.flatnonzero(r["counts"][i]).tolist() == bins
        want = np.zeros(33)
        want[bins] = 200.0   # SPFH = 100 per group; the blend normalises the one neighbour's row to 100 per group as well
        assert np.abs(r["fpfh"][i] - want).max() < 1e-9
    far = two_points([0, 0, 0], [0.5, 0, 0], [0, 0, 1], [0.6, 0, 0.8], radius=0.5)     # strict: d2 == r^2 is outside
    assert not far["m"].any() and not far["fpfh"].any()


def test_duplicate_counts_in_the_middle_bins_and_is_skipped_in_the_blend():
    xyz = np.array([[0, 0, 0], [0, 0, 0], [0.25, 0, 0]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0, 0.8]], np.float32)
    r = U.fpfh_ref(xyz, nrm, np.array([3], np.int32), 1.0, 3)
    assert r["m"].tolist() == [2, 2, 2]
    for i in (0, 1):       # the twin has d = 0: f = (0, 0, 0) -> bins 5, 16, 27
        assert r["counts"][i][[5, 16, 27]].min() >= 1
    # point 0 blends over point 2 alone (the twin has d2 = 0): F = SPFH_2 / d2 normalised to 100 per group, plus its own SPFH
    spfh = r["spfh"]
    want = spfh[2] * 100.0 / np.repeat(spfh[2].reshape(3, 11).sum(1), 11) + spfh[0]
    assert np.abs(r["fpfh"][0] - want).max() < 1e-9
    alone = U.fpfh_ref(xyz[:2], nrm[:2], np.array([2], np.int32), 1.0, 2)      # nothing to blend: F = SPFH
    assert np.array_equal(alone["fpfh"], alone["spfh"]) and np.flatnonzero(alone["fpfh"][0]).tolist() == [5, 16, 27]
    assert alone["fpfh"][0][5] == 100.0


def test_normal_parallel_to_the_offset_takes_the_zero_branch():
    # both normals along dp: |a1| = |a2| = 1, no swap, v = dp x n1 = 0 -> f = (0, 0, 0), f2 included
    r = two_points([0, 0, 0], [0.5, 0, 0], [1, 0, 0], [1, 0, 0])
    assert np.flatnonzero(r["counts"][0]).tolist() == [5, 16, 27] and np.flatnonzero(r["counts"][1]).tolist() == [5, 16, 27]
    f, x, _ = U.pair_features(np.array([1.0, 0, 0]), np.array([1.0, 0, 0]), np.array([0.5, 0, 0]), np.array(0.25))
    assert not f.any() and np.abs(x - 5.5).max() < 1e-12
    # zero normals: a1 = a2 = 0, v = 0 as well
    z = two_points([0, 0, 0], [0.5, 0, 0], [0, 0, 0], [0, 0, 0])
    assert np.flatnonzero(z["counts"][0]).tolist() == [5, 16, 27]


@pytest.mark.parametrize("name", ["nn16_cut", "nn65", "nn100", "dups", "ragged"])
def test_every_group_sums_to_200(name):
    r = U.reference(name)
    idx, keep, m = r["idx"], r["keep"], r["m"]
    mj = np.where(keep, m[idx], 0)
    # S != 0 for a group iff a kept neighbour at d2 > 0 has neighbours of its own
    xyz = U.fixture(name)["xyz"].astype(np.float64)
    d2 = ((xyz[idx] - xyz[:, None]) ** 2).sum(2)
    blended = (keep & (d2 > 0) & (mj > 0)).any(1)
    sums = r["fpfh"].reshape(-1, 3, 11).sum(2)
    assert blended.sum() > 100 and np.abs(sums[blended] - 200.0).max() < 1e-9
    rest = ~blended & (m > 0)
    assert np.abs(sums[rest] - 100.0).max(initial=0.0) < 1e-9 and not r["fpfh"][m == 0].any()
    assert r["fpfh"].min() >= 0.0 and r["fpfh"].max() <= 200.0 + 1e-9


def test_header_prototypes_and_workspace_size():
    import ctypes
    from roitr_amd import _lib
    I, D, P, SZ = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    protos = _lib.header_prototypes()
    assert protos["roitr_fpfh_workspace_bytes"] == (SZ, [I, I, I])
    assert protos["roitr_fpfh_batch"] == (I, [I, I, P, P, P, D, I, I, P, P, P, P, P, SZ, P])
    assert "roitr_fpfh_batch" not in _lib.BOUND and len(_lib.BOUND) == 35
    lib = ctypes.CDLL(_lib.LIB_PATH)     # host-only: no device is touched
    assert hasattr(lib, "roitr_fpfh_batch")
    f = lib.roitr_fpfh_workspace_bytes
    f.restype, f.argtypes = protos["roitr_fpfh_workspace_bytes"]
    assert f(0, 100, 16) == 0 and f(1, -1, 16) == 0 and f(1, 100, 1) == 0 and f(1, 100, 101) == 0
    sizes = [f(1, n, 100) for n in (0, 1, 1000, 5000, 100000)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] >= 100000 * (100 * 4 + 36 + 12)
    assert f(1, 5000, 2) < f(1, 5000, 100) and f(1, 5000, 100) <= f(64, 5000, 100)
    assert lib.roitr_abi_version() == 4


def test_main_parser_accepts_the_new_options():
    from roitr_amd.main import parser
    a = parser().parse_args(["c.yaml", "--evaluate", "--register", "--estimator", "compat", "--fpfh-baseline", "--fpfh-radius", "0.2",
                             "--fpfh-max-nn", "64"])
    assert (a.fpfh_baseline, a.fpfh_radius, a.fpfh_max_nn, a.estimator) == (True, 0.2, 64, "compat")
    d = parser().parse_args(["c.yaml"])
    assert (d.fpfh_baseline, d.fpfh_radius, d.fpfh_max_nn, d.estimator) == (False, 0.125, 100, "ransac")
