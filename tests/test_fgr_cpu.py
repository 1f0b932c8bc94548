"""CPU: the float64 restatement of fast global registration (tests/fgr_util.py) on the project's seeded sets, the fixtures of the GPU
tests (every one is well posed), the header's prototypes, the refusals, the command line and the Tester.

Measured with the restatement on compat_util.make_set (3 m box, 5 mm noise), unit scores, max_dist 0.1, division 1.4, a decrease every
4 iterations, 128 iterations:
  seed 5, n 400, 30 % planted:  RRE 0.0019 deg, RTE 0.0009 m        seed 6, n 600, 10 %:  RRE 0.095 deg, RTE 0.0011 m
  seed 3, n 1000, 10 %:         RRE 0.017 deg,  RTE 0.0016 m        seed 7, n 800, 5 %:   RRE 143.6 deg, RTE 0.26 m (fails)
  seed 7 with the tuple test under the project's stream (key 0, seed 0), drawn / accepted / RRE:
    4 096 / 1 / 0.35    16 384 / 9 / 0.15    32 768 / 21 / 0.15    65 536 / 39 / 160.6 (fails)    98 304 / 58 / 128.8 (fails)
    131 072 / 84 / 0.064    262 144 / 153 / 0.059
  The success is not monotone in the count: with few accepted triples they are all planted, and one accepted outlier triple among 39
  rows-times-three is enough to lose the pose.  The count the tests and the benchmark use is the first of 65 536, 131 072, ... at
  which the pose is recovered: 131 072.
"""
import ctypes

import numpy as np
import pytest

import compat_util as CU
import fgr_util as U

SUCCESS_RRE, SUCCESS_RTE = 15.0, 0.3   # tester.SUCCESS_RRE / SUCCESS_RTE


def recovered(r, pose):
    rre, rte = U.pose_errors(r["T"], pose)
    return rre < 0.5 and rte < 0.02


@pytest.mark.parametrize("seed,n,ratio", [(5, 400, 0.30), (6, 600, 0.10), (3, 1000, 0.10)])
def test_planted_pose_is_recovered_without_the_tuple_test(seed, n, ratio):
    src, tgt, _, mask, pose = CU.make_set(seed, n, ratio)
    r = U.fgr_ref(src, tgt, None)
    assert recovered(r, pose), U.pose_errors(r["T"], pose)
    assert r["status"] == 0 and r["steps"] == 128 and r["n_used"] == n and r["inliers"] == int(mask.sum())
    assert r["mu"] == float(np.float32(0.1)) ** 2 and r["trace"][0, 12] > r["mu"] and (r["trace"][:, 15] == 1.0).all()
    assert np.array_equal(r["trace"][0, :12].reshape(3, 4), np.eye(3, 4))


def test_five_percent_needs_the_tuple_test_and_the_count_is_found_here():
    src, tgt, _, mask, pose = CU.make_set(7, 800, 0.05)
    r = U.fgr_ref(src, tgt, None)
    rre, rte = U.pose_errors(r["T"], pose)
    assert rre > SUCCESS_RRE and not recovered(r, pose)                     # 143.6 degrees
    found = None
    for count in (65536, 131072, 262144):
        r = U.fgr_ref(src, tgt, None, tuples=count)
        if recovered(r, pose):
            found = count
            break
    assert found == U.TUPLES_05
    assert r["tuples_accepted"] == 84 and r["inliers"] == int(mask.sum()) and r["status"] == 0 and U.well_posed(r)
    assert r["n_used"] == int((r["multiplicity"] > 0).sum()) < 3 * 84 + 1 and r["multiplicity"].sum() == 3 * 84


def test_a_row_permutation_changes_the_transform_by_less_than_1e_9():
    src, tgt, _, _, _ = CU.make_set(6, 600, 0.10)
    p = np.random.default_rng(0).permutation(600)
    a, b = U.fgr_ref(src, tgt, None), U.fgr_ref(src[p], tgt[p], None)
    d = float(np.abs(a["T64"] - b["T64"]).max())
    print("permutation:", d)
    assert d < 1e-9                                                          # measured 5e-16


@pytest.mark.parametrize("name", U.GPU_CASES)
def test_every_gpu_fixture_is_well_posed(name):
    (src, tgt, w, mask, pose), kw = U.fixture(name)
    r = U.reference(name)
    assert U.well_posed(r), (name, max(r["conds"], default=0), r["margin"], r["near"])
    if name.startswith(("n_", "it_128", "ratio_", "m_", "zero_", "other_")) and name not in ("n_3", "n_4"):
        # every planted row is an inlier; an outlier whose random target falls inside the radius may add to the count
        assert recovered(r, pose) and int(mask.sum()) <= r["inliers"] <= int(mask.sum()) + 2, (name, U.pose_errors(r["T"], pose))


def test_fixture_shapes_cover_the_kernel_borders():
    assert [U.fixture(f"n_{n}")[0][0].shape[0] for n in (3, 4, 255, 256, 257, 1535, 1536, 1537, 20000)] == \
        [3, 4, 255, 256, 257, 1535, 1536, 1537, 20000] and U.LDS_ROWS == 1536
    assert [U.reference(f"it_{k}")["steps"] for k in (1, 3, 4, 5, 128)] == [1, 3, 4, 5, 128]
    mus = [U.reference(f"it_{k}")["mu"] for k in (3, 4, 5)]
    assert mus[0] == U.reference("it_3")["trace"][0, 12] and mus[1] == mus[0] / 1.4 == mus[2]   # the first decrease follows step 3
    acc = [U.reference(f"tuples_{t}")["tuples_accepted"] for t in (1, 63, 64, 65, 4096)]
    assert acc == sorted(acc) and acc[0] <= 1 and acc[-1] > acc[1] > 0, acc
    r = U.reference("tuples_4096")
    assert r["multiplicity"].max() > 1 and (r["multiplicity"] == 0).any() and r["status"] == 0
    assert U.reference("other_params")["mu"] == float(np.float32(0.05)) ** 2


def test_degenerate_cases_of_the_definition():
    r = U.reference("no_tuples")
    (src, tgt, w, _, _), kw = U.fixture("no_tuples")
    assert r["status"] == U.NO_TUPLES and r["tuples_accepted"] == 0 and (r["multiplicity"] == 1).all()
    plain = U.fgr_ref(src, tgt, w, **dict(kw, tuples=0))
    assert np.array_equal(plain["T64"], r["T64"]) and plain["status"] == 0 and np.array_equal(plain["trace"], r["trace"])
    r = U.reference("zero_scores")
    (src, tgt, w, mask, _), _ = U.fixture("zero_scores")
    assert r["n_used"] == int((w > 0).sum()) < len(w) and r["inliers"] == int(mask.sum()) > int((mask & (w > 0)).sum())
    r = U.reference("two_used")
    assert r["status"] == U.TOO_FEW and r["n_used"] == 2 and r["steps"] == 0 and np.array_equal(r["T"], np.eye(4)) and not r["trace"].any()
    r = U.reference("line")
    assert r["status"] == U.SINGULAR and r["steps"] == 0 and r["trace"][0, 15] == 1.0 and not r["trace"][1:].any()
    assert np.array_equal(r["T"][:3], np.concatenate([np.eye(3), [[2.0], [-0.75], [0.5]]], 1)) and r["inliers"] == 12
    e = U.fgr_ref(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), None, tuples=5)
    assert e["status"] == U.NO_ROWS and np.array_equal(e["T"], np.eye(4)) and e["inliers"] == 0
    short = U.fgr_ref(*[x[:2] for x in U.fixture("n_4")[0][:3]], tuples=5)
    assert short["status"] == U.TOO_FEW and short["tuples_accepted"] == 0          # n < 3: no tuple test, so no NO_TUPLES either


def test_the_sums_equal_a_row_loop_and_a_step_lowers_the_objective():
    (src, tgt, w, _, _), _ = U.fixture("n_255")
    P, Q = src[:9].astype(np.float64), tgt[:9].astype(np.float64)
    Pc, Qc, wu = P - P.mean(0), Q - Q.mean(0), w[:9].astype(np.float64)
    S, mu = np.eye(3, 4), 2.0
    A, g, obj, so = U.sums(S, mu, Pc, Qc, wu)
    A2, g2, obj2 = np.zeros((6, 6)), np.zeros(6), 0.0
    for p, q, wi in zip(Pc, Qc, wu):
        y = p
        r = y - q
        e = r @ r
        K = -np.array([[0, -y[2], y[1]], [y[2], 0, -y[0]], [-y[1], y[0], 0]])
        J = np.concatenate([K, np.eye(3)], 1)
        om = wi * (mu / (e + mu)) ** 2
        A2 += om * J.T @ J
        g2 += om * J.T @ r
        obj2 += wi * mu * e / (e + mu)
    assert np.abs(A - A2).max() < 1e-12 and np.abs(g - g2).max() < 1e-12 and abs(obj - obj2) < 1e-12
    # the six structural zeros, the three equal diagonals and the antisymmetric block the kernel does not carry
    assert A[0, 3] == A[1, 4] == A[2, 5] == A[3, 4] == A[3, 5] == A[4, 5] == 0.0
    assert abs(A[3, 3] - so) < 1e-12 and abs(A[0, 4] + A[1, 3]) < 1e-12 and abs(A[0, 5] + A[2, 3]) < 1e-12 and abs(A[1, 5] + A[2, 4]) < 1e-12
    Sn, _ = U.advance(S, mu, A, g, 0, 0.01)
    assert U.sums(Sn, mu, Pc, Qc, wu)[2] < obj
    R, _ = U.delta(np.array([0.3, -0.2, 0.1, 0, 0, 0]))
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15


def test_header_prototypes_exports_and_workspace_size():
    from roitr_amd import _lib
    I, F, D, P, SZ, U64 = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    protos = _lib.header_prototypes()
    assert protos["roitr_fgr_workspace_bytes"] == (SZ, [I, I])
    head, tail = [I, P, I, P, P, P, P, U64, F, D, I, I, I, F, F], [P, SZ] + [P] * 11
    assert protos["roitr_fgr_batch"] == (I, head + tail) and protos["roitr_fgr_batch_staged"] == (I, head + [I] + tail)
    assert "roitr_fgr_batch" not in _lib.BOUND and "roitr_fgr_workspace_bytes" not in _lib.BOUND and len(_lib.BOUND) == 35
    lib = ctypes.CDLL(_lib.LIB_PATH)     # host-only: no device is touched
    assert all(hasattr(lib, n) for n in ("roitr_fgr_batch", "roitr_fgr_batch_staged", "roitr_fgr_workspace_bytes"))
    assert lib.roitr_abi_version() == 4
    f = lib.roitr_fgr_workspace_bytes
    f.restype, f.argtypes = protos["roitr_fgr_workspace_bytes"]
    assert f(0, 100) == 0 and f(1, -1) == 0 and f(65536, 100) == 0
    sizes = [f(1, n) for n in (0, 1, 1000, 20000, 10 ** 6)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] >= 4 * 10 ** 6
    assert f(1, 5000) <= f(2, 5000) <= f(512, 5000) <= f(65535, 5000)


def test_refusals():
    """ROITR_ERR_ARG before anything is launched or written: parameters out of range with null device pointers, then the pointer and
    workspace checks with host addresses that are never read."""
    from roitr_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    protos = _lib.header_prototypes()
    lib.roitr_fgr_batch.restype, lib.roitr_fgr_batch.argtypes = protos["roitr_fgr_batch"]
    lib.roitr_fgr_batch_staged.restype, lib.roitr_fgr_batch_staged.argtypes = protos["roitr_fgr_batch_staged"]
    lib.roitr_last_error.restype = ctypes.c_char_p
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)
    good = dict(pairs=1, starts=a, total_rows=10, src=a, tgt=a, scores=None, keys=a, seed=0, max_dist=0.1, division=1.4, iterations=8,
                mu_every=4, tuples=0, scale=0.95, radius=0.1, ws=a, ws_bytes=0, T=a, inliers=a, n_used=a, acc=a, steps=a, mu=a, obj=a,
                status=a, mult=None, trace=None, stream=None)

    def call(**kw):
        return lib.roitr_fgr_batch(*dict(good, **kw).values())

    inf, nan = float("inf"), float("nan")
    bad = [dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=inf), dict(max_dist=nan), dict(radius=0.0), dict(radius=inf),
           dict(division=1.0), dict(division=0.5), dict(division=inf), dict(division=nan), dict(iterations=0), dict(iterations=1025),
           dict(mu_every=0), dict(tuples=-1), dict(tuples=2 ** 28 + 1), dict(scale=0.0), dict(scale=1.0), dict(scale=nan),
           dict(total_rows=-1), dict(pairs=65536)]
    null = dict(starts=None, src=None, tgt=None, keys=None, ws=None, T=None, inliers=None, n_used=None, acc=None, steps=None, mu=None,
                obj=None, status=None)
    for kw in bad:
        assert call(**dict(null, **kw)) == 1, kw                         # ROITR_ERR_ARG, with null pointers everywhere
    for name in ("starts", "src", "tgt", "T", "inliers", "n_used", "acc", "steps", "mu", "obj", "status"):
        assert call(**{name: None}) == 1 and b"null pointer" in lib.roitr_last_error(), name
    assert call(keys=None, tuples=1) == 1 and b"pair_keys" in lib.roitr_last_error()
    assert call() == 1 and b"workspace" in lib.roitr_last_error()       # a short workspace (0 bytes)
    assert call(ws=None, ws_bytes=1 << 20) == 1 and b"workspace" in lib.roitr_last_error()
    vals = list(good.values())
    for cap in (-1, 1537):
        assert lib.roitr_fgr_batch_staged(*vals[:15], cap, *vals[15:]) == 1 and b"lds_rows" in lib.roitr_last_error()
    assert call(**dict(null, pairs=0)) == 0                              # no pairs: nothing to do, as the sibling operators


def test_main_parser_accepts_the_new_options_and_keeps_every_old_default():
    from roitr_amd.main import parser
    a = parser().parse_args(["c.yaml", "--register", "--estimator", "fgr", "--fgr-max-dist", "0.05", "--fgr-iterations", "64",
                             "--fgr-tuples", "4096"])
    assert (a.estimator, a.fgr_max_dist, a.fgr_iterations, a.fgr_tuples) == ("fgr", 0.05, 64, 4096)
    d = parser().parse_args(["c.yaml"])
    assert (d.estimator, d.fgr_max_dist, d.fgr_iterations, d.fgr_tuples) == ("ransac", 0.1, 128, 0)
    assert (d.ransac_iterations, d.ransac_points, d.lgr_radius, d.lgr_steps, d.compat_dist, d.compat_seeds, d.compat_k) == \
        (50000, 1000, 0.1, 5, 0.1, 64, 20)
    assert (d.refine, d.icp_distance, d.icp_iterations, d.gicp_epsilon, d.fpfh_baseline, d.fpfh_radius, d.fpfh_max_nn) == \
        ("none", 0.05, 30, 1e-3, False, 0.125, 100)
    assert (d.pairs_per_forward, d.n_points, d.overlap_radius, d.subsample_seed, d.voxel_size, d.points_lim) == (8, 5000, 0.0375, 0, None, None)
    with pytest.raises(SystemExit):
        parser().parse_args(["c.yaml", "--estimator", "icp"])


def test_the_tester_and_the_baseline_take_the_estimator():
    from roitr_amd.tester import Pose, Tester
    cfg = {"benchmark": "3DMatch"}
    t = Tester(cfg, None, [], register=True, evaluate=True, estimator="fgr", fgr=dict(iterations=64, tuples=4096), fpfh_baseline={})
    assert [s.name for s in t.stages] == ["pose", "fpfh"] and t.fgr == dict(iterations=64, tuples=4096)
    pose = t.stages[0]
    assert pose.estimator == "fgr" and pose.kw == dict(iterations=64, tuples=4096)
    assert Pose("fgr", {}, {}, {}, None, {}, False).kw == {} and Pose("ransac", dict(a=1), {}, {}, None, {}, False).kw == dict(a=1)
    assert Tester(cfg, None, [], register=True, estimator="fgr").fgr == {}
    for bad in (dict(estimator="icp"), dict(estimator="lgr", fpfh_baseline={})):
        with pytest.raises(ValueError):
            Tester(cfg, None, [], **bad)
    from roitr_amd.fpfh import _estimate
    with pytest.raises(ValueError, match="lgr"):
        _estimate({}, (None, None, None), "lgr", {})


def test_the_module_is_imported_only_in_its_own_mode():
    import os
    import subprocess
    import sys
    code = ("import sys; from roitr_amd.tester import Tester; import roitr_amd.main; "
            "Tester({'benchmark': '3DMatch'}, None, [], register=True, evaluate=True, estimator='fgr', fpfh_baseline={}); "
            "sys.exit(int('roitr_amd.fgr' in sys.modules))")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0
