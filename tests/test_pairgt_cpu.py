"""CPU: the float64 restatement of the pair ground truth (tests/pairgt_util.py) on a case worked out by hand, against scipy's KD-tree,
the first-order property that fixes the factor 2 of the information matrix, the gt.info layout against three records of a Redwood
file, the new symbols of the C ABI and the absence of a CPU fallback in the wrappers."""
import os

import numpy as np
import pytest

import pairgt_util as U

HERE = os.path.dirname(os.path.abspath(__file__))


def test_hand_computed_strict_radius_ties_and_cap():
    # coordinates in units of 1/8, r = 5/8: the 3-4-5 points lie at d2 = 25/64 == r * r exactly and are OUT (strict inequality)
    src = np.array([[0, 0, 0], [8, 8, 9], [-40, -40, -40]], np.float32) / 8
    tgt = np.array([[3, 4, 0],    # d2 = 25/64 from source 0: exactly r, out
                    [0, 0, 4],    # 16/64: ties with 2 and 5, ordered by index
                    [4, 0, 0],
                    [1, 0, 0],    # 1/64: the nearest
                    [0, 3, 4],    # 25/64: out
                    [0, 4, 0],
                    [8, 8, 8]], np.float32) / 8
    r = U.pair_brute(src, tgt, np.eye(3), np.zeros(3), 0.625)
    assert r["d2"][0, 0] == 0.625 * 0.625 and r["d2"][0, 4] == 0.625 * 0.625
    assert r["count"].tolist() == [4, 1, 0] and r["nn_idx"].tolist() == [3, 6, -1]
    assert r["nn_dist2"].tolist() == [1 / 64, 1 / 64, np.inf]
    assert r["corr"].tolist() == [[0, 3], [0, 1], [0, 2], [0, 5], [1, 6]]
    assert r["n_hit"] == 2 and r["overlap"] == 2 / 3 and r["info"][0, 0] == 2
    assert U.pair_brute(src, tgt, np.eye(3), np.zeros(3), 0.625, K=2)["corr"].tolist() == [[0, 3], [0, 1], [1, 6]]
    assert U.pair_brute(src, tgt, np.eye(3), np.zeros(3), 0.625, K=1)["corr"].tolist() == [[0, 3], [1, 6]]
    # a hair above r lets the two 3-4-5 points in, behind the ties
    assert U.pair_brute(src, tgt, np.eye(3), np.zeros(3), np.nextafter(np.float32(0.625), np.float32(1)))["corr"][:6].tolist() == \
        [[0, 3], [0, 1], [0, 2], [0, 5], [0, 0], [0, 4]]
    # the transform maps source to target, and the swapped call undoes it
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    t = np.array([1, 2, 3], np.float32)
    moved_tgt = (tgt @ Rz.T + t).astype(np.float32)
    assert U.pair_brute(src, moved_tgt, Rz, t, 0.625)["corr"].tolist() == r["corr"].tolist()
    back = U.pair_brute(moved_tgt, src, Rz, t, 0.625, inverse=True)
    assert sorted(map(tuple, back["corr"][:, ::-1].tolist())) == sorted(map(tuple, r["corr"].tolist()))


def test_status_of_the_restatement():
    a = np.zeros((3, 3), np.float32)
    bad = a.copy(); bad[1, 1] = np.nan
    assert U.pair_brute(bad, a, np.eye(3), np.zeros(3), 1.0)["status"] == U.STATUS_NONFINITE
    assert U.pair_brute(a, a, np.eye(3), [0, np.inf, 0], 1.0)["status"] == U.STATUS_NONFINITE
    r = U.pair_brute(a, a[:0], np.eye(3), np.zeros(3), 1.0)
    assert r["status"] == U.STATUS_EMPTY and r["count"].tolist() == [0, 0, 0] and np.isnan(r["overlap"]) and r["n_hit"] == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_against_scipy_ball_query(seed):
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(seed)
    src = rng.uniform(-1, 1, size=(700, 3)).astype(np.float32)
    tgt = rng.uniform(-1, 1, size=(900, 3)).astype(np.float32)
    R, t = U.random_rigid(rng, shift=0.2)
    radius = 0.2
    mine = U.pair_brute(src, tgt, R, t, radius)
    moved = U.move(src, R, t)
    tree = spatial.cKDTree(tgt.astype(np.float64))
    r64 = float(np.float32(radius))
    ref = {(i, j) for i, js in enumerate(tree.query_ball_point(moved, r64)) for j in js}
    d = np.sqrt(mine["d2"])
    near = {(i, j) for i, j in zip(*np.nonzero(np.abs(d - r64) < 1e-9))}
    assert len(ref) > 1000
    assert len(near & ref) <= 0.01 * len(ref)
    assert len(near) == 0     # seeded uniform clouds: no pair within 1e-9 of the boundary
    assert {tuple(x) for x in mine["corr"].tolist()} - near == ref - near


@pytest.mark.parametrize("eps,tol", [(1e-3, 0.01), (1e-2, 0.05)])
def test_first_order_property_pins_the_factor_two(eps, tol):
    """er^T info er / info[0][0] with er = [t, q_xyz] of E (registration.compute_transformation_err) is, to first order, the mean
    squared displacement |E p - p|^2 of the hit points: the rotation vector is about 2 q_xyz, hence G = [ I | -2 [p]x ].  The margins
    are the second-order term (measured: 0.06 % at 1e-3, 0.35 % at 1e-2); with a factor 1 the ratio is 0.48 .. 0.71."""
    from roitr_amd.registration import compute_transformation_err
    rng = np.random.default_rng(11)
    src = rng.uniform(-1.5, 2.5, size=(1500, 3)).astype(np.float32)
    R, t = U.random_rigid(rng)
    tgt = (U.move(src[::2], R, t) + rng.normal(size=(750, 3)) * 0.01).astype(np.float32)
    r = U.pair_brute(src, tgt, R, t, 0.05)
    hit = src[r["count"] > 0].astype(np.float64)
    assert 300 < len(hit) < 1500 and r["info"][0, 0] == len(hit)
    for _ in range(8):
        w, v = rng.normal(size=3), rng.normal(size=3)
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = U.rodrigues(w * eps / np.linalg.norm(w)), v * eps / np.linalg.norm(v)
        want = np.mean(np.sum((hit @ E[:3, :3].T + E[:3, 3] - hit) ** 2, 1))
        got = compute_transformation_err(E, r["info"])
        assert abs(got / want - 1) < tol, (got, want)


def _layout_identities(info):
    n = info[0, 0]
    assert np.array_equal(info[:3, :3], n * np.eye(3))
    tr = info[:3, 3:]
    assert np.array_equal(tr, -tr.T) and np.array_equal(info[3:, :3], tr.T)
    assert np.allclose(info[3:, 3:], info[3:, 3:].T, rtol=1e-9, atol=0)
    return n, np.array([tr[1, 2], -tr[0, 2], tr[0, 1]]) / 2, np.trace(info[3:, 3:]) / 8   # n, sum p, sum |p|^2 under G = [I | -2[p]x]


def test_info_layout_matches_redwood_records():
    from roitr_amd.registration import read_trajectory_info
    rng = np.random.default_rng(3)
    p = rng.uniform(-2, 3, size=(400, 3))
    info = U.info_matrix(p)
    n, s, q = _layout_identities(info)
    assert n == 400 and np.isclose(info[0, 4], 2 * p[:, 2].sum(), rtol=1e-12)   # another summation order
    assert np.allclose(s, p.sum(0), rtol=1e-12) and np.isclose(q, (p * p).sum(), rtol=1e-12)
    assert np.allclose(info[3:, 3:], 4 * ((p * p).sum() * np.eye(3) - p.T @ p), rtol=1e-11)
    n_frame, sample = read_trajectory_info(os.path.join(HERE, "golden", "redwood_info_sample.info"))
    assert n_frame == 60 and sample.shape == (3, 6, 6)
    for rec in sample:
        n, s, q = _layout_identities(rec)
        assert n > 0 and float(n).is_integer()
        assert s @ s <= n * q                      # Cauchy-Schwarz between sum p and sum |p|^2 as the layout reads them
        assert np.all(np.linalg.eigvalsh(rec) > -1e-6 * n)   # a sum of G^T G is positive semi-definite


def test_new_symbols_are_exported():
    from roitr_amd import _lib
    lib = _lib.lib()
    for name in ("roitr_pairgt_workspace_bytes", "roitr_pairgt_stats", "roitr_pairgt_correspondences"):
        assert hasattr(lib, name), name
    assert lib.roitr_abi_version() == 4


def test_wrappers_have_no_cpu_fallback():
    import torch
    from roitr_amd import _lib, pairgt
    x = torch.zeros(8, 3)
    o = torch.tensor([8], dtype=torch.int32)
    R, t = torch.eye(3).reshape(1, 3, 3), torch.zeros(1, 3)
    with pytest.raises(_lib.RoitrError):
        pairgt.pair_ground_truth(x, o, x, o, R, t, 0.1)
    with pytest.raises(_lib.RoitrError):
        pairgt.radius_correspondences(x, o, x, o, R, t, 0.1)
    with pytest.raises(_lib.RoitrError):
        pairgt.get_correspondences(x, x, torch.eye(4), 0.1)


@pytest.mark.parametrize("offset", [[3, 9], [5, 4, 8], [-1, 8], []])
def test_host_offsets_are_checked(offset):
    from roitr_amd import _lib, pairgt
    with pytest.raises(_lib.RoitrError, match="cumulative"):
        pairgt._check_offsets("src_offset", offset, 8)
    pairgt._check_offsets("src_offset", [0, 3, 3, 8], 8)


def test_host_side_errors_launch_nothing():
    """radius, K, B and null pointers are checked before anything touches a device: these calls return the argument status here."""
    import ctypes
    from roitr_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(256)   # never dereferenced
    stats = lambda b, r, status=one: lib.roitr_pairgt_stats(b, 4, 4, one, one, one, one, one, one, r, 0, None, None, None, one, one, None,
                                                            status, one, None)
    assert stats(1, 0.0) == 1 and stats(1, -1.0) == 1 and stats(1, float("nan")) == 1 and stats(1, float("inf")) == 1
    assert stats(0, 0.1) == 1 and stats(65537, 0.1) == 1 and stats(1, 0.1, None) == 1
    assert b"radius" in lib.roitr_last_error() or b"null" in lib.roitr_last_error()
    corr = lambda k, cap: lib.roitr_pairgt_correspondences(1, 4, 4, one, one, one, one, one, one, 0.1, k, cap, one, one, one, one, one, None)
    assert corr(-1, 16) == 1 and corr(0, -1) == 1 and corr(0, 2 ** 31) == 1
    assert lib.roitr_pairgt_workspace_bytes(2, 1000, 1000, 5000) > 1000 * 16 + 5000 * 12
