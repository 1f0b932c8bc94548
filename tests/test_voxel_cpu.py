"""CPU: the float64 restatement of the voxel grid and the point cap (tests/voxel_util.py) on cases worked out by hand, the new
symbols of the C ABI, and the absence of a CPU fallback in the two wrappers."""
import numpy as np
import pytest

import voxel_util as V


def test_hand_computed_six_points_two_voxels():
    # voxel 1.0, min_bound (0, 0, 0) -> vmb = -0.5: voxel 0 covers [-0.5, 0.5), voxel 1 covers [0.5, 1.5) on x.
    # x = 0.5 lies exactly on the face between them and belongs to the upper voxel (floor((0.5 + 0.5) / 1) = 1).
    p = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.5, 0.0, 0.0], [1.25, 0.25, 0.0], [0.125, 0.25, 0.25]], np.float32)
    attr = np.arange(6, dtype=np.float32).reshape(6, 1)
    pts, a, inv, cnt, status = V.voxel_cloud(p, 1.0, attr)
    assert status == 0
    assert inv.tolist() == [0, 1, 0, 1, 1, 0] and cnt.tolist() == [3, 3]
    want = np.array([[(0.0 + 0.25 + 0.125) / 3, 0.25 / 3, 0.25 / 3], [(1.0 + 0.5 + 1.25) / 3, 0.25 / 3, 0.0]])
    assert np.array_equal(pts, want.astype(np.float32))
    assert np.array_equal(a, np.array([[(0 + 2 + 5) / 3], [(1 + 3 + 4) / 3]]).astype(np.float32))


def lattice_cloud(n=4000, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.integers(-40, 41, size=(n, 3)) * 0.125).astype(np.float32)


def test_lattice_points_lie_inside_their_voxel_box():
    p = lattice_cloud()
    vs = 0.25
    pts, _, inv, cnt, status = V.voxel_cloud(p, vs)
    assert status == 0 and np.array_equal(cnt, np.bincount(inv, minlength=len(cnt)))
    vmb = p.min(0).astype(np.float64) - vs * 0.5
    ijk = np.floor((p.astype(np.float64) - vmb) / vs)
    lo = vmb + ijk * vs
    assert ((p >= lo) & (p < lo + vs)).all()            # every point inside its voxel's box (multiples of 0.125: all exact)
    lo_v = np.zeros((len(cnt), 3)); lo_v[inv] = lo
    assert ((pts >= lo_v) & (pts < lo_v + vs)).all()    # and so is every mean
    key = ijk[:, 0] * 2.0 ** 32 + ijk[:, 1] * 2.0 ** 16 + ijk[:, 2]
    first = np.full(len(cnt), -1.0); first[inv] = key
    assert (np.diff(first) > 0).all()                   # output rows ascend in (ix, iy, iz)


def test_summation_order_has_teeth():
    ch = np.tile(np.array([2.0 ** 60, 1.0, -2.0 ** 60, 1.0, 3.0], np.float32), 7)
    p = np.zeros((len(ch), 3), np.float32)
    _, a, _, cnt, _ = V.voxel_cloud(p, 1.0, ch.reshape(-1, 1))
    assert cnt.tolist() == [35]
    assert a[0, 0] == np.float32(4.0 / 35.0)               # input order: everything before the last 2^60 is absorbed, then -2^60, 1, 3
    _, ar, _, _, _ = V.voxel_cloud(p, 1.0, ch[::-1].reshape(-1, 1))
    assert ar[0, 0] == np.float32(0.0)                     # reversed order: the sum ends on 1 absorbed by 2^60, then -2^60 ... + 2^60


def test_status_and_empty_clouds():
    far = np.array([[0, 0, 0], [70, 0, 0]], np.float32)
    assert V.voxel_cloud(far, 0.001)[4] == V.STATUS_RANGE
    nan = np.array([[0, 0, 0], [np.nan, 0, 0]], np.float32)
    assert V.voxel_cloud(nan, 0.1)[4] == V.STATUS_NONFINITE
    xyz = np.concatenate([far, lattice_cloud(50)])
    r = V.voxel_batch(xyz, [2, 2, 52], 0.001)
    assert r["status"].tolist() == [1, 0, 0] and r["offset"][:2].tolist() == [0, 0] and (r["inverse"][:2] == -1).all()
    assert r["inverse"][2:].min() == 0


def test_cap_restatement():
    idx, off = V.subsample_batch([10, 10, 1010], 64, seed=3)
    assert off.tolist() == [10, 10, 74] and idx[:10].tolist() == list(range(10)) and (np.diff(idx) > 0).all()
    u = V.subsample_u(1000, 2, 3)
    assert u.max() < 2 ** 48 and set(idx[10:] - 10) == set(np.argsort(u, kind="stable")[:64])
    other, _ = V.subsample_batch([10, 10, 1010], 64, seed=4)
    assert set(other.tolist()) != set(idx.tolist())
    # the kept set of a cloud follows its key, not its position in the call
    alone, _ = V.subsample_batch([1000], 64, seed=3, cloud_keys=[2])
    assert np.array_equal(alone, idx[10:] - 10)


def test_new_symbols_are_exported():
    from roitr_amd import _lib
    lib = _lib.lib()
    for name in ("roitr_voxel_workspace_bytes", "roitr_voxel_downsample", "roitr_subsample_workspace_bytes", "roitr_random_subsample"):
        assert hasattr(lib, name), name
    assert lib.roitr_abi_version() == 4


def test_wrappers_have_no_cpu_fallback():
    import torch
    from roitr_amd import _lib, prep
    with pytest.raises(_lib.RoitrError):
        prep.voxel_down_sample(torch.zeros(8, 3), torch.tensor([8], dtype=torch.int32), 0.1)
    with pytest.raises(_lib.RoitrError):
        prep.random_subsample(torch.tensor([8], dtype=torch.int32), 4)
