"""GPU: roitr_amd.prep.voxel_down_sample and random_subsample against the float64 restatement of tests/voxel_util.py.

Everything is compared BIT for bit (floats through their uint32 images): the operation order is defined -- float64 sums in input
order, one correctly rounded division, one rounding to fp32 -- so there is no tolerance to choose.  The sizes walk the edges of the
sort's tile (4096 items per workgroup), of a wave (64) and of a workgroup (256); the 300 000-point cloud spans many workgroups."""
import numpy as np
import pytest
import torch

import voxel_util as V

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65537)
VOXEL = 0.025


def scan_cloud(n, seed):
    from roitr_amd.synthetic import surface_points
    return surface_points(np.random.default_rng(seed), n, 0.0, 2.0).astype(np.float32)


_CACHE = {}


def big_cloud():
    """300 000 scan-like points with two attribute channels and their restatement, computed once."""
    if "big" not in _CACHE:
        p = scan_cloud(300000, 11)
        a = np.random.default_rng(12).standard_normal((len(p), 2)).astype(np.float32)
        _CACHE["big"] = (p, a, V.voxel_batch(p, [len(p)], VOXEL, a))
    return _CACHE["big"]


def run(clouds, vs, attrs=None, strict=False):
    from roitr_amd.prep import voxel_down_sample
    xyz = np.concatenate(clouds) if clouds else np.zeros((0, 3), np.float32)
    off = np.cumsum([len(c) for c in clouds]).astype(np.int32)
    attr = None if attrs is None else torch.from_numpy(np.concatenate(attrs)).cuda()
    r = voxel_down_sample(torch.from_numpy(xyz).cuda(), torch.from_numpy(off).cuda(), vs, attr, strict=strict)
    got = {k: (None if v is None else v.cpu().numpy()) for k, v in r._asdict().items()}
    return got, V.voxel_batch(xyz, off, vs, None if attrs is None else np.concatenate(attrs))


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what=""):
    for k in ("offset", "status", "counts", "inverse", "points", "attr"):
        if want[k] is None:
            assert got[k] is None, (what, k)
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k, int((bits(got[k]) != bits(want[k])).sum()))


def test_single_clouds_at_the_tile_edges():
    p, a, _ = big_cloud()
    for n in SIZES:
        got, want = run([p[:n]], VOXEL, [a[:n]])
        assert_same(got, want, n)


def test_ragged_batch_with_empty_clouds():
    p, a, _ = big_cloud()
    sizes = (0, 1000, 0, 4097, 65, 0)
    cuts = np.cumsum((0,) + sizes)
    clouds = [p[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]
    got, want = run(clouds, VOXEL, [a[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert_same(got, want)
    assert want["offset"][0] == 0 and want["offset"][2] == want["offset"][1] and want["offset"][5] == want["offset"][4]
    got, want = run([np.zeros((0, 3), np.float32)], VOXEL)      # n = 0 altogether
    assert_same(got, want)


def test_one_cloud_over_many_workgroups():
    p, a, want = big_cloud()
    from roitr_amd.prep import voxel_down_sample
    r = voxel_down_sample(torch.from_numpy(p).cuda(), torch.tensor([len(p)], dtype=torch.int32).cuda(), VOXEL, torch.from_numpy(a).cuda())
    assert_same({k: (None if v is None else v.cpu().numpy()) for k, v in r._asdict().items()}, want)
    assert 50000 < len(want["counts"]) < 120000 and want["counts"].max() > 8


def test_extremes_of_run_length():
    same = np.tile(np.array([[0.3, -1.7, 2.9]], np.float32), (50000, 1))
    got, want = run([same], VOXEL, [np.arange(50000, dtype=np.float32).reshape(-1, 1)])
    assert_same(got, want, "one voxel")
    assert want["counts"].tolist() == [50000]
    rng = np.random.default_rng(3)
    cells = rng.permutation(40 * 40 * 40)[:20000]
    alone = (np.stack([cells // 1600, (cells // 40) % 40, cells % 40], 1) * 0.0625).astype(np.float32)
    got, want = run([alone], VOXEL)
    assert_same(got, want, "one point per voxel")
    assert len(want["counts"]) == 20000


def test_lattice_case():
    from test_voxel_cpu import lattice_cloud
    got, want = run([lattice_cloud(), lattice_cloud(777, 6)], 0.25)
    assert_same(got, want)


def test_stable_sort_keeps_input_order_inside_a_voxel():
    """The mixed-magnitude channel of tests/test_voxel_cpu.py in one voxel whose points alternate in the input with points of other
    voxels: any other order of the voxel's points gives another sum (4 in input order, 0 reversed)."""
    ch = np.tile(np.array([2.0 ** 60, 1.0, -2.0 ** 60, 1.0, 3.0], np.float32), 7)
    rng = np.random.default_rng(9)
    n = 3 * len(ch)
    p = (rng.random((n, 3)) * 4.0 + 1.0).astype(np.float32)     # other voxels, with keys on both sides of the voxel of (10, 10, 10)
    p[2::6] += np.float32(11.0)
    p[::3] = np.float32(10.0)
    attr = rng.standard_normal((n, 1)).astype(np.float32)
    attr[::3, 0] = ch
    got, want = run([p], 0.25, [attr])
    assert_same(got, want)
    v = want["inverse"][0]
    assert want["counts"][v] == 35 and want["attr"][v, 0] == np.float32(4.0 / 35.0)
    assert len(want["counts"]) > 20


def test_high_key_bits():
    rng = np.random.default_rng(21)
    line = np.zeros((400, 3), np.float32)
    line[:, 0] = np.concatenate([[0.0, 60.0], rng.random(398) * 60.0]).astype(np.float32)
    line[:, 1] = (rng.random(400) * 30.0).astype(np.float32); line[0, 1] = 0.0
    got, want = run([line], 0.001)
    assert_same(got, want, "indices up to 60 000")
    assert want["status"].tolist() == [0]
    clouds = [scan_cloud(int(k), 100 + i) for i, k in enumerate(rng.integers(5, 41, size=300))]
    got, want = run(clouds, 0.2)
    assert_same(got, want, "300 clouds")
    assert len(want["offset"]) == 300 and want["status"].max() == 0


def test_status_bits_leave_the_other_clouds_alone():
    from roitr_amd import _lib
    good0, good1 = scan_cloud(3000, 31), scan_cloud(5000, 32) * np.float32(0.01)
    far = np.array([[0, 0, 0], [0, 70.0, 0], [0, 1, 0]], np.float32)
    nan = scan_cloud(500, 33) * np.float32(0.01); nan[250, 2] = np.nan
    got, want = run([good0, far, nan, good1], 0.001)
    assert_same(got, want)
    assert got["status"].tolist() == [0, V.STATUS_RANGE, V.STATUS_NONFINITE, 0]
    assert got["offset"][1] == got["offset"][0] == got["offset"][2] and (got["inverse"][3000:3503] == -1).all()
    for k, (cloud, lo) in enumerate(((good0, 0), (good1, 3503))):
        alone, _ = run([cloud], 0.001)
        v0 = 0 if k == 0 else got["offset"][2]
        assert np.array_equal(bits(alone["points"]), bits(got["points"][v0:v0 + len(alone["points"])]))
        assert np.array_equal(alone["inverse"] + v0, got["inverse"][lo:lo + len(cloud)])
    with pytest.raises(_lib.RoitrError, match="cloud 1"):
        run([good0, far, nan, good1], 0.001, strict=True)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.RoitrError):
            run([good0], bad)


def test_determinism_and_batch_invariance():
    p, a, _ = big_cloud()
    clouds = [p[:70000], p[70000:70100], p[100000:165537]]
    attrs = [a[:70000], a[70000:70100], a[100000:165537]]
    first, want = run(clouds, VOXEL, attrs)
    assert_same(first, want)
    for _ in range(2):
        again, _ = run(clouds, VOXEL, attrs)
        assert_same(again, first, "repeat")
    alone, _ = run([clouds[2]], VOXEL, [attrs[2]])
    v0 = first["offset"][1]
    assert np.array_equal(bits(alone["points"]), bits(first["points"][v0:])) and np.array_equal(bits(alone["attr"]), bits(first["attr"][v0:]))
    assert np.array_equal(alone["counts"], first["counts"][v0:]) and np.array_equal(alone["inverse"] + v0, first["inverse"][70100:])


# ---------------------------------------------------------------------------------------------------------------- the cap
def cap(sizes, limit, seed=0, keys=None):
    from roitr_amd.prep import random_subsample
    off = torch.from_numpy(np.cumsum(sizes).astype(np.int32)).cuda()
    idx, new_off = random_subsample(off, limit, seed, None if keys is None else torch.tensor(keys, dtype=torch.int32))
    return idx.cpu().numpy(), new_off.cpu().numpy()


def test_cap_equals_the_restatement_at_the_edges():
    # 4081 .. 4111: the flag array holds n bytes and no padding, its last group of 16 flags is read byte by byte at these lengths
    for n in SIZES + tuple(range(4081, 4112, 5)):
        for limit in sorted({1, 64, n - 1, n, n + 1} - {0}):
            idx, off = cap([n], limit, seed=5)
            want_idx, want_off = V.subsample_batch([n], limit, seed=5)
            assert idx.dtype == np.int32 and np.array_equal(idx, want_idx) and np.array_equal(off, want_off), (n, limit)
            assert len(idx) == min(n, limit) and (np.diff(idx) > 0).all()


def test_cap_batched_counts_keys_and_seeds():
    sizes = [4097, 0, 300, 65537, 1, 30000]
    keys = [7, 8, 9, 70000, 11, 12]
    idx, off = cap(sizes, 300, seed=1, keys=keys)
    want_idx, want_off = V.subsample_batch(np.cumsum(sizes), 300, seed=1, cloud_keys=keys)
    assert np.array_equal(idx, want_idx) and np.array_equal(off, want_off)
    assert np.diff(np.concatenate([[0], off])).tolist() == [min(s, 300) for s in sizes] and (np.diff(idx) > 0).all()
    # the cloud of 65537 points at another position of another call, under the same key: the same rows
    moved, moved_off = cap([65537, 500], 300, seed=1, keys=[70000, 3])
    lo = int(np.cumsum(sizes)[2])
    assert np.array_equal(moved[:300], idx[off[2]:off[3]] - lo)
    other, _ = cap(sizes, 300, seed=2, keys=keys)
    assert not np.array_equal(other, idx)
    # default keys are the positions in the call
    d_idx, d_off = cap(sizes, 300, seed=1)
    w_idx, w_off = V.subsample_batch(np.cumsum(sizes), 300, seed=1)
    assert np.array_equal(d_idx, w_idx) and np.array_equal(d_off, w_off)
    third, _ = cap(sizes, 300, seed=1, keys=keys)
    assert np.array_equal(third, idx)
    many, many_off = cap([50] * 300, 20, seed=4)
    w_many, w_many_off = V.subsample_batch(np.cumsum([50] * 300), 20, seed=4)
    assert np.array_equal(many, w_many) and np.array_equal(many_off, w_many_off)
