"""GPU: roitr_fpfh_batch (csrc/fpfh.hip) against the float64 restatement of tests/fpfh_util.py on fixtures that test_fpfh_cpu.py
asserts decided: the integer stages exact, the values within 1e-4 (they lie in [0, 200], one fp32 ulp at 200 is 1.5e-5, and ordered
float64 sums leave no other error source), bitwise invariance, the status word, every refusal, and the baseline end to end."""
import numpy as np
import pytest
import torch

import fpfh_util as U

pytestmark = pytest.mark.gpu

_RUNS = {}


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))   # a copy: the fixtures are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def run(f, pad_to=36, stages=True):
    from roitr_amd.fpfh import compute_fpfh
    r = compute_fpfh(dev(f["xyz"]), dev(f["normals"]), dev(f["offset"]), f["radius"], f["max_nn"], pad_to=pad_to, return_stages=stages,
                     strict=False)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in r) if stages else r.cpu().numpy()


def named(name):
    if name not in _RUNS:
        _RUNS[name] = run(U.fixture(name))
    return _RUNS[name]


@pytest.mark.parametrize("name", U.DECIDED)
def test_stages_exact_and_values_within_1e4(name):
    assert U.is_decided(name)
    want = U.reference(name)
    fpfh, counts, nbr, status = named(name)
    assert not status.any() and fpfh.shape == (want["m"].shape[0], 36) and fpfh.dtype == np.float32
    assert np.array_equal(nbr, want["m"]), (name, np.flatnonzero(nbr != want["m"])[:8])
    assert np.array_equal(counts, want["counts"]), (name, np.flatnonzero((counts != want["counts"]).any(1))[:8])
    err = float(np.abs(fpfh[:, :33].astype(np.float64) - want["fpfh"]).max(initial=0.0))
    print(name, "max |fpfh - restatement| =", err)
    assert err < 1e-4, (name, err)
    assert not fpfh[:, 33:].any() and fpfh.min(initial=0.0) >= 0.0 and fpfh.max(initial=0.0) <= 200.0 + 1e-4


def test_planar_lattice_is_exactly_200():
    f = U.lattice()
    fpfh, counts, nbr, status = run(f)
    want = U.fpfh_ref(**f)
    assert np.array_equal(nbr, want["m"]) and np.array_equal(counts, want["counts"]) and not status.any()
    has = nbr > 0
    row = np.zeros(36, np.float32)
    row[[5, 16, 27]] = 200.0
    assert np.array_equal(fpfh[has], np.tile(row, (int(has.sum()), 1))) and not fpfh[~has].any() and (~has).sum() == 3


@pytest.mark.parametrize("name", ["ragged", "sizes16", "sizes100"])
def test_a_cloud_alone_equals_the_cloud_in_a_batch_at_any_position(name):
    f = U.fixture(name)
    whole = named(name)
    off = np.concatenate([[0], f["offset"]])
    b = len(f["offset"])
    for c in range(b):
        one = run(U.split(f, c))
        for got, ref in zip(one[:3], whole[:3]):
            assert np.array_equal(got, ref[off[c]:off[c + 1]]), (name, c)
    # the clouds in reverse order: every cloud at another batch position, behind other neighbours
    order = list(range(b))[::-1]
    parts = [U.split(f, c) for c in order]
    rev = dict(f, xyz=np.concatenate([p["xyz"] for p in parts]), normals=np.concatenate([p["normals"] for p in parts]),
               offset=np.cumsum([p["xyz"].shape[0] for p in parts]).astype(np.int32))
    got = run(rev)
    roff = np.concatenate([[0], rev["offset"]])
    for pos, c in enumerate(order):
        for g, ref in zip(got[:3], whole[:3]):
            assert np.array_equal(g[roff[pos]:roff[pos + 1]], ref[off[c]:off[c + 1]]), (name, c)


@pytest.mark.parametrize("name", ["ragged", "nn100", "dups"])
def test_repeat_stride_and_optional_outputs_change_nothing(name):
    f = U.fixture(name)
    fpfh, counts, nbr, _ = named(name)
    again = run(f)
    assert all(np.array_equal(a, b) for a, b in zip(again, (fpfh, counts, nbr)))
    narrow = run(f, pad_to=33)
    assert narrow[0].shape[1] == 33 and np.array_equal(narrow[0], fpfh[:, :33]) and np.array_equal(narrow[1], counts)
    wide = run(f, pad_to=70, stages=False)       # more columns than a wave has lanes; spfh_counts / nbr_count NULL
    assert wide.shape[1] == 70 and np.array_equal(wide[:, :33], fpfh[:, :33]) and not wide[:, 33:].any()
    assert np.array_equal(run(f, stages=False), fpfh)


def test_status_flags_the_cloud_and_leaves_the_others_alone():
    from roitr_amd._lib import RoitrError
    from roitr_amd.fpfh import compute_fpfh
    f = U.fixture("ragged")                       # clouds of 300, 0, 700 and 450 points
    clean = named("ragged")
    off = np.concatenate([[0], f["offset"]])
    xyz, nrm = f["xyz"].copy(), f["normals"].copy()
    xyz[off[2] + 5, 1] = np.nan
    nrm[off[2] + 600, 0] = np.inf
    bad = dict(f, xyz=xyz, normals=nrm)
    fpfh, counts, nbr, status = run(bad)
    assert status.tolist() == [0, 0, 1, 0]
    s, e = off[2], off[3]
    assert not fpfh[s:e].any() and not counts[s:e].any() and not nbr[s:e].any()
    for got, ref in zip((fpfh, counts, nbr), clean[:3]):
        assert np.array_equal(got[:s], ref[:s]) and np.array_equal(got[e:], ref[e:])
    for which in ("xyz", "normals"):              # each cause alone
        one = dict(f, **{which: bad[which]})
        assert run(one)[3].tolist() == [0, 0, 1, 0]
    with pytest.raises(RoitrError, match="cloud 2"):
        compute_fpfh(dev(xyz), dev(nrm), dev(f["offset"]), f["radius"], f["max_nn"])


def test_refusals_and_empty_input():
    from roitr_amd import fpfh as F
    lib = F._lib()
    f = U.fixture("nn2")
    n = f["xyz"].shape[0]
    xyz, nrm, off = dev(f["xyz"]), dev(f["normals"]), dev(f["offset"])
    out = torch.zeros((n, 36), dtype=torch.float32, device="cuda")
    status = torch.zeros((1,), dtype=torch.int32, device="cuda")
    nbytes = int(lib.roitr_fpfh_workspace_bytes(1, n, 16))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    good = dict(b=1, n=n, xyz=xyz.data_ptr(), normals=nrm.data_ptr(), offset=off.data_ptr(), radius=0.2, max_nn=16, out_stride=36,
                fpfh=out.data_ptr(), counts=None, nbr=None, status=status.data_ptr(), ws=ws.data_ptr(), nbytes=nbytes)

    def call(**kw):
        a = dict(good, **kw)
        return lib.roitr_fpfh_batch(a["b"], a["n"], a["xyz"], a["normals"], a["offset"], a["radius"], a["max_nn"], a["out_stride"], a["fpfh"],
                                    a["counts"], a["nbr"], a["status"], a["ws"], a["nbytes"], None)

    assert call() == 0
    for kw in (dict(max_nn=1), dict(max_nn=101), dict(max_nn=0), dict(out_stride=32), dict(radius=0.0), dict(radius=-1.0),
               dict(radius=float("nan")), dict(radius=float("inf")), dict(b=-1), dict(n=-1), dict(b=0), dict(xyz=None), dict(normals=None),
               dict(offset=None), dict(fpfh=None), dict(status=None), dict(ws=None), dict(nbytes=nbytes - 1), dict(nbytes=0)):
        assert call(**kw) == 1, kw                # ROITR_ERR_ARG
        assert b"fpfh_batch" in lib.roitr_last_error()
    torch.cuda.synchronize()
    # no points, and a batch of empty clouds only: not an error
    assert call(n=0, xyz=None, normals=None, fpfh=None, ws=None, nbytes=0) == 0
    empty = F.compute_fpfh(xyz[:0], nrm[:0], torch.zeros((3,), dtype=torch.int32, device="cuda"), return_stages=True)
    assert empty[0].shape == (0, 36) and empty[3].tolist() == [0, 0, 0]


def pose_error(T):
    R, t = T[:3, :3], T[:3, 3]
    rre = np.degrees(np.arccos(np.clip((np.trace(R.T @ U.E2E_R) - 1) / 2, -1, 1)))
    return rre, float(np.linalg.norm(t - U.E2E_T))


def test_end_to_end_the_exact_copy_is_registered():
    from roitr_amd.fpfh import fpfh_match_batch, fpfh_pose_estimation
    f = U.fixture("e2e")
    g = U.moved(f)
    assert U.is_decided(g)
    a, b = named("e2e"), run(g)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])          # spfh_counts and nbr_count of the copy
    n = f["xyz"].shape[0]
    m = fpfh_match_batch(dev(f["xyz"]), dev(f["normals"]), [n], dev(g["xyz"]), dev(g["normals"]), [n], f["radius"], f["max_nn"])
    corr = m["corr"].cpu().numpy()
    assert corr.shape[0] > 0.9 * n and (corr[:, 0] == corr[:, 1]).mean() > 0.95
    for estimator in ("compat", "ransac"):     # both with their defaults; measured 0 deg / 0 m for either
        T = fpfh_pose_estimation(f["xyz"], g["xyz"], f["normals"], g["normals"], radius=f["radius"], max_nn=f["max_nn"], estimator=estimator)
        rre, rte = pose_error(T)
        print(estimator, "RRE", rre, "deg, RTE", rte, "m")
        assert T.shape == (4, 4) and T.dtype == np.float64 and rre < 0.1 and rte < 1e-3, (estimator, rre, rte)
    with pytest.raises(ValueError):
        fpfh_pose_estimation(f["xyz"], g["xyz"], f["normals"], g["normals"], estimator="lgr")


def test_raw_pair_through_voxel_grid_and_estimated_normals():
    """Smoke: the pair after voxel_down_sample and estimate_normals on the GPU; finiteness and shapes only."""
    from roitr_amd.fpfh import compute_fpfh, fpfh_pose_estimation
    from roitr_amd.prep import estimate_normals, voxel_down_sample
    f = U.fixture("e2e")
    g = U.moved(f)
    n = f["xyz"].shape[0]
    v = voxel_down_sample(dev(np.concatenate([f["xyz"], g["xyz"]])), torch.tensor([n, 2 * n], dtype=torch.int32), 0.03)
    nrm = estimate_normals(v.points, v.offset, 33, None)
    desc = compute_fpfh(v.points, nrm, v.offset, 0.15, 100)
    k = int(v.offset[0])
    assert desc.shape == (v.points.shape[0], 36) and bool(torch.isfinite(desc).all()) and 0 < k < n
    T = fpfh_pose_estimation(v.points[:k], v.points[k:], nrm[:k], nrm[k:], radius=0.15, max_nn=100)
    assert T.shape == (4, 4) and np.isfinite(T).all()
