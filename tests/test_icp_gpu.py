"""GPU: roitr_icp_batch (csrc/icp.hip) against the float64 restatement of tests/icp_util.py, on the fixtures tests/test_icp_cpu.py
verifies as decided and chain-stable.

Bounds.  Matches, counts, steps and status bits are compared exactly (the match is an exact float64 decision, restated operation by
operation).  A state against the float64 single step from the GPU's own previous state: 1e-5, the project's bound for fp32 transforms
against float64 (tests/test_registration_gpu.py).  fitness / rmse: 1e-9 relative (reordering a float64 sum of at most 1e5 positive
terms moves it by less than 1e-11)."""
import numpy as np
import pytest
import torch

import icp_util as U

pytestmark = pytest.mark.gpu

T_TOL, STAT_TOL = 1e-5, 1e-9
KEYS = ("T", "fitness", "rmse", "n_corr", "steps", "status", "trace_T", "trace_stat")


def pair_of(name):
    f = U.fixture(name)
    return dict(src=f["src"], tgt=f["tgt"], normals=f["normals"], T0=f["T0"])


def run(pairs, plane, **kw):
    """icp_batch on a list of pairs (dicts of src, tgt, T0 and, for plane, normals); every output as numpy, nn_idx split per pair."""
    from roitr_amd.icp import icp_batch
    cat = lambda k: torch.from_numpy(np.concatenate([np.asarray(p[k], np.float32).reshape(-1, 3) for p in pairs])).cuda()
    so = np.cumsum([len(p["src"]) for p in pairs]).astype(np.int32)
    to = np.cumsum([len(p["tgt"]) for p in pairs]).astype(np.int32)
    T0 = torch.from_numpy(np.stack([np.asarray(p["T0"], np.float64) for p in pairs]).astype(np.float32)).cuda()
    kw.setdefault("max_dist", U.MAX_DIST)
    out = icp_batch(cat("src"), so.tolist(), cat("tgt"), to.tolist(), T0, tgt_normals=cat("normals") if plane else None,
                    return_matches=True, return_trace=True, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["nn"] = np.split(out.pop("nn_idx"), so[:-1])
    return out


def replay(out, b, pair, plane, max_dist=U.MAX_DIST, iterations=U.ITERATIONS, check_T=True):
    """Every trace row of pair b against the restatement fed the GPU's own state of that row."""
    src, tgt, nrm = pair["src"], pair["tgt"], pair.get("normals")
    steps, status = int(out["steps"][b]), int(out["status"][b])
    assert out["trace_T"].shape[0] == iterations + 1 and 0 <= steps <= iterations
    assert np.array_equal(out["trace_T"][0, b], np.asarray(pair["T0"], np.float64)[:3].astype(np.float32))
    for s in range(steps + 1):
        T = out["trace_T"][s, b].astype(np.float64)
        e = U.evaluate(T, src, tgt, max_dist)
        fit, rmse = out["trace_stat"][s, b]
        assert abs(fit - e["fitness"]) <= STAT_TOL * e["fitness"] and abs(rmse - e["rmse"]) <= STAT_TOL * e["rmse"], (s, fit, rmse, e)
        if s < steps:
            Tn, bits = (U.step_plane(T, src, tgt, nrm, e["nn"]) if plane else U.step_point(T, src, tgt, e["nn"]))
            assert bits == 0, (s, bits)
            if check_T:
                err = np.abs(out["trace_T"][s + 1, b] - Tn).max()
                assert err <= T_TOL, (s, err)
        else:   # the row the outputs belong to
            assert int(out["n_corr"][b]) == e["n_corr"] and np.array_equal(out["nn"][b], e["nn"])
            assert out["fitness"][b] == fit and out["rmse"][b] == rmse
            assert np.array_equal(out["T"][b, :3], out["trace_T"][s, b]) and np.array_equal(out["T"][b, 3], [0, 0, 0, 1])
            if status & (U.TOO_FEW | U.SINGULAR):
                bits = (U.step_plane(T, src, tgt, nrm, e["nn"]) if plane else U.step_point(T, src, tgt, e["nn"]))[1]
                assert bits == status & (U.TOO_FEW | U.SINGULAR)
    for s in range(steps + 1, iterations + 1):   # rows after the stop repeat it
        assert np.array_equal(out["trace_T"][s, b], out["trace_T"][steps, b])
        assert np.array_equal(out["trace_stat"][s, b], out["trace_stat"][steps, b])


def same_pair(a, ia, b, ib):
    for k in KEYS:
        x, y = (a[k][ia], b[k][ib]) if a[k].ndim == 1 or k == "T" else (a[k][:, ia], b[k][:, ib])
        assert np.array_equal(x, y, equal_nan=True), k
    assert np.array_equal(a["nn"][ia], b["nn"][ib])


# ---------------------------------------------------------------------------------------------------- replay and chain
@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("name", ["room_a", "n255", "n256", "n257"])
def test_step_replay_and_chain(name, plane):
    """Every GPU step against the float64 single step from the GPU's own state; on these chain-stable fixtures the stop, the status and
    the final transform are the restatement's too.  255 / 256 / 257 source points: the match kernel's block and the update stride."""
    p = pair_of(name)
    out = run([p], plane, iterations=U.ITERATIONS)
    replay(out, 0, p, plane)
    ref = U.reference(name, plane)
    assert int(out["steps"][0]) == ref["steps"] and int(out["status"][0]) == ref["status"] == U.CONVERGED
    assert int(out["n_corr"][0]) == ref["n_corr"] and np.array_equal(out["nn"][0], ref["nn"])
    assert np.abs(out["T"][0] - ref["T"]).max() <= T_TOL


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_every_step_runs_with_zero_tolerances(plane):
    p = pair_of("room_b")
    out = run([p], plane, iterations=8, rel_fitness=0.0, rel_rmse=0.0)
    assert int(out["steps"][0]) == 8 and int(out["status"][0]) == 0
    replay(out, 0, p, plane, iterations=8)


# ---------------------------------------------------------------------------------------------------- existing code
def test_zero_iterations_is_the_pair_ground_truth_search():
    from roitr_amd.pairgt import pair_ground_truth
    pairs = [pair_of("room_a"), pair_of("n257"), pair_of("room_c")]
    out = run(pairs, False, iterations=0)
    cat = lambda k: torch.from_numpy(np.concatenate([p[k] for p in pairs])).cuda()
    so, to = (np.cumsum([len(p[k]) for p in pairs]).astype(np.int32).tolist() for k in ("src", "tgt"))
    T0 = np.stack([p["T0"] for p in pairs]).astype(np.float32)
    gt = pair_ground_truth(cat("src"), so, cat("tgt"), to, torch.from_numpy(T0[:, :3, :3].copy()).cuda(),
                           torch.from_numpy(T0[:, :3, 3].copy()).cuda(), U.MAX_DIST, both_sides=False)
    assert np.array_equal(out["T"], T0) and not out["steps"].any() and not out["status"].any()
    assert np.array_equal(np.concatenate(out["nn"]), gt.nn_idx.cpu().numpy())
    assert np.array_equal(out["n_corr"], gt.n_src_hit.cpu().numpy())
    d2 = np.split(gt.nn_dist2.cpu().numpy(), so[:-1])
    for b in range(len(pairs)):
        total = d2[b][np.isfinite(d2[b])].sum()
        assert abs(out["rmse"][b] ** 2 * out["n_corr"][b] - total) <= 1e-9 * total
        assert out["fitness"][b] == out["n_corr"][b] / len(pairs[b]["src"])


# ---------------------------------------------------------------------------------------------------- shapes
def tiny_pair(n_src, m=None, seed=0):
    """n_src source points that are exact copies of target points of a noise-free room under T_gt, a start 1 degree / 1 cm off."""
    f = U.make_fixture(20 + seed, n_src=8, n_tgt=60 if m is None else m, noise=0.0, outliers=0.0)
    Tg = f["T_gt"]
    sel = np.arange(n_src) % len(f["tgt"])
    src = ((f["tgt"][sel].astype(np.float64) - Tg[:3, 3]) @ Tg[:3, :3]).astype(np.float32)
    T0 = U.euler_pose(1.0, (0.01, -0.01, 0.01)) @ Tg
    T0[:3] = U.as_state(T0)
    return dict(src=src, tgt=f["tgt"], normals=f["normals"], T0=T0)


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("n_src", [1, 2, 3, 5, 6, 7])
def test_few_source_points(n_src, plane):
    """Around the TOO_FEW limits (3 and 6 matched points): below them the pair stops at s = 0 with its start; from them on it steps
    (the 6 x 6 systems of this fixture have condition numbers below 1e5, its triangles are not degenerate)."""
    p = tiny_pair(n_src)
    out = run([p], plane, iterations=3, rel_fitness=0.0, rel_rmse=0.0)
    few = n_src < (6 if plane else 3)
    replay(out, 0, p, plane, iterations=3)
    assert out["trace_stat"][0, 0, 0] == 1.0      # every point has a match at the start
    if few:
        assert int(out["status"][0]) == U.TOO_FEW and int(out["steps"][0]) == 0 and int(out["n_corr"][0]) == n_src
        assert np.array_equal(out["T"][0, :3], p["T0"][:3].astype(np.float32))
    else:
        assert int(out["status"][0]) == 0 and int(out["steps"][0]) == 3


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_single_target_point(plane):
    """m = 1: every source point matches the one target point.  Its normal is a coordinate axis, so the plane system has an exactly
    zero first pivot (SINGULAR); the rigid solve of a zero cross-covariance is arbitrary, so only the evaluations are compared."""
    p = tiny_pair(7)
    k = int(np.flatnonzero(np.abs(p["normals"]).max(1) == 1.0)[0])
    p = dict(p, tgt=p["tgt"][k:k + 1], normals=p["normals"][k:k + 1])
    out = run([p], plane, iterations=2, max_dist=10.0, rel_fitness=0.0, rel_rmse=0.0)
    replay(out, 0, p, plane, max_dist=10.0, iterations=2, check_T=False)
    assert out["trace_stat"][0, 0, 0] == 1.0 and (out["nn"][0] == 0).all()
    assert (int(out["status"][0]), int(out["steps"][0])) == ((U.SINGULAR, 0) if plane else (0, 2))


@pytest.mark.parametrize("scale", [0.01, 0.3, 1.0, 3.0, 100.0])
def test_max_dist_from_a_fraction_of_a_cell_to_beyond_the_cloud(scale):
    """The grid of this 650-point target (about 6 points per occupied cell) has cells of 0.1 - 0.2 m: max_dist from a hundredth of
    that to far larger than the cloud."""
    p = pair_of("room_b")
    d = 0.1 * scale
    out = run([p], False, iterations=2, max_dist=d, rel_fitness=0.0, rel_rmse=0.0)
    replay(out, 0, p, False, max_dist=d, iterations=2)
    if scale >= 3.0:     # larger than the room: the in-range three quarters all match; at 10 m the displaced quarter does too
        assert int(out["n_corr"][0]) >= 525
    if scale == 100.0:
        assert int(out["n_corr"][0]) == 700


def test_one_large_pair():
    """About 20 000 x 20 000 points: many match blocks per pair, a grid with thousands of cells.  One update, two evaluations."""
    f = U.make_fixture(31, n_src=20011, n_tgt=19997, outliers=0.1)
    p = dict(src=f["src"], tgt=f["tgt"], normals=f["normals"], T0=f["T0"])
    out = run([p], True, iterations=1, max_dist=0.05, rel_fitness=0.0, rel_rmse=0.0)
    assert int(out["steps"][0]) == 1 and int(out["n_corr"][0]) > 15000
    replay(out, 0, p, True, max_dist=0.05, iterations=1)


# ---------------------------------------------------------------------------------------------------- batches
@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_ragged_batch(plane):
    a, c = pair_of("room_a"), pair_of("n257")
    none = lambda k: np.zeros((0, 3), np.float32)
    empty_src = dict(a, src=none(0))
    empty_tgt = dict(a, tgt=none(0), normals=none(0))
    nan = dict(c, src=c["src"].copy())
    nan["src"][5, 2] = np.nan
    far = dict(c, T0=c["T0"].copy())
    far["T0"][:3, 3] += 50.0     # nothing in range
    pairs = [a, empty_src, empty_tgt, nan, far, c]
    out = run(pairs, plane)
    assert out["status"].tolist() == [U.CONVERGED, U.EMPTY, U.EMPTY, U.NONFINITE, U.TOO_FEW, U.CONVERGED]
    for b in (1, 2, 3):   # init_T, nan, nothing else
        assert np.array_equal(out["T"][b, :3], pairs[b]["T0"][:3].astype(np.float32)) and np.array_equal(out["T"][b, 3], [0, 0, 0, 1])
        assert np.isnan(out["fitness"][b]) and np.isnan(out["rmse"][b]) and out["n_corr"][b] == 0 and out["steps"][b] == 0
        assert (out["nn"][b] == -1).all() and np.isnan(out["trace_stat"][:, b]).all()
        assert all(np.array_equal(row, out["T"][b, :3]) for row in out["trace_T"][:, b])
    assert np.array_equal(out["T"][4, :3], far["T0"][:3].astype(np.float32)) and out["steps"][4] == 0 and out["n_corr"][4] == 0
    assert out["fitness"][4] == 0.0 and out["rmse"][4] == 0.0 and (out["nn"][4] == -1).all()
    # every good pair: bitwise itself alone, in another slot, and on a repeat
    for b in (0, 5):
        same_pair(out, b, run([pairs[b]], plane), 0)
    swapped = run([c, far, a], plane)
    same_pair(out, 5, swapped, 0)
    same_pair(out, 4, swapped, 1)
    same_pair(out, 0, swapped, 2)
    again = run(pairs, plane)
    for b in range(len(pairs)):
        same_pair(out, b, again, b)
    replay(out, 0, a, plane)
    replay(out, 5, c, plane)
    for name, b in (("room_a", 0), ("n257", 5)):
        ref = U.reference(name, plane)
        assert int(out["steps"][b]) == ref["steps"] and np.abs(out["T"][b] - ref["T"]).max() <= T_TOL


def test_nonfinite_normal_and_start():
    a = pair_of("room_a")
    bad_n = dict(a, normals=a["normals"].copy())
    bad_n["normals"][7, 0] = np.inf
    bad_T = dict(a, T0=a["T0"].copy())
    bad_T["T0"][1, 3] = np.nan
    out = run([bad_n, a, bad_T], True)
    assert out["status"].tolist() == [U.NONFINITE, U.CONVERGED, U.NONFINITE]
    same_pair(out, 1, run([a], True), 0)
    assert run([bad_n], False)["status"].tolist() == [U.CONVERGED]      # the normals are not read in point-to-point mode


def test_singular_plane_system_keeps_the_state():
    """A target on one plane with equal normals (0, 0, 1): the rows of J for the in-plane motions are exactly zero, the third pivot is
    exactly 0."""
    rng = np.random.default_rng(5)
    tgt = np.concatenate([rng.uniform(0, 1, (400, 2)), np.zeros((400, 1))], 1).astype(np.float32)
    src = (tgt[:300].astype(np.float64) + [0.01, -0.02, 0.03]).astype(np.float32)
    nrm = np.zeros_like(tgt)
    nrm[:, 2] = 1.0
    p = dict(src=src, tgt=tgt, normals=nrm, T0=np.eye(4))
    out = run([p], True)
    assert int(out["status"][0]) == U.SINGULAR and int(out["steps"][0]) == 0 and int(out["n_corr"][0]) == 300
    assert np.array_equal(out["T"][0], np.eye(4, dtype=np.float32))
    replay(out, 0, p, True)
    assert int(run([p], False)["status"][0]) == U.CONVERGED     # the rigid solve has no such limit


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_freeze_after_convergence(plane):
    """A pair that converges at step k under 30 iterations equals, bitwise, the same pair stopped by iterations = k."""
    p = pair_of("room_c")
    long = run([p], plane, iterations=30)
    k = int(long["steps"][0])
    assert 2 <= k < 30 and int(long["status"][0]) == U.CONVERGED
    short = run([p], plane, iterations=k)
    assert int(short["steps"][0]) == k
    for key in ("T", "fitness", "rmse", "n_corr"):
        assert np.array_equal(long[key], short[key]), key
    assert np.array_equal(long["nn"][0], short["nn"][0])
    assert np.array_equal(long["trace_T"][:k + 1], short["trace_T"]) and np.array_equal(long["trace_stat"][:k + 1], short["trace_stat"])
    for s in range(k + 1, 31):
        assert np.array_equal(long["trace_T"][s], long["trace_T"][k]) and np.array_equal(long["trace_stat"][s], long["trace_stat"][k])


def test_exact_lattice():
    f = U.lattice_pair()
    p = dict(src=f["src"], tgt=f["tgt"], T0=U.lattice_start(f))
    out = run([p], False, max_dist=1.5 * f["h"])
    assert int(out["status"][0]) == U.CONVERGED and out["rmse"][0] < 1e-6 and np.array_equal(out["nn"][0], f["sel"])
    assert np.abs(out["T"][0] - f["T_gt"]).max() <= T_TOL
    replay(out, 0, p, False, max_dist=1.5 * f["h"])


def test_open3d_style_entry():
    from roitr_amd.icp import registration_icp
    f = U.fixture("room_a")
    T, fitness, rmse, corr = registration_icp(f["src"], f["tgt"], U.MAX_DIST, f["T0"], target_normals=f["normals"])
    ref = U.reference("room_a", True)
    assert T.shape == (4, 4) and np.abs(T.cpu().numpy() - ref["T"]).max() <= T_TOL
    assert abs(fitness - ref["fitness"]) < 1e-12 and abs(rmse - ref["rmse"]) <= STAT_TOL * ref["rmse"]
    hit = np.flatnonzero(ref["nn"] >= 0)
    assert corr.dtype == torch.int64 and np.array_equal(corr.cpu().numpy(), np.stack([hit, ref["nn"][hit]], 1))


def test_host_errors_raise_and_launch_nothing():
    from roitr_amd import _lib
    from roitr_amd.icp import icp_batch
    f = U.fixture("n255")
    src, tgt = torch.from_numpy(f["src"]).cuda(), torch.from_numpy(f["tgt"]).cuda()
    T0 = torch.from_numpy(f["T0"].astype(np.float32)).cuda().reshape(1, 4, 4)
    ok = dict(max_dist=0.1, iterations=3)
    for bad in (dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(max_dist=float("inf")), dict(iterations=-1),
                dict(rel_fitness=-1e-9), dict(rel_rmse=-1.0)):
        with pytest.raises(_lib.RoitrError):
            icp_batch(src, [255], tgt, [300], T0, **dict(ok, **bad))
    empty = torch.zeros((0,), dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.RoitrError, match="65536"):      # B = 0 through device offsets (host offsets are refused before)
        icp_batch(src, empty, tgt, empty, T0[:0], **ok)
    with pytest.raises(_lib.RoitrError, match="cumulative"):
        icp_batch(src, [200], tgt, [300], T0, **ok)
    with pytest.raises(_lib.RoitrError):
        icp_batch(src, [255], tgt, [300], T0, tgt_normals=tgt[:10], **ok)
    with pytest.raises(_lib.RoitrError):
        icp_batch(src.cpu(), [255], tgt, [300], T0, **ok)
    torch.cuda.synchronize()
    assert int(icp_batch(src, [255], tgt, [300], T0, **ok)["steps"][0]) == 3      # the device is as it was
