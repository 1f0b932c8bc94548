"""GPU: roitr_gicp_batch (csrc/gicp.hip) against the float64 restatement of tests/gicp_util.py, on the fixtures tests/test_gicp_cpu.py
verifies as decided and chain-stable.

Bounds (the project's own, those of tests/test_icp_gpu.py).  Matches, counts, steps and status bits are compared exactly.  A state
against the float64 single step from the GPU's own previous state: 1e-5.  fitness / rmse / objective: 1e-9 relative (the objective is
a float64 sum of at most 2e4 positive terms, each with a relative error of a few cond(M) 2^-53 <= 1e-12 at eps = 1e-3)."""
import numpy as np
import pytest
import torch

import gicp_util as G

pytestmark = pytest.mark.gpu

T_TOL, STAT_TOL = 1e-5, 1e-9
KEYS = ("T", "fitness", "rmse", "objective", "n_corr", "steps", "status", "trace_T", "trace_stat")


def pair_of(name):
    f = G.fixture(name)
    return dict(src=f["src"], tgt=f["tgt"], src_normals=f["src_normals"], tgt_normals=f["tgt_normals"], T0=f["T0"])


def run(pairs, matches=True, trace=True, **kw):
    """gicp_batch on a list of pairs (dicts of src, tgt, src_normals, tgt_normals, T0); every output as numpy, nn_idx split per pair."""
    from roitr_amd.gicp import gicp_batch
    cat = lambda k: torch.from_numpy(np.concatenate([np.asarray(p[k], np.float32).reshape(-1, 3) for p in pairs])).cuda()
    so = np.cumsum([len(p["src"]) for p in pairs]).astype(np.int32)
    to = np.cumsum([len(p["tgt"]) for p in pairs]).astype(np.int32)
    T0 = torch.from_numpy(np.stack([np.asarray(p["T0"], np.float64) for p in pairs]).astype(np.float32)).cuda()
    kw.setdefault("max_dist", G.MAX_DIST)
    out = gicp_batch(cat("src"), so.tolist(), cat("tgt"), to.tolist(), T0, src_normals=cat("src_normals"), tgt_normals=cat("tgt_normals"),
                     return_matches=matches, return_trace=trace, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    if matches:
        out["nn"] = np.split(out.pop("nn_idx"), so[:-1])
    return out


def close(got, want):
    return abs(got - want) <= STAT_TOL * abs(want)


def replay(out, b, pair, eps=G.EPSILON, max_dist=G.MAX_DIST, iterations=G.ITERATIONS, rows=None):
    """Trace rows of pair b (all up to its stop, or those listed) against the restatement fed the GPU's own state of that row."""
    nrm = (pair["src_normals"], pair["tgt_normals"])
    src, tgt = pair["src"], pair["tgt"]
    steps, status = int(out["steps"][b]), int(out["status"][b])
    assert out["trace_T"].shape[0] == iterations + 1 and out["trace_stat"].shape[2] == 3 and 0 <= steps <= iterations
    assert np.array_equal(out["trace_T"][0, b], np.asarray(pair["T0"], np.float64)[:3].astype(np.float32))
    for s in (range(steps + 1) if rows is None else rows):
        T = out["trace_T"][s, b].astype(np.float64)
        e = G.evaluate(T, src, tgt, max_dist)
        obj = G.gicp_system(T, src, tgt, *nrm, e["nn"], eps)[2]
        fit, rmse, gobj = out["trace_stat"][s, b]
        print(f"row {s}: fitness {fit:.6f} rmse {rmse:.6e} objective {gobj:.6e} (restated {obj:.6e}, rel {abs(gobj - obj) / max(obj, 1e-300):.1e})")
        assert close(fit, e["fitness"]) and close(rmse, e["rmse"]) and close(gobj, obj), (s, fit, rmse, gobj, e["fitness"], e["rmse"], obj)
        if s < steps:
            Tn, bits = G.step_gicp(T, src, tgt, *nrm, e["nn"], eps)
            assert bits == 0, (s, bits)
            err = np.abs(out["trace_T"][s + 1, b] - Tn).max()
            print(f"row {s}: step error {err:.2e}")
            assert err <= T_TOL, (s, err)
        else:   # the row the outputs belong to
            assert int(out["n_corr"][b]) == e["n_corr"] and np.array_equal(out["nn"][b], e["nn"])
            assert out["fitness"][b] == fit and out["rmse"][b] == rmse and out["objective"][b] == gobj
            assert np.array_equal(out["T"][b, :3], out["trace_T"][s, b]) and np.array_equal(out["T"][b, 3], [0, 0, 0, 1])
            if status & (G.TOO_FEW | G.SINGULAR):
                assert G.step_gicp(T, src, tgt, *nrm, e["nn"], eps)[1] == status & (G.TOO_FEW | G.SINGULAR)
    for s in range(steps + 1, iterations + 1):   # rows after the stop repeat it
        assert np.array_equal(out["trace_T"][s, b], out["trace_T"][steps, b])
        assert np.array_equal(out["trace_stat"][s, b], out["trace_stat"][steps, b])


def same_pair(a, ia, b, ib, keys=KEYS):
    for k in keys:
        if k not in a and k not in b:
            continue
        x, y = (a[k][ia], b[k][ib]) if a[k].ndim == 1 or k == "T" else (a[k][:, ia], b[k][:, ib])
        assert np.array_equal(x, y, equal_nan=True), k
    if "nn" in a and "nn" in b:
        assert np.array_equal(a["nn"][ia], b["nn"][ib])


# ---------------------------------------------------------------------------------------------------- replay and chain
@pytest.mark.parametrize("name", ["room_a", "n255", "n256", "n257"])
def test_step_replay_and_chain(name):
    """Every GPU step against the float64 single step from the GPU's own state; on these chain-stable fixtures the stop, the status and
    the final transform are the restatement's too.  255 / 256 / 257 source points: the match kernel's block and the update stride."""
    p = pair_of(name)
    out = run([p])
    replay(out, 0, p)
    ref = G.reference(name)
    assert int(out["steps"][0]) == ref["steps"] and int(out["status"][0]) == ref["status"] == G.CONVERGED
    assert int(out["n_corr"][0]) == ref["n_corr"] and np.array_equal(out["nn"][0], ref["nn"])
    assert np.abs(out["T"][0] - ref["T"]).max() <= T_TOL


def test_every_step_runs_with_zero_tolerances():
    p = pair_of("room_b")
    out = run([p], iterations=8, rel_fitness=0.0, rel_rmse=0.0)
    assert int(out["steps"][0]) == 8 and int(out["status"][0]) == 0
    replay(out, 0, p, iterations=8)


def test_zero_iterations_is_the_pair_ground_truth_search():
    from roitr_amd.pairgt import pair_ground_truth
    pairs = [pair_of("room_a"), pair_of("n257"), pair_of("room_c")]
    out = run(pairs, iterations=0)
    cat = lambda k: torch.from_numpy(np.concatenate([p[k] for p in pairs])).cuda()
    so, to = (np.cumsum([len(p[k]) for p in pairs]).astype(np.int32).tolist() for k in ("src", "tgt"))
    T0 = np.stack([p["T0"] for p in pairs]).astype(np.float32)
    gt = pair_ground_truth(cat("src"), so, cat("tgt"), to, torch.from_numpy(T0[:, :3, :3].copy()).cuda(),
                           torch.from_numpy(T0[:, :3, 3].copy()).cuda(), G.MAX_DIST, both_sides=False)
    assert np.array_equal(out["T"], T0) and not out["steps"].any() and not out["status"].any()
    assert np.array_equal(np.concatenate(out["nn"]), gt.nn_idx.cpu().numpy())
    assert np.array_equal(out["n_corr"], gt.n_src_hit.cpu().numpy())
    d2 = np.split(gt.nn_dist2.cpu().numpy(), so[:-1])
    for b in range(len(pairs)):
        total = d2[b][np.isfinite(d2[b])].sum()
        assert abs(out["rmse"][b] ** 2 * out["n_corr"][b] - total) <= 1e-9 * total
        assert out["fitness"][b] == out["n_corr"][b] / len(pairs[b]["src"])
        replay(out, b, pairs[b], iterations=0)


# ---------------------------------------------------------------------------------------------------- isotropy
def test_exact_isotropy():
    """All-zero normals at eps = 1e-3 and arbitrary unit normals at eps = 1: M = 2I exactly in both, so every output and the whole trace
    are bitwise the same.  (Normals at eps = 1e-3 give something else: the comparison is not vacuous.)"""
    p = pair_of("n257")
    zero = dict(p, src_normals=np.zeros_like(p["src_normals"]), tgt_normals=np.zeros_like(p["tgt_normals"]))
    a = run([zero], epsilon=1e-3, iterations=6, rel_fitness=0.0, rel_rmse=0.0)
    b = run([p], epsilon=1.0, iterations=6, rel_fitness=0.0, rel_rmse=0.0)
    same_pair(a, 0, b, 0)
    assert int(a["steps"][0]) == 6
    c = run([p], epsilon=1e-3, iterations=6, rel_fitness=0.0, rel_rmse=0.0)
    assert not np.array_equal(a["trace_T"][1], c["trace_T"][1])
    # M = 2I: the objective is half the mean squared distance
    assert np.abs(a["trace_stat"][:, 0, 2] - 0.5 * a["trace_stat"][:, 0, 1] ** 2).max() <= 1e-12 * a["trace_stat"][0, 0, 2]
    replay(b, 0, p, eps=1.0, iterations=6)


# ---------------------------------------------------------------------------------------------------- shapes
def tiny_pair(n_src, seed=0):
    """n_src source points that are exact copies of target points of a noise-free room under T_gt, a start 1 degree / 1 cm off."""
    f = G.make_fixture(20 + seed, n_src=8, n_tgt=60, noise=0.0, outliers=0.0)
    Tg = f["T_gt"]
    sel = np.arange(n_src) % len(f["tgt"])
    src = ((f["tgt"][sel].astype(np.float64) - Tg[:3, 3]) @ Tg[:3, :3]).astype(np.float32)
    T0 = G.U.euler_pose(1.0, (0.01, -0.01, 0.01)) @ Tg
    T0[:3] = G.as_state(T0)
    return dict(src=src, tgt=f["tgt"], src_normals=(f["tgt_normals"][sel].astype(np.float64) @ Tg[:3, :3]).astype(np.float32),
                tgt_normals=f["tgt_normals"], T0=T0)


@pytest.mark.parametrize("n_src", [1, 5, 6, 7])
def test_few_source_points(n_src):
    """Around the TOO_FEW limit (6 matched points): below it the pair stops at s = 0 with its start; from it on it steps (six points on
    the three walls of the room: the isotropic part of the metric keeps the 6 x 6 system regular)."""
    p = tiny_pair(n_src)
    out = run([p], iterations=3, rel_fitness=0.0, rel_rmse=0.0)
    replay(out, 0, p, iterations=3)
    assert out["trace_stat"][0, 0, 0] == 1.0      # every point has a match at the start
    if n_src < 6:
        assert int(out["status"][0]) == G.TOO_FEW and int(out["steps"][0]) == 0 and int(out["n_corr"][0]) == n_src
        assert np.array_equal(out["T"][0, :3], p["T0"][:3].astype(np.float32))
    else:
        assert int(out["status"][0]) == 0 and int(out["steps"][0]) == 3


def test_exact_singular_system_keeps_the_state():
    """Eight points on the x axis at exactly representable coordinates, the target the same points, identity start, zero normals:
    W = I / 2 and A[0][0] = sum (py K20 - pz K10) = 0 exactly, the first pivot."""
    line = np.zeros((8, 3), np.float32)
    line[:, 0] = np.arange(8) * 0.25
    zero = np.zeros_like(line)
    p = dict(src=line, tgt=line.copy(), src_normals=zero, tgt_normals=zero, T0=np.eye(4))
    out = run([p], max_dist=0.1)
    assert int(out["status"][0]) == G.SINGULAR and int(out["steps"][0]) == 0 and int(out["n_corr"][0]) == 8
    assert np.array_equal(out["T"][0], np.eye(4, dtype=np.float32)) and np.array_equal(out["nn"][0], np.arange(8))
    assert out["rmse"][0] == 0.0 and out["objective"][0] == 0.0 and out["fitness"][0] == 1.0
    replay(out, 0, p, max_dist=0.1)


def test_one_large_pair():
    """About 20 000 x 20 000 points: many match blocks per pair, 79 points per thread of the update.  One update, two evaluations,
    replayed at the first and the last step."""
    f = G.make_fixture(31, n_src=20011, n_tgt=19997, outliers=0.1)
    p = dict(src=f["src"], tgt=f["tgt"], src_normals=f["src_normals"], tgt_normals=f["tgt_normals"], T0=f["T0"])
    out = run([p], iterations=1, max_dist=0.05, rel_fitness=0.0, rel_rmse=0.0)
    assert int(out["steps"][0]) == 1 and int(out["n_corr"][0]) > 15000
    replay(out, 0, p, max_dist=0.05, iterations=1, rows=(0, 1))


# ---------------------------------------------------------------------------------------------------- batches
def test_nonfinite_source_normal_flags_only_its_pair():
    a, c = pair_of("room_a"), pair_of("n256")
    bad_s = dict(a, src_normals=a["src_normals"].copy())
    bad_s["src_normals"][7, 0] = np.inf
    bad_t = dict(c, tgt_normals=c["tgt_normals"].copy())
    bad_t["tgt_normals"][299, 2] = np.nan
    out = run([bad_s, a, bad_t, c])
    assert out["status"].tolist() == [G.NONFINITE, G.CONVERGED, G.NONFINITE, G.CONVERGED]
    for b, p in ((0, bad_s), (2, bad_t)):
        assert np.array_equal(out["T"][b, :3], p["T0"][:3].astype(np.float32)) and np.array_equal(out["T"][b, 3], [0, 0, 0, 1])
        assert np.isnan(out["fitness"][b]) and np.isnan(out["rmse"][b]) and np.isnan(out["objective"][b])
        assert out["n_corr"][b] == 0 and out["steps"][b] == 0 and (out["nn"][b] == -1).all() and np.isnan(out["trace_stat"][:, b]).all()
        assert all(np.array_equal(row, out["T"][b, :3]) for row in out["trace_T"][:, b])
    same_pair(out, 1, run([a]), 0)
    same_pair(out, 3, run([c]), 0)


def test_ragged_batch():
    a, c = pair_of("room_a"), pair_of("n257")
    none = np.zeros((0, 3), np.float32)
    empty = dict(a, src=none, src_normals=none)
    far = dict(c, T0=c["T0"].copy())
    far["T0"][:3, 3] += 50.0     # nothing in range
    pairs = [a, far, empty, c]
    out = run(pairs)
    assert out["status"].tolist() == [G.CONVERGED, G.TOO_FEW, G.EMPTY, G.CONVERGED]
    assert np.isnan(out["objective"][2]) and np.isnan(out["trace_stat"][:, 2]).all() and out["n_corr"][2] == 0
    assert out["n_corr"][1] == 0 and out["objective"][1] == 0.0 and out["rmse"][1] == 0.0 and out["fitness"][1] == 0.0
    # every good pair: bitwise itself alone, in another slot, on repeats, and with the optional outputs left out
    for b in (0, 1, 3):
        same_pair(out, b, run([pairs[b]]), 0)
    swapped = run([c, a, far])
    same_pair(out, 3, swapped, 0)
    same_pair(out, 0, swapped, 1)
    same_pair(out, 1, swapped, 2)
    for _ in range(3):
        again = run(pairs)
        for b in range(len(pairs)):
            same_pair(out, b, again, b)
    bare = run(pairs, matches=False, trace=False)
    assert "nn" not in bare and "trace_T" not in bare
    for b in range(len(pairs)):
        same_pair(out, b, bare, b, keys=("T", "fitness", "rmse", "objective", "n_corr", "steps", "status"))
    replay(out, 0, a)
    replay(out, 3, c)
    for name, b in (("room_a", 0), ("n257", 3)):
        ref = G.reference(name)
        assert int(out["steps"][b]) == ref["steps"] and np.abs(out["T"][b] - ref["T"]).max() <= T_TOL


def test_freeze_after_convergence():
    """A pair that converges at step k under 30 iterations equals, bitwise, the same pair stopped by iterations = k."""
    p = pair_of("room_c")
    long = run([p], iterations=30)
    k = int(long["steps"][0])
    assert 2 <= k < 30 and int(long["status"][0]) == G.CONVERGED
    short = run([p], iterations=k)
    assert int(short["steps"][0]) == k
    for key in ("T", "fitness", "rmse", "objective", "n_corr"):
        assert np.array_equal(long[key], short[key]), key
    assert np.array_equal(long["nn"][0], short["nn"][0])
    assert np.array_equal(long["trace_T"][:k + 1], short["trace_T"]) and np.array_equal(long["trace_stat"][:k + 1], short["trace_stat"])
    for s in range(k + 1, 31):
        assert np.array_equal(long["trace_T"][s], long["trace_T"][k]) and np.array_equal(long["trace_stat"][s], long["trace_stat"][k])


# ---------------------------------------------------------------------------------------------------- entry points
def test_open3d_style_entry():
    from roitr_amd.gicp import gicp_batch, registration_generalized_icp
    from roitr_amd.prep import estimate_normals
    f = G.fixture("room_a")
    T, fitness, rmse, corr = registration_generalized_icp(f["src"], f["tgt"], G.MAX_DIST, f["T0"], source_normals=f["src_normals"],
                                                          target_normals=f["tgt_normals"])
    ref = G.reference("room_a")
    assert T.shape == (4, 4) and np.abs(T.cpu().numpy() - ref["T"]).max() <= T_TOL
    assert abs(fitness - ref["fitness"]) < 1e-12 and abs(rmse - ref["rmse"]) <= STAT_TOL * ref["rmse"]
    hit = np.flatnonzero(ref["nn"] >= 0)
    assert corr.dtype == torch.int64 and np.array_equal(corr.cpu().numpy(), np.stack([hit, ref["nn"][hit]], 1))
    # without normals: estimated with knn = 20, unoriented; the same pose as gicp_batch on those normals
    src, tgt = torch.from_numpy(f["src"]).cuda(), torch.from_numpy(f["tgt"]).cuda()
    one = lambda t: torch.tensor([len(t)], dtype=torch.int32, device="cuda")
    ns, nt = estimate_normals(src, one(src), knn=20, view_point=None), estimate_normals(tgt, one(tgt), knn=20, view_point=None)
    T0 = torch.from_numpy(f["T0"].astype(np.float32)).cuda().reshape(1, 4, 4)
    want = gicp_batch(src, [len(src)], tgt, [len(tgt)], T0, src_normals=ns, tgt_normals=nt, max_dist=G.MAX_DIST)
    T2, fit2, _, _ = registration_generalized_icp(f["src"], f["tgt"], G.MAX_DIST, f["T0"])
    assert np.abs(T2.cpu().numpy() - want["T"][0].cpu().numpy()).max() <= T_TOL and fit2 == float(want["fitness"][0])
    flipped = gicp_batch(src, [len(src)], tgt, [len(tgt)], T0, src_normals=-ns, tgt_normals=nt, max_dist=G.MAX_DIST)
    assert torch.equal(flipped["T"], want["T"])      # n n^T does not see the sign


def test_host_errors_raise_and_launch_nothing():
    from roitr_amd import _lib
    from roitr_amd.gicp import gicp_batch
    f = G.fixture("n255")
    src, tgt = torch.from_numpy(f["src"]).cuda(), torch.from_numpy(f["tgt"]).cuda()
    ns, nt = torch.from_numpy(f["src_normals"]).cuda(), torch.from_numpy(f["tgt_normals"]).cuda()
    T0 = torch.from_numpy(f["T0"].astype(np.float32)).cuda().reshape(1, 4, 4)
    ok = dict(src_normals=ns, tgt_normals=nt, max_dist=0.1, iterations=3)
    for bad in (dict(epsilon=0.0), dict(epsilon=1e-7), dict(epsilon=1.5), dict(epsilon=float("nan")), dict(max_dist=0.0),
                dict(max_dist=float("inf")), dict(iterations=-1), dict(rel_fitness=-1e-9), dict(rel_rmse=-1.0)):
        with pytest.raises(_lib.RoitrError):
            gicp_batch(src, [255], tgt, [300], T0, **dict(ok, **bad))
    with pytest.raises(_lib.RoitrError, match="cumulative"):
        gicp_batch(src, [200], tgt, [300], T0, **ok)
    with pytest.raises(_lib.RoitrError):
        gicp_batch(src, [255], tgt, [300], T0, **dict(ok, tgt_normals=nt[:10]))
    with pytest.raises(_lib.RoitrError):
        gicp_batch(src, [255], tgt, [300], T0, **dict(ok, src_normals=None))
    with pytest.raises(_lib.RoitrError):
        gicp_batch(src.cpu(), [255], tgt, [300], T0, **ok)
    torch.cuda.synchronize()
    assert int(gicp_batch(src, [255], tgt, [300], T0, **ok)["steps"][0]) == 3      # the device is as it was
