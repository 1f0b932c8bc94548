"""GPU: multiway registration (roitr_amd/posegraph.py, csrc/posegraph.hip) against the float64 restatement of tests/posegraph_util.py.

edge_information: the inlier count against roitr_lgr_batch's own (bitwise), the matrix within 1e-12 of the magnitude of the terms each
entry adds up, pairs of 0, 1, 255 ... 257 and 5000 rows, and bitwise independence of batch, slot, row offset and repeats.

pose_graph_batch: EVERY solve is replayed by the restatement from the GPU's own trace (the state before the solve and its lambda), so
no difference accumulates: delta, F, rho and lambda must lie within 8 x the deviation between the restatement's two solve paths on the
same fixture (posegraph_util.two_solver_deviation; the margin the losses row uses); the accepted flags, steps, solves, pruned and
status are exact; the poses within 1e-5, the fp32 output bound of rows f10 to f15.  Every test prints its figures before it asserts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posegraph_util as U  # noqa: E402

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def run(graphs, **kw):
    """pose_graph_batch of a list of scenes (the first scene's mu for all unless given); everything back on the host as numpy."""
    from roitr_amd import posegraph as PG
    b = U.batch(graphs)
    kw.setdefault("mu", graphs[0].get("mu", 0.5))
    out = PG.pose_graph_batch(b["node_starts"], b["edge_starts"], b["edge_i"], b["edge_j"], b["edge_T"], b["edge_info"], b["edge_uncertain"],
                              b["init_poses"], **kw)
    _torch().cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, b


def scene_slice(out, b, s):
    """Scene s's part of every output of a batch, as a dict of arrays."""
    n0, n1, e0, e1 = b["node_starts"][s], b["node_starts"][s + 1], b["edge_starts"][s], b["edge_starts"][s + 1]
    per = dict(poses=(n0, n1), trace_poses=(n0, n1), trace_delta=(n0, n1), line_weight=(e0, e1), pruned=(e0, e1))
    return {k: (v[per[k][0]:per[k][1]] if k in per else v[s]) for k, v in out.items()}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------------ edge information
ROWS = (0, 1, 255, 256, 257, 5000)


def _pairs():
    rng = np.random.default_rng(7)
    srcs, tgts, Ts = [], [], []
    for k, n in enumerate(ROWS):
        T = U.rigid(rng, 0.7, 1.0)
        src = rng.uniform(-1.5, 1.5, size=(n, 3))
        tgt = src @ T[:3, :3].T + T[:3, 3] + rng.normal(size=(n, 3)) * 0.06   # about half the rows within 0.1
        srcs.append(src.astype(np.float32)); tgts.append(tgt.astype(np.float32)); Ts.append(T.astype(np.float32))
    return srcs, tgts, Ts


def _edge_info(srcs, tgts, Ts, lead=0):
    """edge_information of the pairs in one call, `lead` rows of padding in front of the first."""
    from roitr_amd import posegraph as PG
    pad = np.full((lead, 3), 9.0, np.float32)
    starts = lead + np.concatenate([[0], np.cumsum([len(s) for s in srcs])])
    out = PG.edge_information(starts.astype(np.int32), np.concatenate([pad] + srcs), np.concatenate([pad] + tgts), np.stack(Ts), radius=0.1)
    return out["info"].cpu().numpy(), out["n_inlier"].cpu().numpy()


def test_edge_information_against_the_restatement_and_lgr():
    from roitr_amd import lgr
    srcs, tgts, Ts = _pairs()
    info, cnt = _edge_info(srcs, tgts, Ts)
    for b, n in enumerate(ROWS):
        ref, ref_cnt = U.edge_information(srcs[b], Ts[b], tgts[b], 0.1)
        d2 = ((srcs[b].astype(np.float64) @ Ts[b][:3, :3].astype(np.float64).T + Ts[b][:3, 3] - tgts[b]) ** 2).sum(1)
        inl = d2 < np.float64(np.float32(0.1) * np.float32(0.1))
        scale = U.information_abs_terms(srcs[b][inl])
        err = np.abs(info[b] - U.information_from_points(srcs[b][inl].astype(np.float64)))
        print(f"rows {n}: inliers {cnt[b]} (restatement {ref_cnt}, float64 {int(inl.sum())}), worst error / term magnitude "
              f"{float((err / np.maximum(scale, 1e-300)).max()) if n else 0.0:.2e}, bitwise as the restatement: {same_bits(info[b], ref)}")
        assert cnt[b] == ref_cnt
        if int(inl.sum()) == ref_cnt:   # no row sits within fp32 rounding of the radius: the float64 set is the fp32 set
            assert (err <= 1e-12 * scale).all()
        assert (np.abs(info[b] - ref) <= 1e-12 * np.maximum(scale, np.abs(ref))).all()
        assert info[b][3, 3] == info[b][4, 4] == info[b][5, 5] == cnt[b]
    assert cnt[0] == 0 and not info[0].any() and 1500 < cnt[5] < 4000
    # LGR's own pose and count: rows in patches of 32
    sizes = [len(s) for s in srcs]
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    patch = np.concatenate([np.arange(n) // 32 for n in sizes]).astype(np.int32)
    r = lgr.lgr_batch(starts, np.concatenate(srcs), np.concatenate(tgts), None, patch, radius=0.1)
    from roitr_amd import posegraph as PG
    e = PG.edge_information(starts, np.concatenate(srcs), np.concatenate(tgts), r["T"], radius=0.1)
    print("LGR inliers", r["inliers"].cpu().numpy(), "edge_information", e["n_inlier"].cpu().numpy())
    assert same_bits(r["inliers"].cpu().numpy(), e["n_inlier"].cpu().numpy())


def test_edge_information_does_not_depend_on_batch_slot_offset_or_repeat():
    srcs, tgts, Ts = _pairs()
    info, cnt = _edge_info(srcs, tgts, Ts)
    again = _edge_info(srcs, tgts, Ts)
    assert same_bits(info, again[0]) and same_bits(cnt, again[1])
    order = [5, 2, 0, 4, 1, 3]
    i2, c2 = _edge_info([srcs[k] for k in order], [tgts[k] for k in order], [Ts[k] for k in order], lead=77)
    for slot, k in enumerate(order):
        assert same_bits(info[k], i2[slot]) and cnt[k] == c2[slot]
        alone = _edge_info([srcs[k]], [tgts[k]], [Ts[k]], lead=3)
        assert same_bits(info[k], alone[0][0]) and cnt[k] == alone[1][0]


# ------------------------------------------------------------------------------------------------------------------ pose graph
def replay(name, g, oa, ref, dev):
    """One scene on the GPU with its traces, every solve replayed by the restatement; prints the figures, then asserts."""
    out, _ = run([g], return_trace=True, **oa)
    solves, iters = int(out["solves"][0]), oa["iterations"]
    tr, tp, td = out["trace_scalars"][0], out["trace_poses"], out["trace_delta"]
    worst = dict(delta=0.0, F=0.0, rho=0.0, lam=0.0)
    den_excess = 0.0                       # the denominator of rho against its own bound, as a ratio
    flags_gpu, flags_ref = [], []
    lam_want, nu = None, 2.0
    X_final = U.states(g["init_poses"])    # the state the call ends in, as the replay follows it
    for s in range(solves):
        X, lam = np.ascontiguousarray(tp[:, s, :]), float(tr[s, 1])
        X_final = X
        r = U.solve_once(X, g, g["mu"], lam)
        if lam_want is None:
            lam_want = 1e-3 * np.max(np.diag(r["H"]))   # tau's default
        worst["lam"] = max(worst["lam"], abs(lam - lam_want) / lam_want)
        worst["F"] = max(worst["F"], abs(tr[s, 0] - r["F"]))
        assert tr[s, 7] == 1.0
        if r["delta"] is None:
            break
        worst["delta"] = max(worst["delta"], float(np.abs(td[1:, s, :].reshape(-1) - r["delta"]).max()), abs(tr[s, 3] - r["maxd"]))
        # sum_q delta_q (lambda delta_q - b_q): what 8 x the deviation of delta moves it by, plus 8 units in the last place of its terms
        d, b = r["delta"], r["b"]
        den_bound = 8 * dev["delta"] * np.abs(2 * lam * d - b).sum() + 8 * U.EPS * np.abs(d * (lam * d - b)).sum()
        den_excess = max(den_excess, abs(tr[s, 6] - r["den"]) / den_bound)
        assert not td[0, s].any()
        if r["maxd"] < oa["step_tol"]:
            assert s == solves - 1 and tr[s, 4] == 0.0 and tr[s, 2] == 0.0 and tr[s, 5] == 0.0
            break
        worst["rho"] = max(worst["rho"], abs(tr[s, 2] - r["rho"]))
        worst["F"] = max(worst["F"], abs(tr[s, 5] - r["Fn"]))          # F' of the trial state
        lam_want, nu, acc = U.damping_update(lam, nu, r["rho"])
        flags_gpu.append(int(tr[s, 4])); flags_ref.append(int(acc))
        if acc:
            X_final = r["Xn"]
    # what the call leaves behind: the damping after the last solve, the objective and the line weights of the final state
    lam_err = abs(out["lambda_out"][0] - lam_want) / lam_want
    F_final, l_final = U.objective(X_final, g, g["mu"])
    F_err = abs(out["objective"][0] - F_final)
    print(f"{name}: lambda_out {lam_err:.3g} (relative) / {8 * dev['lam']:.3g}, objective {F_err:.3g} / {8 * dev['F']:.3g}, "
          f"denominator of rho at most {den_excess:.3g} of its bound")
    print(f"{name}: {solves} solves, {int(out['steps'][0])} accepted, status {int(out['status'][0])}; worst difference over the solves / "
          f"8 x two-solver deviation: " + ", ".join(f"{k} {worst[k]:.3g} / {8 * dev[k]:.3g}" for k in worst))
    pose_err = float(np.abs(out["poses"].astype(np.float64) - ref["poses"].astype(np.float64)).max())
    print(f"{name}: poses against the restatement's run {pose_err:.3g} (bound 1e-5); lambda_out {out['lambda_out'][0]:.6g} / {ref['lam']:.6g}")
    assert not tr[solves:].any() and not tp[:, solves:].any() and not td[:, solves:].any()
    assert flags_gpu == flags_ref == [int(t["accepted"]) for t in ref["trace"]][:len(flags_gpu)]
    assert (int(out["steps"][0]), solves, int(out["status"][0])) == (ref["steps"], ref["solves"], ref["status"])
    assert np.array_equal(out["pruned"], ref["pruned"])
    for k in worst:
        assert worst[k] <= 8 * dev[k], (k, worst[k], dev[k])
    assert pose_err <= 1e-5
    # l_e lies in [0, 1] and is read off the final state; 1e-9 is four orders below the fp32 pose bound and eight below the distance the
    # fixtures keep from the pruning threshold (0.05, tests/test_posegraph_cpu.py)
    assert np.abs(out["line_weight"] - ref["line_weight"]).max() <= 1e-9 and np.abs(out["line_weight"] - l_final).max() <= 1e-9
    assert lam_err <= 8 * dev["lam"] and F_err <= 8 * dev["F"] and den_excess <= 1.0
    return out


@pytest.mark.parametrize("name", sorted(U.FIXTURES))
def test_every_solve_replayed_from_the_trace(name):
    """2, 5, 12 and 33 nodes from a chained start, the identity start with its rejected steps, the noise-free graph."""
    g, oa, ref, dev = U.fixture(name)
    out = replay(name, g, oa, ref, dev)
    if name == "identity12":
        assert int(out["solves"][0]) - int(out["steps"][0]) >= 1
    assert same_bits(out["poses"][0], g["init_poses"][0])   # the gauge


def test_65_nodes_in_at_most_8_solves():
    g = U.make_graph(n=65, seed=65, loops=130, wrong=0.15)
    oa = dict(iterations=8, step_tol=1e-9)
    ref, dev = U.optimise(g, g["mu"], **oa), U.two_solver_deviation(g, g["mu"], **oa)
    out = replay("chain65", g, oa, ref, dev)
    assert int(out["solves"][0]) <= 8 and int(out["steps"][0]) >= 3


def test_all_certain_edges_have_weight_one_and_zero_iterations_return_the_start():
    g, oa, _, _ = U.fixture("chain12")
    certain = dict(g, edge_uncertain=np.zeros_like(g["edge_uncertain"]))
    out, _ = run([certain], iterations=6)
    assert (out["line_weight"] == 1.0).all() and not out["pruned"].any() and int(out["steps"][0]) >= 1
    out, _ = run([g], iterations=0, return_trace=True)
    assert same_bits(out["poses"], g["init_poses"]) and int(out["solves"][0]) == int(out["steps"][0]) == int(out["status"][0]) == 0
    F, l = U.objective(U.states(g["init_poses"]), g, g["mu"])
    print("objective at the start", out["objective"][0], F)
    assert abs(out["objective"][0] - F) <= 1e-12 * abs(F) and out["trace_scalars"].shape == (1, 0, 8)


def test_line_process_weight_is_open3d_rule_on_the_device():
    """preference * max_dist^2 * the mean of info[5][5] over the uncertain edges, against numpy."""
    import torch
    from roitr_amd import posegraph as PG
    g = U.fixture("chain12")[0]
    info, unc = torch.from_numpy(g["edge_info"]).cuda(), torch.from_numpy(g["edge_uncertain"]).cuda()
    info[:, 5, 5] += torch.arange(len(unc), device="cuda", dtype=torch.float64)      # the counts differ from edge to edge
    info[:, 4, 4] += 1000.0                                                            # and from the other diagonal entries
    got = PG.line_process_weight(info, unc, 0.05, 2.0)
    want = 2.0 * 0.05 ** 2 * info.cpu().numpy()[g["edge_uncertain"] != 0, 5, 5].mean()
    print("line_process_weight", float(got), want)
    assert got.is_cuda and got.dtype == torch.float64 and abs(float(got) - want) <= 1e-12 * want
    assert abs(g["mu"] - float(PG.line_process_weight(torch.from_numpy(g["edge_info"]).cuda(), unc, 0.05, 1.0))) <= 1e-12 * g["mu"]


def _ragged():
    """Live scenes of 2, 5, 12 and 33 nodes with a ONE_NODE, a NO_EDGES and a BAD_EDGE scene between them."""
    live = [U.fixture(k)[0] for k in ("chain5", "chain2", "chain33", "chain12")]
    one = U.make_graph(n=1, seed=1, loops=0)
    none = U.make_graph(n=4, seed=4, loops=3)
    none = dict(none, **{k: none[k][:0] for k in ("edge_i", "edge_j", "edge_T", "edge_info", "edge_uncertain")})
    bad = U.make_graph(n=5, seed=55, loops=6)
    bad = dict(bad, edge_j=bad["edge_j"].copy())
    bad["edge_j"][3] = 5
    bad2 = dict(bad, edge_j=bad["edge_j"].copy())
    bad2["edge_j"][3] = bad2["edge_i"][3]
    return [live[0], one, live[1], none, live[2], bad, bad2, live[3]], (1, 3, 5, 6), (U.ONE_NODE, U.NO_EDGES, U.BAD_EDGE, U.BAD_EDGE)


def test_ragged_batch_with_status_scenes_and_bitwise_invariance():
    scenes, dead, bits = _ragged()
    kw = dict(mu=0.5, iterations=12, step_tol=1e-6, return_trace=True)
    out, b = run(scenes, **kw)
    again, _ = run(scenes, **kw)
    for k in out:
        assert same_bits(out[k], again[k]), k
    for s, bit in zip(dead, bits):
        sc = scene_slice(out, b, s)
        assert int(sc["status"]) == bit and same_bits(sc["poses"], scenes[s]["init_poses"].astype(np.float32).reshape(-1, 4, 4))
        assert (sc["line_weight"] == 1.0).all() and not sc["pruned"].any() and not sc["trace_scalars"].any()
        assert int(sc["steps"]) == int(sc["solves"]) == 0 and sc["objective"] == 0.0 and sc["lambda_out"] == 0.0
    # a live scene: alone, and in another slot behind other node and edge offsets, bit for bit
    order = [7, 5, 0, 1, 4, 2]
    other, b2 = run([scenes[s] for s in order], **kw)
    for slot, s in enumerate(order):
        if s in dead:
            continue
        want, alone = scene_slice(out, b, s), run([scenes[s]], **kw)
        for k in want:
            assert same_bits(np.asarray(want[k]), np.asarray(scene_slice(other, b2, slot)[k])), (s, k)
            assert same_bits(np.asarray(want[k]), np.asarray(scene_slice(alone[0], alone[1], 0)[k])), (s, k)
        assert int(want["steps"]) >= 2 and not int(want["status"]) & ~U.CONVERGED


def test_singular_scene_from_a_non_finite_information_entry():
    scenes = [U.fixture(k)[0] for k in ("chain5", "chain12", "chain2")]
    kw = dict(mu=0.5, iterations=12, step_tol=1e-6)
    clean, b = run(scenes, **kw)
    broken = dict(scenes[1], edge_info=scenes[1]["edge_info"].copy())
    broken["edge_info"][2, 1, 1] = np.inf
    out, _ = run([scenes[0], broken, scenes[2]], **kw)
    sc = scene_slice(out, b, 1)
    print("singular scene: status", int(sc["status"]), "solves", int(sc["solves"]), "steps", int(sc["steps"]))
    assert int(sc["status"]) == U.SINGULAR and int(sc["solves"]) == 1 and int(sc["steps"]) == 0
    assert same_bits(sc["poses"], scenes[1]["init_poses"])
    for s in (0, 2):
        a, c = scene_slice(out, b, s), scene_slice(clean, b, s)
        assert all(same_bits(np.asarray(a[k]), np.asarray(c[k])) for k in a)
