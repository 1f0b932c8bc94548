"""CPU: multiway registration without a device.  The fixtures of tests/posegraph_util.py are DECIDED (no gain ratio near 0, no final line
weight near the pruning threshold, no step near step_tol), so that the exact comparisons of tests/test_posegraph_gpu.py cannot turn
on rounding; the restatement converges and prunes what was planted; the first-order meaning of the information matrix;
info_from_redwood against the pair-ground-truth layout; the host-only workspace query and every refusal.

The deviation between the restatement's two solve paths (posegraph_util.two_solver_deviation: delta, F, rho absolute, lambda relative),
as test_two_solver_deviation_is_recorded prints it; the GPU tests allow 8 x these:
    chain2      delta 9.7e-19  F 1.2e-16  rho 2.3e-16  lambda 2.2e-16
    chain5      delta 5.9e-16  F 1.3e-15  rho 1.1e-08  lambda 2.2e-16
    chain12     delta 6.1e-16  F 3.6e-15  rho 4.6e-08  lambda 2.2e-16
    chain33     delta 7.2e-16  F 3.6e-15  rho 9.1e-10  lambda 2.2e-16
    identity12  delta 7.0e-10  F 1.2e-10  rho 7.8e-08  lambda 3.3e-08
    clean12     delta 3.6e-20  F 5.5e-16  rho 6.4e-15  lambda 2.2e-16
(lambda, and chain2's figures, sit on the floor of one unit in the last place of the quantity: there the two paths agree to the last bit.)"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairgt_util as PU  # noqa: E402
import posegraph_util as U  # noqa: E402

NAMES = sorted(U.FIXTURES)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_decided(name):
    g, oa, r, _ = U.fixture(name)
    n = len(g["init_poses"])
    assert n in (2, 5, 12, 33)
    rhos = [t["rho"] for t in r["trace"] if t["delta"] is not None and t["maxd"] >= oa["step_tol"]]
    maxd = [t["maxd"] for t in r["trace"]]
    print(name, "steps", r["steps"], "solves", r["solves"], "min |rho|", min(abs(v) for v in rhos), "max |delta|", maxd)
    assert rhos and all(abs(v) > 1e-6 for v in rhos)
    assert all(not (0.2 <= l <= 0.3) for l in r["line_weight"])
    assert all(not (oa["step_tol"] / 2 <= d <= oa["step_tol"] * 2) for d in maxd)
    assert r["status"] in (0, U.CONVERGED)


@pytest.mark.parametrize("name", [k for k in NAMES if k.startswith("chain")])
def test_chained_start_converges_and_prunes_the_wrong_edges(name):
    g, oa, r, _ = U.fixture(name)
    unc = g["edge_uncertain"] != 0
    assert r["status"] == U.CONVERGED and 2 <= r["steps"] <= 10 and all(t["accepted"] for t in r["trace"][:-1])
    assert all(t["rho"] >= 1.0 for t in r["trace"][:-1])                      # the line weights of X' only lower F' further
    assert (r["line_weight"][g["wrong"]] <= 4e-4).all() and (r["line_weight"][unc & ~g["wrong"]] >= 0.65).all()
    assert np.array_equal(r["pruned"].astype(bool), g["wrong"]) and (r["line_weight"][~unc] == 1.0).all()


def test_identity_start_rejects_steps():
    g, oa, r, _ = U.fixture("identity12")
    rejected = [t for t in r["trace"] if not t["accepted"]]
    assert len(rejected) >= 1 and r["solves"] == 60 and all(abs(t["rho"]) >= 0.01 for t in r["trace"])
    lam = [t["lam"] for t in r["trace"]]
    assert lam[1] == lam[0] * 2.0 and lam[2] == lam[1] * 4.0                  # two rejections in a row: nu = 2, then 4


def test_noise_free_graph_returns_the_planted_poses():
    """Within what its pruned edges still pull: their line weights are small, not zero.  First order: the step the system at the
    planted poses asks for, where only the wrong edges have a residual."""
    g, oa, r, _ = U.fixture("clean12")
    planted = U.states(g["planted"].astype(np.float32))
    _, _, H, b = U.linearise(planted, g, g["mu"])
    pull = float(np.abs(np.linalg.solve(H, -b)).max())
    fp32 = 2.0 ** -23 * float(np.abs(g["planted"][:, :3]).max())              # the planted poses and the output are fp32
    err = float(np.abs(r["poses"].astype(np.float64) - g["planted"]).max())
    print("deviation from the planted poses", err, "first-order pull of the pruned edges", pull, "fp32", fp32)
    assert np.array_equal(r["pruned"].astype(bool), g["wrong"]) and g["wrong"].sum() == 5
    assert err <= 2 * pull + 2 * fp32


@pytest.mark.parametrize("name", NAMES)
def test_two_solver_deviation_is_recorded(name):
    g, oa, r, dev = U.fixture(name)
    print(name, {k: float("%.2g" % v) for k, v in dev.items()})
    assert all(np.isfinite(v) and v > 0 for v in dev.values())
    assert dev["delta"] <= 1e-8 and dev["lam"] <= 1e-6                        # the two paths follow the same run


def test_ldl_against_numpy_and_a_bad_pivot():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(30, 30))
    H, b = A @ A.T + 30 * np.eye(30), rng.normal(size=30)
    x = U.ldl_solve(H, b, 0.5)
    assert np.abs(x - np.linalg.solve(H + 0.5 * np.eye(30), -b)).max() <= 1e-13
    H[4, 4] = -1.0
    assert U.ldl_solve(H, b, 0.0) is None
    H[4, 4] = np.nan
    assert U.ldl_solve(H, b, 0.0) is None


def test_block_sum_is_the_sum():
    rng = np.random.default_rng(4)
    for n in (0, 1, 255, 256, 257, 1000):
        v = rng.normal(size=n)
        assert abs(U.block_sum(v) - v.sum()) <= 1e-13 * max(1.0, np.abs(v).sum())


def test_information_matrix_first_order():
    """For a small step delta, sum |dT(delta) p - p|^2 over the points is delta^T Lambda delta up to third order."""
    rng = np.random.default_rng(5)
    p = rng.uniform(-1, 1, size=(300, 3)).astype(np.float32)
    T = np.eye(4, dtype=np.float32)
    info, n = U.edge_information(p, T, p, 0.1)
    assert n == 300 and np.abs(info - U.information_from_points(p.astype(np.float64))).max() <= 1e-12 * 600
    assert np.array_equal(info, info.T) and info[3, 3] == info[4, 4] == info[5, 5] == 300
    for scale in (1e-3, 1e-4):
        delta = rng.normal(size=6) * scale
        S = U.compose(delta[None], U.states(np.eye(4)[None]))[0].reshape(3, 4)
        moved = p.astype(np.float64) @ S[:, :3].T + S[:, 3]
        want, got = ((moved - p) ** 2).sum(), delta @ info @ delta
        print("scale", scale, "sum of squares", want, "quadratic form", got)
        assert abs(want - got) <= 10 * scale * want                           # the next order: a factor |delta| smaller


def test_info_from_redwood_against_the_pair_ground_truth_layout():
    from roitr_amd import posegraph as PG
    rng = np.random.default_rng(6)
    p = rng.uniform(-2, 2, size=(100, 3))
    red, want = PU.info_matrix(p), U.information_from_points(p)
    got = PG.info_from_redwood(red)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    import torch
    both = PG.info_from_redwood(torch.from_numpy(np.stack([red, 2 * red])))
    assert both.shape == (2, 6, 6) and np.array_equal(both[0].numpy(), got) and np.array_equal(both[1].numpy(), 2 * got)


def test_fma32_rounds_once():
    """The fp32 fused multiply-add of the restatement against exact rational arithmetic, and the case a float64 multiply-add gets
    wrong: the float64 sum lands exactly between two fp32 values although the exact sum does not."""
    from fractions import Fraction
    f = np.float32
    a, b, c = f(2.0 ** 18 + 2.0 ** -5), f(2.0 ** 18 - 2.0 ** -5), f(2.0 ** 60 + 2.0 ** 37)      # a b = 2^36 - 2^-10
    assert f(np.float64(a) * np.float64(b) + np.float64(c)) == f(2.0 ** 60 + 2.0 ** 38)          # rounded twice: up to the even value
    assert U.fma32(np.array([a]), np.array([b]), np.array([c]))[0] == c                            # rounded once: below the midpoint
    assert U.fma32(np.array([a]), np.array([-b]), np.array([-c]))[0] == -c
    rng = np.random.default_rng(8)
    x, y, z = (rng.normal(size=400).astype(f) * f(10.0) ** rng.integers(-3, 4, size=400).astype(f) for _ in range(3))
    got = U.fma32(x, y, z)
    for k in range(400):
        exact = Fraction(float(x[k])) * Fraction(float(y[k])) + Fraction(float(z[k]))
        near = f(float(exact))
        cands = (np.nextafter(near, f(-np.inf)), near, np.nextafter(near, f(np.inf)))
        best = min(cands, key=lambda v: abs(Fraction(float(v)) - exact))
        assert got[k] == best, (k, x[k], y[k], z[k])


def test_spanning_poses_follow_the_edges_by_inlier_count():
    """A 4-cloud graph with known transforms: the tree takes a cloud's edges by descending inlier count, walks an edge in either
    direction (X_i = X_j T for an edge i -> j) and leaves an unreached cloud at the identity."""
    from roitr_amd import scene as S
    rng = np.random.default_rng(9)
    X = [np.eye(4)] + [U.rigid(rng, 0.8, 1.0) for _ in range(3)]
    rel = lambda i, j: np.linalg.inv(X[j]) @ X[i]                       # cloud i into cloud j's frame
    wrong = U.rigid(rng, 1.0, 1.0)
    # cloud 1 is reached from 0 over the edge with more inliers (listed 1 -> 0), cloud 2 from 1 likewise (listed 2 -> 1), cloud 3 from 1
    pairs = [(0, 1), (1, 0), (2, 1), (1, 2), (1, 3)]
    Ts = [wrong, rel(1, 0), rel(2, 1), wrong, rel(1, 3)]
    got = S.spanning_poses(4, pairs, np.stack(Ts), [10, 50, 40, 30, 7])
    print("spanning tree error", np.abs(got - np.stack(X)).max())
    assert got.shape == (4, 4, 4) and np.abs(got - np.stack(X)).max() <= 1e-12
    # the counts of the two edges 0 - 1 the other way round: the wrong one wins, and the rest of the tree hangs on it
    got = S.spanning_poses(4, pairs, np.stack(Ts), [50, 10, 40, 30, 7])
    assert np.abs(got[1] - np.linalg.inv(wrong)).max() <= 1e-12 and np.abs(got[2] - got[1] @ rel(2, 1)).max() <= 1e-12
    assert np.abs(got[3] - got[1] @ np.linalg.inv(rel(1, 3))).max() <= 1e-12
    # breadth first: cloud 0's own edge to cloud 2 is taken before the better edge from cloud 1
    got = S.spanning_poses(3, [(0, 1), (0, 2), (2, 1)], np.stack([rel(0, 1), wrong, rel(2, 1)]), [50, 5, 40])
    assert np.abs(got[1] - X[1]).max() <= 1e-12 and np.abs(got[2] - np.linalg.inv(wrong)).max() <= 1e-12
    # ties go by list order; a cloud no edge reaches keeps the identity
    got = S.spanning_poses(4, [(0, 1), (0, 1)], np.stack([rel(0, 1), wrong]), [9, 9])
    assert np.abs(got[1] - X[1]).max() <= 1e-12 and np.array_equal(got[2], np.eye(4)) and np.array_equal(got[3], np.eye(4))


def test_uncertain_flags():
    from roitr_amd import scene as S
    pairs = [(0, 1), (2, 0), (2, 1), (3, 2)]
    assert S.uncertain_flags(pairs, "consecutive") == [0, 1, 0, 0]
    assert S.uncertain_flags(pairs, "all") == [0, 0, 0, 0] and S.uncertain_flags(pairs, "none") == [1, 1, 1, 1]
    assert S.uncertain_flags(pairs, [True, False, 0, 1]) == [0, 1, 1, 0]
    with pytest.raises(ValueError):
        S.uncertain_flags(pairs, [True])
    with pytest.raises(KeyError):
        S.uncertain_flags(pairs, "some")


# ------------------------------------------------------------------------------------------------------------------ host-only entry points
def _arr(v):
    return (ctypes.c_int * len(v))(*v)


def _lib():
    from roitr_amd import posegraph as PG
    return PG._lib()


def test_workspace_query_is_host_only():
    from roitr_amd import posegraph as PG
    lib = _lib()
    one = lib.roitr_pose_graph_workspace_bytes(1, _arr([0, 60]), _arr([0, 400]))
    u = 6 * 59
    assert one >= 8 * (u * u + 139 * 400) and one % 256 == 0
    assert one == PG.workspace_bytes([0, 60], [0, 400])
    two = lib.roitr_pose_graph_workspace_bytes(2, _arr([0, 60, 120]), _arr([0, 400, 800]))
    assert two == 2 * (one - 256) + 256                                       # a slice per scene behind one table of offsets
    assert lib.roitr_pose_graph_workspace_bytes(3, _arr([0, 1, 3, 3]), _arr([0, 0, 1, 1])) > 0
    assert lib.roitr_pose_graph_workspace_bytes(1, _arr([0, 256]), _arr([0, 0])) >= 8 * 1530 * 1530
    for bad in ((0, [0], [0]), (1, [0, 257], [0, 1]), (1, [1, 2], [0, 1]), (1, [0, 2], [0, -1]), (2, [0, 5, 3], [0, 1, 2]), (70000, [0] * 70001, [0] * 70001)):
        assert lib.roitr_pose_graph_workspace_bytes(bad[0], _arr(bad[1]), _arr(bad[2])) == 0, bad
    assert lib.roitr_pose_graph_workspace_bytes(1, None, _arr([0, 1])) == 0


def _call(lib, **over):
    """roitr_pose_graph_batch with pointers that are never dereferenced (every case here is refused before a launch)."""
    p = ctypes.c_void_p(256)
    a = dict(scenes=1, node_starts=p, edge_starts=p, node_starts_host=_arr([0, 3]), edge_starts_host=_arr([0, 2]), edge_i=p, edge_j=p,
             edge_T=p, edge_info=p, edge_uncertain=p, init_poses=p, mu=0.5, tau=1e-3, step_tol=1e-6, prune_threshold=0.25,
             iterations=10, workspace=p, workspace_bytes=1 << 30, poses=p, line_weight=p, pruned=p, steps=p, solves=p, objective=p,
             lambda_out=p, status=p, trace_scalars=None, trace_poses=None, trace_delta=None, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return lib.roitr_pose_graph_batch(*a.values())


REFUSED = [dict(mu=0.0), dict(mu=float("nan")), dict(mu=float("inf")), dict(tau=0.0), dict(tau=float("inf")), dict(step_tol=-1.0),
           dict(step_tol=float("nan")), dict(prune_threshold=1.5), dict(prune_threshold=-0.1), dict(iterations=-1), dict(iterations=1025),
           dict(scenes=65536), dict(workspace_bytes=1024), dict(workspace=None)] + \
          [{k: None} for k in ("node_starts", "edge_starts", "node_starts_host", "edge_starts_host", "edge_i", "edge_j", "edge_T", "edge_info",
                               "edge_uncertain", "init_poses", "poses", "line_weight", "pruned", "steps", "solves", "objective",
                               "lambda_out", "status")]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_pose_graph_refusals(case):
    lib = _lib()
    assert _call(lib, **case) == 1                                            # ROITR_ERR_ARG, nothing launched
    assert b"roitr_pose_graph_batch" in lib.roitr_last_error()


def test_pose_graph_refuses_bad_host_counts_and_accepts_an_empty_batch():
    lib = _lib()
    assert _call(lib, node_starts_host=_arr([0, 257])) == 1                  # more than ROITR_POSEGRAPH_MAX_NODES nodes in a scene
    assert _call(lib, node_starts_host=_arr([1, 3])) == 1 and _call(lib, edge_starts_host=_arr([0, -2])) == 1
    assert _call(lib, scenes=2, node_starts_host=_arr([0, 3, 2]), edge_starts_host=_arr([0, 1, 2])) == 1
    assert _call(lib, scenes=0) == 0


def test_edge_information_refusals():
    lib, p = _lib(), ctypes.c_void_p(256)
    ok = dict(pairs=1, starts=p, total_rows=10, src=p, tgt=p, T=p, radius=0.1, info=p, n=p, stream=None)
    for over in (dict(radius=0.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(total_rows=-1), dict(pairs=65536),
                 dict(starts=None), dict(src=None), dict(tgt=None), dict(T=None), dict(info=None), dict(n=None)):
        assert lib.roitr_edge_information(*dict(ok, **over).values()) == 1, over
        assert b"roitr_edge_information" in lib.roitr_last_error()
    assert lib.roitr_edge_information(*dict(ok, pairs=0).values()) == 0


def test_module_surface():
    from roitr_amd import _lib as L, posegraph as PG
    assert len(L.BOUND) == 35 and not {"roitr_edge_information", "roitr_pose_graph_batch"} & set(L.BOUND)
    assert (PG.ONE_NODE, PG.NO_EDGES, PG.BAD_EDGE, PG.SINGULAR, PG.CONVERGED, PG.BAD_COUNTS) == (1, 2, 4, 8, 16, 32) and PG.MAX_NODES == 256
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "roitr_engine.h")).read()
    for name, value in (("MAX_NODES", 256), ("ONE_NODE", 1), ("NO_EDGES", 2), ("BAD_EDGE", 4), ("SINGULAR", 8), ("CONVERGED", 16), ("BAD_COUNTS", 32)):
        assert f"#define ROITR_POSEGRAPH_{name} {value}\n" in header
