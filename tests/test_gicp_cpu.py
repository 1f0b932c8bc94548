"""CPU: the float64 restatement of the generalized-ICP operator (tests/gicp_util.py), the fixtures the GPU tests compare on, and the
host side of the C ABI (size query, argument refusals, the header binding, the command line)."""
import numpy as np
import pytest

import gicp_util as G
import icp_util as U


def test_fixtures_are_the_icp_fixtures_with_source_normals():
    """The replayed random stream gives the surface normals of the very points icp_util.make_fixture drew."""
    for name in ("room_a", "n257"):
        seed, kw = U.FIXTURES[name]
        f, g = U.fixture(name), G.fixture(name)
        assert all(np.array_equal(f[k], g[k]) for k in ("src", "tgt", "T_gt", "T0")) and np.array_equal(f["normals"], g["tgt_normals"])
        rng = np.random.default_rng(seed)
        _, nq = U.surface(rng, len(f["tgt"]))
        assert np.array_equal(nq.astype(np.float32), f["normals"])         # the stream is in step after the first draw ...
        p, n_p = U.surface(rng, len(f["src"]))
        keep = len(f["src"]) - int(round(0.25 * len(f["src"])))             # ... and after the second: the in-range source points lie
        back = (p[:keep] - f["T_gt"][:3, 3]) @ f["T_gt"][:3, :3]            # within the noise of the noise-free draw
        assert np.abs(back - f["src"][:keep]).max() < 0.02
        assert np.allclose(g["src_normals"], n_p @ f["T_gt"][:3, :3], atol=1e-6)
        assert np.allclose(np.linalg.norm(g["src_normals"], axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("name", sorted(G.FIXTURES))
def test_fixture_is_decided_and_chain_stable(name):
    """Zero near points, no near convergence decision, a well-conditioned system; and the chain with every state moved by up to one
    fp32 ulp keeps the matches, the step count and the status, with a final T within 1e-6."""
    r = G.reference(name)
    assert (r["near_tie"], r["near_radius"], r["near_stop"]) == (0, 0, 0) and r["cond"] < 1e6 and r["decided"]
    assert r["status"] == G.CONVERGED and 2 <= r["steps"] < G.ITERATIONS
    f = G.fixture(name)
    for seed in (0, 1):
        p = G.gicp_ref(f["src"], f["tgt"], f["T0"], f["src_normals"], f["tgt_normals"], perturb=G.ulp_perturb(seed))
        assert p["steps"] == r["steps"] and p["status"] == r["status"] and p["n_corr"] == r["n_corr"]
        assert np.array_equal(p["nn"], r["nn"])
        assert np.abs(p["T"] - r["T"]).max() < 1e-6


@pytest.mark.parametrize("name", sorted(G.FIXTURES))
def test_refinement_brings_both_errors_below_a_fifth_of_the_start(name):
    f, r = G.fixture(name), G.reference(name)
    rre0, rte0 = G.pose_error(f["T0"], f["T_gt"])
    rre, rte = G.pose_error(r["T"], f["T_gt"])
    print(f"{name}: RRE {rre0:.3f} -> {rre:.4f} deg ({rre / rre0:.3f}), RTE {rte0:.4f} -> {rte:.5f} m ({rte / rte0:.3f}), steps {r['steps']}")
    assert rre < 0.2 * rre0 and rte < 0.2 * rte0


@pytest.mark.parametrize("eps", [1e-6, 1e-3, 1.0])
def test_cofactor_inverse_equals_linalg_inv(eps):
    """Random unit normals (and zero ones: isotropic points, on one side and on both): 1e-12 relative.  Equal normals on both sides are
    the worst case the operator admits, cond(M) = 1 / eps: there NEITHER inverse is better than about cond(M) 2^-53 times a small
    constant (a handful of roundings each), so those rows are held to 16 cond(M) 2^-53 (1.8e-9 at eps = 1e-6)."""
    rng = np.random.default_rng(3)
    a, b = (G.unit(rng.normal(size=(2000, 3)).astype(np.float32)) for _ in range(2))
    a[:50], b[25:75] = 0.0, 0.0
    a[100:150] = b[100:150]
    M = G.plane_metric(a, b, eps)
    W, ref = G.cofactor_inverse(M), np.linalg.inv(M)
    rel = np.abs(W - ref).max((1, 2)) / np.abs(ref).max((1, 2))
    same = np.zeros(len(M), bool)
    same[100:150] = True
    print(f"eps {eps:g}: random / zero normals {rel[~same].max():.2e} (cond <= {np.linalg.cond(M[~same]).max():.0f}), equal normals "
          f"{rel[same].max():.2e} (cond {np.linalg.cond(M[same]).max():.3g})")
    assert rel[~same].max() < 1e-12, rel[~same].max()
    assert (rel[same] <= 16 * np.linalg.cond(M[same]) * 2.0 ** -53).all(), rel[same].max()
    assert np.array_equal(G.plane_metric(a[:1] * 0, b[:1] * 0, 1e-3), 2 * np.eye(3)[None])
    assert np.array_equal(G.plane_metric(a[200:201], b[200:201], 1.0), 2 * np.eye(3)[None])


def test_epsilon_one_converges_to_kabsch_on_fixed_matches():
    """eps = 1: M = 2I, the objective is half the point-to-point one, so Gauss-Newton on fixed matches ends on the rigid solve.  The
    state is kept in float64 (exact_state): rounded to fp32 after every step, as the operator does, it cannot come closer than 1e-7."""
    f = G.fixture("n256")
    args = (f["src"], f["tgt"], f["src_normals"], f["tgt_normals"])
    nn = U.evaluate(f["T0"], f["src"], f["tgt"], G.MAX_DIST)["nn"]
    T = np.asarray(f["T0"], np.float64)[:3].copy()
    u, _, vt = np.linalg.svd(T[:, :3])     # T0 holds fp32 values: its rotation is orthonormal to 3e-8 only, and a product of exact
    T[:, :3] = u @ vt                      # rotations in front of it keeps that defect; start from the nearest rotation instead
    for _ in range(8):
        T, bits = G.step_gicp(T, *args, nn, 1.0, exact_state=True)
        assert bits == 0
    hit = nn >= 0
    want = U.kabsch(f["src"].astype(np.float64)[hit], f["tgt"].astype(np.float64)[nn[hit]])
    assert np.abs(T - want).max() < 1e-9, np.abs(T - want).max()
    rounded = U.as_state(f["T0"])
    for _ in range(8):
        rounded, bits = G.step_gicp(rounded, *args, nn, 1.0)
    assert np.abs(rounded - want).max() < 1e-6


def test_one_step_lowers_the_objective_on_fixed_matches():
    for name in ("room_a", "n257"):
        f = G.fixture(name)
        args = (f["src"], f["tgt"], f["src_normals"], f["tgt_normals"])
        nn = U.evaluate(f["T0"], f["src"], f["tgt"], G.MAX_DIST)["nn"]
        Tn, bits = G.step_gicp(f["T0"], *args, nn)
        assert bits == 0
        before, after = G.gicp_system(f["T0"], *args, nn)[2], G.gicp_system(Tn, *args, nn)[2]     # the same matches
        assert after < 0.5 * before, (before, after)


def test_step_status_bits_of_the_restatement():
    f = G.fixture("room_a")
    args = (f["src"], f["tgt"], f["src_normals"], f["tgt_normals"])
    nn = np.full(len(f["src"]), -1, np.int32)
    nn[:5] = 0
    assert G.step_gicp(f["T0"], *args, nn)[1] == G.TOO_FEW
    nn[:6] = np.arange(6)
    assert G.step_gicp(f["T0"], *args, nn)[1] == 0
    # points on the x axis, isotropic: A[0][0] = sum (py^2 + pz^2) / 2 = 0 exactly
    line = np.zeros((8, 3), np.float32)
    line[:, 0] = np.arange(8) * 0.25
    zero = np.zeros_like(line)
    assert G.step_gicp(np.eye(4), line, line, zero, zero, np.arange(8, dtype=np.int32))[1] == G.SINGULAR
    bad = f["src_normals"].copy()
    bad[3, 1] = np.nan
    assert G.gicp_ref(f["src"], f["tgt"], f["T0"], bad, f["tgt_normals"])["status"] == G.NONFINITE
    bad_t = f["tgt_normals"].copy()
    bad_t[0, 0] = np.inf
    assert G.gicp_ref(f["src"], f["tgt"], f["T0"], f["src_normals"], bad_t)["status"] == G.NONFINITE
    assert G.gicp_ref(f["src"][:0], f["tgt"], f["T0"], f["src_normals"][:0], f["tgt_normals"])["status"] == G.EMPTY


def _bound():
    from roitr_amd import gicp
    return gicp._lib()


def test_prototypes_resolve_through_bind():
    import ctypes
    from roitr_amd import _lib
    I, F, D, P = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
    lib = _bound()
    protos = _lib.header_prototypes()
    assert protos["roitr_gicp_workspace_bytes"] == (ctypes.c_size_t, [I] * 4)
    ret, args = protos["roitr_gicp_batch"]
    assert ret is I and args == [I, I, I] + [P] * 7 + [F, D, I, D, D] + [P] * 12
    assert lib.roitr_gicp_batch.argtypes == args and lib.roitr_gicp_workspace_bytes.restype is ctypes.c_size_t
    assert lib.roitr_gicp_workspace_bytes.argtypes == [I] * 4
    assert "roitr_gicp_batch" not in _lib.BOUND and lib.roitr_abi_version() == 4


def test_workspace_bytes_is_host_only_and_monotone():
    lib = _bound()
    size = lib.roitr_gicp_workspace_bytes
    base = (2, 1000, 900, 30)
    assert size(*base) > 1000 * 12 + 900 * 12 + lib.roitr_knn_workspace_bytes(2, 900, 0)
    for k in range(4):
        bigger = list(base)
        bigger[k] = bigger[k] * 2 + 1
        assert size(*bigger) >= size(*base), k
    assert size(3, 1000, 900, 30) > size(*base) and size(2, 2000, 900, 30) > size(*base) and size(2, 1000, 1800, 30) > size(*base)
    assert size(0, 10, 10, 1) == 0 and size(1, -1, 10, 1) == 0 and size(1, 10, 10, -1) == 0


def test_host_side_errors_launch_nothing():
    """epsilon, the normals' pointers and the ICP operator's checks are made before anything touches a device."""
    import ctypes
    lib = _bound()
    one = ctypes.c_void_p(256)   # never dereferenced

    def call(b=1, max_dist=0.1, eps=1e-3, iterations=5, rf=1e-6, rr=1e-6, T=one, status=one, ws=one, init=one, so=one, ns=one, nt=one):
        return lib.roitr_gicp_batch(b, 4, 4, one, so, one, one, ns, nt, init, max_dist, eps, iterations, rf, rr, T, None, None, None, None,
                                    None, status, None, None, None, ws, None)
    for bad in (0.0, 0.99e-6, 1.0000001, -1e-3, float("nan"), float("inf")):
        assert call(eps=bad) == 1, bad
    assert b"epsilon" in lib.roitr_last_error()
    assert call(ns=None) == 1 and b"normals" in lib.roitr_last_error()
    assert call(nt=None) == 1 and b"normals" in lib.roitr_last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(max_dist=bad) == 1
    assert b"max_dist" in lib.roitr_last_error()
    assert call(iterations=-1) == 1 and call(rf=-1e-9) == 1 and call(rr=-1.0) == 1 and call(rf=float("nan")) == 1
    assert call(b=0) == 1 and call(b=65537) == 1
    assert call(T=None) == 1 and call(status=None) == 1 and call(ws=None) == 1 and call(init=None) == 1 and call(so=None) == 1
    assert b"null" in lib.roitr_last_error()


def test_wrappers_have_no_cpu_fallback_and_check_their_arguments():
    import torch
    from roitr_amd import _lib, gicp
    x = torch.zeros(8, 3)
    with pytest.raises(_lib.RoitrError):
        gicp.gicp_batch(x, [8], x, [8], torch.eye(4).reshape(1, 4, 4), src_normals=x, tgt_normals=x)
    with pytest.raises(TypeError):       # the normals are required keyword arguments
        gicp.gicp_batch(x, [8], x, [8], torch.eye(4).reshape(1, 4, 4))
    assert (gicp.NONFINITE, gicp.EMPTY, gicp.TOO_FEW, gicp.SINGULAR, gicp.CONVERGED) == (1, 2, 4, 8, 16)


def test_parser_accepts_the_gicp_mode():
    from roitr_amd.main import parser
    args = parser().parse_args(["cfg.yaml", "--refine", "gicp", "--gicp-epsilon", "0.01"])
    assert args.refine == "gicp" and args.gicp_epsilon == 0.01
    assert parser().parse_args(["cfg.yaml"]).gicp_epsilon == 1e-3 and parser().parse_args(["cfg.yaml", "--refine", "plane"]).refine == "plane"
    with pytest.raises(SystemExit):
        parser().parse_args(["cfg.yaml", "--refine", "colored"])


def test_other_modes_do_not_import_the_module():
    """A fresh interpreter (this one has imported gicp.py already): the Tester with refine='plane' and the command line leave it out."""
    import os
    import subprocess
    import sys
    code = ("import sys; from roitr_amd.tester import Tester; import roitr_amd.main, roitr_amd.icp; "
            "Tester({'benchmark': '3DMatch'}, None, [], refine='plane'); sys.exit(int('roitr_amd.gicp' in sys.modules))")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0


def test_tester_accepts_gicp_and_refuses_other_strings():
    from roitr_amd.tester import Tester
    t = Tester({"benchmark": "3DMatch"}, None, [], refine="gicp", icp=dict(epsilon=1e-2))
    assert t.refine == "gicp" and t.icp == dict(epsilon=1e-2) and t.refinement == {} and t.register
    with pytest.raises(ValueError):
        Tester({"benchmark": "3DMatch"}, None, [], refine="colored")
