"""CPU: the float64 restatement of the ICP operator (tests/icp_util.py), the fixtures the GPU tests compare on, and the host side of
the C ABI (size query, argument refusals, the header binding)."""
import numpy as np
import pytest

import icp_util as U


@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("name", sorted(U.FIXTURES))
def test_fixture_is_decided_and_chain_stable(name, plane):
    """Zero near points, no near convergence decision, a well-conditioned system; and the chain with every state moved by up to one
    fp32 ulp stops at the same step with a final T within 1e-6."""
    r = U.reference(name, plane)
    assert (r["near_tie"], r["near_radius"], r["near_stop"]) == (0, 0, 0) and r["cond"] < 1e6 and r["decided"]
    assert r["status"] == U.CONVERGED and 2 <= r["steps"] < U.ITERATIONS
    f = U.fixture(name)
    for seed in (0, 1):
        p = U.icp_ref(f["src"], f["tgt"], f["T0"], normals=f["normals"] if plane else None, perturb=U.ulp_perturb(seed))
        assert p["steps"] == r["steps"] and p["status"] == r["status"] and p["n_corr"] == r["n_corr"]
        assert np.abs(p["T"] - r["T"]).max() < 1e-6


def test_refinement_improves_on_the_start():
    """The room fixtures: both modes end closer to the ground truth than the start, the plane mode within the noise."""
    for name in ("room_a", "room_b", "room_c"):
        f = U.fixture(name)
        start = np.abs(f["T0"] - f["T_gt"]).max()
        assert np.abs(U.reference(name, False)["T"] - f["T_gt"]).max() < start
        assert np.abs(U.reference(name, True)["T"] - f["T_gt"]).max() < 0.01 < start


@pytest.mark.parametrize("plane", [False, True])
def test_known_pose_is_recovered_on_exact_data(plane):
    """The source is an exact subset of the target under T_gt: the restatement ends on T_gt to fp32 rounding of the state."""
    f = U.make_fixture(11, noise=0.0, outliers=0.0)
    sel = np.arange(0, len(f["tgt"]), 2)
    Tg = f["T_gt"]
    src = ((f["tgt"][sel].astype(np.float64) - Tg[:3, 3]) @ Tg[:3, :3]).astype(np.float32)
    T0 = U.euler_pose(1.0, (0.01, -0.01, 0.01)) @ Tg
    r = U.icp_ref(src, f["tgt"], T0, normals=f["normals"] if plane else None)
    assert r["status"] == U.CONVERGED and r["n_corr"] == len(sel) and np.array_equal(r["nn"], sel)
    assert np.abs(r["T"] - Tg).max() < 2e-6 and r["rmse"] < 2e-6


def test_lattice_pair_is_exact():
    f = U.lattice_pair()
    T0 = U.lattice_start(f)
    r = U.icp_ref(f["src"], f["tgt"], T0, max_dist=1.5 * f["h"])
    assert r["status"] == U.CONVERGED and np.array_equal(r["nn"], f["sel"]) and r["rmse"] < 1e-6
    assert np.abs(r["T"] - f["T_gt"]).max() < 1e-5


def test_euler_convention_of_the_step():
    """x = (a, 0, 0, ...) rotates about X by a; (a, 0, g) is Rz(g) Rx(a), not Rx(a) Rz(g); the last three entries are the translation."""
    a, g = 0.3, 0.5
    M = U.vector_to_matrix(np.array([a, 0, 0, 1.0, 2.0, 3.0]))
    assert np.allclose(M[:3, :3], [[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]], atol=1e-15)
    assert np.array_equal(M[:3, 3], [1.0, 2.0, 3.0]) and np.array_equal(M[3], [0, 0, 0, 1])
    Rx, Rz = M[:3, :3], U.vector_to_matrix(np.array([0, 0, g, 0, 0, 0]))[:3, :3]
    assert np.allclose(Rz, [[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]], atol=1e-15)
    both = U.vector_to_matrix(np.array([a, 0, g, 0, 0, 0]))[:3, :3]
    # hand-written: Rz Rx sends e_y to (-sin g cos a, cos g cos a, sin a); Rx Rz would send it to (-sin g, cos a cos g, sin a cos g)
    assert np.allclose(both @ [0, 1, 0], [-np.sin(g) * np.cos(a), np.cos(g) * np.cos(a), np.sin(a)], atol=1e-15)
    assert np.allclose(both, Rz @ Rx, atol=1e-15) and np.abs(both - Rx @ Rz).max() > 0.05
    b = 0.2
    Ry = U.vector_to_matrix(np.array([0, b, 0, 0, 0, 0]))[:3, :3]
    assert np.allclose(Ry @ [0, 0, 1], [np.sin(b), 0, np.cos(b)], atol=1e-15)


def test_step_plane_reduces_the_objective():
    for name in ("room_a", "n257"):
        f = U.fixture(name)
        e = U.evaluate(f["T0"], f["src"], f["tgt"], U.MAX_DIST)
        Tn, bits = U.step_plane(f["T0"], f["src"], f["tgt"], f["normals"], e["nn"])
        assert bits == 0
        before = U.plane_objective(f["T0"], f["src"], f["tgt"], f["normals"], e["nn"])
        after = U.plane_objective(Tn, f["src"], f["tgt"], f["normals"], e["nn"])     # the same matches
        assert after < 0.5 * before


def test_step_status_bits_of_the_restatement():
    f = U.fixture("room_a")
    nn = np.full(len(f["src"]), -1, np.int32)
    nn[:2] = 0
    assert U.step_point(f["T0"], f["src"], f["tgt"], nn)[1] == U.TOO_FEW
    nn[:5] = 0
    assert U.step_point(f["T0"], f["src"], f["tgt"], nn)[1] == 0 and U.step_plane(f["T0"], f["src"], f["tgt"], f["normals"], nn)[1] == U.TOO_FEW
    flat = np.zeros_like(f["normals"])
    flat[:, 2] = 1.0     # equal normals: a rank-3 system
    e = U.evaluate(f["T0"], f["src"], f["tgt"], U.MAX_DIST)
    assert U.step_plane(f["T0"], f["src"], f["tgt"], flat, e["nn"])[1] == U.SINGULAR
    bad = f["src"].copy()
    bad[3, 1] = np.nan
    assert U.icp_ref(bad, f["tgt"], f["T0"])["status"] == U.NONFINITE
    assert U.icp_ref(bad[:0], f["tgt"], f["T0"])["status"] == U.EMPTY


def _bound():
    from roitr_amd import icp
    return icp._lib()


def test_prototypes_resolve_through_bind():
    import ctypes
    from roitr_amd import _lib
    lib = _bound()
    protos = _lib.header_prototypes()
    assert protos["roitr_icp_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    ret, args = protos["roitr_icp_batch"]
    assert ret is ctypes.c_int and len(args) == 24 and args[9] is ctypes.c_float and args[11] is ctypes.c_double
    assert lib.roitr_icp_batch.argtypes == args and lib.roitr_icp_workspace_bytes.restype is ctypes.c_size_t
    assert len(_lib.BOUND) == 35 and "roitr_icp_batch" not in _lib.BOUND and lib.roitr_abi_version() == 4


def test_workspace_bytes_is_host_only_and_monotone():
    lib = _bound()
    size = lib.roitr_icp_workspace_bytes
    base = (2, 1000, 900, 30)
    assert size(*base) > 1000 * 12 + 900 * 12 + lib.roitr_knn_workspace_bytes(2, 900, 0)
    for k in range(4):
        bigger = list(base)
        bigger[k] = bigger[k] * 2 + 1
        assert size(*bigger) >= size(*base), k
    assert size(3, 1000, 900, 30) > size(*base) and size(2, 2000, 900, 30) > size(*base) and size(2, 1000, 1800, 30) > size(*base)
    assert size(0, 10, 10, 1) == 0 and size(1, -1, 10, 1) == 0 and size(1, 10, 10, -1) == 0


def test_host_side_errors_launch_nothing():
    """max_dist, iterations, the tolerances, B and null pointers are checked before anything touches a device."""
    import ctypes
    lib = _bound()
    one = ctypes.c_void_p(256)   # never dereferenced

    def call(b=1, max_dist=0.1, iterations=5, rf=1e-6, rr=1e-6, T=one, status=one, ws=one, init=one, so=one):
        return lib.roitr_icp_batch(b, 4, 4, one, so, one, one, None, init, max_dist, iterations, rf, rr, T, None, None, None, None, status,
                                   None, None, None, ws, None)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(max_dist=bad) == 1
    assert b"max_dist" in lib.roitr_last_error()
    assert call(iterations=-1) == 1 and call(rf=-1e-9) == 1 and call(rr=-1.0) == 1 and call(rf=float("nan")) == 1
    assert call(b=0) == 1 and call(b=65537) == 1
    assert call(T=None) == 1 and call(status=None) == 1 and call(ws=None) == 1 and call(init=None) == 1 and call(so=None) == 1
    assert b"null" in lib.roitr_last_error()


def test_wrappers_have_no_cpu_fallback_and_check_their_arguments():
    import torch
    from roitr_amd import _lib, icp
    x = torch.zeros(8, 3)
    with pytest.raises(_lib.RoitrError):
        icp.icp_batch(x, [8], x, [8], torch.eye(4).reshape(1, 4, 4))
