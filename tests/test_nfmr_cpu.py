"""CPU: the ground the NFMR GPU tests stand on -- the float64 restatement (tests/nfmr_util.py) against what the reference's
registration/evaluate_fdmatch.py computed (tests/golden/nfmr_ref.npz), the new ABI, and the non-rigid synthetic pair."""
import os

import numpy as np

import nfmr_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "nfmr_ref.npz"))


def test_float64_restatement_reproduces_the_reference_recall_exactly():
    g = golden()
    for seed in range(6):
        case = U.make_case(seed, True)
        assert U.checksum(case) == str(g[f"checksum_{seed}"]), seed   # the regenerated inputs are the ones the reference saw
        r = U.nfmr_f64(case)
        assert r["hits"] == round(float(g[f"recall_{seed}"]) * 600), seed
        assert abs(r["nfmr"] - float(g[f"recall_{seed}"])) < 1e-6
        # blend_anchor_motion itself: the reference works in fp32, the restatement in float64
        keep = ~U.ambiguous(case, r)
        assert np.array_equal(r["mask"][keep], g[f"mask_{seed}"][keep])
        assert np.abs(r["flow"] - g[f"flow_{seed}"])[keep].max() < 1e-5
        assert (~keep).sum() <= 6


def test_generator_cases_are_what_the_tests_assume():
    cases = U.twelve_cases()
    assert len(cases) == 12
    shapes = {(c["src_raw"].shape[0], c["src_corr"].shape[0], len(c["metric_index"])) for c in cases}
    assert len(shapes) >= 5                                  # differing N, C and M for the ragged batch
    for c in cases:
        assert all(c[k].dtype == np.float32 for k in U.KEYS if k != "metric_index") and c["metric_index"].dtype == np.int64
        assert max(np.abs(c[k]).max() for k in ("src_raw", "src_deformed", "src_corr", "tgt_corr")) < 4.0   # the 1e-5 bound's premise
    dup = cases[7]                                            # duplicate points in the deformed cloud
    assert len(np.unique(dup["src_deformed"], axis=0)) <= dup["src_deformed"].shape[0] - 60
    rep = cases[8]                                            # every correspondence twice
    h = rep["src_corr"].shape[0] // 2
    assert np.array_equal(rep["src_corr"][:h], rep["src_corr"][h:])
    r = U.nfmr_f64(rep)
    assert np.array_equal(r["anchor_idx"][:h], r["anchor_idx"][h:])
    assert (r["nn_idx"] < h).sum() > (r["nn_idx"] >= h).sum()   # the lower copy of a repeated anchor comes first


def test_library_exports_the_nfmr_symbols():
    import __graft_entry__ as G
    from roitr_amd import _lib
    lib = _lib.lib()
    names = G.declared_symbols()
    for n in ("roitr_nfmr_workspace_bytes", "roitr_nfmr_batch", "roitr_blend_anchor_motion"):
        assert n in names and hasattr(lib, n), n
    import ctypes
    lib.roitr_nfmr_workspace_bytes.restype = ctypes.c_size_t
    assert lib.roitr_nfmr_workspace_bytes(64, 6000 * 64, 2500 * 64) >= 6000 * 64 * 24
    assert lib.roitr_abi_version() == 4   # functions added, no struct changed


def test_nonrigid_entry_points_refuse_host_tensors():
    import pytest
    import torch
    from roitr_amd import _lib, nonrigid
    z, o = torch.zeros(8, 3), torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(_lib.RoitrError):
        nonrigid.nfmr_batch(o, z, z, o, z, z, o, torch.arange(8), torch.eye(3)[None], torch.zeros(1, 3))
    with pytest.raises(NotImplementedError):
        nonrigid.blend_anchor_motion(z.numpy(), z.numpy(), z.numpy(), knn=4)


def test_make_nonrigid_pair_contract():
    from roitr_amd.synthetic import make_nonrigid_pair, make_pair
    p = make_nonrigid_pair(1500, 1300, pair_index=3)
    assert p["src_points"].shape == p["raw_src_pcd"].shape == p["src_normals"].shape == (1500, 3)
    assert p["tgt_points"].shape == p["tgt_normals"].shape == (1300, 3)
    assert p["src_feats"].shape == (1500, 1) and p["tgt_feats"].shape == (1300, 1)
    assert p["rot"].shape == (3, 3) and p["trans"].shape == (3, 1)
    for k in set(make_pair(64)) | {"metric_index"}:
        assert k in p, k
    assert all(p[k].dtype == np.float32 for k in make_pair(64))
    move = np.linalg.norm(p["src_points"] - p["raw_src_pcd"], axis=1)
    assert 0.02 < np.median(move) and move.max() < 0.16, (np.median(move), move.max())   # a real, bounded deformation
    np.testing.assert_allclose(np.linalg.norm(p["src_normals"], axis=1), 1.0, atol=1e-5)
    s, t = p["reobserved_src"], p["reobserved_tgt"]
    assert len(s) == len(t) > 300
    warped = p["src_points"][s].astype(np.float64) @ p["rot"].astype(np.float64).T + p["trans"].astype(np.float64).T
    assert np.abs(warped - p["tgt_points"][t]).max() < 0.012       # jitter 2 mm (sigma), the DEFORMED points are re-observed
    raw_warped = p["raw_src_pcd"][s].astype(np.float64) @ p["rot"].astype(np.float64).T + p["trans"].astype(np.float64).T
    assert np.abs(raw_warped - p["tgt_points"][t]).max() > 0.03
    mi = p["metric_index"]
    assert mi.dtype == np.int64 and len(mi) == 1500 // 4 and mi.min() >= 0 and mi.max() < 1500 and len(np.unique(mi)) == len(mi)
    q = make_nonrigid_pair(1500, 1300, pair_index=3)
    assert all(np.array_equal(p[k], q[k]) for k in p)
    r = make_nonrigid_pair(1500, 1300, pair_index=4)
    assert not np.array_equal(p["src_points"], r["src_points"])
    # make_pair keeps its output (bench.py and the goldens depend on it): raw == src there
    m = make_pair(256, config=4, pair_index=1)
    assert np.array_equal(m["raw_src_pcd"], m["src_points"]) and "metric_index" not in m
