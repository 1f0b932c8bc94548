"""GPU: fast global registration behind the engine handle, the Tester, the descriptor-matching entry point and the FPFH baseline.
Engine batches run on the closed-form selective weights, 2 pairs of 1024 points, as tests/test_compat_tester_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_PAIRS, N_POINTS = 2, 1024
FIELDS = ("T", "inliers", "n_used", "tuples_accepted", "steps", "mu", "objective", "status")
KW = dict(iterations=32, tuples=4096)     # the tuple test on, so that the keys matter
_RUN = {}


def items():
    from roitr_amd.synthetic import make_pair
    return [{k: torch.from_numpy(v) for k, v in make_pair(N_POINTS, config=1, pair_index=i).items()} for i in range(N_PAIRS)]


def engine_run(tmp_path_factory):
    """One Tester run with estimator="fgr" (one forward of both pairs), one with a pair per forward, and the same batch through
    launch_batch by hand."""
    if _RUN:
        return _RUN
    from gpu_util import build_model
    from roitr_amd.config import test_config
    from roitr_amd.fgr import fgr_handle
    from roitr_amd.tester import Tester
    model = build_model("3DMatch", weights="selective")
    runs = {}
    for ppf in (N_PAIRS, 1):
        d = tmp_path_factory.mktemp(f"fgr_{ppf}")
        t = Tester(test_config("3DMatch"), model, items(), str(d), pairs_per_forward=ppf, recall=True, estimator="fgr", fgr=KW)
        t.test()
        runs[ppf] = (t, [torch.load(d / "3DMatch" / f"{i}.pth") for i in range(N_PAIRS)])
    pairs = [dict(src_pcd=it["src_points"].cuda(), tgt_pcd=it["tgt_points"].cuda(), src_feats=it["src_feats"].cuda(),
                  tgt_feats=it["tgt_feats"].cuda(), src_normals=it["src_normals"].cuda(), tgt_normals=it["tgt_normals"].cuda(),
                  rot=it["rot"].cuda(), trans=it["trans"].cuda(), src_raw_pcd=it["raw_src_pcd"].cuda()) for it in items()]
    with torch.no_grad():
        h = model.launch_batch(pairs)
        model.finish_batch(h)
        reg = fgr_handle(h, pair_keys=list(range(N_PAIRS)), return_multiplicity=True, **KW)
        swapped = fgr_handle(h, pair_keys=[5, 6], return_multiplicity=True, **KW)
    torch.cuda.synchronize()
    _RUN.update(runs=runs, handle=h, reg=reg, swapped=swapped, model=model)
    return _RUN


def test_tester_equals_the_handle_by_hand_and_does_not_depend_on_pairs_per_forward(tmp_path_factory):
    from roitr_amd.registration import pose_errors
    e = engine_run(tmp_path_factory)
    reg = e["reg"]
    (t, files), (t1, files1) = e["runs"][N_PAIRS], e["runs"][1]
    assert t.estimator == "fgr" and sorted(t.registration) == sorted(t.recall) == list(range(N_PAIRS))
    # a pair whose correspondences hold no length-preserving triple among those drawn runs without the tuple test (NO_TUPLES)
    assert (reg["steps"] == KW["iterations"]).all() and (reg["status"] & ~8 == 0).all() and (reg["tuples_accepted"] > 0).any()
    assert not torch.equal(e["swapped"]["multiplicity"], reg["multiplicity"])                # the keys do reach the stream
    for i in range(N_PAIRS):
        assert torch.equal(files[i]["est_transform"], reg["T"][i].cpu())
        assert torch.equal(files1[i]["est_transform"], reg["T"][i].cpu())                   # a pair per forward: keyed on the global id
        rre, rte = pose_errors(files[i]["est_transform"], files[i]["rot"].reshape(1, 3, 3), files[i]["trans"].reshape(1, 3))
        assert abs(t.registration[i][0] - float(rre[0])) < 1e-9 and abs(t.registration[i][1] - float(rte[0])) < 1e-9
        assert t.registration[i][2] == t1.registration[i][2] == int(reg["inliers"][i])
    assert any("registration (fgr) over 2 pairs" in line for line in t.report)


def test_handle_equals_batch_on_copied_tensors(tmp_path_factory):
    from roitr_amd.fgr import fgr_batch
    e = engine_run(tmp_path_factory)
    out, reg = e["handle"]["out"], e["reg"]
    starts = out["pair_starts"].clone()
    n = int(starts[-1])
    assert n > 100
    again = fgr_batch(starts, out["out_src_pts"][:n].clone(), out["out_tgt_pts"][:n].clone(), out["out_scores"][:n].clone(),
                      pair_keys=[0, 1], **KW)
    for k in FIELDS:
        assert torch.equal(reg[k], again[k]), k
    for b in range(N_PAIRS):   # every pair alone
        s, t = int(starts[b]), int(starts[b + 1])
        one = fgr_batch(torch.tensor([0, t - s], dtype=torch.int32), out["out_src_pts"][s:t].clone(), out["out_tgt_pts"][s:t].clone(),
                        out["out_scores"][s:t].clone(), pair_keys=[b], **KW)
        for k in FIELDS:
            assert torch.equal(reg[k][b], one[k][0]), (b, k)


def test_fpfh_baseline_registers_the_exact_copy_with_fgr():
    """The bound tests/test_fpfh_gpu.py uses for compat and RANSAC: RRE < 0.1 degrees, RTE < 1e-3 m."""
    import fpfh_util as FU
    from roitr_amd.fpfh import fpfh_pose_estimation
    f = FU.fixture("e2e")
    g = FU.moved(f)
    assert FU.is_decided(g)
    for kw in ({}, dict(tuples=4096, pair_keys=[0])):
        T = fpfh_pose_estimation(f["xyz"], g["xyz"], f["normals"], g["normals"], radius=f["radius"], max_nn=f["max_nn"], estimator="fgr", **kw)
        rre = np.degrees(np.arccos(np.clip((np.trace(T[:3, :3].T @ FU.E2E_R) - 1) / 2, -1, 1)))
        rte = float(np.linalg.norm(T[:3, 3] - FU.E2E_T))
        print("fgr", kw, "RRE", rre, "deg, RTE", rte, "m")
        assert T.shape == (4, 4) and T.dtype == np.float64 and rre < 0.1 and rte < 1e-3, (kw, rre, rte)
    with pytest.raises(ValueError, match="lgr"):
        fpfh_pose_estimation(f["xyz"], g["xyz"], f["normals"], g["normals"], estimator="lgr")


def test_fpfh_handle_takes_the_estimator_and_the_keys(tmp_path_factory):
    from roitr_amd.fpfh import fpfh_handle
    h = engine_run(tmp_path_factory)["handle"]
    a = fpfh_handle(h, estimator="fgr", estimator_kw=dict(iterations=16, tuples=256), pair_keys=[0, 1])["reg"]
    b = fpfh_handle(h, estimator="fgr", estimator_kw=dict(iterations=16, tuples=256), pair_keys=[0, 1])["reg"]
    assert all(torch.equal(a[k], b[k]) for k in FIELDS) and a["T"].shape == (N_PAIRS, 4, 4)
    assert torch.isfinite(a["T"]).all() and (a["steps"] <= 16).all()


def test_fgr_pose_estimation_on_planted_descriptors():
    """The set of tests/test_compat_tester_gpu.py: unit descriptors shared by a planted third of the points, random ones elsewhere.
    With the mutual check the matches are almost all planted and the pose comes back."""
    from roitr_amd.registration import fgr_pose_estimation
    import lgr_util as LU
    rng = np.random.default_rng(3)
    n, good, dim = 600, 200, 32
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    R, t = LU.random_pose(rng)
    src = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    tgt = (src.astype(np.float64) @ R.T + t + 0.003 * rng.normal(size=(n, 3))).astype(np.float32)
    perm = np.concatenate([np.arange(good), good + rng.permutation(n - good)])     # the planted points keep their partner
    tgt = tgt[perm]
    sf = unit(rng.normal(size=(n, dim)))
    tf = unit(rng.normal(size=(n, dim)))
    tf[:good] = sf[:good]
    T = fgr_pose_estimation(src, tgt, sf, tf, mutual=True)
    assert T.shape == (4, 4) and T.dtype == np.float64
    assert np.abs(T[:3, :3] - R).max() < 5e-3 and np.abs(T[:3, 3] - t).max() < 1e-2
