"""GPU: the ICP refinement behind the engine handle and the Tester.  Two pairs of 1024 points on the closed-form selective weights; the
target cloud of each is an exact copy of its source under the ground-truth pose (rounded to fp32), its normals the rotated source
normals, so the refinement has an exact answer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_PAIRS, N_POINTS = 2, 1024
ICP = dict(max_dist=0.05, iterations=30)
RANSAC_ITERATIONS = 50000
# The floor of a refined pose on these pairs, from the fixture and the metric alone.  Translation: the target coordinates (magnitude
# below 4) carry an fp32 rounding of at most 2^-23 * 4 = 4.8e-7 m each and the state one of 2^-24 relative per entry, so a pose that fits
# the copies exactly is off by a few 1e-7 m; ten times that is allowed.  Rotation: pose_errors takes the angle from arccos((trace - 1) /
# 2) of R_est R_gt^T, both fp32 matrices: six roundings of 2^-24 can move the trace by 6 * 2^-24 = 3.6e-7, and arccos turns a trace
# error d at the identity into an angle of sqrt(d) = 6e-4 rad = 0.034 degrees, whatever produced the pose.
RTE_FLOOR, RRE_FLOOR = 1e-5, 0.05


def items():
    from roitr_amd.synthetic import make_pair
    out = []
    for i in range(N_PAIRS):
        it = make_pair(N_POINTS, config=1, pair_index=i)
        R, t = it["rot"].astype(np.float64), it["trans"].astype(np.float64).reshape(1, 3)
        it["tgt_points"] = (it["src_points"].astype(np.float64) @ R.T + t).astype(np.float32)
        it["tgt_normals"] = (it["src_normals"].astype(np.float64) @ R.T).astype(np.float32)
        it["tgt_feats"] = it["src_feats"].copy()
        out.append({k: torch.from_numpy(v) for k, v in it.items()})
    return out


_RUNS = {}


def engine_run(estimator, refine, tmp_path_factory):
    """One Tester run (one forward of both pairs) and the same batch through launch_batch, the estimator and icp_handle by hand."""
    key = (estimator, refine)
    if key in _RUNS:
        return _RUNS[key]
    from gpu_util import build_model
    from roitr_amd.config import test_config
    from roitr_amd.tester import Tester
    if "model" not in _RUNS:
        _RUNS["model"] = build_model("3DMatch", weights="selective")
    model = _RUNS["model"]
    d = tmp_path_factory.mktemp(f"icp_{estimator}_{refine}")
    t = Tester(test_config("3DMatch"), model, items(), str(d), pairs_per_forward=N_PAIRS, evaluate=True, register=True,
               estimator=estimator, ransac=dict(iterations=RANSAC_ITERATIONS), refine=refine, icp=ICP)
    t.test()
    raw = [open(d / "3DMatch" / f"{i}.pth", "rb").read() for i in range(N_PAIRS)]
    files = [torch.load(d / "3DMatch" / f"{i}.pth") for i in range(N_PAIRS)]
    _RUNS[key] = dict(tester=t, files=files, raw=raw, model=model)
    return _RUNS[key]


def by_hand(model, estimator, refine):
    from roitr_amd.icp import icp_handle
    from roitr_amd.lgr import lgr_handle
    from roitr_amd.registration import register_handle
    pairs = [dict(src_pcd=it["src_points"].cuda(), tgt_pcd=it["tgt_points"].cuda(), src_feats=it["src_feats"].cuda(),
                  tgt_feats=it["tgt_feats"].cuda(), src_normals=it["src_normals"].cuda(), tgt_normals=it["tgt_normals"].cuda(),
                  rot=it["rot"].cuda(), trans=it["trans"].cuda(), src_raw_pcd=it["raw_src_pcd"].cuda()) for it in items()]
    with torch.no_grad():
        h = model.launch_batch(pairs)
        model.finish_batch(h)
        reg = lgr_handle(h) if estimator == "lgr" else register_handle(h, pair_keys=list(range(N_PAIRS)), iterations=RANSAC_ITERATIONS)
        ref = icp_handle(h, reg["T"], plane=refine == "plane", **ICP)
    torch.cuda.synchronize()
    return h, reg, ref


@pytest.mark.parametrize("refine", ["point", "plane"])
@pytest.mark.parametrize("estimator", ["ransac", "lgr"])
def test_tester_refines_the_estimated_pose(estimator, refine, tmp_path_factory):
    from roitr_amd.registration import pose_errors
    run = engine_run(estimator, refine, tmp_path_factory)
    t, files = run["tester"], run["files"]
    h, reg, ref = by_hand(run["model"], estimator, refine)
    assert sorted(t.refinement) == sorted(t.refinement_status) == sorted(t.registration) == list(range(N_PAIRS))
    for i, f in enumerate(files):
        assert torch.equal(f["est_transform"], ref["T"][i].cpu())       # bitwise the refinement called by hand
        gt = (f["rot"].reshape(1, 3, 3), f["trans"].reshape(1, 3))
        before, after = pose_errors(reg["T"][i].cpu(), *gt), pose_errors(f["est_transform"], *gt)
        row = t.refinement[i]
        print(f"{estimator} {refine} pair {i}: RRE {row[0]:.3e} -> {row[2]:.3e} deg, RTE {row[1]:.3e} -> {row[3]:.3e} m, "
              f"fitness {row[4]:.4f} rmse {row[5]:.3e} steps {row[6]} status {t.refinement_status[i]}")
        assert len(row) == 7
        assert row[:4] == (float(before[0][0]), float(before[1][0]), float(after[0][0]), float(after[1][0]))
        assert row[4:] == (float(ref["fitness"][i]), float(ref["rmse"][i]), int(ref["steps"][i]))
        assert t.refinement_status[i] == int(ref["status"][i])
        assert t.registration[i][:2] == (row[2], row[3])                 # everything downstream sees the refined pose
        assert row[2] <= max(row[0], RRE_FLOOR) and row[3] <= max(row[1], RTE_FLOOR)


def test_handle_equals_batch_on_copied_tensors(tmp_path_factory):
    from roitr_amd.icp import icp_batch
    from roitr_amd.pairgt import handle_clouds
    from roitr_amd.riga import handle_normals
    run = engine_run("lgr", "plane", tmp_path_factory)
    h, reg, ref = by_hand(run["model"], "lgr", "plane")
    src, so, tgt, to, _, _ = handle_clouds(h)
    nrm = handle_normals(h)
    assert nrm.shape == (2 * N_PAIRS * N_POINTS, 3)
    want = torch.cat([it["tgt_normals"] for it in items()]).cuda()
    assert torch.equal(nrm[N_PAIRS * N_POINTS:], want)
    again = icp_batch(src.clone(), so.clone(), tgt.clone(), to.clone(), reg["T"].clone(), tgt_normals=want.clone(), **ICP)
    for k in ("T", "fitness", "rmse", "n_corr", "steps", "status"):
        assert torch.equal(ref[k], again[k]), k


def test_without_refine_nothing_changes(tmp_path_factory, tmp_path):
    """refine=None: files byte-equal to and metrics equal to a run that does not pass the new arguments at all."""
    from roitr_amd.config import test_config
    from roitr_amd.tester import Tester
    run = engine_run("lgr", None, tmp_path_factory)
    t = Tester(test_config("3DMatch"), run["model"], items(), str(tmp_path), pairs_per_forward=N_PAIRS, evaluate=True, register=True,
               estimator="lgr", ransac=dict(iterations=RANSAC_ITERATIONS))
    t.test()
    assert run["tester"].refinement is None and t.refinement is None and t.refine is None
    assert t.metrics == run["tester"].metrics and t.registration == run["tester"].registration
    for i in range(N_PAIRS):
        assert open(tmp_path / "3DMatch" / f"{i}.pth", "rb").read() == run["raw"][i]
    refined = engine_run("lgr", "point", tmp_path_factory)["files"]
    for f, g in zip(run["files"], refined):   # the refinement changes est_transform and nothing else in a file
        assert set(f) == set(g) and all(torch.equal(f[k], g[k]) for k in f if torch.is_tensor(f[k]) and k != "est_transform")


def test_unknown_mode_is_refused():
    from roitr_amd.tester import Tester
    with pytest.raises(ValueError):
        Tester({"benchmark": "3DMatch"}, None, [], refine="colored")
