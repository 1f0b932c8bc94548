"""GPU: the generalized-ICP refinement behind the engine handle and the Tester.  Two pairs of 1024 points on the closed-form selective
weights, built as tests/test_icp_tester_gpu.py builds them: the target cloud of each is an exact copy of its source under the
ground-truth pose (rounded to fp32), its normals the rotated source normals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_PAIRS, N_POINTS = 2, 1024
GICP = dict(max_dist=0.05, iterations=30, epsilon=1e-3)
# the floor of a refined pose on these pairs: tests/test_icp_tester_gpu.py derives it from the fixture and the metric alone
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


def model():
    from gpu_util import build_model
    if "model" not in _RUNS:
        _RUNS["model"] = build_model("3DMatch", weights="selective")
    return _RUNS["model"]


def run_tester(directory, **kw):
    from roitr_amd.config import test_config
    from roitr_amd.tester import Tester
    t = Tester(test_config("3DMatch"), model(), items(), str(directory), pairs_per_forward=N_PAIRS, evaluate=True, register=True,
               estimator="lgr", **kw)
    t.test()
    raw = [open(directory / "3DMatch" / f"{i}.pth", "rb").read() for i in range(N_PAIRS)]
    files = [torch.load(directory / "3DMatch" / f"{i}.pth") for i in range(N_PAIRS)]
    return t, raw, files


def by_hand():
    from roitr_amd.gicp import gicp_handle
    from roitr_amd.lgr import lgr_handle
    pairs = [dict(src_pcd=it["src_points"].cuda(), tgt_pcd=it["tgt_points"].cuda(), src_feats=it["src_feats"].cuda(),
                  tgt_feats=it["tgt_feats"].cuda(), src_normals=it["src_normals"].cuda(), tgt_normals=it["tgt_normals"].cuda(),
                  rot=it["rot"].cuda(), trans=it["trans"].cuda(), src_raw_pcd=it["raw_src_pcd"].cuda()) for it in items()]
    with torch.no_grad():
        h = model().launch_batch(pairs)
        model().finish_batch(h)
        reg = lgr_handle(h)
        ref = gicp_handle(h, reg["T"], **GICP)
    torch.cuda.synchronize()
    return h, reg, ref


def test_tester_refines_with_gicp(tmp_path):
    from roitr_amd.registration import pose_errors
    t, _, files = run_tester(tmp_path, refine="gicp", icp=GICP)
    h, reg, ref = by_hand()
    assert sorted(t.refinement) == sorted(t.refinement_status) == sorted(t.registration) == list(range(N_PAIRS))
    for i, f in enumerate(files):
        assert torch.equal(f["est_transform"], ref["T"][i].cpu())       # bitwise the refinement called by hand
        gt = (f["rot"].reshape(1, 3, 3), f["trans"].reshape(1, 3))
        before, after = pose_errors(reg["T"][i].cpu(), *gt), pose_errors(f["est_transform"], *gt)
        row = t.refinement[i]
        print(f"lgr gicp pair {i}: RRE {row[0]:.3e} -> {row[2]:.3e} deg, RTE {row[1]:.3e} -> {row[3]:.3e} m, fitness {row[4]:.4f} "
              f"rmse {row[5]:.3e} steps {row[6]} status {t.refinement_status[i]} objective {float(ref['objective'][i]):.3e}")
        assert len(row) == 7
        assert row[:4] == (float(before[0][0]), float(before[1][0]), float(after[0][0]), float(after[1][0]))
        assert row[4:] == (float(ref["fitness"][i]), float(ref["rmse"][i]), int(ref["steps"][i]))
        assert t.refinement_status[i] == int(ref["status"][i])
        assert t.registration[i][:2] == (row[2], row[3])                 # everything downstream sees the refined pose
        assert row[2] <= max(row[0], RRE_FLOOR) and row[3] <= max(row[1], RTE_FLOOR)


def test_handle_takes_both_halves_of_the_normals():
    from roitr_amd.gicp import gicp_batch
    from roitr_amd.pairgt import handle_clouds
    from roitr_amd.riga import handle_normals
    h, reg, ref = by_hand()
    src, so, tgt, to, _, _ = handle_clouds(h)
    nrm = handle_normals(h)
    n = N_PAIRS * N_POINTS
    assert nrm.shape == (2 * n, 3)
    want_s, want_t = (torch.cat([it[k] for it in items()]).cuda() for k in ("src_normals", "tgt_normals"))
    assert torch.equal(nrm[:n], want_s) and torch.equal(nrm[n:], want_t)
    again = gicp_batch(src.clone(), so.clone(), tgt.clone(), to.clone(), reg["T"].clone(), src_normals=want_s.clone(),
                       tgt_normals=want_t.clone(), **GICP)
    for k in ("T", "fitness", "rmse", "objective", "n_corr", "steps", "status"):
        assert torch.equal(ref[k], again[k]), k


def test_without_refine_nothing_changes(tmp_path_factory):
    """refine=None: files byte-equal to and metrics equal to a run that does not pass the new arguments at all."""
    a, raw_a, _ = run_tester(tmp_path_factory.mktemp("none"), refine=None, icp=GICP)
    b, raw_b, _ = run_tester(tmp_path_factory.mktemp("bare"))
    assert a.refinement is None and b.refinement is None and a.refine is None
    assert a.metrics == b.metrics and a.registration == b.registration and raw_a == raw_b
