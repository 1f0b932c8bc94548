"""GPU: the FPFH baseline behind the engine handle and the Tester: four synthetic pairs of 1024 points on the closed-form selective
weights.  The baseline's four metrics do not depend on pairs_per_forward; with the option off, files and metrics are those of a run
without it; lgr is refused."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

N_PAIRS, N_POINTS = 4, 1024
KEYS = ("fpfh_ir", "fpfh_rre", "fpfh_rte", "fpfh_success")
_RUNS = {}


def items():
    from roitr_amd.synthetic import make_pair
    return [{k: torch.from_numpy(v) for k, v in make_pair(N_POINTS, config=1, pair_index=i).items()} for i in range(N_PAIRS)]


def run_tester(tmp_path_factory, estimator, per_forward, baseline):
    key = (estimator, per_forward, baseline)
    if key not in _RUNS:
        from gpu_util import build_model
        from roitr_amd.config import test_config
        from roitr_amd.tester import Tester
        d = tmp_path_factory.mktemp(f"fpfh_{estimator}_{per_forward}_{int(baseline)}")
        t = Tester(test_config("3DMatch"), build_model("3DMatch", weights="selective"), items(), str(d), pairs_per_forward=per_forward,
                   evaluate=True, register=True, estimator=estimator, ransac=dict(iterations=4000),
                   fpfh_baseline=dict(radius=0.3, max_nn=64) if baseline else None)
        t.test()
        _RUNS[key] = (t, [torch.load(d / "3DMatch" / f"{i}.pth") for i in range(N_PAIRS)])
    return _RUNS[key]


def same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("estimator", ["compat", "ransac"])
def test_baseline_metrics_do_not_depend_on_pairs_per_forward(tmp_path_factory, estimator):
    whole, _ = run_tester(tmp_path_factory, estimator, N_PAIRS, True)
    split, _ = run_tester(tmp_path_factory, estimator, 3, True)      # a forward of three pairs and one of one
    assert sorted(whole.fpfh) == sorted(split.fpfh) == list(range(N_PAIRS))
    for i in range(N_PAIRS):
        ir, rre, rte, cnt = whole.fpfh[i]
        assert cnt > 0 and 0.0 <= ir <= 1.0 and math.isfinite(rre) and math.isfinite(rte)
        assert all(same(a, b) for a, b in zip(whole.fpfh[i], split.fpfh[i])), (i, whole.fpfh[i], split.fpfh[i])
    for k in KEYS + ("fpfh_pairs",):
        assert k in whole.metrics and same(whole.metrics[k], split.metrics[k]), k
    assert whole.metrics["fpfh_pairs"] == N_PAIRS and 0.0 <= whole.metrics["fpfh_success"] <= 1.0


def test_baseline_equals_the_handle_call(tmp_path_factory):
    from gpu_util import build_model
    from roitr_amd.fpfh import fpfh_handle
    from roitr_amd.registration import pose_errors
    t, _ = run_tester(tmp_path_factory, "compat", N_PAIRS, True)
    model = build_model("3DMatch", weights="selective")
    pairs = [dict(src_pcd=it["src_points"].cuda(), tgt_pcd=it["tgt_points"].cuda(), src_feats=it["src_feats"].cuda(),
                  tgt_feats=it["tgt_feats"].cuda(), src_normals=it["src_normals"].cuda(), tgt_normals=it["tgt_normals"].cuda(),
                  rot=it["rot"].cuda(), trans=it["trans"].cuda(), src_raw_pcd=it["raw_src_pcd"].cuda()) for it in items()]
    with torch.no_grad():
        h = model.launch_batch(pairs)
        model.finish_batch(h)
        m = fpfh_handle(h, radius=0.3, max_nn=64, estimator="compat", inlier_distance_threshold=0.1)
    assert m["fpfh"].shape == (2 * N_PAIRS * N_POINTS, 36) and m["reg"]["T"].shape == (N_PAIRS, 4, 4)
    rre, rte = pose_errors(m["reg"]["T"].cpu(), torch.stack([p["rot"].reshape(3, 3) for p in pairs]).cpu(),
                           torch.stack([p["trans"].reshape(3) for p in pairs]).cpu())
    for i in range(N_PAIRS):
        assert t.fpfh[i] == (float(m["ir"][i]), float(rre[i]), float(rte[i]), int(m["n_matches"][i]))


def test_option_off_changes_nothing(tmp_path_factory):
    on, files_on = run_tester(tmp_path_factory, "compat", N_PAIRS, True)
    off, files_off = run_tester(tmp_path_factory, "compat", N_PAIRS, False)
    assert off.fpfh is None and not any(k.startswith("fpfh") for k in off.metrics)
    assert {k: v for k, v in on.metrics.items() if not k.startswith("fpfh")} == off.metrics
    assert on.registration == off.registration
    for f, g in zip(files_on, files_off):
        assert set(f) == set(g) and not any("fpfh" in k for k in f)
        assert all(torch.equal(f[k], g[k]) for k in f if torch.is_tensor(f[k]))


def test_lgr_is_refused_for_the_baseline(tmp_path):
    from roitr_amd.config import test_config
    from roitr_amd.tester import Tester
    with pytest.raises(ValueError, match="lgr"):
        Tester(test_config("3DMatch"), None, items(), str(tmp_path), evaluate=True, register=True, estimator="lgr", fpfh_baseline={})
    t = Tester(test_config("3DMatch"), None, items(), str(tmp_path), evaluate=True, register=True, estimator="lgr")
    assert t.fpfh is None and t.fpfh_baseline is None
