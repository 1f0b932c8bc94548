"""GPU: the local-to-global registration behind the engine handle, the Tester and the dense entry point.  Engine batches run on the
closed-form selective weights (thousands of correspondences per pair), 2 pairs of 1024 points, in the strided (3DMatch) and the
compacted (4DMatch) patch layout."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_PAIRS, N_POINTS = 2, 1024
FIELDS = ("T", "inliers", "best_hypothesis", "best_first_row", "hypotheses", "local_inliers", "status")


def items(config):
    from roitr_amd.synthetic import make_pair
    return [{k: torch.from_numpy(v) for k, v in make_pair(N_POINTS, config=config, pair_index=i).items()} for i in range(N_PAIRS)]


LAYOUTS = {"strided": ("3DMatch", 1), "compacted": ("4DMatch", 4)}
_RUNS = {}


def engine_run(layout, tmp_path_factory):
    """One Tester run with estimator="lgr" (one forward of both pairs) and the same batch through launch_batch by hand; once per layout."""
    if layout in _RUNS:
        return _RUNS[layout]
    from gpu_util import build_model
    from roitr_amd.config import test_config
    from roitr_amd.lgr import lgr_handle
    from roitr_amd.tester import Tester
    benchmark, config = LAYOUTS[layout]
    model = build_model(benchmark, weights="selective")
    d = tmp_path_factory.mktemp("lgr_" + benchmark)
    t = Tester(test_config(benchmark), model, items(config), str(d), pairs_per_forward=N_PAIRS, recall=True, estimator="lgr")
    t.test()
    files = [torch.load(d / benchmark / f"{i}.pth") for i in range(N_PAIRS)]
    pairs = [dict(src_pcd=it["src_points"].cuda(), tgt_pcd=it["tgt_points"].cuda(), src_feats=it["src_feats"].cuda(),
                  tgt_feats=it["tgt_feats"].cuda(), src_normals=it["src_normals"].cuda(), tgt_normals=it["tgt_normals"].cuda(),
                  rot=it["rot"].cuda(), trans=it["trans"].cuda(), src_raw_pcd=it["raw_src_pcd"].cuda()) for it in items(config)]
    with torch.no_grad():
        h = model.launch_batch(pairs)
        model.finish_batch(h)
        reg = lgr_handle(h)
    torch.cuda.synchronize()
    _RUNS[layout] = dict(tester=t, files=files, handle=h, reg=reg, model=model, benchmark=benchmark)
    return _RUNS[layout]


@pytest.fixture(params=sorted(LAYOUTS))
def engine(request, tmp_path_factory):
    return engine_run(request.param, tmp_path_factory)


def test_handle_equals_batch_on_copied_tensors(engine):
    from roitr_amd.lgr import lgr_batch
    out, reg = engine["handle"]["out"], engine["reg"]
    starts = out["pair_starts"].clone()
    n = int(starts[-1])
    assert n > 100 and (reg["hypotheses"] > 0).all()
    again = lgr_batch(starts, out["out_src_pts"][:n].clone(), out["out_tgt_pts"][:n].clone(), out["out_scores"][:n].clone(),
                      out["out_patch"][:n].clone())
    for k in FIELDS:
        assert torch.equal(reg[k], again[k]), k
    for b in range(N_PAIRS):   # every pair alone
        s, e = int(starts[b]), int(starts[b + 1])
        one = lgr_batch(torch.tensor([0, e - s], dtype=torch.int32), out["out_src_pts"][s:e].clone(), out["out_tgt_pts"][s:e].clone(),
                        out["out_scores"][s:e].clone(), out["out_patch"][s:e].clone())
        for k in FIELDS:
            assert torch.equal(reg[k][b], one[k][0]), (b, k)


def test_tester_writes_the_lgr_pose(engine):
    from roitr_amd.registration import pose_errors
    from roitr_amd.tester import recall_error
    t, files, reg = engine["tester"], engine["files"], engine["reg"]
    assert sorted(t.registration) == sorted(t.recall) == list(range(N_PAIRS))
    for i, f in enumerate(files):
        assert torch.equal(f["est_transform"], reg["T"][i].cpu())
        rre, rte = pose_errors(f["est_transform"], f["rot"].reshape(1, 3, 3), f["trans"].reshape(1, 3))
        assert abs(t.registration[i][0] - float(rre[0])) < 1e-9 and abs(t.registration[i][1] - float(rte[0])) < 1e-9
        assert t.registration[i][2] == int(reg["inliers"][i])
        T_gt = np.eye(4)
        T_gt[:3, :3], T_gt[:3, 3] = f["rot"].reshape(3, 3).double().numpy(), f["trans"].reshape(3).double().numpy()
        ov_s, ov_t, p, ok = t.recall[i]
        assert f["gt_overlap"].tolist() == [ov_s, ov_t]
        assert p == recall_error(T_gt, f["est_transform"].double().numpy(), f["gt_info"].numpy()) and ok == (p <= 0.04)


def test_default_estimator_is_ransac_as_before(tmp_path_factory, tmp_path):
    """The default run writes what register_handle gives (keyed on the pair ids) and nothing else changes in the files."""
    from roitr_amd.config import test_config
    from roitr_amd.registration import register_handle
    from roitr_amd.tester import Tester
    engine = engine_run("strided", tmp_path_factory)
    kw = dict(iterations=4000)
    t = Tester(test_config("3DMatch"), engine["model"], items(1), str(tmp_path), pairs_per_forward=N_PAIRS, evaluate=True, register=True,
               ransac=kw)
    t.test()
    assert t.estimator == "ransac"
    want = register_handle(engine["handle"], pair_keys=list(range(N_PAIRS)), **kw)
    for i, lgr_file in enumerate(engine["files"]):
        f = torch.load(tmp_path / "3DMatch" / f"{i}.pth")
        assert torch.equal(f["est_transform"], want["T"][i].cpu()) and t.registration[i][2] == int(want["inliers"][i])
        assert set(lgr_file) - set(f) == {"gt_overlap", "gt_info"} and not set(f) - set(lgr_file)
        assert all(torch.equal(f[k], lgr_file[k]) for k in f if torch.is_tensor(f[k]) and k != "est_transform")


def test_dense_entry_agrees_with_the_batch_entry():
    import lgr_util as U
    from roitr_amd.lgr import lgr_batch, local_global_registration
    src, tgt, w, patch, _, _ = U.fixture("mixed_runs")
    # dense (P, K, K): row k of patch p becomes entry (p, k, k), so nonzero() returns the rows in their order; K = 20 points per patch
    P, K = int(patch.max()) + 1, 20
    ref_knn, src_knn = np.zeros((P, K, 3), np.float32), np.zeros((P, K, 3), np.float32)
    score, corr = np.zeros((P, K, K), np.float32), np.zeros((P, K, K), bool)
    keep = np.zeros(len(w), bool)
    for p in range(P):
        rows = np.flatnonzero(patch == p)
        if len(rows) > K:      # a longer run keeps its first K rows
            rows = rows[:K]
        keep[rows] = True
        for k, r in enumerate(rows):     # row k of the patch: ref point k with src point k
            ref_knn[p, k], src_knn[p, k], score[p, k, k], corr[p, k, k] = tgt[r], src[r], w[r], True
    ref_pts, src_pts, scores, T = local_global_registration(torch.from_numpy(ref_knn), torch.from_numpy(src_knn),
                                                            torch.from_numpy(score), torch.from_numpy(corr))
    assert np.array_equal(ref_pts.cpu().numpy(), tgt[keep]) and np.array_equal(src_pts.cpu().numpy(), src[keep])
    assert np.array_equal(scores.cpu().numpy(), w[keep])
    want = lgr_batch(torch.tensor([0, int(keep.sum())], dtype=torch.int32), src[keep], tgt[keep], w[keep], patch[keep])
    assert T.shape == (4, 4) and torch.equal(T, want["T"][0]) and int(want["status"][0]) == 0
