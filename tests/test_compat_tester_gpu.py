"""GPU: the spatial-compatibility registration behind the engine handle, the Tester, the descriptor-matching entry point and the
command line.  Engine batches run on the closed-form selective weights, 2 pairs of 1024 points, in the strided (3DMatch) and the
compacted (4DMatch) patch layout."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_PAIRS, N_POINTS = 2, 1024
FIELDS = ("T", "inliers", "best_rank", "best_seed_row", "seeds", "hypotheses", "local_inliers", "status")


def items(config):
    from roitr_amd.synthetic import make_pair
    return [{k: torch.from_numpy(v) for k, v in make_pair(N_POINTS, config=config, pair_index=i).items()} for i in range(N_PAIRS)]


LAYOUTS = {"strided": ("3DMatch", 1), "compacted": ("4DMatch", 4)}
_RUNS = {}


def engine_run(layout, tmp_path_factory):
    """One Tester run with estimator="compat" (one forward of both pairs) and the same batch through launch_batch by hand; once per
    layout."""
    if layout in _RUNS:
        return _RUNS[layout]
    from gpu_util import build_model
    from roitr_amd.compat import compat_handle
    from roitr_amd.config import test_config
    from roitr_amd.tester import Tester
    benchmark, config = LAYOUTS[layout]
    model = build_model(benchmark, weights="selective")
    d = tmp_path_factory.mktemp("compat_" + benchmark)
    t = Tester(test_config(benchmark), model, items(config), str(d), pairs_per_forward=N_PAIRS, recall=True, estimator="compat")
    t.test()
    files = [torch.load(d / benchmark / f"{i}.pth") for i in range(N_PAIRS)]
    pairs = [dict(src_pcd=it["src_points"].cuda(), tgt_pcd=it["tgt_points"].cuda(), src_feats=it["src_feats"].cuda(),
                  tgt_feats=it["tgt_feats"].cuda(), src_normals=it["src_normals"].cuda(), tgt_normals=it["tgt_normals"].cuda(),
                  rot=it["rot"].cuda(), trans=it["trans"].cuda(), src_raw_pcd=it["raw_src_pcd"].cuda()) for it in items(config)]
    with torch.no_grad():
        h = model.launch_batch(pairs)
        model.finish_batch(h)
        reg = compat_handle(h)
    torch.cuda.synchronize()
    _RUNS[layout] = dict(tester=t, files=files, handle=h, reg=reg, model=model, benchmark=benchmark)
    return _RUNS[layout]


@pytest.fixture(params=sorted(LAYOUTS))
def engine(request, tmp_path_factory):
    return engine_run(request.param, tmp_path_factory)


def test_handle_equals_batch_on_copied_tensors(engine):
    from roitr_amd.compat import compat_batch
    out, reg = engine["handle"]["out"], engine["reg"]
    starts = out["pair_starts"].clone()
    n = int(starts[-1])
    assert n > 100 and (reg["seeds"] > 0).all()
    again = compat_batch(starts, out["out_src_pts"][:n].clone(), out["out_tgt_pts"][:n].clone(), out["out_scores"][:n].clone())
    for k in FIELDS:
        assert torch.equal(reg[k], again[k]), k
    cap = min(2048, int(out["out_src_pts"].reshape(-1, 3).shape[0]))
    for b in range(N_PAIRS):   # every pair alone, under the row capacity of the handle's call
        s, e = int(starts[b]), int(starts[b + 1])
        one = compat_batch(torch.tensor([0, e - s], dtype=torch.int32), out["out_src_pts"][s:e].clone(), out["out_tgt_pts"][s:e].clone(),
                           out["out_scores"][s:e].clone(), max_rows=cap)
        for k in FIELDS:
            assert torch.equal(reg[k][b], one[k][0]), (b, k)


def test_tester_writes_the_compat_pose(engine):
    from roitr_amd.registration import pose_errors
    from roitr_amd.tester import recall_error
    t, files, reg = engine["tester"], engine["files"], engine["reg"]
    assert t.estimator == "compat" and sorted(t.registration) == sorted(t.recall) == list(range(N_PAIRS))
    for i, f in enumerate(files):
        assert torch.equal(f["est_transform"], reg["T"][i].cpu())
        rre, rte = pose_errors(f["est_transform"], f["rot"].reshape(1, 3, 3), f["trans"].reshape(1, 3))
        assert abs(t.registration[i][0] - float(rre[0])) < 1e-9 and abs(t.registration[i][1] - float(rte[0])) < 1e-9
        assert t.registration[i][2] == int(reg["inliers"][i])
        T_gt = np.eye(4)
        T_gt[:3, :3], T_gt[:3, 3] = f["rot"].reshape(3, 3).double().numpy(), f["trans"].reshape(3).double().numpy()
        ov_s, ov_t, p, ok = t.recall[i]
        assert p == recall_error(T_gt, f["est_transform"].double().numpy(), f["gt_info"].numpy()) and ok == (p <= 0.04)


def test_default_estimator_is_ransac_as_before(tmp_path_factory, tmp_path):
    """A run without the argument and one with estimator="ransac" write the same records, those of register_handle."""
    from roitr_amd.config import test_config
    from roitr_amd.registration import register_handle
    from roitr_amd.tester import Tester
    engine = engine_run("strided", tmp_path_factory)
    kw = dict(iterations=4000)
    runs = []
    for name, extra in (("default", {}), ("named", dict(estimator="ransac", compat=dict(k=5)))):
        t = Tester(test_config("3DMatch"), engine["model"], items(1), str(tmp_path / name), pairs_per_forward=N_PAIRS, evaluate=True,
                   register=True, ransac=kw, **extra)
        t.test()
        assert t.estimator == "ransac"
        runs.append((t, [torch.load(tmp_path / name / "3DMatch" / f"{i}.pth") for i in range(N_PAIRS)]))
    want = register_handle(engine["handle"], pair_keys=list(range(N_PAIRS)), **kw)
    (t0, f0), (t1, f1) = runs
    assert t0.registration == t1.registration
    for i in range(N_PAIRS):
        assert torch.equal(f0[i]["est_transform"], want["T"][i].cpu()) and t0.registration[i][2] == int(want["inliers"][i])
        assert set(f0[i]) == set(f1[i])
        assert all(torch.equal(f0[i][k], f1[i][k]) for k in f0[i] if torch.is_tensor(f0[i][k]))
    with pytest.raises(ValueError):
        Tester(test_config("3DMatch"), engine["model"], items(1), str(tmp_path / "bad"), estimator="sc2")


def test_compat_pose_estimation_on_planted_descriptors():
    """Unit descriptors shared by a planted third of the points, random ones elsewhere: the matches are the planted pairs plus one
    wrong target for every other source point; the pose comes back, with and without the mutual check."""
    from roitr_amd.registration import compat_pose_estimation
    rng = np.random.default_rng(3)
    n, good, dim = 600, 200, 32
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    t = rng.uniform(-1, 1, 3)
    src = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    tgt = (src.astype(np.float64) @ R.T + t + 0.003 * rng.normal(size=(n, 3))).astype(np.float32)
    perm = np.concatenate([np.arange(good), good + rng.permutation(n - good)])     # the planted points keep their partner
    tgt = tgt[perm]
    sf = unit(rng.normal(size=(n, dim)))
    tf = unit(rng.normal(size=(n, dim)))
    tf[:good] = sf[:good]
    for mutual in (False, True):
        T = compat_pose_estimation(src, tgt, sf, tf, mutual=mutual)
        assert T.shape == (4, 4) and T.dtype == np.float64
        assert np.abs(T[:3, :3] - R).max() < 5e-3 and np.abs(T[:3, 3] - t).max() < 1e-2, mutual


def test_main_parser_accepts_the_new_options():
    from roitr_amd.main import parser
    a = parser().parse_args(["c.yaml", "--register", "--estimator", "compat", "--compat-dist", "0.05", "--compat-seeds", "32",
                             "--compat-k", "12", "--refine", "plane", "--recall"])
    assert (a.estimator, a.compat_dist, a.compat_seeds, a.compat_k, a.refine, a.recall) == ("compat", 0.05, 32, 12, "plane", True)
    d = parser().parse_args(["c.yaml"])
    assert (d.estimator, d.compat_dist, d.compat_seeds, d.compat_k) == ("ransac", 0.1, 64, 20)
