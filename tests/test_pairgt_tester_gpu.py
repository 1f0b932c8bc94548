"""GPU: Tester(recall=True) on synthetic pairs with the closed-form weights -- the recall values against registration.
compute_transformation_err applied on the host to what the files hold, invariance under pairs_per_forward, the option switched off,
and the gt.log / gt.info / gt_overlap.log files of write_gt through the readers and evaluate_registration."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_PAIRS = 5


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from gpu_util import build_model
    from roitr_amd.config import test_config
    from roitr_amd.tester import SyntheticPairs, Tester
    model = build_model("3DMatch", weights="selective")
    data = SyntheticPairs(N_PAIRS, 1024, config=1)
    out = {}
    for name, kw in (("ppf4", dict(pairs_per_forward=4, recall=True)), ("ppf1", dict(pairs_per_forward=1, recall=True)),
                     ("off", dict(pairs_per_forward=4, evaluate=True, register=True))):
        d = tmp_path_factory.mktemp(name)
        t = Tester(test_config("3DMatch"), model, data, str(d), ransac=dict(iterations=4000), **kw)
        t.test()
        out[name] = (t, [torch.load(d / "3DMatch" / f"{i}.pth") for i in range(N_PAIRS)])
    return out


def T_gt(f):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = f["rot"].reshape(3, 3).double().numpy(), f["trans"].reshape(3).double().numpy()
    return T


def test_recall_values_follow_the_saved_files(runs):
    from roitr_amd.registration import compute_transformation_err
    from roitr_amd.tester import recall_error, recall_metrics
    t, files = runs["ppf4"]
    assert sorted(t.recall) == list(range(N_PAIRS)) and t.registration is not None
    good = []
    for i, f in enumerate(files):
        ov_s, ov_t, p, ok = t.recall[i]
        assert 0.0 <= ov_s <= 1.0 and 0.0 <= ov_t <= 1.0 and f["gt_overlap"].tolist() == [ov_s, ov_t]
        info = f["gt_info"].numpy()
        assert info.shape == (6, 6) and info.dtype == np.float64 and info[0, 0] == round(ov_s * f["src_pcd"].shape[0]) > 0
        want = compute_transformation_err(np.linalg.inv(T_gt(f)) @ f["est_transform"].double().numpy(), info)
        assert p == want and ok == (want <= 0.04)
        # the Tester's own formula (tester.recall_error, what _recall_rows stores) with the ground truth as the estimate: p is 0 up to
        # the rounding of inv(T) @ T and of the quaternion's eigenvector (~1e-16 each, squared in p, times |info| / n ~ 10)
        assert recall_error(T_gt(f), f["est_transform"].double().numpy(), info) == p
        assert 0.0 <= recall_error(T_gt(f), T_gt(f), info) <= 1e-24
        good.append(ok)
    m = t.metrics
    assert m["RR"] == sum(good) / N_PAIRS and m["RR_pairs"] == N_PAIRS and m["pairs_without_overlap"] == 0
    assert m["RR_overlap_ge_0.3_pairs"] + m["RR_overlap_0.1_0.3_pairs"] + m["RR_overlap_lt_0.1_pairs"] == N_PAIRS
    for name, lo, hi in (("ge_0.3", 0.3, 9.0), ("0.1_0.3", 0.1, 0.3), ("lt_0.1", -1.0, 0.1)):
        sel = [t.recall[i][3] for i in range(N_PAIRS) if lo <= t.recall[i][0] < hi]
        assert m[f"RR_overlap_{name}_pairs"] == len(sel)
        assert (m[f"RR_overlap_{name}"] == sum(sel) / len(sel)) if sel else np.isnan(m[f"RR_overlap_{name}"])
    # a pair without a source point within the radius has no p: left out and counted
    mm = recall_metrics({0: (0.5, 0.5, 0.01, True), 1: (0.0, 0.0, float("nan"), False), 2: (0.2, 0.2, 0.5, False)})
    assert mm["RR"] == 0.5 and mm["RR_pairs"] == 2 and mm["pairs_without_overlap"] == 1 and mm["RR_overlap_0.1_0.3"] == 0.0
    assert np.isnan(mm["RR_overlap_lt_0.1"]) and mm["RR_overlap_lt_0.1_pairs"] == 0


def same_values(x, y):
    """dict equality where nan (the rate of an empty overlap bin) equals nan"""
    return x.keys() == y.keys() and all(x[k] == y[k] or (x[k] != x[k] and y[k] != y[k]) for k in x)


def test_recall_is_independent_of_pairs_per_forward(runs):
    (a, fa), (b, fb) = runs["ppf4"], runs["ppf1"]
    assert a.recall == b.recall and same_values(a.metrics, b.metrics)
    for x, y in zip(fa, fb):
        assert torch.equal(x["gt_info"], y["gt_info"]) and torch.equal(x["gt_overlap"], y["gt_overlap"])


def test_option_off_changes_nothing(runs):
    (on, f_on), (off, f_off) = runs["ppf4"], runs["off"]
    assert off.recall is None and off.gt is None
    assert not [k for k in off.metrics if k.startswith("RR") or k == "pairs_without_overlap"]
    assert {k: v for k, v in on.metrics.items() if k in off.metrics} == off.metrics
    assert on.registration == off.registration and on.records.n_scores == off.records.n_scores
    for a, b in zip(f_on, f_off):
        assert set(a) - set(b) == {"gt_overlap", "gt_info"} and not set(b) - set(a)
        assert all(torch.equal(a[k], b[k]) for k in b if torch.is_tensor(b[k]))
    for i in range(N_PAIRS):
        assert torch.equal(on.records[i], off.records[i])


def test_write_gt_round_trips_and_feeds_evaluate_registration(runs, tmp_path):
    from roitr_amd.registration import evaluate_registration, read_trajectory, read_trajectory_info
    from roitr_amd.tester import write_gt
    t, files = runs["ppf4"]
    write_gt(str(tmp_path), t.gt)
    keys, traj = read_trajectory(str(tmp_path / "gt.log"))
    est_keys, est = read_trajectory(str(tmp_path / "est.log"))
    n_frame, info = read_trajectory_info(str(tmp_path / "gt.info"))
    # one filler record first (the reference never tests the record at index 0), then pair k as fragments (k, k + 2)
    assert keys.astype(int).tolist() == [[0, 1, N_PAIRS + 2]] + [[k, k + 2, N_PAIRS + 2] for k in range(N_PAIRS)]
    assert n_frame == N_PAIRS + 2 and np.array_equal(est_keys, keys) and info.shape == (N_PAIRS + 1, 6, 6)
    for i, f in enumerate(files):
        assert np.allclose(traj[i + 1], T_gt(f), rtol=0, atol=1e-12)                  # 12 decimals
        assert np.allclose(est[i + 1], f["est_transform"].double().numpy(), rtol=0, atol=1e-12)
        assert np.allclose(info[i + 1], f["gt_info"].numpy(), rtol=0, atol=1e-12 + 1e-15 * np.abs(f["gt_info"].numpy()).max())
    lines = open(tmp_path / "gt_overlap.log").read().split()
    assert lines == [f"{k},{k + 2},{t.recall[k][0]:.4f}" for k in range(N_PAIRS)]
    pairs = keys.astype(int)
    _, recall, flags = evaluate_registration(n_frame, est, pairs, pairs, traj, info)
    # the filler is not a tested pair; every pair of the run is, and the recall is the Tester's
    assert flags[0] == 2 and [fl == 0 for fl in flags[1:]] == [t.recall[k][3] for k in range(N_PAIRS)]
    assert recall == sum(t.recall[k][3] for k in range(N_PAIRS)) / N_PAIRS == t.metrics["RR"]
