"""GPU: Tester(outlier=...) on four synthetic pairs of 1024 points with 5 % planted points appended to raw_src_pcd / src_points /
tgt_points: the model is fed exactly the rows the float64 restatement of tests/outlier_util.py keeps (both methods), metric_index keeps
pointing at the same physical points, and outlier=None is the run without the argument, bit for bit."""
import numpy as np
import pytest
import torch

import outlier_util as U

pytestmark = pytest.mark.gpu

N_PAIRS, N_POINTS, PER_FORWARD, SHARE = 4, 1024, 3, 0.05
METHODS = {"statistical": dict(method="statistical"), "radius": dict(method="radius", nb_points=10, radius=0.3)}


class Planted(torch.utils.data.Dataset):
    """The items of `base` with round(SHARE * n) uniform points of the bounding box appended to both clouds (the same rows go behind
    raw_src_pcd and src_points, so a deformed cloud stays row-aligned with its raw one)."""

    def __init__(self, base):
        self.items = []
        for i in range(len(base)):
            it = dict(base[i])
            rng = np.random.default_rng(900 + i)
            raw = U.planted(rng, it["raw_src_pcd"].numpy(), SHARE)
            extra = raw[it["raw_src_pcd"].shape[0]:]
            it["raw_src_pcd"] = torch.from_numpy(raw)
            it["src_points"] = torch.from_numpy(np.concatenate([it["src_points"].numpy(), extra]))
            it["tgt_points"] = torch.from_numpy(U.planted(rng, it["tgt_points"].numpy(), SHARE))
            self.items.append(it)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return dict(self.items[i])


def restated(data, method, side):
    """The restatement's result for the clouds of one side, every cloud alone (a cloud's result does not depend on its batch)."""
    kw = {k: v for k, v in METHODS[method].items() if k != "method"}
    ref = U.statistical_ref if method == "statistical" else U.radius_ref
    out = []
    for i in range(len(data)):
        x = data[i][side].numpy()
        f = dict(xyz=x, offset=np.array([len(x)], np.int32), **kw)
        if method == "statistical":
            assert U.is_decided(dict(U.params(), **f)), (side, i)
        out.append(ref(**f))
    return out


def run(tmp_path, benchmark, data, **kw):
    from gpu_util import build_model
    from roitr_amd.config import test_config
    from roitr_amd.tester import Tester
    t = Tester(test_config(benchmark), build_model(benchmark, weights="selective"), data, str(tmp_path), pairs_per_forward=PER_FORWARD, **kw)
    t.test()
    return t, [torch.load(tmp_path / benchmark / f"{i}.pth") for i in range(len(data))]


@pytest.mark.parametrize("method", sorted(METHODS))
def test_the_model_is_fed_the_rows_the_restatement_keeps(tmp_path, method):
    from roitr_amd.tester import SyntheticPairs
    data = Planted(SyntheticPairs(N_PAIRS, N_POINTS, config=1))
    t, files = run(tmp_path, "3DMatch", data, evaluate=True, outlier=METHODS[method])
    src, tgt = restated(data, method, "raw_src_pcd"), restated(data, method, "tgt_points")
    removed = [0, 0]
    for i, d in enumerate(files):
        it = data[i]
        ks, kt = torch.from_numpy(src[i]["index"]).long(), torch.from_numpy(tgt[i]["index"]).long()
        assert 0 < len(ks) < len(it["raw_src_pcd"]) and 0 < len(kt) < len(it["tgt_points"]), (i, len(ks), len(kt))
        assert torch.equal(d["src_raw_pcd"], it["raw_src_pcd"][ks]) and torch.equal(d["src_pcd"], it["src_points"][ks]), i
        assert torch.equal(d["tgt_pcd"], it["tgt_points"][kt]), i
        assert t.outlier_rows[i] == (len(it["raw_src_pcd"]), len(ks), len(it["tgt_points"]), len(kt))
        removed[0] += len(it["raw_src_pcd"]) - len(ks)
        removed[1] += len(it["tgt_points"]) - len(kt)
    assert t.metrics["pairs"] == N_PAIRS and len(files[0]) == 16
    line = [ln for ln in t.report if "outlier removal" in ln]
    assert len(line) == 1 and f"({method})" in line[0] and f"({removed[0]} of " in line[0] and f"({removed[1]} of " in line[0], t.report


def test_metric_index_points_at_the_same_physical_points(tmp_path):
    from roitr_amd.tester import SyntheticPairs
    data = Planted(SyntheticPairs(2, N_POINTS, nonrigid=True))
    t, files = run(tmp_path, "4DMatch", data, evaluate=True, outlier=METHODS["statistical"])
    src = restated(data, "statistical", "raw_src_pcd")
    for i, d in enumerate(files):
        it = data[i]
        keep, old = src[i]["keep"], it["metric_index"].numpy()
        survivors = old[keep[old]]
        new = d["metric_index_list"].numpy()
        assert 0 < len(survivors) <= len(old) and len(new) == len(survivors) and (np.diff(new) > 0).all()
        assert torch.equal(d["src_raw_pcd"][new], it["raw_src_pcd"][survivors]) and torch.equal(d["src_pcd"][new], it["src_points"][survivors])
        assert not torch.equal(d["src_pcd"], d["src_raw_pcd"])           # the deformed cloud went along as the attribute
    assert t.nonrigid is not None and [t.nonrigid[i][1] for i in range(2)] == [len(f["metric_index_list"]) for f in files]


def test_outlier_none_is_the_run_without_the_argument(tmp_path):
    from roitr_amd.tester import SyntheticPairs
    data = SyntheticPairs(N_PAIRS, N_POINTS, config=1)
    a, files_a = run(tmp_path / "none", "3DMatch", data, evaluate=True, outlier=None)
    b, files_b = run(tmp_path / "plain", "3DMatch", data, evaluate=True)
    assert a.metrics == b.metrics and a.report == b.report and not any("outlier" in ln for ln in a.report) and not a.estimate_normals
    for i, (f, g) in enumerate(zip(files_a, files_b)):
        assert list(f) == list(g) and len(f) == 16
        for k in f:
            assert torch.equal(f[k], g[k]) if torch.is_tensor(f[k]) else f[k] == g[k], (i, k)
        assert torch.equal(a.records[i], b.records[i])
