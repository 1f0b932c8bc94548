"""GPU: Tester(voxel_size=..., points_lim=...) against a plain Tester(estimate_normals=True) on a dataset whose items went through the
float64 restatement of tests/voxel_util.py on the host.  The result records and the metrics of the two runs must be bit-equal: the
device-side preparation hands the engine the very same points.

Voxel size 0.125 on SyntheticPairs(2, n_points=20000): 4704 / 4518 and 4728 / 4539 points survive in the two pairs (restatement, CPU);
the cap test then keeps 3000 of each."""
import numpy as np
import pytest
import torch

import voxel_util as V

pytestmark = pytest.mark.gpu

VOXEL, CAP, SEED = 0.125, 3000, 7


class HostPrepared(torch.utils.data.Dataset):
    """The items of `base`, voxel-downsampled (and capped) on the host by the restatement, with the keys the Tester uses."""

    def __init__(self, base, voxel, points_lim=None, seed=0):
        self.items = []
        for i in range(len(base)):
            it = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in base[i].items()}
            s = V.voxel_batch(it["raw_src_pcd"], [len(it["raw_src_pcd"])], voxel, it["src_points"])
            t = V.voxel_batch(it["tgt_points"], [len(it["tgt_points"])], voxel)
            raw, deformed, tgt = s["points"], s["attr"], t["points"]
            metric = np.unique(s["inverse"][it["metric_index"]]).astype(np.int64) if "metric_index" in it else None
            if points_lim is not None:
                ks, kt = V.subsample_cloud(len(raw), points_lim, 2 * i, seed), V.subsample_cloud(len(tgt), points_lim, 2 * i + 1, seed)
                if metric is not None:
                    pos = np.full(len(raw), -1, np.int64); pos[ks] = np.arange(len(ks))
                    metric = pos[metric][pos[metric] >= 0]
                raw, deformed, tgt = raw[ks], deformed[ks], tgt[kt]
            out = dict(it, raw_src_pcd=raw, src_points=deformed, tgt_points=tgt, src_normals=np.zeros_like(raw), tgt_normals=np.zeros_like(tgt),
                       src_feats=np.ones((len(raw), 1), np.float32), tgt_feats=np.ones((len(tgt), 1), np.float32))
            if metric is not None:
                out["metric_index"] = metric
            self.items.append({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return dict(self.items[i])


def run_both(tmp_path, benchmark, base, points_lim=None, ppf=2):
    from gpu_util import build_model
    from roitr_amd.config import test_config
    from roitr_amd.tester import Tester
    model = build_model(benchmark, weights="selective")
    cfg = test_config(benchmark)
    dev = Tester(cfg, model, base, str(tmp_path / "dev"), pairs_per_forward=ppf, evaluate=True, voxel_size=VOXEL, points_lim=points_lim,
                 subsample_seed=SEED)
    dev.test()
    host = Tester(cfg, model, HostPrepared(base, VOXEL, points_lim, SEED), str(tmp_path / "host"), pairs_per_forward=ppf, evaluate=True,
                  estimate_normals=True)
    host.test()
    return dev, host, str(benchmark)


def assert_same_run(tmp_path, dev, host, benchmark, n):
    assert dev.metrics == host.metrics and dev.metrics["pairs"] == n, (dev.metrics, host.metrics)
    assert dev.records.n_scores == host.records.n_scores and min(dev.records.n_scores.values()) > 0
    for i in range(n):
        assert np.array_equal(np.array(dev.records.aux[i]).view(np.uint64), np.array(host.records.aux[i]).view(np.uint64)), i
        assert torch.equal(dev.records[i], host.records[i]), i
        a, b = torch.load(tmp_path / "dev" / benchmark / f"{i}.pth"), torch.load(tmp_path / "host" / benchmark / f"{i}.pth")
        for k in ("src_raw_pcd", "src_pcd", "tgt_pcd", "src_corr_pts", "tgt_corr_pts", "confidence"):
            assert torch.equal(a[k], b[k]), (i, k)


def test_tester_voxel_grid_equals_host_prepared_dataset(tmp_path):
    from roitr_amd.tester import SyntheticPairs
    dev, host, bm = run_both(tmp_path, "3DMatch", SyntheticPairs(2, n_points=20000))
    assert_same_run(tmp_path, dev, host, bm, 2)
    d = torch.load(tmp_path / "dev" / bm / "0.pth")
    assert d["src_pcd"].shape[0] == 4704 and d["tgt_pcd"].shape[0] == 4518 and torch.equal(d["src_pcd"], d["src_raw_pcd"])


def test_tester_cap_after_the_grid_and_sharding_invariance(tmp_path):
    from roitr_amd.tester import SyntheticPairs
    dev, host, bm = run_both(tmp_path, "3DMatch", SyntheticPairs(2, n_points=20000), points_lim=CAP)
    assert_same_run(tmp_path, dev, host, bm, 2)
    d = torch.load(tmp_path / "dev" / bm / "1.pth")
    assert d["src_pcd"].shape[0] == CAP and d["tgt_pcd"].shape[0] == CAP
    # one pair per forward: the kept rows follow the GLOBAL pair id, not the position in the call
    one, host1, _ = run_both(tmp_path / "one", "3DMatch", SyntheticPairs(2, n_points=20000), points_lim=CAP, ppf=1)
    assert one.metrics == dev.metrics
    assert torch.equal(torch.load(tmp_path / "one" / "dev" / bm / "1.pth")["src_pcd"], d["src_pcd"])


def test_tester_points_lim_alone(tmp_path):
    from gpu_util import build_model
    from roitr_amd.config import test_config
    from roitr_amd.tester import SyntheticPairs, Tester
    t = Tester(test_config("3DMatch"), build_model("3DMatch", weights="selective"), SyntheticPairs(1, n_points=4000), str(tmp_path),
               evaluate=True, points_lim=2500, subsample_seed=SEED)
    t.test()
    d = torch.load(tmp_path / "3DMatch" / "0.pth")
    src = SyntheticPairs(1, n_points=4000)[0]["src_points"]
    assert torch.equal(d["src_pcd"], src[torch.from_numpy(V.subsample_cloud(4000, 2500, 0, SEED)).long()])
    assert d["tgt_pcd"].shape[0] == 2500 and t.metrics["pairs"] == 1


def test_tester_nonrigid_pair_attribute_mean_and_metric_index(tmp_path):
    from roitr_amd.tester import SyntheticPairs
    base = SyntheticPairs(1, n_points=20000, nonrigid=True)
    dev, host, bm = run_both(tmp_path, "4DMatch", base, ppf=1)
    assert_same_run(tmp_path, dev, host, bm, 1)
    a, b = torch.load(tmp_path / "dev" / bm / "0.pth"), torch.load(tmp_path / "host" / bm / "0.pth")
    it = {k: v.numpy() for k, v in base[0].items()}
    s = V.voxel_batch(it["raw_src_pcd"], [20000], VOXEL, it["src_points"])
    assert np.array_equal(a["src_pcd"].numpy().view(np.uint32), s["attr"].view(np.uint32))            # the deformed cloud: attribute means
    assert np.array_equal(a["src_raw_pcd"].numpy().view(np.uint32), s["points"].view(np.uint32))
    assert not torch.equal(a["src_pcd"], a["src_raw_pcd"])
    mi = a["metric_index_list"].numpy()
    assert np.array_equal(mi, np.unique(s["inverse"][it["metric_index"]])) and np.array_equal(mi, b["metric_index_list"].numpy())
    assert (np.diff(mi) > 0).all() and mi.max() < len(s["points"])
    assert dev.nonrigid == host.nonrigid and dev.nonrigid[0][1] == len(mi)
