"""GPU: the batched NFMR (roitr_amd/nonrigid.py, csrc/nonrigid.hip) against the float64 restatement of tests/nfmr_util.py and
against what the reference computed (tests/golden/nfmr_ref.npz).

Bounds.  anchor_idx: exact -- the fp32 difference-form distances order like the float64 ones unless two DIFFERENT points are within
rounding of each other, and bit-equal distances (duplicate points) go to the lowest index in both.  err: 1e-5 absolute -- every
coordinate is below 4 m (tests/test_nfmr_cpu.py asserts it), one fp32 ulp there is 4.8e-7 and the chain after the search is about
twenty operations.  Metric points nfmr_util.ambiguous() names (a third / fourth anchor within 1e-6 of each other, a neighbour within
1e-6 of the radius, an error within 1e-5 of the threshold) are left out of the per-point checks and bound the hit-count difference;
they must stay at most 1 % of a case."""
import os

import numpy as np
import pytest
import torch

import nfmr_util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_F64 = {}


def cases():
    if "cases" not in _F64:
        _F64["cases"] = U.twelve_cases()
        _F64["res"] = [U.nfmr_f64(c) for c in _F64["cases"]]
        _F64["amb"] = [U.ambiguous(c, r) for c, r in zip(_F64["cases"], _F64["res"])]
    return _F64["cases"], _F64["res"], _F64["amb"]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def run(case_list, **kw):
    """nfmr_batch over the given cases as ONE ragged batch."""
    from roitr_amd.nonrigid import nfmr_batch
    def offs(key):
        return dev(np.concatenate([[0], np.cumsum([len(c[key]) for c in case_list])]).astype(np.int32))
    def cat(key):
        return dev(np.concatenate([c[key] for c in case_list]))
    kw.setdefault("return_errors", True)
    out = nfmr_batch(offs("src_raw"), cat("src_raw"), cat("src_deformed"), offs("src_corr"), cat("src_corr"), cat("tgt_corr"),
                     offs("metric_index"), cat("metric_index"), dev(np.stack([c["rot"] for c in case_list])),
                     dev(np.stack([c["trans"] for c in case_list])), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def split(out, case_list):
    """Per-case views of a batch result."""
    co = np.concatenate([[0], np.cumsum([len(c["src_corr"]) for c in case_list])])
    mo = np.concatenate([[0], np.cumsum([len(c["metric_index"]) for c in case_list])])
    return [dict(anchor_idx=out["anchor_idx"][co[i]:co[i + 1]], err=out["err"][mo[i]:mo[i + 1]], hits=int(out["hits"][i]),
                 nfmr=float(out["nfmr"][i]), status=int(out["status"][i]), n_metric=int(out["n_metric"][i])) for i in range(len(case_list))]


@pytest.fixture(scope="module")
def alone():
    cs, _, _ = cases()
    return [split(run([c]), [c])[0] for c in cs]


def test_anchor_indices_are_the_float64_lowest_index_argmin(alone):
    cs, res, _ = cases()
    for i, (got, want) in enumerate(zip(alone, res)):
        assert np.array_equal(got["anchor_idx"], want["anchor_idx"]), (i, int((got["anchor_idx"] != want["anchor_idx"]).sum()))
    # the duplicate-point case really exercises the rule: some correspondences sit on a point that exists twice
    dup = cs[7]
    d = dup["src_deformed"]
    twice = (d[:, None, :] == d[None, -64:, :]).all(-1).sum(1) > 0
    assert twice[res[7]["anchor_idx"]].sum() > 0


def test_per_point_error_within_1e5_of_float64(alone):
    _, res, amb = cases()
    for i, (got, want, a) in enumerate(zip(alone, res, amb)):
        worst = float(np.abs(got["err"] - want["err"])[~a].max())
        print(f"case {i}: max |err - float64| = {worst:.3e} over {int((~a).sum())} points, {int(a.sum())} ambiguous")
        assert a.sum() <= 0.01 * len(a), (i, int(a.sum()))
        assert worst < 1e-5, (i, worst)


def test_hit_count_matches_float64_up_to_the_ambiguous_points(alone):
    _, res, amb = cases()
    for i, (got, want, a) in enumerate(zip(alone, res, amb)):
        print(f"case {i}: hits {got['hits']} vs float64 {want['hits']} ({int(a.sum())} ambiguous)")
        assert abs(got["hits"] - want["hits"]) <= int(a.sum()), (i, got["hits"], want["hits"])
        assert got["n_metric"] == len(a) and got["status"] == 0
        assert abs(got["nfmr"] - got["hits"] / len(a)) < 1e-6
        assert got["hits"] == int((got["err"] < U.THR).sum())


def test_golden_reference_recall_and_blend(alone):
    from roitr_amd.nonrigid import blend_anchor_motion, compute_nrfmr
    cs, res, amb = cases()
    g = np.load(os.path.join(ROOT, "tests", "golden", "nfmr_ref.npz"))
    for s in range(6):
        c, a = cs[s], amb[s]
        assert U.checksum(c) == str(g[f"checksum_{s}"])
        ref_hits = round(float(g[f"recall_{s}"]) * len(a))
        assert abs(alone[s]["hits"] - ref_hits) <= int(a.sum()), (s, alone[s]["hits"], ref_hits)
        # the reference's signature over one saved-file dict
        data = dict(src_raw_pcd=torch.from_numpy(c["src_raw"]), src_pcd=torch.from_numpy(c["src_deformed"]),
                    src_corr_pts=torch.from_numpy(c["src_corr"]), tgt_corr_pts=torch.from_numpy(c["tgt_corr"]),
                    metric_index_list=torch.from_numpy(c["metric_index"]), rot=torch.from_numpy(c["rot"]),
                    trans=torch.from_numpy(c["trans"]).reshape(3, 1))
        r = compute_nrfmr(data, recall_thr=U.THR)
        assert abs(float(r) - alone[s]["nfmr"]) < 1e-7
        anchor = c["src_raw"][res[s]["anchor_idx"]]
        flow, mask = blend_anchor_motion(c["src_raw"][c["metric_index"]], anchor, c["tgt_corr"] - anchor, knn=3, search_radius=U.RADIUS)
        assert flow.dtype == np.float32 and mask.dtype == bool
        worst = float(np.abs(flow - g[f"flow_{s}"])[~a].max())
        print(f"seed {s}: max |flow - reference| = {worst:.3e}")
        assert worst < 1e-5, (s, worst)
        assert np.array_equal(mask[~a], g[f"mask_{s}"][~a])


def test_ragged_batch_is_bitwise_the_cases_alone_and_repeatable(alone):
    cs, _, _ = cases()
    batch = list(cs) + [U.truncated(cs[9], 40)]
    solo = alone + [split(run([batch[-1]]), [batch[-1]])[0]]
    first = run(batch)
    for i, (a, b) in enumerate(zip(split(first, batch), solo)):
        assert np.array_equal(a["anchor_idx"], b["anchor_idx"]), i
        assert np.array_equal(a["err"].view(np.int32), b["err"].view(np.int32)), i
        assert a["hits"] == b["hits"] and a["status"] == b["status"] and a["nfmr"] == b["nfmr"], i
    for _ in range(2):
        again = run(batch)
        for k in first:
            assert np.array_equal(first[k].view(np.int32) if first[k].dtype == np.float32 else first[k],
                                  again[k].view(np.int32) if again[k].dtype == np.float32 else again[k]), k
    for block in (64, 128, 256):    # the block size is a launch parameter, not part of the result
        other = run(batch, block=block)
        for k in ("anchor_idx", "hits", "status"):
            assert np.array_equal(first[k], other[k]), (block, k)
        assert np.array_equal(first["err"].view(np.int32), other["err"].view(np.int32)), block


def test_edges():
    from roitr_amd import _lib
    from roitr_amd.nonrigid import BAD_INDEX, FEW_ANCHORS, NO_METRIC, blend_anchor_motion, nfmr_batch
    cs, _, _ = cases()
    base = cs[3]
    empty_metric = dict(base, metric_index=base["metric_index"][:0])
    batch = [U.truncated(base, 0), U.truncated(base, 2), empty_metric, base]
    out = run(batch)
    parts = split(out, batch)
    assert [p["status"] for p in parts] == [FEW_ANCHORS, FEW_ANCHORS, NO_METRIC, 0]
    assert [p["hits"] for p in parts[:3]] == [0, 0, 0] and [p["nfmr"] for p in parts[:3]] == [0.0, 0.0, 0.0]
    assert np.isinf(parts[0]["err"]).all() and np.isinf(parts[1]["err"]).all()
    assert parts[3]["hits"] == split(run([base]), [base])[0]["hits"] > 0

    # every anchor beyond the radius: three equal weights, the point still counts; and a metric point ON an anchor: the 1e-10 clamp
    rng = np.random.default_rng(5)
    raw = rng.uniform(0.0, 0.2, (64, 3)).astype(np.float32)
    raw[0] = (3.0, 3.0, 3.0)                                      # metric point 0: >= 4.8 m from every anchor
    raw[1] = raw[10]                                              # metric point 1: coincides with the anchor of correspondence 0
    deformed = raw + np.float32(0.01)
    corr_idx = np.arange(10, 40)
    case = dict(src_raw=raw, src_deformed=deformed, src_corr=deformed[corr_idx],
                tgt_corr=(deformed[corr_idx] + rng.uniform(-0.02, 0.02, (30, 3))).astype(np.float32),
                metric_index=np.array([0, 1, 5], np.int64), rot=np.eye(3, dtype=np.float32), trans=np.zeros(3, np.float32))
    want = U.nfmr_f64(case)
    assert not want["mask"][0] and want["d4"][1, 0] == 0.0
    got = split(run([case]), [case])[0]
    assert np.array_equal(got["anchor_idx"], want["anchor_idx"])
    assert np.abs(got["err"] - want["err"]).max() < 1e-5, (got["err"], want["err"])
    assert got["hits"] == want["hits"]
    flow, mask = blend_anchor_motion(raw[case["metric_index"]], raw[want["anchor_idx"]], case["tgt_corr"] - raw[want["anchor_idx"]])
    assert list(mask) == list(want["mask"]) and np.abs(flow - want["flow"]).max() < 1e-5
    np.testing.assert_allclose(flow[0], (case["tgt_corr"] - raw[want["anchor_idx"]])[want["nn_idx"][0]].mean(0), atol=1e-6)  # 1/3 each
    np.testing.assert_allclose(flow[1], (case["tgt_corr"] - raw[want["anchor_idx"]])[want["nn_idx"][1, 0]], atol=1e-6)       # all weight on the coincident anchor

    # an out-of-range metric index is refused, not dereferenced; the next call works
    for bad_value in (64, -1, 2 ** 40):
        bad = dict(case, metric_index=np.array([0, bad_value, 5], np.int64))
        with pytest.raises(_lib.RoitrError, match="metric_index"):
            run([bad])
    assert split(run([case]), [case])[0]["hits"] == want["hits"]
    o = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.RoitrError, match="offset"):   # 31 correspondences claimed, 30 given
        nfmr_batch(o(0, 64), dev(raw), dev(deformed), o(0, 31), dev(case["src_corr"]), dev(case["tgt_corr"]), o(0, 3), dev(case["metric_index"]),
           dev(case["rot"])[None], dev(case["trans"])[None])
    assert BAD_INDEX == 4
    with pytest.raises(NotImplementedError):
        blend_anchor_motion(raw, raw, raw, knn=4)


def test_tester_reports_nfmr_end_to_end(tmp_path):
    """Tester on non-rigid synthetic pairs with the 4DMatch test config and the selective closed-form weights: Tester.nonrigid[i]
    is the float64 restatement applied to the file written for pair i, and does not depend on pairs_per_forward."""
    from gpu_util import build_model
    from roitr_amd.config import test_config
    from roitr_amd.tester import SyntheticPairs, Tester
    model = build_model("4DMatch", weights="selective")
    cfg = test_config("4DMatch")
    n_pairs, results = 4, {}
    for ppf in (1, 4):
        out_dir = tmp_path / f"ppf{ppf}"
        tester = Tester(cfg, model, SyntheticPairs(n_pairs, 1500, nonrigid=True), str(out_dir), pairs_per_forward=ppf, evaluate=True)
        tester.test()
        assert tester.nonrigid is not None and sorted(tester.nonrigid) == list(range(n_pairs))
        results[ppf] = tester.nonrigid
        if ppf != 1:
            continue
        for i in range(n_pairs):
            data = torch.load(os.path.join(str(out_dir), str(cfg["benchmark"]), f"{i}.pth"), map_location="cpu")
            assert "metric_index_list" in data and data["metric_index_list"].numel() == 1500 // 4
            assert not torch.equal(data["src_raw_pcd"], data["src_pcd"])
            case = dict(src_raw=data["src_raw_pcd"].numpy(), src_deformed=data["src_pcd"].numpy(), src_corr=data["src_corr_pts"].numpy(),
                        tgt_corr=data["tgt_corr_pts"].numpy(), metric_index=data["metric_index_list"].numpy(),
                        rot=data["rot"].numpy().reshape(3, 3), trans=data["trans"].numpy().reshape(3))
            assert case["src_corr"].shape[0] >= 3, "the forward found no correspondences: nothing to evaluate"
            want = U.nfmr_f64(case)
            a = int(U.ambiguous(case, want).sum())
            nfmr, n_metric = tester.nonrigid[i]
            print(f"pair {i}: {case['src_corr'].shape[0]} correspondences, NFMR {nfmr:.4f}, float64 {want['nfmr']:.4f}, {a} ambiguous")
            assert n_metric == len(case["metric_index"])
            assert abs(round(nfmr * n_metric) - want["hits"]) <= a, (i, nfmr, want["nfmr"], a)
    assert results[1] == results[4]
    # without metric_index in the items nothing is computed
    plain = Tester(cfg, model, SyntheticPairs(1, 1500, config=4), str(tmp_path / "plain"), pairs_per_forward=1, evaluate=True)
    plain.test()
    assert plain.nonrigid is None
