"""GPU: the batched validation losses (roitr_amd/loss.py, csrc/loss.hip) against the float64 restatements of tests/loss_util.py.

Bounds.  f_count: exact -- every generated case is decided (loss_util's docstring).  f_loss / c_loss: relative F32_BOUND = 8 x the
deviation of the reference's own fp32 result from float64 (1.024e-06).  End to end the engine's outputs are not decided: the count
may differ by the number of ambiguous entries and the loss must lie inside the span those entries allow, widened by the bound.

Sizes.  Fine: L = 64 (the engine's) and L = 37 (row stride 38: no alignment at all), pairs of 0, 1, 3 and 257 patches (the pair
reduction strides by 256).  Coarse: (1, 1), (16, 16), (78, 125), (130, 63) around the 64-wide tile edges and the four-row / 64-column
blocks of the row and column kernels, and one (1024, 1024)."""
import numpy as np
import pytest
import torch

import loss_util as U

pytestmark = pytest.mark.gpu

_CACHE = {}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


# ------------------------------------------------------------------------------------------------ fine loss
def fine_cases(L):
    """Five pairs of 3, 1, 0, 257 and 0 patches.  Pair 0's first patch: every valid row and column is slack (its source points sit
    0.3 m away); pair 1's only patch has all masks false; the rest as generated.  Decided after the edits."""
    if ("fine", L) not in _CACHE:
        cases = []
        for seed, patches in enumerate((3, 1, 0, 257, 0)):
            c = U.make_case(40 + seed, L, max(patches, 1), 4, 4, n_gt=2, decided=False)
            if patches == 0:
                c = {k: (v[:0] if k in ("tgt_pts", "src_pts", "tgt_masks", "src_masks", "scores") else v) for k, v in c.items()}
            if seed == 0:
                away = U.apply(c["rot"].astype(np.float64).T, np.zeros(3), c["tgt_pts"][0].astype(np.float64) + 0.3 - c["trans"])
                c["src_pts"][0] = away.astype(np.float32)
            if seed == 1:
                c["tgt_masks"][:] = False
                c["src_masks"][:] = False
            U.decide(c)
            cases.append(c)
        _CACHE[("fine", L)] = (cases, [U.fine_f64(c) for c in cases])
    return _CACHE[("fine", L)]


def run_fine(case_list, radius=U.RADIUS):
    from roitr_amd.loss import fine_loss_batch
    n = [c["scores"].shape[0] for c in case_list]
    first = np.concatenate([[0], np.cumsum(n)])[:-1].astype(np.int32)
    cat = lambda k: np.concatenate([c[k] for c in case_list])
    out = fine_loss_batch(dev(first), dev(np.asarray(n, np.int32)), dev(cat("tgt_pts")), dev(cat("src_pts")), dev(cat("tgt_masks")),
                          dev(cat("src_masks")), dev(cat("scores")), dev(np.stack([c["rot"] for c in case_list])),
                          dev(np.stack([c["trans"] for c in case_list])), radius)
    return dict(zip(("f_loss", "f_sum", "f_count", "status"), (t.cpu().numpy() for t in out)))


@pytest.mark.parametrize("L", [64, 37])
def test_fine_loss_against_float64_in_a_ragged_batch(L):
    from roitr_amd.loss import FINE_EMPTY
    cases, want = fine_cases(L)
    got = run_fine(cases)
    assert want[0]["labels"][0, :-1, :-1].sum() == 0 and want[0]["labels"][0, :-1, -1].sum() > 0   # the all-slack patch
    for b, w in enumerate(want):
        print(f"L {L} pair {b}: count {got['f_count'][b]} (float64 {w['count']}), f_loss {got['f_loss'][b]:.7f} (float64 {w['loss']:.9f})")
        assert got["f_count"][b] == w["count"], b
        if w["count"] == 0:
            assert np.isnan(got["f_loss"][b]) and got["status"][b] == FINE_EMPTY, b
        else:
            assert got["status"][b] == 0 and U.rel(got["f_loss"][b], w["loss"]) <= U.F32_BOUND, (b, got["f_loss"][b], w["loss"])
            assert U.rel(got["f_sum"][b], w["sum"]) <= U.F32_BOUND
    assert [w["count"] == 0 for w in want] == [False, True, True, False, True]


@pytest.mark.parametrize("L", [64, 37])
def test_fine_loss_is_bitwise_batch_independent_and_repeatable(L):
    cases, _ = fine_cases(L)
    first = run_fine(cases)
    for b, c in enumerate(cases):
        alone = run_fine([c])
        for k in first:
            assert np.array_equal(bits(first[k][b:b + 1]), bits(alone[k])), (b, k)
    other = run_fine(cases[::-1])   # other slots, other neighbours
    for k in first:
        assert np.array_equal(bits(first[k]), bits(other[k][::-1])), k
    for _ in range(2):
        again = run_fine(cases)
        for k in first:
            assert np.array_equal(bits(first[k]), bits(again[k])), k


def test_fine_loss_refusals():
    from roitr_amd import _lib
    from roitr_amd.loss import BAD_OFFSETS, fine_loss_batch
    z = lambda *s: torch.zeros(s, device="cuda")
    one = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")
    eye = torch.eye(3, device="cuda")[None]
    with pytest.raises(_lib.RoitrError, match="status 3"):   # L = 65: unsupported, nothing is launched
        fine_loss_batch(one(0), one(1), z(1, 65, 3), z(1, 65, 3), z(1, 65), z(1, 65), z(1, 66, 66), eye, z(1, 3))
    # a count beyond the buffers: the pair counts as empty, nothing is read through it
    out = fine_loss_batch(one(0), one(3), z(2, 8, 3), z(2, 8, 3), z(2, 8), z(2, 8), z(2, 9, 9), eye, z(1, 3))
    assert int(out[3][0]) & BAD_OFFSETS and torch.isnan(out[0][0])
    # first slots out of order: the slot-to-pair search has nothing to stand on, every pair of the call is emptied and flagged
    two = lambda a, b: torch.tensor([a, b], dtype=torch.int32, device="cuda")
    out = fine_loss_batch(two(1, 0), two(1, 1), z(2, 8, 3), z(2, 8, 3), z(2, 8), z(2, 8), z(2, 9, 9), eye.repeat(2, 1, 1), z(2, 3))
    assert all(int(v) & BAD_OFFSETS for v in out[3]) and bool(torch.isnan(out[0]).all())
    cases, want = fine_cases(64)
    assert run_fine(cases[:1])["f_count"][0] == want[0]["count"]   # the next call works


# ------------------------------------------------------------------------------------------------ coarse loss
def coarse_cases():
    """(1, 1), (16, 16), (78, 125), (130, 63), (1024, 1024), and a (40, 50) pair whose overlaps all lie in (0, 0.1]: no positive."""
    if "coarse" not in _CACHE:
        sizes = ((1, 1, 1), (16, 16, 60), (78, 125, 300), (130, 63, 300), (1024, 1024, 20000), (40, 50, 100))
        cases = [U.make_case(60 + i, 4, 1, nt, ns, n_gt=g, decided=False) for i, (nt, ns, g) in enumerate(sizes)]
        cases[5]["gt_overlaps"] = (cases[5]["gt_overlaps"] * np.float32(0.1)).astype(np.float32)
        _CACHE["coarse"] = (cases, [U.coarse_f64(c) for c in cases])
    return _CACHE["coarse"]


def run_coarse(case_list):
    from roitr_amd.loss import coarse_loss_batch
    nt, ns = [c["tgt_feats"].shape[0] for c in case_list], [c["src_feats"].shape[0] for c in case_list]
    cap = max(len(c["gt_overlaps"]) for c in case_list)
    gi, go = np.zeros((len(case_list), cap, 2), np.int32), np.zeros((len(case_list), cap), np.float32)
    for b, c in enumerate(case_list):
        gi[b, :len(c["gt_idx"])], go[b, :len(c["gt_overlaps"])] = c["gt_idx"], c["gt_overlaps"]
    first = lambda n: np.concatenate([[0], np.cumsum(n)])[:-1].astype(np.int32)
    i32 = lambda v: dev(np.asarray(v, np.int32))
    c_loss, status = coarse_loss_batch(dev(np.concatenate([c["tgt_feats"] for c in case_list])), dev(first(nt)), i32(nt),
                                       dev(np.concatenate([c["src_feats"] for c in case_list])), dev(first(ns)), i32(ns), max(nt), max(ns),
                                       dev(gi), dev(go), i32([len(c["gt_overlaps"]) for c in case_list]), **U.CIRCLE)
    return dict(c_loss=c_loss.cpu().numpy(), status=status.cpu().numpy())


def test_coarse_loss_against_float64():
    from roitr_amd.loss import COARSE_EMPTY
    cases, want = coarse_cases()
    ov = cases[2]["gt_overlaps"]
    assert ((ov > 0) & (ov <= 0.1)).sum() > 0   # listed pairs that are neither positive nor negative
    got = run_coarse(cases)
    for b, w in enumerate(want):
        print(f"pair {b} {cases[b]['tgt_feats'].shape[0]} x {cases[b]['src_feats'].shape[0]}: c_loss {got['c_loss'][b]:.7f} (float64 {w['loss']:.9f})")
        if np.isnan(w["loss"]):
            assert np.isnan(got["c_loss"][b]) and got["status"][b] == COARSE_EMPTY, b
        else:
            assert got["status"][b] == 0 and U.rel(got["c_loss"][b], w["loss"]) <= U.F32_BOUND, (b, got["c_loss"][b], w["loss"])
    assert [bool(np.isnan(w["loss"])) for w in want] == [True, False, False, False, False, True]


def test_coarse_loss_is_bitwise_batch_independent_and_repeatable():
    cases, _ = coarse_cases()
    first = run_coarse(cases)
    for b, c in enumerate(cases):
        alone = run_coarse([c])
        for k in first:
            assert np.array_equal(bits(first[k][b:b + 1]), bits(alone[k])), (b, k)
    for _ in range(2):
        again = run_coarse(cases)
        for k in first:
            assert np.array_equal(bits(first[k]), bits(again[k])), k


def test_coarse_loss_refusals():
    from roitr_amd import _lib
    from roitr_amd.loss import BAD_INDEX, coarse_loss_batch
    cases, want = coarse_cases()
    c = dict(cases[1])
    i32 = lambda v: dev(np.asarray(v, np.int32))
    args = lambda feats_t, gi: (dev(feats_t), i32([0]), i32([16]), dev(c["src_feats"]), i32([0]), i32([16]), 16, 16, dev(gi[None].astype(np.int32)),
                                dev(c["gt_overlaps"][None]), i32([len(c["gt_overlaps"])]))
    with pytest.raises(_lib.RoitrError, match="status 3"):   # D % 4 != 0
        coarse_loss_batch(dev(c["tgt_feats"][:, :254]), i32([0]), i32([16]), dev(c["src_feats"][:, :254]), i32([0]), i32([16]), 16, 16,
                          dev(c["gt_idx"][None].astype(np.int32)), dev(c["gt_overlaps"][None]), i32([len(c["gt_overlaps"])]))
    bad = c["gt_idx"].copy()
    bad[0] = (16, 0)   # one past the last target node: skipped, never dereferenced
    _, status = coarse_loss_batch(*args(c["tgt_feats"], bad), **U.CIRCLE)
    assert int(status[0]) & BAD_INDEX
    got, status = coarse_loss_batch(*args(c["tgt_feats"], c["gt_idx"]), **U.CIRCLE)
    assert int(status[0]) == 0 and U.rel(float(got[0]), want[1]["loss"]) <= U.F32_BOUND


# ------------------------------------------------------------------------------------------------ end to end
def _case_of(o, pair):
    """A loss_util case from one pair's output dict."""
    n = lambda t: t.cpu().numpy()
    return dict(tgt_feats=n(o["tgt_node_feats"]), src_feats=n(o["src_node_feats"]), gt_idx=n(o["gt_node_corr_indices"]),
                gt_overlaps=n(o["gt_node_corr_overlaps"]), tgt_pts=n(o["tgt_node_corr_knn_points"]), src_pts=n(o["src_node_corr_knn_points"]),
                tgt_masks=n(o["tgt_node_corr_knn_masks"]), src_masks=n(o["src_node_corr_knn_masks"]), scores=n(o["matching_scores"]),
                rot=n(pair["rot"]).reshape(3, 3), trans=n(pair["trans"]).reshape(3))


@pytest.mark.parametrize("benchmark,config", [("3DMatch", 1), ("4DMatch", 4)])
def test_loss_batch_end_to_end_in_both_patch_layouts(benchmark, config):
    from gpu_util import build_model, pair_to_device
    from roitr_amd.config import test_config
    from roitr_amd.loss import OverallLoss, loss_batch
    from roitr_amd.synthetic import make_pair
    model = build_model(benchmark, weights="selective")
    cfg = test_config(benchmark)
    pairs = [pair_to_device(make_pair(1024, config=config, pair_index=20 + i, normals="field")) for i in range(3)]
    with torch.no_grad():
        h = model.launch_batch(pairs, want_gt=True)
        outs = model.finish_batch(h)
        assert h["compacted"] == (benchmark == "4DMatch")
        loss, c_loss, f_loss, f_count, status = (t.cpu().numpy() for t in loss_batch(h, cfg))
        single = OverallLoss(cfg)
        for b, (o, p) in enumerate(zip(outs, pairs)):
            case = _case_of(o, p)
            assert case["scores"].shape[0] > 0, "the forward selected no patches: nothing to evaluate"
            c64, f64 = U.coarse_f64(case), U.fine_f64(case)
            lo, hi, n_amb = U.fine_interval(case)
            print(f"{benchmark} pair {b}: {case['scores'].shape[0]} patches, f_count {f_count[b]} (float64 {f64['count']}, {n_amb} ambiguous), "
                  f"f_loss {f_loss[b]:.7f} in [{lo:.7f}, {hi:.7f}], c_loss {c_loss[b]:.7f} (float64 {c64['loss']:.9f}), status {status[b]}")
            assert abs(int(f_count[b]) - f64["count"]) <= n_amb, b
            if n_amb == 0 and f64["count"] == 0:
                assert np.isnan(f_loss[b])
            else:
                assert lo - abs(lo) * U.F32_BOUND <= f_loss[b] <= hi + abs(hi) * U.F32_BOUND, (b, f_loss[b], lo, hi)
            if np.isnan(c64["loss"]):
                assert np.isnan(c_loss[b])
            else:
                assert U.rel(c_loss[b], c64["loss"]) <= U.F32_BOUND, (b, c_loss[b], c64["loss"])
            r = single(o, dict(rot=p["rot"], trans=p["trans"]))
            for key, batch_value in (("loss", loss[b]), ("c_loss", c_loss[b]), ("f_loss", f_loss[b])):
                assert np.array_equal(bits(np.float32(r[key].cpu().numpy()).reshape(1)), bits(batch_value.reshape(1))), (b, key)
            assert np.array_equal(bits(r["o_loss"].cpu().numpy().reshape(1)), bits((np.float32(0.0) * f_loss[b]).reshape(1)))
    from roitr_amd import _lib
    with torch.no_grad():
        h2 = model.launch_batch(pairs, want_gt=False)
        model.finish_batch(h2)
    with pytest.raises(_lib.RoitrError, match="rot / trans"):
        loss_batch(h2, cfg)


def test_tester_validate_reports_the_six_means(tmp_path):
    from gpu_util import build_model
    from roitr_amd.config import test_config
    from roitr_amd.tester import SyntheticPairs, Tester
    model = build_model("3DMatch", weights="selective")
    cfg = test_config("3DMatch")
    t = Tester(cfg, model, SyntheticPairs(4, 1024), str(tmp_path / "val"), pairs_per_forward=3, validate=True)
    t.test()
    v = t.validation
    assert set(("loss", "c_loss", "f_loss", "o_loss", "PIR", "IR")) <= set(v) and v["pairs"] == 4 and sorted(t.losses) == [0, 1, 2, 3]
    for col, key in enumerate(("loss", "c_loss", "f_loss", "o_loss")):
        vals = [x[col] for x in t.losses.values() if x[col] == x[col]]
        assert v["skipped"][key] == 4 - len(vals)
        assert abs(v[key] - sum(vals) / len(vals)) < 1e-12 if vals else v[key] != v[key], key
    assert v["PIR"] == t.metrics["PIR"] and v["IR"] == t.metrics["IR"]
    irs = [a[0] for a in t.records.aux.values()]
    assert abs(v["IR"] - sum(irs) / 4) < 1e-12
    assert v["o_loss"] == 0.0 and v["f_loss"] > 0.0
    # the per-pair values do not depend on how the pairs are batched
    one = Tester(cfg, model, SyntheticPairs(4, 1024), str(tmp_path / "one"), pairs_per_forward=1, validate=True)
    one.test()
    assert one.losses == t.losses
    plain = Tester(cfg, model, SyntheticPairs(2, 1024), str(tmp_path / "plain"), pairs_per_forward=2, evaluate=True)
    plain.test()
    assert plain.validation is None and plain.losses is None
