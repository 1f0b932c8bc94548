"""CPU: the ground the validation-loss GPU tests stand on -- the float64 restatements (tests/loss_util.py) against what the
reference's lib/loss.py OverallLoss computed (tests/golden/loss_ref.npz), the decided-case rule, the new ABI and the config keys."""
import ctypes
import os

import numpy as np

import loss_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "loss_ref.npz"))


def test_float64_restatement_reproduces_the_reference_losses():
    g = golden()
    worst = 0.0
    for i, case in enumerate(U.golden_cases()):
        assert U.checksum(case) == str(g[f"checksum_{i}"]), i   # the regenerated inputs are the ones the reference saw
        c, f = U.coarse_f64(case), U.fine_f64(case)
        assert f["count"] == int(g[f"f_count_{i}"]), i          # decided cases: the label count is exact
        dc, df = U.rel(g[f"c_loss_{i}"], c["loss"]), U.rel(g[f"f_loss_{i}"], f["loss"])
        print(f"case {i}: c_loss rel {dc:.3e}, f_loss rel {df:.3e}")
        worst = max(worst, dc, df)
    assert worst <= U.REF_DEVIATION, worst
    assert worst >= 0.5 * U.REF_DEVIATION, worst   # the recorded figure is the measured one, not a loose guess
    assert U.F32_BOUND == 8 * U.REF_DEVIATION


def test_generated_cases_are_decided_and_cover_what_the_tests_assume():
    for i, size in enumerate(U.GOLDEN_SIZES):
        raw = U.make_case(i, *size, decided=False)
        before = raw["src_masks"].copy()
        share = U.decide(raw)                                  # asserts the 2 % cap itself
        assert share <= U.MAX_MASKED and share == (before & ~raw["src_masks"]).mean()
        case = U.make_case(i, *size)
        assert np.array_equal(case["src_masks"], raw["src_masks"])
        assert not U.ambiguous_entries(case).any()
        assert U.fine_error_bound(case) < 1e-6                 # |coordinates| < 0.5 m
        lo, hi, n = U.fine_interval(case)
        f = U.fine_f64(case)
        assert n == 0 and abs(lo - f["loss"]) < 1e-12 and abs(hi - f["loss"]) < 1e-12
        labels = f["labels"]
        assert labels[:, :-1, :-1].sum() > 0 and labels[:, :-1, -1].sum() > 0 and labels[:, -1, :-1].sum() > 0
        ov = case["gt_overlaps"]
        assert ((ov > 0) & (ov <= 0.1)).sum() > 0 and (ov > 0.1).sum() > 0
        c = U.coarse_f64(case)
        assert len(c["rows"]) > 0 and len(c["cols"]) > 0 and np.isfinite(c["loss"])
    # an undecided case has a real interval around its float64 value
    raw = U.make_case(1, decided=False)
    lo, hi, n = U.fine_interval(raw)
    assert n > 0 and lo < U.fine_f64(raw)["loss"] < hi


def test_restatement_edges():
    case = U.make_case(0, 16, 3, 5, 7, n_gt=10)
    none = dict(case, tgt_masks=np.zeros_like(case["tgt_masks"]), src_masks=np.zeros_like(case["src_masks"]))
    f = U.fine_f64(none)
    assert f["count"] == 0 and np.isnan(f["loss"])
    no_pos = dict(case, gt_overlaps=np.full_like(case["gt_overlaps"], 0.05))
    assert np.isnan(U.coarse_f64(no_pos)["loss"])
    # a non-positive entry adds exp(0) to the positive sum: one row, one positive with weight 0 (d < positive_optimal), one negative
    # beyond negative_optimal -> both log-sum-exps are log(2), the loss softplus(2 log 2) / 24
    t = np.zeros((1, 4), np.float32)
    s = np.array([[0.05, 0, 0, 0], [2.0, 0, 0, 0]], np.float32)
    one = dict(tgt_feats=t, src_feats=s, gt_idx=np.array([[0, 0]]), gt_overlaps=np.array([0.5], np.float32))
    c = U.coarse_f64(one)
    assert abs(c["rows"][0] - np.log1p(4.0) / 24) < 1e-12 and len(c["cols"]) == 0 and np.isnan(c["loss"])


def test_library_exports_the_loss_symbols():
    import __graft_entry__ as G
    from roitr_amd import _lib
    lib = _lib.lib()
    names = G.declared_symbols()
    for n in ("roitr_fine_loss_workspace_bytes", "roitr_fine_loss_batch", "roitr_coarse_loss_workspace_bytes", "roitr_coarse_loss_batch"):
        assert n in names and hasattr(lib, n), n
    lib.roitr_fine_loss_workspace_bytes.restype = ctypes.c_size_t
    lib.roitr_coarse_loss_workspace_bytes.restype = ctypes.c_size_t
    assert lib.roitr_fine_loss_workspace_bytes(512 * 256) >= 512 * 256 * 8
    assert lib.roitr_coarse_loss_workspace_bytes(512, 78, 125) >= 512 * 78 * 125 * 8
    assert lib.roitr_abi_version() == 4   # functions added, no struct changed


def test_config_keys_and_host_refusals():
    import pytest
    import torch
    from roitr_amd import _lib, loss
    from roitr_amd.config import test_config
    for bench in ("3DMatch", "4DMatch"):
        cfg = test_config(bench)
        for k, v in loss.DEFAULTS.items():
            assert cfg[k] == v, (bench, k)
    o = loss.OverallLoss({})   # the reference's values are the defaults
    assert o.weight_coarse_loss == 1.0 and o.weight_fine_loss == 1.0 and o.weight_occ_loss == 0.0
    assert o.fine_loss.positive_radius == 0.05 and o.coarse_loss.positive_overlap == 0.1 and o.coarse_loss.weighted_circle_loss.log_scale == 24
    z = torch.zeros(2, 4, 3)
    with pytest.raises(_lib.RoitrError):
        loss.fine_loss_batch(torch.zeros(1, dtype=torch.int32), torch.ones(1, dtype=torch.int32), z, z, torch.ones(2, 4), torch.ones(2, 4),
                             torch.zeros(2, 5, 5), torch.eye(3)[None], torch.zeros(1, 3))
    with pytest.raises(_lib.RoitrError):
        loss.loss_batch(dict(out={}, B=1, P=1, n4=[1, 1], have_gt=False), {})


def test_weighted_circle_loss_general_form_matches_the_restatement():
    import torch
    from roitr_amd.loss import WeightedCircleLoss
    case = U.make_case(2, 16, 2, 33, 41)
    want = U.coarse_f64(case)
    t, s = torch.from_numpy(case["tgt_feats"]).double(), torch.from_numpy(case["src_feats"]).double()
    d = torch.sqrt(torch.clamp((-2.0 * t @ s.T + (t ** 2).sum(1)[:, None]) + (s ** 2).sum(1)[None, :], min=1e-12))
    ov = torch.zeros_like(d)
    ov[torch.from_numpy(case["gt_idx"][:, 0]), torch.from_numpy(case["gt_idx"][:, 1])] = torch.from_numpy(case["gt_overlaps"]).double()
    pos, neg = ov > float(np.float32(0.1)), ov == 0
    got = WeightedCircleLoss(0.1, 1.4, 0.1, 1.4, 24)(pos, neg, d, torch.sqrt(ov * pos))
    assert abs(float(got) - want["loss"]) < 1e-9
