"""GPU: the Tester's optional evaluations do not disturb each other.  Four synthetic pairs of 1024 points in two forwards (three pairs
and one) on the closed-form selective weights, through the public API only: one Tester with everything on at once (estimator
"compat", refine "plane", recall, descriptor_eval, validate, fpfh_baseline) against two narrower runs, one with only the pose options
and one with only the evaluation options.  Every attribute, metric key, record and file key that two runs share is bit-equal.

The evaluation run has no refinement, so what hangs on the refined pose there (est_transform, the registration rows, the p / success
columns of the recall rows, the estimate in the gt rows, the RR metrics) is compared between the other two runs only."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_PAIRS, N_POINTS, PER_FORWARD = 4, 1024, 3
POSE = dict(evaluate=True, estimator="compat", refine="plane")
EVALUATION = dict(estimator="compat", recall=True, descriptor_eval=True, validate=True, fpfh_baseline=dict(radius=0.3, max_nn=64))
OPTIONS = {"all": {**EVALUATION, **POSE}, "pose": POSE, "evaluation": EVALUATION}
ATTRIBUTES = ("registration", "refinement", "refinement_status", "fpfh", "recall", "gt", "descriptor", "losses", "nonrigid", "validation",
              "metrics")
# what follows the refined pose: not comparable with the evaluation run, which estimates with "compat" and does not refine
REFINED = {"file": ("est_transform",), "attribute": ("registration",), "metric": ("RR",)}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from gpu_util import build_model
    from roitr_amd.config import test_config
    from roitr_amd.tester import SyntheticPairs, Tester
    model = build_model("3DMatch", weights="selective")
    data = SyntheticPairs(N_PAIRS, N_POINTS, config=1)
    out = {}
    for name, kw in OPTIONS.items():
        d = tmp_path_factory.mktemp(name)
        t = Tester(test_config("3DMatch"), model, data, str(d), pairs_per_forward=PER_FORWARD, **kw)
        t.test()
        out[name] = (t, [torch.load(d / "3DMatch" / f"{i}.pth") for i in range(N_PAIRS)])
    return out


def same(a, b):
    """Bit equality through dicts, tuples, lists, tensors, arrays and numbers; nan equals nan."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.numpy(), b.numpy(), equal_nan=a.is_floating_point())
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return type(a) is type(b) and a == b


def test_the_runs_are_what_they_are_meant_to_be(runs):
    every, pose, evaluation = (runs[k][0] for k in ("all", "pose", "evaluation"))
    assert all(getattr(every, a) is not None for a in ATTRIBUTES if a != "nonrigid") and every.nonrigid is None
    assert pose.refinement and pose.registration and pose.recall is None and pose.descriptor is None and pose.fpfh is None
    assert evaluation.recall and evaluation.fpfh and evaluation.losses and evaluation.descriptor and evaluation.refinement is None
    assert sorted(every.registration) == sorted(every.recall) == sorted(every.fpfh) == sorted(every.losses) == list(range(N_PAIRS))
    assert set(runs["all"][1][0]) - set(runs["pose"][1][0]) == {"gt_overlap", "gt_info"} and len(runs["all"][1][0]) == 19
    assert {"desc_FMR", "RR", "fpfh_success", "PIR"} <= set(every.metrics) and every.validation["pairs"] == N_PAIRS


@pytest.mark.parametrize("one, other", [("all", "pose"), ("all", "evaluation"), ("pose", "evaluation")])
def test_what_two_runs_share_is_bit_equal(runs, one, other):
    (a, files_a), (b, files_b) = runs[one], runs[other]
    refined = other != "evaluation"       # both runs refine: the pose-dependent values are comparable too
    compared = []
    for name in ATTRIBUTES:
        x, y = getattr(a, name), getattr(b, name)
        if x is None or y is None or (name in REFINED["attribute"] and not refined):
            continue
        if name == "metrics":
            shared = [k for k in x if k in y and (refined or not k.startswith(REFINED["metric"]))]
            assert shared and all(same(x[k], y[k]) for k in shared), (name, x, y)
        elif name == "recall" and not refined:
            assert same({k: v[:2] for k, v in x.items()}, {k: v[:2] for k, v in y.items()}), (name, x, y)     # the overlap ratios
        elif name == "gt" and not refined:
            assert same({k: v[:3] for k, v in x.items()}, {k: v[:3] for k, v in y.items()}), (name, x, y)     # T_gt, info, overlap_src
        else:
            assert same(x, y), (name, x, y)
        compared.append(name)
    assert "metrics" in compared, compared
    assert sorted(a.records.keys()) == sorted(b.records.keys()) == list(range(N_PAIRS))
    assert all(torch.equal(a.records[i], b.records[i]) for i in range(N_PAIRS))
    assert same(dict(a.records.aux), dict(b.records.aux)) and a.records.n_scores == b.records.n_scores
    for f, g in zip(files_a, files_b):
        keys = [k for k in f if k in g]
        assert keys == [k for k in g if k in f] and len(keys) >= 16          # the shared keys stand in the same order
        for k in keys:
            if refined or k not in REFINED["file"]:
                assert same(f[k], g[k]), k
