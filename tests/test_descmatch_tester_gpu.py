"""GPU: Tester(evaluate=True, descriptor_eval=True) -- the desc_* metrics exist, do not depend on pairs_per_forward, and nothing that
existed before changes."""
import pytest

pytestmark = pytest.mark.gpu


def test_tester_descriptor_eval(tmp_path):
    from gpu_util import build_model
    from roitr_amd.config import test_config
    from roitr_amd.tester import SyntheticPairs, Tester
    model = build_model("3DMatch")
    cfg = test_config("3DMatch")
    def run(name, ppf, desc):
        t = Tester(cfg, model, SyntheticPairs(4, 1024), str(tmp_path / name), pairs_per_forward=ppf, evaluate=True, descriptor_eval=desc)
        counts = t.test()
        return t, counts
    t2, c2 = run("ppf2", 2, True)
    t4, c4 = run("ppf4", 4, True)
    t0, c0 = run("plain", 2, False)
    for k in ("desc_IR_wo", "desc_IR_w", "desc_FMR"):
        assert k in t2.metrics and t2.metrics[k] == t4.metrics[k], k
        assert 0.0 <= t2.metrics[k] <= 1.0
        assert k not in t0.metrics
    assert sorted(t2.descriptor) == [0, 1, 2, 3] and t2.descriptor == t4.descriptor
    assert all(n_w >= 1 for _, _, n_w in t2.descriptor.values())   # the global maximum of a score matrix is always mutual
    assert t0.descriptor is None
    print({k: v for k, v in t2.metrics.items() if k.startswith("desc_")}, t2.descriptor)
    assert c0 == c2 == c4
    for k, v in t0.metrics.items():   # every key that existed before, bit for bit
        assert t2.metrics[k] == v or (v != v and t2.metrics[k] != t2.metrics[k]), k
    assert t0.records.n_scores == t2.records.n_scores and repr(t0.records.aux) == repr(t2.records.aux)
