"""GPU: roitr_fgr_batch (csrc/fgr.hip through roitr_amd/fgr.py) against the float64 restatement of tests/fgr_util.py, on fixtures that
tests/test_fgr_cpu.py asserts well posed.

Exact: multiplicity, tuples_accepted, n_used, steps, status, inliers.  T within 1e-5, the project's bound for an fp32 transform against
a float64-restated solve (tests/test_lgr_gpu.py, tests/test_compat_gpu.py).  mu, objective and every trace row within 1e-9, the
bound tests/test_icp_gpu.py uses for its float64 statistics: relative for mu, objective and sum_omega, and for the 12 state values
relative to the largest of them (a rotation has entries of order 1; a translation entry near 0 has no relative error of its own).
Each step is additionally replayed in float64 from the GPU's own trace row k to its row k + 1, which bounds one step's error without
the accumulation of the chain.

Measured maxima on an MI355X over all fixtures are recorded in DESIGN.md section 7.11.
"""
import numpy as np
import pytest
import torch

import fgr_util as U

pytestmark = pytest.mark.gpu

T_TOL, STAT_TOL = 1e-5, 1e-9
FIELDS = ("T", "inliers", "n_used", "tuples_accepted", "steps", "mu", "objective", "status")
_RUNS = {}


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))   # a copy: the fixtures are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def call(sets, keys=None, offset=0, **kw):
    """fgr_batch over the (src, tgt, scores) of `sets` (scores None: no scores at all) behind `offset` rows no pair owns; numpy results."""
    from roitr_amd.fgr import fgr_batch
    sizes = [s[0].shape[0] for s in sets]
    starts = offset + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pad = np.full((offset, 3), 7.5, np.float32)
    src = np.concatenate([pad] + [s[0] for s in sets]).astype(np.float32).reshape(-1, 3)
    tgt = np.concatenate([pad] + [s[1] for s in sets]).astype(np.float32).reshape(-1, 3)
    w = None if sets[0][2] is None else np.concatenate([np.ones(offset, np.float32)] + [s[2] for s in sets])
    r = fgr_batch(dev(starts), dev(src), dev(tgt), None if w is None else dev(w), pair_keys=keys, return_trace=True,
                  return_multiplicity=True, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in r.items()}
    out["starts"] = starts
    return out


def named(name):
    if name not in _RUNS:
        (src, tgt, w, _, _), kw = U.fixture(name)
        kw = dict(kw)
        key = kw.pop("key", 0)
        _RUNS[name] = call([(src, tgt, w)], keys=[key], **kw)
    return _RUNS[name]


def rel(a, b):
    return float(abs(a - b) / max(abs(b), 1e-300))


@pytest.mark.parametrize("name", U.GPU_CASES)
def test_against_the_restatement(name):
    (src, tgt, w, _, _), kw = U.fixture(name)
    ref, got = U.reference(name), named(name)
    assert U.well_posed(ref)
    n, iters = src.shape[0], kw.get("iterations", U.ITERATIONS)
    assert np.array_equal(got["multiplicity"], ref["multiplicity"]), name
    for k in ("tuples_accepted", "n_used", "steps", "status", "inliers"):
        assert int(got[k][0]) == int(ref[k]), (name, k, got[k][0], ref[k])
    err_T = float(np.abs(got["T"][0].astype(np.float64) - ref["T"]).max())
    assert err_T < T_TOL, (name, err_T)
    assert np.array_equal(got["T"][0, 3], [0, 0, 0, 1]) and got["trace"].shape == (1, iters, 16)
    tr, rt = got["trace"][0], ref["trace"]
    ran = ref["steps"] + (1 if ref["status"] & U.SINGULAR else 0)
    assert not tr[ran:].any() and (tr[:ran, 15] == 1.0).all()
    err_state = err_stat = err_replay = 0.0
    if ran:
        err_stat = max(rel(got["mu"][0], ref["mu"]), rel(got["objective"][0], ref["objective"]))
        assert got["objective"][0] == tr[ran - 1, 13]                       # the objective of the last evaluated iteration
        scale = np.maximum(np.abs(rt[:ran, :12]).max(1), 1.0)
        err_state = float((np.abs(tr[:ran, :12] - rt[:ran, :12]).max(1) / scale).max())
        err_stat = max(err_stat, float((np.abs(tr[:ran, 12:15] - rt[:ran, 12:15]) / np.maximum(np.abs(rt[:ran, 12:15]), 1e-300)).max()))
        # one step at a time, from the GPU's own state
        used = (np.ones(n) if w is None else w.astype(np.float64)) * ref["multiplicity"] > 0
        wu = ((np.ones(n) if w is None else w.astype(np.float64)) * ref["multiplicity"])[used]
        Pc, Qc = src.astype(np.float64)[used] - ref["cs"], tgt.astype(np.float64)[used] - ref["ct"]
        md2 = float(np.float32(kw.get("max_dist", U.MAX_DIST))) ** 2
        for k in range(ran):
            S, mu = tr[k, :12].reshape(3, 4), tr[k, 12]
            A, g, obj, so = U.sums(S, mu, Pc, Qc, wu)
            err_replay = max(err_replay, rel(tr[k, 13], obj), rel(tr[k, 14], so))
            nxt = U.advance(S, mu, A, g, k, md2, kw.get("division_factor", U.DIVISION), kw.get("mu_every", U.MU_EVERY))
            if nxt is None:
                assert k == ran - 1 and ref["status"] & U.SINGULAR
            elif k + 1 < ran:
                err_replay = max(err_replay, float(np.abs(tr[k + 1, :12] - nxt[0].reshape(-1)).max() / max(np.abs(nxt[0]).max(), 1.0)),
                                 rel(tr[k + 1, 12], nxt[1]))
            else:
                err_replay = max(err_replay, rel(got["mu"][0], nxt[1]))
    else:
        assert got["mu"][0] == 0.0 and got["objective"][0] == 0.0
    print(f"{name}: |T - ref| {err_T:.2e}, trace state {err_state:.2e}, mu / objective / sum_omega {err_stat:.2e}, replayed step {err_replay:.2e}")
    assert err_state < STAT_TOL and err_stat < STAT_TOL and err_replay < STAT_TOL, (name, err_state, err_stat, err_replay)


def test_status_cases_by_their_values():
    line, two, zero = named("line"), named("two_used"), named("zero_scores")
    assert line["status"][0] == U.SINGULAR and line["steps"][0] == 0 and line["inliers"][0] == 12
    want = np.eye(4, dtype=np.float32)
    want[:3, 3] = [2.0, -0.75, 0.5]                                          # the translation that aligns the centroids, exactly
    assert np.array_equal(line["T"][0], want)
    assert two["status"][0] == U.TOO_FEW and two["n_used"][0] == 2 and np.array_equal(two["T"][0], np.eye(4, dtype=np.float32))
    assert two["steps"][0] == 0 and not two["trace"].any()
    (_, _, w, mask, _), _ = U.fixture("zero_scores")
    assert zero["n_used"][0] == int((w > 0).sum()) and zero["inliers"][0] == int(mask.sum()) > int((mask & (w > 0)).sum())
    empty = call([(np.zeros((0, 3), np.float32),) * 2 + (np.zeros(0, np.float32),)], keys=[1], tuples=64, iterations=4)
    assert empty["status"][0] == U.NO_ROWS and np.array_equal(empty["T"][0], np.eye(4, dtype=np.float32))
    assert empty["inliers"][0] == empty["n_used"][0] == empty["steps"][0] == empty["tuples_accepted"][0] == 0 and not empty["trace"].any()


def test_no_accepted_triple_equals_no_tuple_test_bitwise():
    (src, tgt, w, _, _), kw = U.fixture("no_tuples")
    a = named("no_tuples")
    b = call([(src, tgt, w)], **dict({k: v for k, v in kw.items() if k not in ("key", "seed")}, tuples=0))
    assert a["status"][0] == U.NO_TUPLES and b["status"][0] == 0 and a["tuples_accepted"][0] == 0
    for k in ("T", "inliers", "n_used", "steps", "mu", "objective", "trace", "multiplicity"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["multiplicity"] == 1).all()


def pair_view(r, b):
    s, e = int(r["starts"][b]), int(r["starts"][b + 1])
    return {k: r[k][b] for k in FIELDS} | dict(trace=r["trace"][b], multiplicity=r["multiplicity"][s:e])


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def test_bitwise_alone_in_a_ragged_batch_at_an_offset_on_a_repeat_and_on_either_path():
    """257 rows (two rows for one lane), 120 rows with repeated multiplicities, 1537 rows (one past the staging capacity: the global
    path), with empty pairs between them, behind 5 rows no pair owns."""
    names = ("n_257", "tuples_4096", "n_1537")
    sets = [U.fixture(n)[0][:3] for n in names]
    kw = dict(tuples=4096, iterations=16, seed=11)
    keys = [3, 7, 9]
    alone = [pair_view(call([s], keys=[k], **kw), 0) for s, k in zip(sets, keys)]
    assert all(a["tuples_accepted"] > 0 and a["steps"] == 16 and a["status"] == 0 for a in alone)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32))
    batch_sets = [empty, sets[0], empty, empty, sets[1], sets[2], empty]
    batch_keys = [100, 3, 101, 102, 7, 9, 103]
    runs = {cap: call(batch_sets, keys=batch_keys, offset=5, _lds_rows=cap, **kw) for cap in (None, 0, 256, 1536)}
    again = call(batch_sets, keys=batch_keys, offset=5, **kw)
    for k in runs[None]:
        assert np.array_equal(runs[None][k], again[k]), k                    # a repeat
        for cap in (0, 256, 1536):
            assert np.array_equal(runs[None][k], runs[cap][k]), (k, cap)     # staged in LDS or swept from global memory
    for slot, a in zip((1, 4, 5), alone):
        assert same(a, pair_view(runs[None], slot)), slot
    for slot in (0, 2, 3, 6):
        assert runs[None]["status"][slot] == U.NO_ROWS
    assert not runs[None]["multiplicity"][:5].any()                          # rows outside every pair are not written
    other_key = pair_view(call([sets[1]], keys=[8], **kw), 0)
    assert not np.array_equal(other_key["multiplicity"], alone[1]["multiplicity"])   # the key does reach the triples
    shuffled_slot = call([sets[1], sets[0]], keys=[7, 3], **kw)
    assert same(alone[1], pair_view(shuffled_slot, 0)) and same(alone[0], pair_view(shuffled_slot, 1))


def test_the_triples_are_those_of_ransac_samples():
    """One drawn triple: its three rows carry the multiplicity, or nothing does and the fallback sets every m to 1."""
    from roitr_amd.registration import ransac_samples
    (src, tgt, w, _, _), kw = U.fixture("tuples_1")
    tri = ransac_samples(torch.tensor([src.shape[0]], dtype=torch.int32, device="cuda"), pair_keys=[kw["key"]], seed=kw["seed"], count=1)
    tri = tri.cpu().numpy().reshape(-1)
    got = named("tuples_1")
    if got["tuples_accepted"][0] == 1:
        want = np.zeros(src.shape[0], np.int32)
        want[tri] = 1
        assert np.array_equal(got["multiplicity"], want) and got["n_used"][0] == 3
    else:
        assert got["status"][0] & U.NO_TUPLES and (got["multiplicity"] == 1).all()


def test_refusals_reach_python_as_errors():
    from roitr_amd._lib import RoitrError
    from roitr_amd.fgr import fgr_batch
    (src, tgt, w, _, _), _ = U.fixture("n_4")
    args = (dev(np.array([0, 4], np.int32)), dev(src), dev(tgt), dev(w))
    for bad in (dict(max_dist=0.0), dict(division_factor=1.0), dict(iterations=0), dict(iterations=1025), dict(mu_every=0),
                dict(tuples=-1), dict(tuple_scale=1.0), dict(radius=float("inf")), dict(_lds_rows=1537)):
        with pytest.raises(RoitrError):
            fgr_batch(*args, **bad)
    with pytest.raises(RoitrError):
        fgr_batch(*args, pair_keys=[1, 2], tuples=4)
    ok = fgr_batch(*args, iterations=1)
    assert int(ok["steps"][0]) == 1
