"""GPU: roitr_lgr_batch (csrc/lgr.hip) against the float64 restatement of tests/lgr_util.py on its decided fixtures.

Bounds.  Transforms: 1e-5, the project's bound for fp32 transforms against float64 (tests/test_registration_gpu.py).  A hypothesis's
count: within its number of near rows (|d^2 - r^2| < 1e-4 r^2; every fixture is decided, so for the hypotheses that can win and for
every global step that number is 0 and the comparison is exact).  Everything else is exact or bitwise.

Shapes: run lengths 1, 2, 3, 4, 63, 64, 65, 300 around the 16-lane moment groups and the wave; 511 / 512 / 513 rows around the
verification kernel's row tile = row chunk (512), alone at row 0 and shifted inside a batch; 255 / 256 / 257 hypotheses around one
workgroup's worth; two sets with a noise level per patch, whose counts differ and whose winner is not among the first patches."""
import numpy as np
import pytest
import torch

import lgr_util as U

pytestmark = pytest.mark.gpu

CASES = ["mixed_runs", "rows_511", "rows_512", "rows_513", "hyps_255", "hyps_256", "hyps_257", "tie", "graded", "graded_tail"]
RAGGED = ["rows_513", None, "no_local", "empty_refit", "mixed_runs"]   # None: a pair without rows
FIELDS = ("T", "inliers", "best_hypothesis", "best_first_row", "hypotheses", "local_inliers", "status")


def run(sets, **kw):
    """lgr_batch on a list of (src, tgt, scores, patch, ...) sets (None: an empty pair); numpy results."""
    from roitr_amd.lgr import lgr_batch
    sets = [(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32))
            if s is None else s for s in sets]
    starts = np.concatenate([[0], np.cumsum([s[0].shape[0] for s in sets])]).astype(np.int32)
    cat = lambda k: torch.from_numpy(np.concatenate([s[k] for s in sets])).cuda()
    scores = kw.pop("scores", "own")
    r = lgr_batch(torch.from_numpy(starts).cuda(), cat(0), cat(1), cat(2) if scores == "own" else scores, cat(3),
                  return_hypotheses=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def pair_of(r, b):
    """Pair b's results, its hypotheses cut out of the hyp_* arrays."""
    h0, H = int(r["hyp_starts"][b]), int(r["hypotheses"][b])
    out = {k: r[k][b] for k in FIELDS}
    out.update(hyp_first_row=r["hyp_first_row"][h0:h0 + H], hyp_T=r["hyp_T"][h0:h0 + H], hyp_counts=r["hyp_counts"][h0:h0 + H])
    return out


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.fixture(scope="module")
def refs():
    """The restatement of every fixture, computed once."""
    return {name: U.lgr_ref(*U.fixture(name)[:4]) for name in U.SEEDS}


@pytest.fixture(scope="module")
def alone():
    """Every fixture as a batch of its own."""
    return {name: pair_of(run([U.fixture(name)]), 0) for name in U.SEEDS}


@pytest.fixture(scope="module")
def ragged():
    return run([None if n is None else U.fixture(n) for n in RAGGED])


def check_against_ref(got, ref, name):
    assert ref["decided"]
    assert int(got["hypotheses"]) == ref["hypotheses"] and got["hyp_first_row"].tolist() == ref["hyp_first_row"], name
    if ref["hypotheses"]:
        err = np.abs(got["hyp_T"].astype(np.float64) - ref["hyp_T"]).max()
        print(name, "max |hyp_T - ref|", err)
        assert err < 1e-5, (name, err)
        off = np.abs(got["hyp_counts"] - np.array(ref["hyp_counts"]))
        assert (off <= np.array(ref["hyp_near"])).all(), (name, off.max())
    assert int(got["best_hypothesis"]) == ref["best"] and int(got["best_first_row"]) == ref["best_first_row"], name
    assert int(got["local_inliers"]) == ref["local_inliers"] and int(got["status"]) == ref["status"], name
    err = np.abs(got["T"].astype(np.float64) - ref["T"]).max()
    print(name, "max |T - ref|", err)
    assert err < 1e-5 and int(got["inliers"]) == ref["inliers"], (name, err, got["inliers"], ref["inliers"])
    assert np.array_equal(got["T"][3], [0, 0, 0, 1])


@pytest.mark.parametrize("name", CASES)
def test_against_restatement(name, alone, refs):
    check_against_ref(alone[name], refs[name], name)


@pytest.mark.parametrize("name,kw", U.PARAM_CASES)
def test_other_parameters(name, kw):
    """min_rows, steps and radius away from their defaults, behind another pair (the hypothesis slots start at starts / min_rows)."""
    s = U.fixture(name)
    r = run([U.fixture("tie"), s], **kw)
    check_against_ref(pair_of(r, 1), U.lgr_ref(*s[:4], **kw), name)
    assert same(pair_of(r, 1), pair_of(run([s], **kw), 0))


def test_winner_away_from_the_front(alone, refs):
    """Counts that differ from patch to patch: the winner is one patch in the middle, and one that a lane meets as its second."""
    assert int(alone["graded"]["best_hypothesis"]) == refs["graded"]["best"] >= 20
    assert int(alone["graded_tail"]["best_hypothesis"]) == refs["graded_tail"]["best"] >= 256
    assert len(set(alone["graded"]["hyp_counts"].tolist())) > 10


def test_tie_goes_to_the_lower_number(alone):
    g = alone["tie"]
    assert int(g["best_hypothesis"]) == 0 and int(g["best_first_row"]) == 0
    assert np.array_equal(g["hyp_T"][0], g["hyp_T"][-1]) and g["hyp_counts"][0] == g["hyp_counts"][-1] == g["hyp_counts"].max()


def test_ragged_batch(ragged, alone, refs):
    assert ragged["status"].tolist() == [0, U.NO_ROWS, U.NO_LOCAL, U.EMPTY_REFIT, 0]
    for b, name in enumerate(RAGGED):
        got = pair_of(ragged, b)
        if name is None:
            assert np.array_equal(got["T"], np.eye(4, dtype=np.float32)) and int(got["inliers"]) == 0
            assert int(got["best_hypothesis"]) == -1 and int(got["best_first_row"]) == -1 and int(got["hypotheses"]) == 0
            continue
        check_against_ref(got, refs[name], name)
        assert same(got, alone[name]), name            # a pair alone vs inside a batch, its rows shifted: bitwise
    e = pair_of(ragged, 3)                             # the winner's transform is kept
    assert np.array_equal(e["T"][:3], e["hyp_T"][0]) and int(e["local_inliers"]) == 0 and int(e["inliers"]) == 0
    assert int(pair_of(ragged, 2)["best_hypothesis"]) == -1


@pytest.mark.parametrize("name", ["rows_512", "hyps_257"])
def test_rows_shifted_by_another_pair(name, alone):
    for front in ("rows_511", "mixed_runs"):           # 511 rows in front: the pair straddles the chunk border one row early
        assert same(pair_of(run([U.fixture(front), U.fixture(name)]), 1), alone[name]), (name, front)


def test_row_patch_values_do_not_matter(alone):
    s = U.fixture("mixed_runs")
    _, inv = np.unique(s[3], return_inverse=True)
    for patch in (s[3] + 1000, s[3] * 7 - 50, inv.max() - inv):     # shifted by a constant, with gaps, renumbered backwards
        assert same(pair_of(run([(s[0], s[1], s[2], patch.astype(np.int32))]), 0), alone["mixed_runs"])


def test_repeats_are_bitwise_equal(ragged):
    for _ in range(3):
        again = run([None if n is None else U.fixture(n) for n in RAGGED])
        for b in range(len(RAGGED)):
            assert same(pair_of(again, b), pair_of(ragged, b))


def test_no_scores_equals_ones():
    s = U.fixture("rows_513")
    ones = np.ones_like(s[2])
    a, b = run([(s[0], s[1], ones, s[3])]), run([(s[0], s[1], ones, s[3])], scores=None)
    assert same(pair_of(a, 0), pair_of(b, 0))
    ref = U.lgr_ref(s[0], s[1], None, s[3])      # decided without scores as well (tests/test_lgr_cpu.py)
    assert np.abs(a["T"][0].astype(np.float64) - ref["T"]).max() < 1e-5 and int(a["inliers"][0]) == ref["inliers"]


def test_degenerate_patches_give_proper_rotations():
    """A patch of collinear points and one of duplicate points: whatever rotation the solve picks is finite and proper."""
    rng = np.random.default_rng(5)
    line = (np.array([0.3, -0.2, 0.5]) + np.outer(np.linspace(-1, 1, 6), [0.6, 0.3, -0.2])).astype(np.float32)
    dup = np.tile(np.array([[0.4, 0.1, -0.7]], np.float32), (4, 1))
    R, t = U.random_pose(rng)
    src = np.concatenate([line, dup])
    tgt = (src.astype(np.float64) @ R.T + t).astype(np.float32)
    r = pair_of(run([(src, tgt, np.ones(10, np.float32), np.repeat([0, 1], [6, 4]).astype(np.int32))]), 0)
    assert int(r["hypotheses"]) == 2
    for T in list(r["hyp_T"]) + [r["T"][:3]]:
        Rg = T[:, :3].astype(np.float64)
        assert np.isfinite(T).all()
        assert np.abs(Rg.T @ Rg - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(Rg) - 1) < 1e-5


BAD = [dict(radius=0.0), dict(radius=-0.1), dict(radius=float("nan")), dict(radius=float("inf")), dict(min_rows=2), dict(steps=0),
       dict(null="src"), dict(null="starts"), dict(null="transforms"), dict(null="row_patch"), dict(short=1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_refusals_leave_the_outputs_untouched(bad):
    from roitr_amd import _lib
    lib = _lib.bind(("roitr_lgr_workspace_bytes", "roitr_lgr_batch"))
    src, tgt, w, patch = (torch.from_numpy(x).cuda() for x in U.fixture("rows_511")[:4])
    n = int(src.shape[0])
    starts = torch.tensor([0, n], dtype=torch.int32, device="cuda")
    nbytes = int(lib.roitr_lgr_workspace_bytes(1, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    T = torch.full((1, 4, 4), 7.0, device="cuda")
    ints = [torch.full((1,), -77, dtype=torch.int32, device="cuda") for _ in range(6)]
    hyp = [torch.full((k,), -77, dtype=torch.int32, device="cuda") for k in (2, n // 3, n // 3)]
    hyp_T = torch.full((n // 3, 12), 7.0, device="cuda")
    null = bad.get("null")
    p = lambda name, t: None if null == name else t.data_ptr()
    status = lib.roitr_lgr_batch(1, p("starts", starts), n, p("src", src), tgt.data_ptr(), w.data_ptr(), p("row_patch", patch),
                                 bad.get("radius", 0.1), bad.get("min_rows", 3), bad.get("steps", 5), ws.data_ptr(),
                                 nbytes - bad.get("short", 0), p("transforms", T), *[t.data_ptr() for t in ints], hyp[0].data_ptr(),
                                 hyp[1].data_ptr(), hyp_T.data_ptr(), hyp[2].data_ptr(), _lib.stream_ptr().value)
    torch.cuda.synchronize()
    assert status == 1 and b"roitr_lgr_batch" in lib.roitr_last_error()     # ROITR_ERR_ARG
    assert (T == 7.0).all() and (hyp_T == 7.0).all() and all((t == -77).all() for t in ints + hyp)
    with pytest.raises(_lib.RoitrError, match="lgr_batch"):
        from roitr_amd.lgr import lgr_batch
        lgr_batch(starts, src, tgt, w, patch, radius=-1.0)
