"""GPU: roitr_compat_batch (csrc/compat.hip) against the float64 restatement of tests/compat_util.py on its decided fixtures.

Exact: degree, seed_rows, seed_members, hyp_counts, best_rank, best_seed_row, seeds, hypotheses, local_inliers, inliers, status (every
fixture is decided: tests/test_compat_cpu.py).  Within 1e-5, the project's bound for an fp32 transform against a float64-restated
solve (tests/test_registration_gpu.py, tests/test_lgr_gpu.py): hyp_transforms and T.  A hypothesis whose member set is not
well_posed is left out of the hyp_T / hyp_counts comparison only (at most 5 % of a fixture's valid ones, never the winner).

Shapes: m = 3, 4, 63, 64, 65, 127, 128, 129, 257, 1000 around the 64-bit word, the 32-row graph block, the 16-word line of the
consensus kernel and its 512-point tile; 2049 rows cut to 2048; k = 3, 20, 64 and more than the members there are; max_seeds 1, 64,
1024 and more than m."""
import numpy as np
import pytest
import torch

import compat_util as U

pytestmark = pytest.mark.gpu

CASES = sorted(n for n in U.CASES)
RAGGED = ["m_65", None, "two_rows", "incompatible", "ratio_10"]   # None: a pair without rows
FIELDS = ("T", "inliers", "best_rank", "best_seed_row", "seeds", "hypotheses", "local_inliers", "status")
STAGES = ("degree", "seed_rows", "seed_members", "hyp_T", "hyp_counts")
EMPTY = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32))
FRONT_SEED = 41   # make_set(FRONT_SEED, 511, 0.3) is decided and within the cap (checked where it is used)


def run(sets, scores="own", **kw):
    """compat_batch on a list of (src, tgt, scores, ...) sets (None: an empty pair); numpy results plus the row starts."""
    from roitr_amd.compat import compat_batch
    sets = [EMPTY if s is None else s for s in sets]
    starts = np.concatenate([[0], np.cumsum([s[0].shape[0] for s in sets])]).astype(np.int32)
    cat = lambda i: torch.from_numpy(np.concatenate([s[i] for s in sets])).cuda()
    r = compat_batch(torch.from_numpy(starts).cuda(), cat(0), cat(1), cat(2) if scores == "own" else scores, return_stages=True, **kw)
    torch.cuda.synchronize()
    r = {n: v.cpu().numpy() for n, v in r.items()}
    r["starts"] = starts
    return r


def pair_of(r, b, seeds=None, k=None):
    """Pair b's results; the stage arrays cut to `seeds` ranks and `k` members, so that runs of different capacity compare."""
    out = {n: r[n][b] for n in FIELDS}
    out["degree"] = r["degree"][r["starts"][b]:r["starts"][b + 1]]
    for n in STAGES[1:]:
        out[n] = r[n][b][:seeds]
    out["seed_members"] = out["seed_members"][:, :k]
    return out


def same(a, b):
    return all(np.array_equal(a[n], b[n]) for n in a)


_alone = {}


def alone(name):
    """A fixture as a batch of its own under its own parameters, run once."""
    if name not in _alone:
        data, kw = U.fixture(name)
        _alone[name] = pair_of(run([data], **kw), 0)
    return _alone[name]


def check_against_ref(got, ref, name, max_seeds=U.MAX_SEEDS, k=U.K, pose=True):
    n, S = len(got["degree"]), len(ref["seeds"])
    deg = np.full(n, -1)
    deg[ref["sel"]] = ref["deg"]
    assert np.array_equal(got["degree"], deg), name
    assert int(got["seeds"]) == S and int(got["status"]) == ref["status"] and int(got["hypotheses"]) == ref["hypotheses"], name
    assert got["seed_rows"].tolist() == ref["seed_rows"] + [-1] * (max_seeds - S), name
    mem = np.full((max_seeds, k), -1)
    for i, rows in enumerate(ref["members"]):     # an invalid hypothesis lists the one or two rows it has
        mem[i, :len(rows)] = rows
    assert np.array_equal(got["seed_members"], mem), name
    keep = np.ones(max_seeds, bool)
    keep[U.excluded(ref)] = False
    want_counts = np.array(list(ref["hyp_counts"]) + [-1] * (max_seeds - S))
    assert np.array_equal(got["hyp_counts"][keep], want_counts[keep]), name
    assert ((got["hyp_counts"] >= 0) == (want_counts >= 0)).all(), name
    want_T = np.concatenate([ref["hyp_T"].reshape(S, 3, 4), np.zeros((max_seeds - S, 3, 4))])
    err = np.abs(got["hyp_T"].astype(np.float64) - want_T)[keep].max()
    print(name, "max |hyp_T - ref|", err, "excluded", U.excluded(ref))
    assert err < 1e-5, (name, err)
    assert int(got["best_rank"]) == ref["best"] and int(got["best_seed_row"]) == ref["best_seed_row"], name
    assert int(got["local_inliers"]) == ref["local_inliers"], name
    err = np.abs(got["T"].astype(np.float64) - ref["T"]).max()
    print(name, "max |T - ref|", err)
    assert (err < 1e-5 or not pose) and int(got["inliers"]) == ref["inliers"], (name, err, got["inliers"], ref["inliers"])
    Rg = got["T"][:3, :3].astype(np.float64)
    assert np.abs(Rg.T @ Rg - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(Rg) - 1) < 1e-5
    assert np.array_equal(got["T"][3], [0, 0, 0, 1])


@pytest.mark.parametrize("name", CASES)
def test_against_restatement(name):
    kw = U.fixture(name)[1]
    # two rows fix no rotation about their axis: the pose of that pair is compared through its inliers only
    check_against_ref(alone(name), U.reference(name), name, kw.get("max_seeds", U.MAX_SEEDS), kw.get("k", U.K), pose=name != "two_rows")


def test_planted_pose_comes_back():
    for name in ("ratio_30", "ratio_10", "ratio_05"):
        (_, _, _, mask, (R, t)), _ = U.fixture(name)
        g = alone(name)
        assert int(g["inliers"]) == int(mask.sum()) and int(g["status"]) == 0
        assert np.abs(g["T"][:3, :3] - R).max() < 5e-3 and np.abs(g["T"][:3, 3] - t).max() < 1e-2


def test_ragged_batch():
    r = run([None if n is None else U.fixture(n)[0] for n in RAGGED])
    assert r["status"].tolist() == [0, U.NO_ROWS, U.reference("two_rows")["status"], U.reference("incompatible")["status"], 0]
    assert r["status"][2] & U.NO_HYPOTHESIS and r["status"][3] & U.NO_HYPOTHESIS
    for b, name in enumerate(RAGGED):
        got = pair_of(r, b)
        if name is None:
            assert np.array_equal(got["T"], np.eye(4, dtype=np.float32)) and int(got["inliers"]) == 0 and int(got["seeds"]) == 0
            assert int(got["best_rank"]) == -1 and int(got["best_seed_row"]) == -1 and int(got["hypotheses"]) == 0
            assert (got["seed_rows"] == -1).all() and (got["hyp_counts"] == -1).all() and (got["seed_members"] == -1).all()
            continue
        check_against_ref(got, U.reference(name), name, pose=name != "two_rows")
        assert same(got, alone(name)), name            # a pair alone vs inside a batch, its rows shifted, in another slot: bitwise
    again = run([None if n is None else U.fixture(n)[0] for n in RAGGED])
    assert all(same(pair_of(again, b), pair_of(r, b)) for b in range(len(RAGGED)))


@pytest.mark.parametrize("name", ["m_129", "m_1000"])
def test_slot_offset_and_repeat_do_not_matter(name):
    data = U.fixture(name)[0]
    for front in ("m_63", "m_257"):
        r = run([U.fixture(front)[0], data])
        assert same(pair_of(r, 1), alone(name)), (name, front)
    assert same(pair_of(run([data]), 0), alone(name))


def test_rows_straddle_a_verification_tile_behind_another_pair():
    """511 rows in front: the next pair's first row is the last of the verification kernel's first 512-row tile, the rest lie in the
    second, so its counts are added from two blocks; the pair behind it has invalid (-1) hypotheses only, which both blocks skip."""
    front = U.make_set(FRONT_SEED, 511, 0.3)
    ref = U.compat_ref(*front[:3])
    assert U.decided(ref) and U.within_cap(ref)
    names = ["m_129", "two_rows"]
    r = run([front] + [U.fixture(n)[0] for n in names])
    assert r["starts"].tolist() == [0, 511, 640, 642] and int(r["seeds"][2]) == 2 and (r["hyp_counts"][2][:2] == -1).all()
    check_against_ref(pair_of(r, 0), ref, "front_511")
    for b, name in enumerate(names, 1):
        check_against_ref(pair_of(r, b), U.reference(name), name, pose=name != "two_rows")
        assert same(pair_of(r, b), alone(name)), name


@pytest.mark.parametrize("name", ["m_63", "m_129", "lattice"])
def test_larger_capacity_changes_nothing(name):
    """max_rows above the pair's rows and max_seeds above its selected rows change no decision: bitwise the same pair."""
    data, kw = U.fixture(name)
    n = data[0].shape[0]
    S, k = kw.get("max_seeds", U.MAX_SEEDS), kw.get("k", U.K)
    want = pair_of(run([data], **dict(kw, max_rows=n)), 0)
    assert same(want, alone(name))
    assert same(pair_of(run([data], **dict(kw, max_rows=n + 500)), 0), want)
    if n <= S:
        more = run([data], **dict(kw, max_seeds=2 * S))
        assert same(pair_of(more, 0, seeds=S), want)
        assert (more["seed_rows"][0][S:] == -1).all() and (more["hyp_counts"][0][S:] == -1).all()


def test_no_scores_equals_ones():
    data = U.fixture("ratio_10")[0]
    ones = np.ones_like(data[2])
    a, b = run([(data[0], data[1], ones)]), run([(data[0], data[1], ones)], scores=None)
    assert same(pair_of(a, 0), pair_of(b, 0))
    ref = U.compat_ref(data[0], data[1], None)
    assert U.decided(ref)
    check_against_ref(pair_of(b, 0), ref, "no scores")


def test_truncation_with_equal_scores_and_without_scores():
    (src, tgt, w, _, _), _ = U.fixture("trunc_300")
    ones = np.ones_like(w)
    a = pair_of(run([(src, tgt, ones)], max_rows=200), 0)
    b = pair_of(run([(src, tgt, ones)], scores=None, max_rows=200), 0)
    assert same(a, b) and int(a["status"]) & U.TRUNCATED
    assert (a["degree"][:200] >= 0).all() and (a["degree"][200:] == -1).all()
    two = np.where(np.arange(300) % 3 == 0, 2.0, 1.0).astype(np.float32)   # 100 rows at 2, then the first 100 of the others
    c = pair_of(run([(src, tgt, two)], max_rows=200), 0)
    assert np.array_equal(np.flatnonzero(c["degree"] >= 0), U.select(300, two, 200))


def test_lattice_ties():
    for name in ("lattice", "lattice_k5"):
        g, r = alone(name), U.reference(name)
        assert g["seed_rows"][:len(r["seed_rows"])].tolist() == r["seed_rows"]
        vals, counts = np.unique(r["deg"][r["seeds"]], return_counts=True)
        assert counts.max() >= 4


def test_largest_graph():
    """8192 rows, the largest max_rows: 128 words per row, the seed kernel's full key array, 16 tiles of 512 points.  The whole matrix
    is not restated (67 million float64 distance pairs); exact against float64 numpy: the degree of 96 rows spread over the range (the
    first and the last among them), the seed ranks from the degrees, and the member set of the first seed from the rows of C of its
    compatible neighbours.  The pose is checked through the planted set."""
    import lgr_util as LU
    n = 8192
    src, tgt, w, mask, (R, t) = U.make_set(31, n, 0.1)
    r = run([(src, tgt, w)], max_rows=n)
    g = pair_of(r, 0)
    assert int(g["status"]) == 0 and int(g["seeds"]) == U.MAX_SEEDS and (g["degree"] >= 0).all() and g["degree"].sum() % 2 == 0
    rows = np.unique(np.concatenate([[0, 1, 63, 64, 4095, 4096, n - 2, n - 1], np.random.default_rng(0).integers(0, n, 88)]))
    C_rows, margin = U.graph_rows(src, tgt, rows, U.COMPAT_DIST)
    assert margin >= U.MARGIN
    assert np.array_equal(g["degree"][rows], C_rows.sum(1))
    deg = g["degree"].astype(np.int64)
    assert g["seed_rows"].tolist() == np.lexsort((np.arange(n), -deg))[:U.MAX_SEEDS].tolist()
    s0 = int(g["seed_rows"][0])
    Cs, m0 = U.graph_rows(src, tgt, [s0], U.COMPAT_DIST)
    nb = np.flatnonzero(Cs[0])
    Cn, m1 = U.graph_rows(src, tgt, nb, U.COMPAT_DIST)
    assert min(m0, m1) >= U.MARGIN and len(nb) == deg[s0]
    c = np.zeros(n, np.int64)
    c[nb] = (Cn & Cs[0]).sum(1)
    mem, _ = U.members_of(c, s0, U.K)
    assert g["seed_members"][0].tolist() == mem.tolist()
    lo_up = LU.counts(g["T"][:3].astype(np.float64), src, tgt, U.RADIUS)
    assert lo_up[2] <= int(g["inliers"]) <= lo_up[3] and int(g["inliers"]) >= int(mask.sum())
    assert np.abs(g["T"][:3, :3] - R).max() < 5e-3 and np.abs(g["T"][:3, 3] - t).max() < 1e-2


BAD = [dict(compat_dist=0.0), dict(compat_dist=float("nan")), dict(radius=-0.1), dict(radius=float("inf")), dict(max_rows=2),
       dict(max_rows=8193), dict(max_seeds=0), dict(max_seeds=1025), dict(k=2), dict(k=65), dict(steps=0), dict(null="src"),
       dict(null="starts"), dict(null="transforms"), dict(null="seeds"), dict(short=1), dict(total_rows=-1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_refusals_leave_the_outputs_untouched(bad):
    from roitr_amd import _lib
    lib = _lib.bind(("roitr_compat_workspace_bytes", "roitr_compat_batch"))
    src, tgt, w = (torch.from_numpy(x).cuda() for x in U.fixture("m_129")[0][:3])
    n, M, S, k = int(src.shape[0]), 256, 16, 20
    starts = torch.tensor([0, n], dtype=torch.int32, device="cuda")
    nbytes = int(lib.roitr_compat_workspace_bytes(1, n, M, S, k))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    T = torch.full((1, 4, 4), 7.0, device="cuda")
    ints = {name: torch.full((1,), -77, dtype=torch.int32, device="cuda")
            for name in ("inliers", "best_rank", "best_seed_row", "seeds", "hypotheses", "local_inliers", "status")}
    stage = [torch.full((c,), -77, dtype=torch.int32, device="cuda") for c in (n, S, S * k)]
    hyp_T = torch.full((S, 12), 7.0, device="cuda")
    hyp_c = torch.full((S,), -77, dtype=torch.int32, device="cuda")
    null = bad.get("null")
    p = lambda name, t: None if null == name else t.data_ptr()
    status = lib.roitr_compat_batch(1, p("starts", starts), bad.get("total_rows", n), p("src", src), tgt.data_ptr(), w.data_ptr(),
                                    bad.get("compat_dist", 0.1), bad.get("radius", 0.1), bad.get("max_rows", M),
                                    bad.get("max_seeds", S), bad.get("k", k), bad.get("steps", 5), ws.data_ptr(),
                                    nbytes - bad.get("short", 0), p("transforms", T),
                                    *[p(name, t) for name, t in ints.items()], *[t.data_ptr() for t in stage], hyp_T.data_ptr(),
                                    hyp_c.data_ptr(), _lib.stream_ptr().value)
    torch.cuda.synchronize()
    assert status == 1 and b"roitr_compat_batch" in lib.roitr_last_error()     # ROITR_ERR_ARG
    assert (T == 7.0).all() and (hyp_T == 7.0).all() and all((t == -77).all() for t in list(ints.values()) + stage + [hyp_c])
    with pytest.raises(_lib.RoitrError, match="compat_batch"):
        from roitr_amd.compat import compat_batch
        compat_batch(starts, src, tgt, w, k=65)
