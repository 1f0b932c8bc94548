"""GPU: roitr_remove_statistical_outlier / roitr_remove_radius_outlier (csrc/outlier.hip) against the float64 restatement of
tests/outlier_util.py on fixtures that test_outlier_cpu.py asserts decided.  Exact: keep, index, new_offset, count, status.  mean_dist
within 1e-12 relative (at most 100 ordered adds of terms good to one float64 ulp: 100 * 2^-52 = 2.2e-14; measured 0: the device's float64
sqrt rounds correctly), stats within 1e-10 relative (the squared-deviation sum amplifies the term error by about 2 mean / std).
Bitwise invariance, the refusals, and nothing written behind the kept rows.  The flags become rows through csrc/flag_compact.h on tiles of
4096 rows: TILE_CASES puts totals around one and two tiles, with the cloud boundary inside a tile and off a multiple of 16."""
import functools

import numpy as np
import pytest
import torch

import outlier_util as U

pytestmark = pytest.mark.gpu

_RUNS = {}
STAT = ("keep", "index", "new_offset", "status", "mean", "stats")
RAD = ("keep", "index", "new_offset", "status", "count")


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))   # a copy: the fixtures are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def run(f, method, optional=True, **kw):
    """The wrapper's result as a dict of numpy arrays under the restatement's names."""
    from roitr_amd import prep
    xyz, off = dev(f["xyz"]), dev(f["offset"])
    if method == "statistical":
        r = prep.remove_statistical_outlier(xyz, off, f["nb_neighbors"], f["std_ratio"], return_stats=optional, **kw)
    else:
        r = prep.remove_radius_outlier(xyz, off, f["nb_points"], f["radius"], return_counts=optional, **kw)
    torch.cuda.synchronize()
    out = dict(keep=r.keep, index=r.index, new_offset=r.offset, status=r.status, mean=r.mean_dist, stats=r.stats, count=r.counts, points=r.points,
               attr=r.attr)
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def named(name, method):
    if (name, method) not in _RUNS:
        _RUNS[name, method] = run(U.fixture(name), method)
    return _RUNS[name, method]


def same(a, b, keys):
    return all(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in keys)


def rel(got, want):
    with np.errstate(all="ignore"):
        e = np.abs(got - want) / np.abs(want)
    e = np.where((got == want) | (np.isnan(got) & np.isnan(want)), 0.0, e)
    return float(np.max(e, initial=0.0))


@pytest.mark.parametrize("name", U.NAMES)
def test_statistical_filter_against_the_restatement(name):
    want, got = U.reference(name, "statistical"), named(name, "statistical")
    assert got["keep"].dtype == np.bool_ and got["index"].dtype == np.int32 and got["mean"].dtype == np.float64
    for k in ("status", "keep", "index", "new_offset"):
        assert np.array_equal(got[k], want[k]), (name, k, np.flatnonzero(got[k] != want[k])[:8] if got[k].shape == want[k].shape else got[k].shape)
    e_mean, e_stats = rel(got["mean"], want["mean"]), rel(got["stats"], want["stats"])
    print(name, "max relative error: mean_dist", e_mean, "stats", e_stats)
    assert e_mean < 1e-12 and e_stats < 1e-10, (name, e_mean, e_stats)
    assert np.array_equal(np.isnan(got["stats"]), np.isnan(want["stats"]))
    assert np.array_equal(got["points"], U.fixture(name)["xyz"][want["index"]], equal_nan=True)


@pytest.mark.parametrize("name", U.NAMES)
def test_radius_filter_is_exact(name):
    want, got = U.reference(name, "radius"), named(name, "radius")
    assert got["count"].dtype == np.int32
    for k in RAD:
        assert np.array_equal(got[k], want[k]), (name, k, np.flatnonzero(got[k] != want[k])[:8] if got[k].shape == want[k].shape else got[k].shape)


# total rows -> (rows of the first cloud, seed, nb_points): two surfaces of outlier_util.batch at radius 0.05.  nb_points sits near the
# median count of the restatement (14 - 16 for 1500 + 2600 rows, 28 for 4100 + 4093), so about half of the rows are kept.
TILE_CASES = {4095: (1500, 21, 14), 4096: (1500, 22, 14), 4097: (1500, 23, 14), 8193: (4100, 24, 28)}


@functools.lru_cache(maxsize=None)
def tile_fixture(total):
    first, seed, nb_points = TILE_CASES[total]
    return U.batch(seed, [first, total - first], radius=0.05, nb_points=nb_points)


@pytest.mark.parametrize("total", sorted(TILE_CASES))
def test_radius_filter_is_exact_across_compaction_tiles(total):
    f = tile_fixture(total)
    want, got = U.radius_ref(**f), run(f, "radius")
    share = float(want["keep"].mean())
    print(total, "kept share", share)
    assert 0.25 < share < 0.75, (total, share)        # a fixture that keeps all or nothing would test no compaction
    for k in RAD:
        assert np.array_equal(got[k], want[k]), (total, k, np.flatnonzero(got[k] != want[k])[:8] if got[k].shape == want[k].shape else got[k].shape)


def test_statistical_filter_across_a_compaction_tile():
    f = U.batch(31, [1500, 2597])
    assert U.is_decided(f)
    want, got = U.statistical_ref(**f), run(f, "statistical")
    for k in ("status", "keep", "index", "new_offset"):
        assert np.array_equal(got[k], want[k]), (k, np.flatnonzero(got[k] != want[k])[:8] if got[k].shape == want[k].shape else got[k].shape)
    e_mean, e_stats = rel(got["mean"], want["mean"]), rel(got["stats"], want["stats"])
    print("max relative error: mean_dist", e_mean, "stats", e_stats)
    assert e_mean < 1e-12 and e_stats < 1e-10, (e_mean, e_stats)
    assert 0 < want["index"].shape[0] < 4097


@pytest.mark.parametrize("method,keys", [("statistical", STAT), ("radius", RAD)])
def test_a_cloud_alone_in_the_batch_and_in_a_permuted_batch(method, keys):
    f = U.fixture("sizes")
    whole = named("sizes", method)
    per_point = [k for k in keys if k in ("keep", "mean", "count")]
    off, new = np.concatenate([[0], f["offset"]]), np.concatenate([[0], whole["new_offset"]])
    b = len(f["offset"])
    order = [7, 2, 9, 0, 4, 8, 1, 6, 3, 5]
    perm = run(U.reorder(f, order), method)
    poff, pnew = np.concatenate([[0], np.cumsum([U.SIZES[c] for c in order])]), np.concatenate([[0], perm["new_offset"]])
    for c in range(b):
        one = run(U.split(f, c), method)
        pos = order.index(c)
        for k in per_point:
            assert np.array_equal(one[k], whole[k][off[c]:off[c + 1]], equal_nan=True), (method, c, k)
            assert np.array_equal(perm[k][poff[pos]:poff[pos + 1]], whole[k][off[c]:off[c + 1]], equal_nan=True), (method, c, k)
        assert np.array_equal(one["index"], whole["index"][new[c]:new[c + 1]] - off[c]), (method, c)
        assert np.array_equal(perm["index"][pnew[pos]:pnew[pos + 1]] - poff[pos], one["index"]), (method, c)
        assert one["status"][0] == whole["status"][c] == perm["status"][pos]
        if method == "statistical":
            assert np.array_equal(one["stats"][0], whole["stats"][c], equal_nan=True) and np.array_equal(perm["stats"][pos], whole["stats"][c], equal_nan=True)


@pytest.mark.parametrize("name", ["sizes", "surface", "nonfinite"])
def test_repeats_optional_outputs_and_the_workspace_split_change_nothing(name):
    f = U.fixture(name)
    for method, keys in (("statistical", STAT), ("radius", RAD)):
        first = named(name, method)
        assert same(run(f, method), first, keys), (name, method)
        bare = run(f, method, optional=False)                   # mean_dist / stats / count NULL: the early exit of the radius walk
        assert not {"mean", "stats", "count"} & set(bare) and same(bare, first, ("keep", "index", "new_offset", "status", "points")), (name, method)
    split = run(f, "statistical", max_workspace_bytes=1)        # every cloud a group of its own
    assert same(split, named(name, "statistical"), STAT + ("points",)), name


def test_attr_rows_are_the_kept_rows():
    from roitr_amd import prep
    f = U.fixture("sizes")
    n = f["xyz"].shape[0]
    attr = torch.arange(n * 5, dtype=torch.float32).reshape(n, 5).cuda()
    for r in (prep.remove_statistical_outlier(dev(f["xyz"]), dev(f["offset"]), attr=attr),
              prep.remove_statistical_outlier(dev(f["xyz"]), dev(f["offset"]), attr=attr, max_workspace_bytes=1),
              prep.remove_radius_outlier(dev(f["xyz"]), dev(f["offset"]), f["nb_points"], f["radius"], attr=attr)):
        assert r.attr.shape == (r.index.shape[0], 5) and torch.equal(r.attr, attr[r.index.long()]) and 0 < r.index.shape[0] < n
        assert torch.equal(r.points, dev(f["xyz"])[r.index.long()]) and int(r.offset[-1]) == r.index.shape[0]


def raw_calls(f):
    """(lib, good arguments, call(method, **overrides)) on sentinel-filled capacity buffers."""
    from roitr_amd import prep
    lib = prep._outlier()
    n, b, k = f["xyz"].shape[0], len(f["offset"]), f["nb_neighbors"]
    t = dict(xyz=dev(f["xyz"]), offset=dev(f["offset"]), keep=torch.full((n + 64,), 7, dtype=torch.uint8, device="cuda"),
             index=torch.full((n + 64,), -7, dtype=torch.int32, device="cuda"), new_offset=torch.full((b + 8,), -7, dtype=torch.int32, device="cuda"),
             status=torch.full((b + 8,), -7, dtype=torch.int32, device="cuda"), mean=torch.full((n + 64,), -7.0, dtype=torch.float64, device="cuda"),
             stats=torch.full((b + 8, 3), -7.0, dtype=torch.float64, device="cuda"), count=torch.full((n + 64,), -7, dtype=torch.int32, device="cuda"))
    nbytes = {m: int(lib.roitr_outlier_workspace_bytes(b, n, kk)) for m, kk in (("statistical", k), ("radius", 0))}
    ws = torch.empty((max(nbytes.values()),), dtype=torch.uint8, device="cuda")
    good = dict({key: v.data_ptr() for key, v in t.items()}, b=b, n=n, k=k, std=f["std_ratio"], radius=f["radius"], points=f["nb_points"],
                ws=ws.data_ptr())

    def call(method, **kw):
        a = {**good, "nbytes": nbytes[method], **kw}
        if method == "statistical":
            return lib.roitr_remove_statistical_outlier(a["b"], a["n"], a["xyz"], a["offset"], a["k"], a["std"], a["keep"], a["index"], a["new_offset"],
                                                        a["status"], a["mean"], a["stats"], a["ws"], a["nbytes"], None)
        return lib.roitr_remove_radius_outlier(a["b"], a["n"], a["xyz"], a["offset"], a["radius"], a["points"], a["keep"], a["index"], a["new_offset"],
                                               a["status"], a["count"], a["ws"], a["nbytes"], None)
    return lib, t, nbytes, call


def test_nothing_is_written_behind_the_kept_rows():
    f = U.fixture("sizes")
    n, b = f["xyz"].shape[0], len(f["offset"])
    lib, t, _, call = raw_calls(f)
    for method in ("statistical", "radius"):
        want = U.reference("sizes", method)
        assert call(method) == 0
        torch.cuda.synchronize()
        m = int(want["new_offset"][-1])
        assert np.array_equal(t["index"][:m].cpu().numpy(), want["index"]) and bool((t["index"][m:] == -7).all())
        assert np.array_equal(t["keep"][:n].cpu().numpy(), want["keep"].astype(np.uint8)) and bool((t["keep"][n:] == 7).all())
        assert np.array_equal(t["new_offset"][:b].cpu().numpy(), want["new_offset"]) and bool((t["new_offset"][b:] == -7).all())
        assert not t["status"][:b].any() and bool((t["status"][b:] == -7).all())
        assert bool((t["mean"][n:] == -7).all()) and bool((t["stats"][b:] == -7).all()) and bool((t["count"][n:] == -7).all())
        for key in ("index", "keep"):
            t[key].fill_(7 if key == "keep" else -7)
    # Rows behind offset[b - 1] (n = 4100, the last offset 4090, past one compaction tile) belong to no cloud: never kept, counted 0, and
    # index stays untouched behind the total.  The radius filter only: the statistical one hands all n rows to the kNN of
    # pointops_knn.hip, whose self-sorted query order is defined for the rows of a cloud alone.
    whole = U.batch(25, [1500, 2600], radius=0.05, nb_points=14)
    inside = dict(whole, xyz=whole["xyz"][:4090], offset=np.array([1500, 4090], np.int32))
    f = dict(inside, xyz=whole["xyz"])
    want = U.radius_ref(**inside)
    lib, t, _, call = raw_calls(f)
    assert call("radius") == 0
    torch.cuda.synchronize()
    m = int(want["new_offset"][-1])
    assert 0.25 * 4090 < m < 0.75 * 4090
    assert np.array_equal(t["index"][:m].cpu().numpy(), want["index"]) and bool((t["index"][m:] == -7).all())
    assert np.array_equal(t["keep"][:4090].cpu().numpy(), want["keep"].astype(np.uint8)) and not t["keep"][4090:4100].any()
    assert bool((t["keep"][4100:] == 7).all()) and np.array_equal(t["new_offset"][:2].cpu().numpy(), want["new_offset"])
    assert np.array_equal(t["count"][:4090].cpu().numpy(), want["count"]) and not t["count"][4090:4100].any()


def test_refusals_and_empty_input():
    from roitr_amd import prep
    f = U.fixture("surface")
    lib, t, nbytes, call = raw_calls(f)
    assert call("statistical") == 0 and call("radius") == 0
    both = (dict(b=-1), dict(n=-1), dict(b=65536), dict(b=0), dict(xyz=None), dict(offset=None), dict(keep=None), dict(index=None),
            dict(new_offset=None), dict(status=None), dict(ws=None), dict(nbytes=0))
    cases = {"statistical": both + (dict(k=1), dict(k=0), dict(k=101), dict(k=-3), dict(std=float("nan")), dict(std=float("inf")),
                                    dict(nbytes=nbytes["statistical"] - 1)),
             "radius": both + (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(points=-1),
                               dict(nbytes=nbytes["radius"] - 1))}
    for method, rows in cases.items():
        for kw in rows:
            assert call(method, **kw) == 1, (method, kw)          # ROITR_ERR_ARG
            assert b"outlier" in lib.roitr_last_error()
    torch.cuda.synchronize()
    # the optional outputs may be NULL; no points, and a batch of empty clouds only: not an error
    assert call("statistical", mean=None, stats=None) == 0 and call("radius", count=None) == 0
    assert call("statistical", n=0, xyz=None, keep=None, index=None, ws=None, nbytes=0) == 0 and call("radius", b=0, n=0) == 0
    xyz = dev(f["xyz"])
    for r in (prep.remove_statistical_outlier(xyz[:0], torch.zeros((3,), dtype=torch.int32, device="cuda"), return_stats=True),
              prep.remove_radius_outlier(xyz[:0], torch.zeros((3,), dtype=torch.int32, device="cuda"), return_counts=True)):
        assert r.points.shape == (0, 3) and r.index.shape == (0,) and r.offset.tolist() == [0, 0, 0] and r.status.tolist() == [0, 0, 0]
    torch.cuda.synchronize()
