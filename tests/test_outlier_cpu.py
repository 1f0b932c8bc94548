"""CPU: the float64 restatement of the outlier filters (tests/outlier_util.py) against an independent brute force, the fixtures of
test_outlier_gpu.py are decided, the definition's corner cases, the command line, the refusal of host tensors and the binding."""
import math

import numpy as np
import pytest
import torch

import outlier_util as U
from roitr_amd.prep import OutlierResult, remove_radius_outlier, remove_statistical_outlier   # the feature under test


def brute(f):
    """Per point, by plain Python float arithmetic (IEEE double, no numpy): the squared distances to every point of its cloud."""
    xyz = [[float(v) for v in row] for row in f["xyz"]]
    ends = [0] + [int(e) for e in f["offset"]]
    out = []
    for c in range(len(ends) - 1):
        for i in range(ends[c], ends[c + 1]):
            row = []
            for j in range(ends[c], ends[c + 1]):
                dx, dy, dz = xyz[j][0] - xyz[i][0], xyz[j][1] - xyz[i][1], xyz[j][2] - xyz[i][2]
                row.append((dx * dx + dy * dy) + dz * dz)
            out.append(row)
    return out


@pytest.mark.parametrize("name", ["sizes", "dups", "lattice"])
def test_restatement_equals_an_independent_brute_force(name):
    f = U.fixture(name)
    d2 = brute(f)
    stat, rad = U.reference(name, "statistical"), U.reference(name, "radius")
    r2 = float(f["radius"]) * float(f["radius"])
    assert rad["count"].tolist() == [sum(1 for v in row if v < r2) for row in d2]
    assert rad["keep"].tolist() == [c > f["nb_points"] for c in rad["count"].tolist()]
    k = f["nb_neighbors"]
    p = f["xyz"].astype(np.float64)
    cloud = np.searchsorted(f["offset"], np.arange(len(d2)), side="right")
    start = np.concatenate([[0], f["offset"]])[cloud]
    for i, row in enumerate(d2):
        v = min(k, len(row))
        mine = sorted(float(U.d2_of(p, i, j)) for j in stat["idx"][i, :v])
        assert mine == sorted(row)[:v], (name, i)                                  # the multiset of the row's distances: the v nearest
        assert ((stat["idx"][i, :v] >= start[i]) & (stat["idx"][i, :v] < start[i] + len(row))).all()
        want = 0.0
        for j in stat["idx"][i, :v]:
            want = want + math.sqrt(row[int(j) - int(start[i])])                  # row order; math.sqrt is the correctly rounded one
        assert stat["mean"][i] == want / v, (name, i)


@pytest.mark.parametrize("name", U.NAMES)
def test_every_fixture_is_decided(name):
    assert U.is_decided(name)
    r = U.reference(name, "statistical")
    assert np.array_equal(r["index"], np.flatnonzero(r["keep"])) and r["new_offset"][-1] == r["keep"].sum()


def test_an_undecided_cloud_is_recognised():
    f = U.lattice(isolated=False, nb_neighbors=2)      # std == 0 on more than two points
    assert not U.is_decided(f)


def test_statistical_filter_keeps_nothing_on_a_pure_lattice_and_on_one_point():
    # nb_neighbors = 2: every mean is (0 + 1/64) / 2, the sums are exact, std == 0 and thr == cloud_mean
    r = U.statistical_ref(**U.lattice(isolated=False, nb_neighbors=2))
    assert not r["keep"].any() and r["stats"][0].tolist() == [1.0 / 128, 0.0, 1.0 / 128] and (r["mean"] == 1.0 / 128).all()
    one = U.statistical_ref(np.array([[0.25, 0.5, 1.0]], np.float32), np.array([1], np.int32))
    assert not one["keep"].any() and one["stats"][0, 0] == 0.0 and np.isnan(one["stats"][0, 1:]).all() and one["new_offset"].tolist() == [0]
    two = U.statistical_ref(np.array([[0, 0, 0], [0.3, 0.1, 0.7]], np.float32), np.array([2], np.int32))
    assert not two["keep"].any() and two["stats"][0, 1] == 0.0


def test_fixture_corner_cases_are_what_the_names_say():
    s = U.reference("sizes", "statistical")
    assert U.fixture("sizes")["offset"].tolist() == np.cumsum(U.SIZES).tolist() and s["new_offset"][:3].tolist() == [0, 0, 0]
    d = U.reference("dups", "statistical")
    zero = d["mean"] == 0
    assert zero.sum() == 25 and not d["keep"][zero].any()                          # counted in V, absent from the sums, removed
    m = d["mean"]
    assert d["stats"][0, 0] == U.cloud_sum(np.where(m > 0, m, 0.0)) / 400.0
    lat = U.reference("lattice", "radius")
    assert sorted(set(lat["count"].tolist())) == [1, 4, 6, 9] and lat["keep"].sum() == 140   # distance 2 / 64 fails the strict test
    interior = U.reference("lattice", "statistical")["mean"][:144].reshape(12, 12)[3:9, 3:9]
    assert (interior == interior[0, 0]).all()
    n = U.reference("nonfinite", "statistical")
    assert n["status"].tolist() == [1, 0, 1] and not n["keep"][:300].any() and not n["keep"][500:].any() and n["keep"][300:500].any()
    assert U.reference("nonfinite", "radius")["status"].tolist() == [1, 0, 1]
    sc = U.reference("surface", "statistical")
    assert sc["keep"][:3000].mean() > 0.99 and sc["keep"][3000:].mean() < 0.6


def test_sequential_sums_are_sequential():
    a = np.array([1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53])
    assert U.seq_sum(a) == 1.0 and U.seq_sum(a[::-1]) > 1.0
    terms = np.concatenate([[1.0], np.full(256, 2.0 ** -53)])       # the 257th term starts a segment of its own
    assert U.cloud_sum(terms) == 1.0 and U.cloud_sum(terms[::-1]) > 1.0


def test_parser_flags_and_defaults():
    from roitr_amd.main import outlier_options, parser
    a = parser().parse_args(["cfg.yaml"])
    assert a.remove_outliers is None and outlier_options(a) is None
    assert (a.outlier_nn, a.outlier_std, a.outlier_points, a.outlier_radius) == (20, 2.0, 16, 0.05)
    a = parser().parse_args(["cfg.yaml", "--remove-outliers", "statistical", "--outlier-nn", "12", "--outlier-std", "1.5"])
    assert outlier_options(a) == dict(method="statistical", nb_neighbors=12, std_ratio=1.5)
    a = parser().parse_args(["cfg.yaml", "--remove-outliers", "radius", "--outlier-points", "7", "--outlier-radius", "0.1"])
    assert outlier_options(a) == dict(method="radius", nb_points=7, radius=0.1)
    with pytest.raises(SystemExit):
        parser().parse_args(["cfg.yaml", "--remove-outliers", "median"])


def test_tester_refuses_an_unknown_method():
    from roitr_amd.tester import Tester
    with pytest.raises(ValueError, match="method"):
        Tester(dict(benchmark="3DMatch"), None, [], outlier=dict(method="median"))


def test_host_tensors_are_refused():
    from roitr_amd._lib import RoitrError
    assert OutlierResult._fields == ("points", "offset", "attr", "index", "keep", "status", "mean_dist", "stats", "counts")
    xyz, off = torch.zeros((8, 3)), torch.tensor([8], dtype=torch.int32)
    for fn in (remove_statistical_outlier, remove_radius_outlier):
        with pytest.raises(RoitrError):
            fn(xyz, off)
    with pytest.raises(RoitrError):
        remove_statistical_outlier(xyz, off, return_stats=True)


def test_prototypes_resolve_with_the_headers_parameter_counts():
    import ctypes
    from roitr_amd import _lib as L
    from roitr_amd import prep
    protos = L.header_prototypes()
    assert protos["roitr_outlier_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert protos["roitr_remove_statistical_outlier"][0] is ctypes.c_int and len(protos["roitr_remove_statistical_outlier"][1]) == 15
    assert protos["roitr_remove_radius_outlier"][0] is ctypes.c_int and len(protos["roitr_remove_radius_outlier"][1]) == 14
    assert protos["roitr_remove_statistical_outlier"][1][5] is ctypes.c_double and protos["roitr_remove_radius_outlier"][1][4] is ctypes.c_double
    lib = prep._outlier()                                    # L.binder: restype / argtypes from the header, on the built library
    for name, (res, args) in ((k, protos[k]) for k in ("roitr_outlier_workspace_bytes", "roitr_remove_statistical_outlier", "roitr_remove_radius_outlier")):
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert not {"roitr_outlier_workspace_bytes", "roitr_remove_statistical_outlier", "roitr_remove_radius_outlier"} & set(L.BOUND)
    stat, rad = lib.roitr_outlier_workspace_bytes(1, 1000, 20), lib.roitr_outlier_workspace_bytes(1, 1000, 0)
    assert stat >= rad + 1000 * 20 * 4 and rad > 0               # the kNN rows come on top of the grid
    assert lib.roitr_outlier_workspace_bytes(1, 1000, 1) == 0 and lib.roitr_outlier_workspace_bytes(1, 1000, 101) == 0
