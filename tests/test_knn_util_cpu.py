"""The numpy side of tests/test_knn_fused_gpu.py: its float64 PPF reference against the known answers of calc_ppf_gpu, and the
input conditions it asserts, on inputs whose answer is known."""
import numpy as np

import knn_util as U


def test_ppf_ref_matches_calc_ppf_gpu_golden(golden_stages):
    """ppf_ref is the reference of every fused-PPF test: it reproduces the recorded calc_ppf_gpu outputs (fp32 torch: 2e-6, as
    test_ppf_stage_golden allows the kernel), the atan2(0, 0) and parallel-normal corner cases among them, in float64 and in fp32."""
    s = golden_stages
    pts, nrm, patches, pn = s["ppf.pts"], s["ppf.nrm"], s["ppf.patches"], s["ppf.pnrm"]
    m, k, _ = patches.shape
    idx = np.arange(m * k, dtype=np.int32).reshape(m, k)
    for dtype in (np.float64, np.float32):
        out = U.ppf_ref(pts, nrm, patches.reshape(-1, 3), pn.reshape(-1, 3), idx, dtype)
        assert out.dtype == dtype and out.shape == (m, k, 4)
        np.testing.assert_allclose(out, s["ppf.out"], rtol=0, atol=2e-6)


def test_ppf_ref_reads_the_query_and_reference_arrays_it_is_given():
    q = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    qn = np.array([[0, 0, 1], [1, 0, 0]], np.float32)
    r = np.array([[0, 0, 2], [1, 3, 0], [5, 5, 5]], np.float32)
    rn = np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0]], np.float32)
    out = U.ppf_ref(q, qn, r, rn, np.array([[0], [1]]))
    # query 0: d = (0, 0, 2) along its normal, neighbour normal perpendicular to both; query 1: d = (0, 3, 0), opposite to n2
    assert np.allclose(out[0, 0], [2.0, 0.0, 0.5, 0.5], atol=1e-15)
    assert np.allclose(out[1, 0], [3.0, 0.5, 1.0, 0.5], atol=1e-15)
    assert U.generic_angles(out).tolist() == [[[False, True, True]], [[True, False, True]]]
    assert U.ppf_errors(out.astype(np.float32), out) == (0.0, 0.0, 0.0)


def test_tied_fraction_ignores_fill_slots_and_later_columns():
    d2 = np.array([[0, 1, 2, 2], [0, 1, 1, 3], [0, 1e10, 1e10, 1e10], [0, 0, 5, 6]], np.float32)
    assert U.tied_fraction(d2, 4) == 0.75
    assert U.tied_fraction(d2, 3) == 0.5      # row 0 ties only in column 3


def test_subset_and_normals():
    rng = np.random.default_rng(0)
    sel = U.subset(rng, [10, 7, 5], [4, 7, 1])
    assert sel.shape == (12,) and (np.diff(sel) > 0).all()
    assert (sel[:4] < 10).all() and np.array_equal(sel[4:11], np.arange(10, 17)) and 17 <= sel[11] < 22
    v = U.unit_normals(rng, 4000, axis_quarter=True)
    assert v.dtype == np.float32 and np.allclose(np.linalg.norm(v, axis=1), 1.0, atol=1e-6)
    axis = (v[:, 0] == 0) & (v[:, 1] == 0) & (np.abs(v[:, 2]) == 1)
    assert 0.2 < axis.mean() < 0.3 and (v[axis, 2] > 0).any() and (v[axis, 2] < 0).any()


def test_branch_names_the_engine_calls():
    """The calls issue_geometry_chain makes at 512 pairs (1024 clouds of 5000 / 1250 / 312 / 78 points) and for one pair."""
    nc = 1024
    assert U.branch(nc, nc * 5000, nc * 5000, 9, True, True) == "prefilter<10,40>+lane<10>"
    assert U.branch(nc, nc * 5000, nc * 1250, 17, True, False) == "lane<18> sort<4096>"
    assert U.branch(nc, nc * 312, nc * 312, 17, False, True) == "lane_brute<18>"
    assert U.branch(nc, nc * 312, nc * 78, 17, False, False) == "lane_brute<18>"
    assert U.branch(2, 2 * 1250, 2 * 1250, 17, True, True) == "cell+gridsel"
    assert U.branch(2, 2 * 5000, 2 * 1250, 17, True, False) == "gridsel"
    assert U.branch(2, 2 * 312, 2 * 312, 17, False, True) == "brute<1>"
    assert U.branch(nc, nc * 1250, nc * 1250, 17, True, True, ppf=True, group=False) == "cell+gridsel"
