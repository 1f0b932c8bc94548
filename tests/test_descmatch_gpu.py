"""GPU: descriptor matching (roitr_amd/descmatch.py, csrc/desc_match.hip) against the float64 restatement of tests/descmatch_util.py
under its decided / undecided rule, bit for bit on integer descriptors (exact in fp32, ties everywhere), on planted ties, tile edges,
ragged batches, the selection modes, the reference's recorded results (tests/golden/descmatch_ref.npz) and end to end."""
import ctypes
import os

import numpy as np
import pytest
import torch

import descmatch_util as U

pytestmark = pytest.mark.gpu
METRIC = {0: "dot", 1: "sqdist"}


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dt) if dt is not None else t).cuda()


def ends(*ns):
    return dev(np.concatenate([[0], np.cumsum(ns)]).astype(np.int32))


def match_one(s, t, metric, mode="mutual"):
    from roitr_amd.descmatch import match_batch
    r = match_batch(ends(s.shape[0]), dev(s), ends(t.shape[0]), dev(t), metric=METRIC[metric], mode=mode)
    return {k: v.cpu().numpy() for k, v in r.items()}


def golden():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "descmatch_ref.npz"))


def assert_exact(s, t, metric, r=None):
    """Bit for bit against the restatement: indices, values (float64 -> fp32 is exact on integer scores) and the three modes."""
    r = match_one(s, t, metric) if r is None else r
    ref = U.match_f64(s, t, metric)
    n, m = ref["score"].shape
    assert np.array_equal(r["row_idx"], ref["row_idx"]) and np.array_equal(r["col_idx"], ref["col_idx"])
    assert np.array_equal(r["row_val"], ref["score"][np.arange(n), ref["row_idx"]].astype(np.float32))
    assert np.array_equal(r["col_val"], ref["score"][ref["col_idx"], np.arange(m)].astype(np.float32))
    assert np.array_equal(r["corr"], U.select(ref["row_idx"], ref["col_idx"], "mutual"))
    assert list(r["corr_starts"]) == [0, len(r["corr"])]
    return ref


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("D", [64, 256, 512])
def test_against_float64(metric, D):
    for seed in range(3):
        for scale in ("unit", "x2"):
            c = U.make_case(seed, D, scale=scale)
            r = match_one(c["src_desc"], c["tgt_desc"], metric)
            U.check_against_f64(c["src_desc"], c["tgt_desc"], metric, r["row_idx"], r["row_val"], r["col_idx"], r["col_val"])


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("shape", [(130, 67), (1, 300)])
def test_exact_integer_descriptors(metric, shape):
    c = U.make_int_case(0, *shape, D=256, r=3)
    s, t = c["src_desc"], c["tgt_desc"]
    ref = assert_exact(s, t, metric)
    for mode in ("row", "col"):
        assert np.array_equal(match_one(s, t, metric, mode)["corr"], U.select(ref["row_idx"], ref["col_idx"], mode)), mode
    # ties are everywhere: some row has its best score at several columns
    sc = ref["score"]
    best = sc.max(1) if metric == 0 else sc.min(1)
    assert ((sc == best[:, None]).sum(1) > 1).any() or shape[0] == 1


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("side,lo,hi", [("tgt", 3, 5), ("tgt", 3, 200), ("src", 2, 4), ("src", 2, 190)])
def test_planted_bitwise_ties_take_the_lower_index(metric, side, lo, hi):
    c = U.make_case(7, 64, n=210, m=230, scale="unit")
    s, t = c["src_desc"].copy(), c["tgt_desc"].copy()
    if side == "tgt":
        t[lo] = t[hi] = s[11]      # source row 11 finds both at distance 0 / the largest dot product
    else:
        s[lo] = s[hi] = t[17]
    r = match_one(s, t, metric)
    idx = r["row_idx"] if side == "tgt" else r["col_idx"]
    assert hi not in idx, "the upper twin of a bitwise tie was reported"
    assert idx[11 if side == "tgt" else 17] == lo


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("D", [4, 1024])
def test_tile_edges(metric, D):
    for k, (n, m) in enumerate([(1, 1), (63, 65), (64, 64), (65, 129), (200, 3)]):
        c = U.make_int_case(10 + k, n, m, D=D, r=3 if D == 4 else 1)
        assert_exact(c["src_desc"], c["tgt_desc"], metric)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("n,m,D,r,twins", [
    # one small pair: the column walk is split over 16 blocks, block y takes tiles y, y + 16, ...: 33 tiles, 2-3 per block.  Target
    # twins 3 / 1027 sit in tiles 0 / 16 (the SAME block: decided in its registers), 5 / 1500 in tiles 0 / 23 (different blocks)
    (130, 2100, 64, 1, ((11, 3, 1027), (12, 5, 1500), (13, 70, 2099))),
    # 65536 source rows: 1024 row tiles, no split; every block walks all 5 column tiles of the pair
    (65536, 300, 4, 3, ((11, 3, 5), (12, 4, 200), (13, 64, 299))),
])
def test_column_walk_over_several_tiles_is_exact(metric, n, m, D, r, twins):
    """A block that walks several column tiles: the register-resident row best across the walk, the accumulator reset, the
    prefetch across the tile boundary -- bit for bit on integer descriptors.  Bitwise-equal target rows are planted in different
    tiles of one walk as the copy of a source row of full magnitude, so that row's best score (its own squared norm, distance 0) is
    reached at both twins: the lower one must be reported, and the upper one never."""
    c = U.make_int_case(30, n, m, D=D, r=r)
    s, t = c["src_desc"].copy(), c["tgt_desc"].copy()
    for k, lo, hi in twins:
        s[k] = np.where(s[k] >= 0, r, -r)
        t[lo] = t[hi] = s[k]
    got = match_one(s, t, metric)
    ref = assert_exact(s, t, metric, got)
    for k, lo, hi in twins:
        assert hi not in got["row_idx"] and got["row_idx"][k] <= lo and (t[got["row_idx"][k]] == s[k]).all()
    sc = ref["score"]
    best = sc.max(1) if metric == 0 else sc.min(1)
    tied = (sc == best[:, None])
    first, last = tied.argmax(1), m - 1 - tied[:, ::-1].argmax(1)
    assert ((last // 64) > (first // 64)).sum() > 10   # many rows have their best score in several tiles: >= for > would show
    for mode in ("row", "col"):
        assert np.array_equal(match_one(s, t, metric, mode)["corr"], U.select(ref["row_idx"], ref["col_idx"], mode)), mode


@pytest.mark.parametrize("metric", [0, 1])
def test_ragged_batch_shared_buffer(metric):
    """Five pairs in one call, source and target clouds back to back in ONE buffer as an engine handle has them (all sources,
    then all targets), one pair without source rows and one without target rows."""
    from roitr_amd.descmatch import match_batch
    D = 64
    sizes_s, sizes_t = [130, 0, 77, 64, 201], [67, 40, 0, 129, 150]
    rng = np.random.default_rng(5)
    buf = rng.integers(-3, 4, (sum(sizes_s) + sum(sizes_t), D)).astype(np.float32)
    o = np.concatenate([[0], np.cumsum(sizes_s + sizes_t)]).astype(np.int32)
    src_off, tgt_off = dev(o[:6]), dev(o[5:])
    b = dev(buf)
    runs = []
    for _ in range(3):
        r = match_batch(src_off, b, tgt_off, b, metric=METRIC[metric], mode="mutual")
        runs.append({k: v.cpu().numpy() for k, v in r.items()})
    for r in runs[1:]:
        assert all(np.array_equal(r[k], runs[0][k]) for k in r)
    r = runs[0]
    assert (r["row_idx"][o[5]:] == -1).all() and (r["col_idx"][:o[5]] == -1).all()   # rows that are on the other side of the buffer
    for p in range(5):
        s, t = buf[o[p]:o[p + 1]], buf[o[5 + p]:o[5 + p + 1]]
        one = match_one(s, t, metric)
        rows, cols = slice(o[p], o[p + 1]), slice(o[5 + p], o[5 + p + 1])
        assert np.array_equal(r["row_idx"][rows], one["row_idx"]) and np.array_equal(r["row_val"][rows].view(np.int32), one["row_val"].view(np.int32))
        assert np.array_equal(r["col_idx"][cols], one["col_idx"]) and np.array_equal(r["col_val"][cols].view(np.int32), one["col_val"].view(np.int32))
        assert np.array_equal(r["corr"][r["corr_starts"][p]:r["corr_starts"][p + 1]], one["corr"])
        if len(s) == 0 or len(t) == 0:
            assert (one["row_idx"] == -1).all() and (one["col_idx"] == -1).all()
            assert (one["row_val"] == 0).all() and (one["col_val"] == 0).all() and len(one["corr"]) == 0
        else:
            assert_exact(s, t, metric, one)


def test_selection_modes_and_capacity():
    from roitr_amd.descmatch import match_batch, select
    # integer descriptors: the restatement's indices are the kernel's, bit for bit, so order and content compare exactly
    cs = [U.make_int_case(20 + s, n, m, D=64) for s, (n, m) in enumerate([(333, 301), (90, 120), (257, 64)])]
    S, T = np.concatenate([c["src_desc"] for c in cs]), np.concatenate([c["tgt_desc"] for c in cs])
    so, to = ends(*[len(c["src_desc"]) for c in cs]), ends(*[len(c["tgt_desc"]) for c in cs])
    for mode in ("row", "col", "mutual"):
        r = match_batch(so, dev(S), to, dev(T), metric="dot", mode=mode)
        starts, corr = r["corr_starts"].cpu().numpy(), r["corr"].cpu().numpy()
        want = []
        for p, c in enumerate(cs):
            ref = U.match_f64(c["src_desc"], c["tgt_desc"], 0)
            want.append(U.select(ref["row_idx"], ref["col_idx"], mode))
            assert np.array_equal(corr[starts[p]:starts[p + 1]], want[-1]), (mode, p)   # order and content
        need = sum(len(w) for w in want)
        assert starts[-1] == need == len(corr)
        st2, cut, needed = select(so, to, r["row_idx"], r["col_idx"], mode, capacity=need - 1)
        assert needed == need and cut.shape[0] == need - 1 and np.array_equal(st2.cpu().numpy(), starts)
        assert np.array_equal(cut.cpu().numpy(), corr[:need - 1])
    # nothing beyond the capacity is written: the raw entry point on a guarded buffer
    from roitr_amd import _lib as L
    guard = torch.full((need + 8, 2), -7, dtype=torch.int32, device="cuda")
    st = torch.empty((4,), dtype=torch.int32, device="cuda")
    n_out = torch.empty((1,), dtype=torch.int32, device="cuda")
    L.check(L.lib().roitr_desc_match_select(3, so.data_ptr(), to.data_ptr(), r["row_idx"].data_ptr(), r["col_idx"].data_ptr(), 2,
                                            st.data_ptr(), guard.data_ptr(), need - 1, n_out.data_ptr(), L.stream_ptr().value), "select")
    g = guard.cpu().numpy()
    assert int(n_out.item()) == need and np.array_equal(g[:need - 1], corr[:need - 1]) and (g[need - 1:] == -7).all()


def test_mirrors_against_the_reference_golden():
    from roitr_amd.descmatch import get_inlier_ratio, matching_descriptors, mutual_selection
    g = golden()
    for seed in range(6):
        c = U.make_case(seed, 64, scale="unit" if seed % 2 == 0 else "x2")
        assert U.checksum(c) == str(g[f"checksum_{seed}"])
        s, t = c["src_desc"], c["tgt_desc"]
        for name, kw in (("row", dict(major="row")), ("col", dict(major="col")), ("union", dict(major=None)), ("mutual", dict(mutual=True))):
            got = matching_descriptors(s, t, **kw)
            assert isinstance(got, np.ndarray) and got.shape[1] == 2
            assert np.array_equal(got, g[f"md_{name}_{seed}"]), (seed, name)
        sel = mutual_selection(torch.from_numpy(s).cuda() @ torch.from_numpy(t).cuda().T)
        assert sel.dtype == np.bool_ and np.array_equal(np.stack(np.nonzero(sel[0]), 1), g[f"ms_{seed}"])
        r = get_inlier_ratio(c["src_pcd"], c["tgt_pcd"], s, t, c["rot"], c["trans"], inlier_distance_threshold=0.1)
        for k in ("wo", "w"):
            assert abs(float(r[k]["inlier_ratio"]) - float(g[f"ir_{k}_{seed}"])) <= 1e-6, (seed, k)
            assert isinstance(r[k]["distance"], np.ndarray) and r[k]["distance"].shape == g[f"dist_{k}_{seed}"].shape
            assert np.abs(r[k]["distance"] - g[f"dist_{k}_{seed}"]).max() < 1e-4


def test_descriptor_handle_end_to_end():
    from gpu_util import build_model, pair_to_device
    from roitr_amd.descmatch import descriptor_handle, get_inlier_ratio
    from roitr_amd.synthetic import make_pair
    model = build_model()
    pairs = [pair_to_device(make_pair(1024, pair_index=i)) for i in range(2)]
    h = model.launch_batch(pairs)
    outs = model.finish_batch(h)
    for which, ks, kt, fs, ft in (("point", "src_points", "tgt_points", "src_point_feats", "tgt_point_feats"),
                                  ("node", "src_nodes", "tgt_nodes", "src_node_feats", "tgt_node_feats")):
        d = descriptor_handle(h, which, 0.1)
        starts = d["starts"].cpu().numpy()
        assert d["src_pts"].shape == d["tgt_pts"].shape == (starts[-1], 3)
        for b, (p, o) in enumerate(zip(pairs, outs)):
            r = get_inlier_ratio(o[ks], o[kt], o[fs], o[ft], p["rot"], p["trans"], 0.1)
            assert int(d["n_wo"][b]) == o[ks].shape[0] and int(d["n_w"][b]) == len(r["w"]["distance"]) == starts[b + 1] - starts[b]
            assert abs(float(d["ir_wo"][b]) - float(r["wo"]["inlier_ratio"])) <= 1e-6, (which, b)
            w = float(r["w"]["inlier_ratio"])
            assert (np.isnan(w) and np.isnan(float(d["ir_w"][b]))) or abs(float(d["ir_w"][b]) - w) <= 1e-6, (which, b)
            corr = d["corr"][starts[b]:starts[b + 1]].long()
            assert torch.equal(d["src_pts"][starts[b]:starts[b + 1]], o[ks].float()[corr[:, 0]])
            assert torch.equal(d["tgt_pts"][starts[b]:starts[b + 1]], o[kt].float()[corr[:, 1]])


def test_ransac_pose_estimation_recovers_a_planted_pose():
    """400 points, the descriptors are the points' own coordinates (the target's mapped back) through a fixed random 64-wide
    projection and unit-normalised after a lift, so the best match of a point is its true correspondence.  Bounds: those of
    tests/test_registration_gpu.py::test_recovery_full_iterations without refinement (3 degrees, 0.05 m at 5 mm noise)."""
    from roitr_amd.registration import ransac_pose_estimation
    rng = np.random.default_rng(3)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    R = q * np.sign(np.linalg.det(q))
    t = rng.uniform(-1, 1, 3)
    src = rng.uniform(-1, 1, (400, 3))
    perm = rng.permutation(400)
    tgt = (src @ R.T + t + rng.normal(0, 0.005, (400, 3)))[perm]
    proj = rng.standard_normal((4, 64))
    def desc(x):   # lifted to the unit sphere first: the dot product then orders by distance
        l = np.concatenate([x, np.ones((len(x), 1))], 1)
        l /= np.linalg.norm(l, axis=1, keepdims=True)
        return (l @ proj).astype(np.float32)
    sf, tf = desc(src), desc((tgt - t) @ R)
    for mutual in (True, False):
        T = ransac_pose_estimation(src.astype(np.float32), tgt.astype(np.float32), sf, tf, mutual=mutual, distance_threshold=0.05)
        assert T.shape == (4, 4) and T.dtype == np.float64
        c = np.clip((np.trace(T[:3, :3].T @ R) - 1) / 2, -1, 1)
        rre, rte = np.degrees(np.arccos(c)), np.linalg.norm(T[:3, 3] - t)
        print(f"mutual {mutual}: RRE {rre:.3f} deg, RTE {rte:.4f} m")
        assert rre <= 3.0 and rte <= 0.05, (mutual, rre, rte)


def test_refusals():
    from roitr_amd import _lib as L
    from roitr_amd.descmatch import match_batch, select
    lib = L.lib()
    UNSUPPORTED, ARG = 3, 1   # csrc/common.h ROITR_ERR_UNSUPPORTED / ROITR_ERR_ARG
    i32, f32 = torch.int32, torch.float32
    off = torch.tensor([0, 8], dtype=i32, device="cuda")
    out_i, out_f = torch.full((8,), -5, dtype=i32, device="cuda"), torch.full((8,), -5.0, dtype=f32, device="cuda")
    ws = torch.empty((int(lib.roitr_desc_match_workspace_bytes(1, 8, 8)),), dtype=torch.uint8, device="cuda")
    def call(dim, desc, metric=0, nbytes=None, offsets=off):
        return lib.roitr_desc_match_batch(1, dim, None if offsets is None else offsets.data_ptr(), 8, desc.data_ptr(), off.data_ptr(), 8,
                                          desc.data_ptr(), metric, out_i.data_ptr(), out_f.data_ptr(), out_i.data_ptr(), out_f.data_ptr(),
                                          ws.data_ptr(), ws.numel() if nbytes is None else nbytes, L.stream_ptr().value)
    d8 = torch.zeros((8, 1032), dtype=f32, device="cuda")
    assert call(6, d8) == UNSUPPORTED and call(1028, d8) == UNSUPPORTED
    assert call(8, d8, offsets=None) == ARG and call(8, d8, nbytes=ws.numel() - 1) == ARG and call(8, d8, metric=2) == ARG
    torch.cuda.synchronize()
    assert (out_i == -5).all() and (out_f == -5).all()   # nothing was launched
    for dim in (6, 1028):
        with pytest.raises(L.RoitrError):
            match_batch(off, torch.zeros((8, dim), device="cuda"), off, torch.zeros((8, dim), device="cuda"))
    with pytest.raises(L.RoitrError):
        match_batch(off, torch.zeros((8, 8), device="cuda"), off, torch.zeros((8, 8), device="cuda"), metric="cosine")
    with pytest.raises(L.RoitrError):
        select(off, off, out_i, out_i, mode="diagonal")
    with pytest.raises(L.RoitrError):
        match_batch(off.cpu(), torch.zeros((8, 8)), off.cpu(), torch.zeros((8, 8)))
    st, n_out = torch.empty((2,), dtype=i32, device="cuda"), torch.empty((1,), dtype=i32, device="cuda")
    assert lib.roitr_desc_match_select(1, off.data_ptr(), off.data_ptr(), out_i.data_ptr(), out_i.data_ptr(), 3, st.data_ptr(),
                                       out_i.data_ptr(), 4, n_out.data_ptr(), L.stream_ptr().value) == ARG
