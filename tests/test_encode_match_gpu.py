"""GPU: encode once / match many (include/roitr_encode.h, RIGA_v2.encode_clouds / launch_match / match_batch, scene.match_pairs).

A pair's forward results are the same bytes alone and anywhere in a batch (tests/test_timed_shape_gpu.py), and the two new engine
calls queue the forward's own stage functions, so a pair matched from cached encodings must equal the forward of that pair BIT FOR
BIT: every comparison below is torch.equal, there is no tolerance anywhere in this module.

Six clouds -- sources and targets of three synthetic pairs of ragged sizes 1024 / 1024, 1500 / 2300, 5000 / 5000 (16, 23, 35 and 78
superpoints: different per cloud, no multiple of a tile of 16 rows except the smallest) -- are encoded ONCE per module, the
seven-pair list is forwarded once and matched once, and the tests share those results and never write to them."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import build_model, pair_to_device  # noqa: E402
from test_timed_shape_gpu import BITWISE_KEYS  # noqa: E402

from roitr_amd import riga, scene  # noqa: E402
from roitr_amd._lib import RoitrError, lib  # noqa: E402
from roitr_amd.synthetic import make_pair  # noqa: E402

KEYS = tuple(k for k in BITWISE_KEYS if not k.startswith("gt_")) + ("src_points", "tgt_points")
GT_KEYS = tuple(k for k in BITWISE_KEYS if k.startswith("gt_"))
SIZES = ((1024, 1024), (1500, 2300), (5000, 5000))
PAIR_INDEX = (3, 4, 5)
# the three true pairs, a cross pair between clouds of different sizes, a pair with the roles swapped, a self pair, one pair twice
PAIRS = [(0, 1), (2, 3), (4, 5), (2, 5), (3, 2), (4, 4), (2, 3)]


def assert_same(a, b, what):
    for k in KEYS:
        x, y = a[k], b[k]
        assert x.shape == y.shape, (what, k, tuple(x.shape), tuple(y.shape))
        assert torch.equal(x, y), (what, k)
    for k in GT_KEYS:
        assert a[k] is None, (what, k)


def forward_pair(clouds, s, t):
    """The forward() arguments of the pair (cloud s, cloud t), built from the same tensors the clouds were encoded from.  The forward
    has one coordinate set for a target, so target-side clouds here have no points_out."""
    assert "points_out" not in clouds[t]
    cs, ct = clouds[s], clouds[t]
    return dict(src_pcd=cs.get("points_out", cs["points"]), src_raw_pcd=cs["points"], src_normals=cs["normals"], src_feats=cs["feats"],
                tgt_pcd=ct["points"], tgt_normals=ct["normals"], tgt_feats=ct["feats"])


@pytest.fixture(scope="module")
def S():
    model = build_model("3DMatch", weights="selective")
    clouds = []
    for (ns, nt), idx in zip(SIZES, PAIR_INDEX):
        p = pair_to_device(make_pair(ns, nt, config=2, pair_index=idx, normals="field"))
        clouds.append(dict(points=p["src_raw_pcd"], normals=p["src_normals"], feats=p["src_feats"]))
        clouds.append(dict(points=p["tgt_pcd"], normals=p["tgt_normals"], feats=p["tgt_feats"]))
    # cloud 0 reports its correspondences in other coordinates than its geometry (src_pcd != src_raw_pcd): a fixed rigid motion
    c, s = 0.8, 0.6
    rot = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], device="cuda")
    clouds[0]["points_out"] = (clouds[0]["points"] @ rot.T + torch.tensor([0.25, -0.5, 1.0], device="cuda")).contiguous()
    with torch.no_grad():
        enc = model.encode_clouds(clouds)
        fwd = model.forward_batch([forward_pair(clouds, s_, t_) for s_, t_ in PAIRS], want_gt=False)
        got = model.match_batch(enc, PAIRS)
    torch.cuda.synchronize()
    return dict(model=model, clouds=clouds, enc=enc, fwd=fwd, got=got)


def test_match_equals_the_forward_bitwise(S):
    model, clouds, fwd, got = S["model"], S["clouds"], S["fwd"], S["got"]
    # the comparison is not empty, and the pad path of the cached gather is on it -- asserted on the FORWARD's results
    n_corr = [int(r["corr_scores"].shape[0]) for r in fwd]
    print("correspondences per pair of the forward:", n_corr, " coarse:", [int(r["src_node_corr_indices"].shape[0]) for r in fwd])
    assert min(n_corr[:3]) > 100, n_corr
    assert not bool(fwd[0]["_src_node_knn_masks"].all()) and not bool(fwd[0]["_tgt_node_knn_masks"].all())   # N = 1024: nodes with < 64 points
    assert not bool(fwd[0]["src_node_corr_knn_masks"].all()), "no selected patch of the 1024-point pair has a pad slot"
    assert not torch.equal(fwd[0]["src_points"], clouds[0]["points"])                                         # the points_out cloud
    assert len(got) == len(PAIRS)
    for j, pair in enumerate(PAIRS):
        assert_same(got[j], fwd[j], f"pair {j} {pair}: match vs the forward of the same list")
    with torch.no_grad():
        for j in (0, 3):
            alone = model.forward_batch([forward_pair(clouds, *PAIRS[j])], want_gt=False)[0]
            assert_same(got[j], alone, f"pair {j} {PAIRS[j]}: match vs the forward of the pair alone")
    # cloud-level entries are views into the cache, not copies
    a = S["enc"].arrays
    assert got[1]["src_point_feats"].untyped_storage().data_ptr() == a["point_feats"].untyped_storage().data_ptr()
    assert got[1]["tgt_nodes"].untyped_storage().data_ptr() == a["node_xyz"].untyped_storage().data_ptr()


def test_cache_of_two_encode_calls_and_of_a_cloud_alone(S):
    model, clouds, enc = S["model"], S["clouds"], S["enc"]
    with torch.no_grad():
        two = model.encode_clouds(clouds, clouds_per_call=3)      # clouds 0 - 2, then 3 - 5, through offset pointers
        alone = model.encode_clouds([clouds[3]])
    per, total = riga.cache_bytes(enc.n_points, 256, 64)
    assert enc.nbytes == total and [a.numel() * 4 for a in enc.arrays.values()] == per
    for k in riga.CACHE_ARRAYS:
        assert torch.equal(two.arrays[k], enc.arrays[k]), k
    rows = enc.cloud(3)
    for k, v in alone.cloud(0).items():
        assert v.shape == rows[k].shape and torch.equal(v, rows[k]), k
    assert bytes(two.seg) == bytes(enc.seg) and torch.equal(two.seg_dev, enc.seg_dev)


def test_slot_and_batch_invariance(S):
    model, enc, got = S["model"], S["enc"], S["got"]
    with torch.no_grad():
        h = model.launch_match(enc, [PAIRS[-1]], want_node_xyz=True)
        one = model.finish_batch(h)
    assert_same(one[0], got[-1], "slot 0 of a 1-pair call vs the last slot of the 7-pair call")
    # the optional node_xyz output: the cache rows of the two slots in the call layout
    s, t = PAIRS[-1]
    assert torch.equal(h["out"]["node_xyz"], torch.cat([enc.cloud(s)["node_xyz"], enc.cloud(t)["node_xyz"]]))


def test_repeats_and_interleaving(S):
    model, clouds, got = S["model"], S["clouds"], S["got"]
    with torch.no_grad():
        again = model.match_batch(S["enc"], PAIRS)
        enc = model.encode_clouds(clouds)
        model.forward_batch([forward_pair(clouds, 4, 5), forward_pair(clouds, 2, 1)], want_gt=False)   # the arenas are shared
        after = model.match_batch(enc, PAIRS)
        h0 = model.launch_match(enc, PAIRS)
        h1 = model.launch_match(enc, PAIRS[::-1])
        r0, r1 = model.finish_batch(h0), model.finish_batch(h1)
    for j in range(len(PAIRS)):
        assert_same(again[j], got[j], f"pair {j}: the same match twice")
        assert_same(after[j], got[j], f"pair {j}: a forward between encode and match")
        assert_same(r0[j], got[j], f"pair {j}: first of two calls in flight")
        assert_same(r1[len(PAIRS) - 1 - j], got[j], f"pair {j}: second of two calls in flight")


def raw_match(model, enc, src, tgt, table=None, stream=None):
    """roitr_engine_match itself with no output buffer: (status, message)."""
    io, keep = model._match_io(enc, src, tgt, {})
    rc = riga._cache_lib().roitr_engine_match(model._engine, ctypes.byref(enc.table if table is None else table), ctypes.byref(io), stream)
    return rc, lib().roitr_last_error().decode()


def copied_table(enc):
    """A copy of the cache's table with a host segment array of its own, to spoil."""
    t = riga._CCloudTable.from_buffer_copy(enc.table)
    seg = (riga._CCloudSeg * len(enc)).from_buffer_copy(enc.seg)
    t.seg = ctypes.cast(seg, ctypes.c_void_p)
    return t, seg


def test_refusals(S):
    model, clouds, enc = S["model"], S["clouds"], S["enc"]
    small = dict(points=clouds[0]["points"][:200].contiguous(), normals=clouds[0]["normals"][:200].contiguous(), feats=clouds[0]["feats"][:200].contiguous())
    with torch.no_grad():
        # modes out of scope: refused by both calls, with the reason
        for kind, kw, word in (("3DMatch", dict(operand_dtype="bf16"), "operand_dtype 1"), ("4DMatch", {}, "adaptive_coarse")):
            other = build_model(kind, weights="selective", **kw)
            with pytest.raises(RoitrError, match=word):
                other.encode_clouds(clouds[:2])
            rc, msg = raw_match(other, enc, [0], [1])
            assert rc == 1 and word in msg, (rc, msg)
            with pytest.raises(RoitrError, match="another engine"):
                other.match_batch(enc, [(0, 1)])
            del other
        # a cloud index outside the table; B outside the forward's range; a cloud smaller than the forward accepts
        with pytest.raises(RoitrError, match="outside the table"):
            model.launch_match(enc, [(0, 1), (0, 6)])
        for src, tgt in (([6], [1]), ([0], [-1])):
            rc, msg = raw_match(model, enc, src, tgt)
            assert rc == 1 and "outside the table" in msg, (rc, msg)
        for B in (0, 200000):                       # 200 000 pairs x 256 patches x 64 points: past the forward's 2^31 patch rows
            rc, msg = raw_match(model, enc, [0] * B, [1] * B)
            assert rc == 1 and "pairs outside the range" in msg, (B, rc, msg)
        # a table the gathers could not walk: a misaligned node_geo array, point rows past 2^31, a negative row
        t, seg = copied_table(enc)
        t.node_geo = enc.arrays["node_geo"].data_ptr() + 4
        rc, msg = raw_match(model, enc, [0], [1], table=t)
        assert rc == 1 and "16-byte aligned" in msg, (rc, msg)
        for field, value in (("pt_row0", 2 ** 31 - 100), ("node_row0", -1)):
            t, seg = copied_table(enc)
            setattr(seg[5], field, value)
            rc, msg = raw_match(model, enc, [0], [1], table=t)
            assert rc == 1 and "past 2^31" in msg, (field, rc, msg)
        with pytest.raises(RoitrError, match="smaller than the model accepts"):
            model.encode_clouds([clouds[1], small])
        eio = riga._CEncodeIO()
        n = (ctypes.c_int * 1)(200)
        eio.clouds, eio.n_points = 1, ctypes.cast(n, ctypes.c_void_p)
        buf = torch.zeros(200 * 256, device="cuda")
        for f, _ in riga._CEncodeIO._fields_[2:]:
            setattr(eio, f, buf.data_ptr())
        assert riga._cache_lib().roitr_engine_encode(model._engine, ctypes.byref(eio), None) == 1
        assert "cloud too small" in lib().roitr_last_error().decode()
        assert model.match_batch(enc, []) == []
        # a match handle is not a forward handle
        h = model.launch_match(enc, [(0, 1)])
        for call in (lambda: riga.handle_layout(h, "point"), lambda: riga.handle_normals(h), lambda: riga.handle_poses(h, "test")):
            with pytest.raises(RoitrError, match="launch_match"):
                call()
        first = model.finish_batch(h)[0]
        for k in GT_KEYS:
            assert first[k] is None
        # the engine serves a correct forward and a correct match afterwards
        assert_same(model.match_batch(enc, [PAIRS[1]])[0], S["got"][1], "match after the refusals")
        alone = model.forward_batch([forward_pair(clouds, *PAIRS[1])], want_gt=False)[0]
        assert_same(S["got"][1], alone, "forward after the refusals")


def test_stale_cache_is_refused(S):
    clouds = S["clouds"]
    model = build_model("3DMatch", weights="selective")          # a model of its own: the change below must not reach the shared one
    with torch.no_grad():
        enc = model.encode_clouds(clouds[:2])
        assert_same(model.match_batch(enc, [(0, 1)])[0], S["got"][0], "a second model with the same weights")
        with pytest.raises(RoitrError, match="another engine"):
            S["model"].match_batch(enc, [(0, 1)])
        model.coarse_proj.bias.add_(0.125)                         # a changed weight between encode and match
        with pytest.raises(RoitrError, match="weights changed"):
            model.match_batch(enc, [(0, 1)])
        enc = model.encode_clouds(clouds[:2])                      # encoded again, the cache serves the new weights
        new = model.match_batch(enc, [(0, 1)])[0]
        ref = model.forward_batch([forward_pair(clouds, 0, 1)], want_gt=False)[0]
    assert_same(new, ref, "after the weight change")


def test_scene_driver_yields_in_list_order(S):
    model, enc = S["model"], S["enc"]
    pairs = PAIRS + [(0, 3), (4, 1), (2, 1)]                       # 10 pairs, calls of 4 + 4 + 2
    with torch.no_grad():
        whole = model.match_batch(enc, pairs)
        out = list(scene.match_pairs(model, S["clouds"], pairs, pairs_per_call=4))
    assert [p for p, _ in out] == pairs
    for j, (_, r) in enumerate(out):
        assert_same(r, whole[j], f"pair {j} {pairs[j]}: driver vs one match call")


def test_f32x3_match_equals_its_own_forward(S):
    """operand_dtype 2 falls out of the engine's shared Gemm object (the K >= 256 layers of both halves take the three-way split exactly
    as the forward's do): supported, bitwise against the f32x3 forward."""
    clouds = S["clouds"]
    model = build_model("3DMatch", operand_dtype="f32x3", weights="selective")
    pairs = [(0, 1), (2, 3), (3, 2)]
    with torch.no_grad():
        enc = model.encode_clouds(clouds[:4])
        got = model.match_batch(enc, pairs)
        fwd = model.forward_batch([forward_pair(clouds, s, t) for s, t in pairs], want_gt=False)
    assert min(int(r["corr_scores"].shape[0]) for r in fwd[:2]) > 100
    for j in range(len(pairs)):
        assert_same(got[j], fwd[j], f"f32x3 pair {j}")


def test_a_capturing_stream_is_refused(S):
    """No graph capture: both calls refuse a stream that is capturing, before they stage or launch anything."""
    from roitr_amd._lib import stream_ptr
    model, clouds, enc = S["model"], S["clouds"], S["enc"]
    x = torch.zeros(16, device="cuda")
    eio = riga._CEncodeIO()
    n = (ctypes.c_int * 1)(1024)
    eio.clouds, eio.n_points = 1, ctypes.cast(n, ctypes.c_void_p)
    buf = torch.zeros(1024 * 256, device="cuda")
    for f, _ in riga._CEncodeIO._fields_[2:]:
        setattr(eio, f, buf.data_ptr())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x += 1                                   # the capture is not empty
        rc_m, msg_m = raw_match(model, enc, [0], [1], stream=stream_ptr())
        rc_e = riga._cache_lib().roitr_engine_encode(model._engine, ctypes.byref(eio), stream_ptr())
        msg_e = lib().roitr_last_error().decode()
    assert rc_m == 1 and "capturing" in msg_m, (rc_m, msg_m)
    assert rc_e == 1 and "capturing" in msg_e, (rc_e, msg_e)
    with torch.no_grad():
        assert_same(model.match_batch(enc, [PAIRS[0]])[0], S["got"][0], "match after the refused capture")
