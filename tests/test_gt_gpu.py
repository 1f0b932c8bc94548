"""GPU: the ground-truth side outputs (csrc/gt.hip: padded clouds, node occlusion scores, node correspondences) against the
float64 restatement of tests/gt_util.py, kernel by kernel through the ctypes fronts of roitr_amd.ops and once through the engine.

Inputs are built in numpy (tests/gt_util.py) with the partition computed in float64, so masks, pad indices and ragged sizes are what
each test wants.  On the lattice inputs every fp32 operation of the kernels is exact (gt_util.is_exact; asserted on the CPU in
tests/test_gt_cpu.py) and the results are demanded bit for bit; on random clouds each value must lie inside its interval and the
list must obey must / must-not in row-major order."""
import os
import re

import numpy as np
import pytest
import torch

import gt_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_IV = {}


def intervals(name, pairs, pos_radius=U.POS_RADIUS):
    """float64 intervals of a seeded batch, computed once per session."""
    if name not in _IV:
        _IV[name] = [(U.corr_intervals(p, pos_radius), U.occ_intervals(p)) for p in pairs]
    return _IV[name]


def run_kernels(pairs, pos_radius=U.POS_RADIUS, thr=U.OCC_THR):
    """The three entry points, wired as the engine wires them: padded clouds -> kNN(1) capped at 1.01 thr^2, both directions, the
    target half addressed by the relative offsets -> occlusion scores; node correspondences.  -> per pair (idx, overlaps, occ_tgt,
    occ_src) as numpy, plus the raw (padded, offsets)."""
    from roitr_amd import ops, pointops
    k = U.pack(pairs)
    B = k["pairs"]
    d = {n: torch.from_numpy(v).cuda() for n, v in k.items() if isinstance(v, np.ndarray)}
    idx, ov, cnt = ops.node_correspondences(d["nodes"], d["node_offset"], d["node_masks"], d["points"], d["pt_offset"], d["knn_idx"],
                                            d["knn_mask"], d["rot"], d["trans"], pos_radius, max_nodes=k["max_nodes"])
    padded, off = ops.build_padded_clouds(d["points"], d["pt_offset"], d["rot"], d["trans"])
    tsp = int(k["pt_offset"][B - 1]) + B
    src_p, tgt_p, off_s, off_t = padded[:tsp], padded[tsp:], off[:B].contiguous(), off[2 * B:].contiguous()
    cap2 = float(np.float32(thr) * np.float32(thr) * np.float32(1.01))
    d2 = torch.cat([pointops.knn_within(tgt_p, src_p, off_t, off_s, cap2), pointops.knn_within(src_p, tgt_p, off_s, off_t, cap2)])
    occ = ops.node_occlusion_score(d["cloud_of_node"], d["pt_offset"], d["knn_idx"], d["knn_mask"], d["node_masks"], d2, thr)
    torch.cuda.synchronize()
    idx, ov, cnt, occ = idx.cpu().numpy(), ov.cpu().numpy(), cnt.cpu().numpy(), occ.cpu().numpy()
    no = np.concatenate([[0], k["node_offset"]])
    res = [(idx[b, :cnt[b]], ov[b, :cnt[b]], occ[no[B + b]:no[B + b + 1]], occ[no[b]:no[b + 1]]) for b in range(B)]
    return res, padded.cpu().numpy(), off.cpu().numpy(), k


def check_interval(p, iv, got, what):
    civ, oiv = iv
    idx, ov, occ_t, occ_s = got
    U.check_corr(idx, ov, civ, what)
    U.check_occ(occ_t, oiv, "tgt", what)
    U.check_occ(occ_s, oiv, "src", what)


def check_exact(p, iv, got, what):
    civ, oiv = iv
    idx, ov, occ_t, occ_s = got
    assert civ["band"] == 0.0 and np.array_equal(civ["lo"], civ["hi"]), what
    want = np.argwhere(civ["lo"] > 0)                      # row-major (i, j)
    assert idx.shape[0] == want.shape[0], (what, "count", idx.shape[0], want.shape[0])
    assert np.array_equal(idx, want), (what, "index list")
    assert np.array_equal(ov, U.exact_overlaps(civ, want)), (what, "overlaps")
    assert np.array_equal(occ_t, U.exact_scores(oiv, p, "tgt")), (what, "tgt occlusion")
    assert np.array_equal(occ_s, U.exact_scores(oiv, p, "src")), (what, "src occlusion")


def test_lattice_batch_is_bit_exact():
    """B = 3 ragged pairs (40, 37), (33, 64), (5, 70), max_nodes 70, a signed permutation and a translation of its own per pair:
    two compaction rounds (1480 entries), several prune workgroups per pair, n_s != max_nodes, rot / trans indexed by pair."""
    pairs = U.lattice_batch()
    assert [(p["tgt_nodes"].shape[0], p["src_nodes"].shape[0]) for p in pairs] == U.SHAPES
    for x in range(3):
        for y in range(x + 1, 3):      # a kernel that reads another pair's rot or trans cannot pass
            assert not np.array_equal(pairs[x]["rot"], pairs[y]["rot"]) and not np.array_equal(pairs[x]["trans"], pairs[y]["trans"])
    res, _, _, k = run_kernels(pairs)
    assert k["max_nodes"] == 70
    for b, (p, iv, got) in enumerate(zip(pairs, intervals("lattice", pairs), res)):
        print(f"lattice pair {b}: {got[0].shape[0]} node pairs listed, band {iv[0]['band']}")
        assert got[0].shape[0] >= 5
        check_exact(p, iv, got, f"lattice pair {b}")
        check_interval(p, iv, got, f"lattice pair {b}")


def test_a_workgroup_takes_a_second_triple():
    """B = 4 pairs of (70, 70) nodes, source = target inside a small ball.  Two pairs sit inside 0.47 pos_radius: all their 9 800
    node pairs survive the prune with overlap exactly 1.  Two sit in a ball wider than pos_radius: their overlaps differ from one
    node pair to the next, so a triple answered from the previous triple's shared records would show.  More node pairs pass the
    sphere test (float64, by a margin of 1e-4) than the patch-overlap kernel's grid has workgroups: its grid-stride loop repeats."""
    src = open(os.path.join(ROOT, "roitr_amd", "csrc", "gt.hip")).read()
    m = re.search(r"node_corr_kernel<<<\(unsigned\)std::min<long>\(total, (\d+)\)", src)
    total = re.search(r"const long total = \(long\)a->pairs \* a->max_nodes \* a->max_nodes;", src)
    assert m and total, "the launch of node_corr_kernel no longer reads min(pairs * max_nodes^2, cap)"
    pairs = U.ball_batch()
    grid = min(len(pairs) * 70 * 70, int(m.group(1)))
    survivors = sum(int(U.sphere_pass(p).sum()) for p in pairs)
    print(f"ball batch: {survivors} node pairs pass the sphere test, grid {grid}")
    assert len(pairs) * 70 * 70 == 19600 and survivors > grid
    res, _, _, _ = run_kernels(pairs)
    want = np.stack(np.meshgrid(np.arange(70), np.arange(70), indexing="ij"), -1).reshape(-1, 2)
    for b, (p, iv, got, steps) in enumerate(zip(pairs, intervals("ball", pairs), res, U.BALL_STEPS)):
        if steps == 6:
            assert np.array_equal(got[0], want), b
            assert np.array_equal(got[1], np.ones(4900, np.float32)), b
            assert np.array_equal(got[2], np.ones(70, np.float32)) and np.array_equal(got[3], np.ones(70, np.float32)), b
        else:
            assert np.unique(got[1]).size > 50, b
        check_exact(p, iv, got, f"ball pair {b}")


@pytest.mark.parametrize("name", U.EDGES)
def test_edges(name):
    """node_masks == 0 on both sides / patches of 1, 17, 63 valid points / a source pad row that reaches target points only through
    the transform / a pair 10 m apart between two ordinary ones / sphere test passed with zero overlap / B = 1."""
    pairs, exact = U.edge_batch(name)
    res, _, _, _ = run_kernels(pairs)
    ivs = intervals("edge_" + name, pairs)
    for b, (p, iv, got, ex) in enumerate(zip(pairs, ivs, res, exact)):
        what = f"{name} pair {b}"
        check_interval(p, iv, got, what)
        if ex:
            check_exact(p, iv, got, what)
    if name == "far_pair":
        assert res[1][0].shape[0] == 0 and not res[1][2].any() and not res[1][3].any()
        assert res[0][0].shape[0] > 0 and res[2][0].shape[0] > 0
    if name == "sphere_zero":
        zero = U.sphere_pass_zero_overlap(pairs[0], ivs[0][0])
        listed = np.zeros_like(zero)
        listed[res[0][0][:, 0], res[0][0][:, 1]] = True
        assert zero.sum() >= 5 and not (zero & listed).any()
    if name == "node_masks":
        p = pairs[0]
        assert p["tgt_node_mask"][res[0][0][:, 0]].all() and p["src_node_mask"][res[0][0][:, 1]].all()
        assert not res[0][2][~p["tgt_node_mask"]].any() and not res[0][3][~p["src_node_mask"]].any()


def test_random_batch_lies_inside_the_intervals():
    """The ragged shapes again on make_pair-like clouds with full-range rotations (nothing exact): interval check."""
    pairs = U.random_batch()
    res, _, _, _ = run_kernels(pairs)
    for b, (p, iv, got) in enumerate(zip(pairs, intervals("random", pairs), res)):
        sp, sn = U.undecided_shares(*iv)
        print(f"random pair {b}: {got[0].shape[0]} listed, band {iv[0]['band']:.3e}, undecided node pairs {sp:.4f}, scores {sn:.4f}")
        check_interval(p, iv, got, f"random pair {b}")


def test_build_padded_clouds():
    """Rows and the 3 * pairs offsets for ragged clouds against float64; the pad row of a source cloud equals trans."""
    pairs = U.random_batch()
    _, padded, off, k = run_kernels(pairs)
    B, po = k["pairs"], np.concatenate([[0], k["pt_offset"]]).astype(np.int64)
    want_off = [po[c + 1] + c + 1 for c in range(2 * B)]
    want_off += [want_off[B + b] - want_off[B - 1] for b in range(B)]
    assert off.tolist() == want_off
    assert padded.shape[0] == po[-1] + 2 * B
    worst, scale = 0.0, 0.0
    for c in range(2 * B):
        rows = padded[po[c] + c:po[c + 1] + c + 1]
        pts = U.f64(k["points"][po[c]:po[c + 1]])
        if c < B:
            rot, trans = U.f64(k["rot"][c]), U.f64(k["trans"][c])
            want = np.concatenate([pts, np.zeros((1, 3))]) @ rot.T + trans
            assert np.array_equal(rows[-1], k["trans"][c]), c
        else:
            want = np.concatenate([pts, np.zeros((1, 3))])
            assert np.array_equal(rows, want.astype(np.float32)), c      # target rows are copies
        worst, scale = max(worst, float(np.abs(rows - want).max())), max(scale, float(np.abs(want).max()), float(np.abs(pts).max()))
    tol = 4 * float(np.spacing(np.float32(scale)))
    print(f"build_padded_clouds: largest coordinate {scale:.4f}, tolerance {tol:.3e}, worst error {worst:.3e}")
    assert worst <= tol


@pytest.mark.parametrize("benchmark", ["3DMatch", "4DMatch"])
def test_engine_side_outputs_lie_inside_the_intervals(benchmark):
    """model.forward_batch on three ragged pairs (node counts on both sides of 32): the restatement is fed the engine's own points,
    nodes and partition plus the pair's rot / trans, so only the wiring of the ground-truth calls inside the engine is under test
    (offsets, the grid switch of the occlusion search, its cap, the side stream)."""
    from gpu_util import build_model, pair_to_device
    from roitr_amd.synthetic import make_pair
    model = build_model(benchmark, weights="selective")
    specs = [(2400, 2600, 0), (3100, 2112, 1), (1024, 1024, 2)]
    pairs = [pair_to_device(make_pair(ns, nt, config=7, pair_index=i, normals="field")) for ns, nt, i in specs]
    with torch.no_grad():
        outs = model.forward_batch(pairs)
    torch.cuda.synchronize()
    n = lambda t: t.cpu().numpy()   # noqa: E731
    sizes = []
    for b, (pair, out) in enumerate(zip(pairs, outs)):
        p = dict(rot=n(pair["rot"]), trans=n(pair["trans"]).reshape(3))
        for s in ("tgt", "src"):
            p[s + "_points"], p[s + "_nodes"] = n(out[s + "_points"]), n(out[s + "_nodes"])
            p[s + "_knn_idx"] = n(out[f"_{s}_node_knn_indices"]).astype(np.int32)
            p[s + "_knn_mask"], p[s + "_node_mask"] = n(out[f"_{s}_node_knn_masks"]).astype(bool), n(out[f"_{s}_node_masks"]).astype(bool)
        sizes += [p["tgt_nodes"].shape[0], p["src_nodes"].shape[0]]
        civ, oiv = U.corr_intervals(p, model.matching_radius), U.occ_intervals(p)
        sp, sn = U.undecided_shares(civ, oiv)
        print(f"{benchmark} pair {b}: nodes {sizes[-2:]}, radius {model.matching_radius}, {out['gt_node_corr_indices'].shape[0]} listed, "
              f"band {civ['band']:.3e}, undecided node pairs {sp:.4f}, scores {sn:.4f}")
        U.check_corr(n(out["gt_node_corr_indices"]), n(out["gt_node_corr_overlaps"]), civ, f"{benchmark} pair {b}")
        U.check_occ(n(out["gt_tgt_node_occ"]), oiv, "tgt", f"{benchmark} pair {b}")
        U.check_occ(n(out["gt_src_node_occ"]), oiv, "src", f"{benchmark} pair {b}")
        assert (civ["lo"] > 0).sum() > 0
    assert min(sizes) < 32 < max(sizes), sizes
