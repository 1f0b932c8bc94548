"""GPU: the pair ground truth of csrc/pairgt.hip (roitr_amd/pairgt.py) against the float64 restatement of tests/pairgt_util.py.

count, nn_idx, nn_dist2, n_hit, the correspondence list, its offsets and the status words are compared BIT FOR BIT (both sides follow
the same float64 rule on the fp32 inputs); the information matrix within 1e-12 x the sum of the absolute terms of each entry (the two
sum in different orders)."""
import numpy as np
import pytest
import torch

import pairgt_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda"


def to_dev(srcs, tgts, Rs, ts):
    cat = lambda cs: torch.from_numpy(np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in cs])).to(DEV)
    off = lambda cs: torch.tensor(np.cumsum([len(c) for c in cs]).astype(np.int32), device=DEV)
    rot = torch.from_numpy(np.stack([np.asarray(R, np.float32).reshape(3, 3) for R in Rs])).to(DEV)
    trans = torch.from_numpy(np.stack([np.asarray(t, np.float32).reshape(3) for t in ts])).to(DEV)
    return cat(srcs), off(srcs), cat(tgts), off(tgts), rot, trans


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_batch(srcs, tgts, Rs, ts, radius, Ks=(None,), capacity=None):
    """Every output of both entry points against the restatement; returns (device result, restatement)."""
    from roitr_amd import pairgt
    args = to_dev(srcs, tgts, Rs, ts)
    got = pairgt.pair_ground_truth(*args, radius)
    want = U.batch_brute(srcs, tgts, Rs, ts, radius)
    swapped = U.batch_brute(tgts, srcs, Rs, ts, radius, inverse=True)
    assert np.array_equal(got.status.cpu().numpy(), want["status"] | swapped["status"])
    assert np.array_equal(got.count.cpu().numpy(), want["count"])
    assert np.array_equal(got.nn_idx.cpu().numpy(), want["nn_idx"])
    assert np.array_equal(bits(got.nn_dist2.cpu().numpy()), bits(want["nn_dist2"]))
    assert np.array_equal(got.n_src_hit.cpu().numpy(), want["n_hit"])
    assert np.array_equal(got.n_tgt_hit.cpu().numpy(), swapped["n_hit"])          # the target side: an integer count, exact
    for key, ref in (("overlap_src", want), ("overlap_tgt", swapped)):
        g = getattr(got, key).cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(ref["overlap"])) and np.array_equal(bits(np.nan_to_num(g)), bits(np.nan_to_num(ref["overlap"])))
    info = got.info.cpu().numpy()
    assert np.array_equal(info[:, 0, 0], want["n_hit"].astype(np.float64))
    for b, r in enumerate(want["pairs"]):
        hit = np.asarray(srcs[b], np.float32).reshape(-1, 3)[r["count"] > 0].astype(np.float64) if r["status"] == 0 else np.zeros((0, 3))
        assert (np.abs(info[b] - r["info"]) <= 1e-12 * U.info_abs_terms(hit)).all(), b
    for K in Ks:
        wk = want if K is None else U.batch_brute(srcs, tgts, Rs, ts, radius, K=K)
        corr, off, status = pairgt.radius_correspondences(*args, radius, K=K, capacity=capacity, return_status=True)
        assert np.array_equal(off.cpu().numpy(), wk["corr_offset"]), K
        assert np.array_equal(corr.cpu().numpy(), wk["corr"]), K
        assert np.array_equal(status.cpu().numpy(), want["status"]), K
    return got, want


def signed_permutation(rng):
    R = np.zeros((3, 3), np.float32)
    R[np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], size=3)
    return R


def test_exact_lattice_with_ties_and_duplicates():
    # multiples of 1/8, signed permutation, lattice translation: every d2 is an exact multiple of 1/64 and r * r = 0.09 lies strictly
    # between 5/64 and 6/64 -- no pair near the boundary, many exact ties (and duplicate points) for the (d2, j) order
    rng = np.random.default_rng(0)
    src = (rng.integers(-17, 18, size=(600, 3)) / 8).astype(np.float32)
    R, t = signed_permutation(rng), (rng.integers(-8, 9, size=3) / 8).astype(np.float32)
    tgt = (rng.integers(-17, 18, size=(700, 3)) / 8).astype(np.float32) @ R.T + t
    tgt[:40] = tgt[40:80]       # duplicates
    got, want = check_batch([src], [tgt], [R], [t], 0.3, Ks=(None, 1, 3))
    d2 = want["pairs"][0]["d2"]
    assert 400 < len(want["corr"]) < 1200 and np.array_equal(d2 * 64, np.round(d2 * 64))
    runs = want["count"][want["count"] > 1]
    assert len(runs) > 50       # runs that need an order at all


def random_pair(rng, n, m, noise=0.01, shift=1.0):
    src = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    R, t = U.random_rigid(rng, shift=shift)
    base = U.move(src[rng.integers(0, n, size=m)] if n else np.zeros((m, 3), np.float32), R, t)
    return src, (base + rng.normal(size=(m, 3)) * noise).astype(np.float32), R, t


def test_random_clouds_random_rigid_transform_and_caps():
    rng = np.random.default_rng(1)
    src, tgt, R, t = random_pair(rng, 2000, 2500, noise=0.03)
    got, want = check_batch([src], [tgt], [R], [t], 0.1, Ks=(None, 1, 3, 10 ** 6))
    assert want["count"].max() > 8 and (want["count"] == 0).any() and len(want["corr"]) > 5000


@pytest.mark.parametrize("B", [1, 2, 37])
def test_ragged_batches_with_empty_and_single_point_clouds(B):
    rng = np.random.default_rng(10 + B)
    srcs, tgts, Rs, ts = [], [], [], []
    for b in range(B):
        n, m = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        if B == 37:
            n, m = {3: (0, m), 4: (n, 0), 5: (1, m), 6: (n, 1), 36: (0, 0)}.get(b, (n, m))
        s, t_, R, t = random_pair(rng, n, m, noise=0.02)
        srcs.append(s); tgts.append(t_); Rs.append(R); ts.append(t)
    got, want = check_batch(srcs, tgts, Rs, ts, 0.08, Ks=(None, 2))
    if B == 37:
        assert [int(want["status"][b]) for b in (3, 4, 5, 6, 36)] == [2, 2, 0, 0, 2]
        assert np.isnan(got.overlap_src.cpu().numpy()[[3, 4, 36]]).all()
    assert len(want["corr"]) > 20 * B


def test_source_counts_around_a_workgroup():
    rng = np.random.default_rng(2)
    parts = [random_pair(rng, n, 400, noise=0.02) for n in (255, 256, 257)]
    for p in parts:                                     # alone: the last workgroup is full, one short, one over
        check_batch([p[0]], [p[1]], [p[2]], [p[3]], 0.08)
    check_batch(*[list(x) for x in zip(*parts)], 0.08)   # and together: pair borders inside a workgroup


def planted(rng, sizes, spread=0.01):
    """Target clusters of the given sizes around centres 2 apart, one source point per centre plus one with nothing near it."""
    centres = np.array([[2.0 * k, 0.5 * (k % 3), -0.25 * k] for k in range(len(sizes))])
    tgt = np.concatenate([c + rng.uniform(-spread, spread, size=(s, 3)) for c, s in zip(centres, sizes)]).astype(np.float32)
    src = np.concatenate([centres, [[-7.0, 3.0, 3.0]]]).astype(np.float32)
    return src, tgt[rng.permutation(len(tgt))]


def test_run_lengths_0_1_2_63_64_65_and_above_1024():
    rng = np.random.default_rng(3)
    sizes = [1, 2, 63, 64, 65, 1500, 129]
    src, tgt = planted(rng, sizes)
    R, t = U.random_rigid(rng)
    tgt = U.move(tgt, R, t).astype(np.float32)
    got, want = check_batch([src], [tgt], [R], [t], 0.05, Ks=(None, 1, 3, 64, 2000))
    assert want["count"].tolist() == sizes + [0]


def test_radius_a_hundredth_of_the_cell_size():
    # 3000 uniform points in a cube of side 2 at ~6 per cell: cells of ~0.25; r = 0.0025
    rng = np.random.default_rng(4)
    src, tgt, R, t = random_pair(rng, 3000, 3000, noise=0.001)
    got, want = check_batch([src], [tgt], [R], [t], 0.0025)
    assert 200 < len(want["corr"]) < 3000


def test_radius_beyond_the_target_extent_takes_every_pair():
    rng = np.random.default_rng(5)
    srcs = [rng.uniform(-1, 1, size=(n, 3)).astype(np.float32) for n in (50, 7)]
    tgts = [rng.uniform(-1, 1, size=(m, 3)).astype(np.float32) for m in (60, 90)]
    Rs, ts = zip(*[U.random_rigid(rng, shift=0.3) for _ in range(2)])
    got, want = check_batch(srcs, tgts, Rs, ts, 10.0, Ks=(None, 5))
    assert want["count"].tolist() == [60] * 50 + [90] * 7


def test_source_cloud_outside_the_target_box():
    rng = np.random.default_rng(6)
    tgt = rng.uniform(-1, 1, size=(500, 3)).astype(np.float32)
    src = rng.uniform(-1, 1, size=(300, 3)).astype(np.float32)
    eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    srcs = [src + np.float32(5), src - np.float32(5), src + np.array([0, 0, 2.5], np.float32), src]
    got, want = check_batch(srcs, [tgt] * 4, [eye] * 4, [zero] * 4, 0.2)
    assert want["n_hit"][:3].tolist() == [0, 0, 0] and want["n_hit"][3] > 100 and len(want["corr"]) == want["corr_offset"][3]


def test_capacity_overflow_then_the_exact_repeat():
    from roitr_amd import pairgt
    rng = np.random.default_rng(7)
    parts = [random_pair(rng, 300, 400, noise=0.02) for _ in range(3)]
    srcs, tgts, Rs, ts = [list(x) for x in zip(*parts)]
    want = U.batch_brute(srcs, tgts, Rs, ts, 0.1, K=2)
    full = U.batch_brute(srcs, tgts, Rs, ts, 0.1)
    args = to_dev(srcs, tgts, Rs, ts)
    prepared = pairgt._inputs(*args)
    need = int(full["corr_offset"][-1])
    cap = int(full["corr_offset"][0]) + 5            # pair 0 fits, pair 1 does not fit as a whole, pair 2 lies beyond
    corr, off, rows, needed, status = pairgt.correspondences_once(*prepared[:6], 0.1, 2, cap, prepared[6], prepared[7])
    assert needed == need and rows == int(want["corr_offset"][-1]) and need > cap
    assert status.cpu().tolist() == [0, 4, 4] and np.array_equal(off.cpu().numpy(), want["corr_offset"])
    n0 = int(want["corr_offset"][0])
    assert np.array_equal(corr[:n0].cpu().numpy(), want["corr"][:n0])
    # the wrapper repeats once with the exact capacity
    check_batch(srcs, tgts, Rs, ts, 0.1, Ks=(None, 2), capacity=cap)
    corr, off, rows, needed, status = pairgt.correspondences_once(*prepared[:6], 0.1, None, need, prepared[6], prepared[7])
    assert status.cpu().tolist() == [0, 0, 0] and rows == need == needed and np.array_equal(corr.cpu().numpy(), full["corr"])


def test_status_pair_between_two_good_ones():
    rng = np.random.default_rng(8)
    parts = [random_pair(rng, 200, 260, noise=0.02) for _ in range(4)]
    srcs, tgts, Rs, ts = [list(x) for x in zip(*parts)]
    srcs[1] = srcs[1].copy(); srcs[1][17, 1] = np.nan
    tgts[2] = tgts[2].copy(); tgts[2][5, 0] = np.inf
    got, want = check_batch(srcs, tgts, Rs, ts, 0.08, Ks=(None, 3))
    assert want["status"].tolist() == [0, 1, 1, 0] and want["n_hit"][0] > 0 and want["n_hit"][3] > 0
    assert np.isnan(got.overlap_src.cpu().numpy()[1:3]).all() and np.isnan(got.overlap_tgt.cpu().numpy()[1:3]).all()
    assert (got.nn_idx.cpu().numpy()[200:600] == -1).all() and np.isinf(got.nn_dist2.cpu().numpy()[200:600]).all()
    assert (got.info.cpu().numpy()[1:3] == 0).all()
    bad_t = [t.copy() for t in ts]; bad_t[0][2] = np.nan
    got, want = check_batch(srcs, tgts, Rs, bad_t, 0.08)
    assert want["status"].tolist() == [1, 1, 1, 0]


def test_bitwise_repeat_and_slot_invariance():
    from roitr_amd import pairgt
    rng = np.random.default_rng(9)
    parts = [random_pair(rng, n, m, noise=0.02) for n, m in ((700, 900), (300, 200), (513, 640), (90, 1000))]
    pair = parts[2]
    alone = to_dev(*[[x] for x in pair])
    order_a, order_b = [parts[0], pair, parts[1], parts[3]], [parts[3], parts[1], parts[0], pair]

    def run(args):
        g = pairgt.pair_ground_truth(*args, 0.08)
        c, o = pairgt.radius_correspondences(*args, 0.08, K=4)
        return g, c, o

    def pair_view(res, args, slot):
        g, c, o = res
        so, to = [0] + args[1].cpu().tolist(), [0] + o.cpu().tolist()
        pt = slice(so[slot], so[slot + 1])
        return [g.count[pt], g.nn_idx[pt], g.nn_dist2[pt].view(torch.int64), g.n_src_hit[slot], g.n_tgt_hit[slot],
                g.overlap_src[slot].view(torch.int64), g.overlap_tgt[slot].view(torch.int64), g.info[slot].view(torch.int64),
                c[to[slot]:to[slot + 1]]]

    first, again = run(alone), run(alone)
    ref = pair_view(first, alone, 0)
    assert all(torch.equal(a, b) for a, b in zip(ref, pair_view(again, alone, 0)))
    assert int(ref[3]) > 100 and ref[8].shape[0] > 300
    for order, slot in ((order_a, 1), (order_b, 3)):
        args = to_dev(*[list(x) for x in zip(*order)])
        view = pair_view(run(args), args, slot)
        assert all(torch.equal(a, b) for a, b in zip(ref, view)), slot


def test_get_correspondences_equals_radius_correspondences():
    from roitr_amd import pairgt
    rng = np.random.default_rng(12)
    src, tgt, R, t = random_pair(rng, 800, 700, noise=0.02)
    T = np.eye(4); T[:3, :3], T[:3, 3] = R, t
    args = to_dev([src], [tgt], [R], [t])
    for K in (None, 2):
        corr, off = pairgt.radius_correspondences(*args, 0.0375, K=K)
        mine = pairgt.get_correspondences(src, tgt, T, 0.0375, K=K)
        assert mine.dtype == torch.int64 and mine.shape[1] == 2 and mine.shape[0] > 200
        assert torch.equal(mine, corr.long()) and int(off[0]) == mine.shape[0]
        assert torch.equal(pairgt.get_correspondences(args[0], args[2], torch.from_numpy(T), 0.0375, K=K), mine)


def test_pairgt_handle_equals_the_plain_call():
    from gpu_util import build_model, pair_to_device
    from roitr_amd import pairgt
    from roitr_amd.synthetic import make_pair
    model = build_model("3DMatch", weights="selective")
    raw = [make_pair(1024, config=1, pair_index=i, normals="field") for i in range(3)]
    pairs = [pair_to_device(p) for p in raw]
    with torch.no_grad():
        h = model.launch_batch(pairs, want_gt=True)
        model.finish_batch(h)
    got = pairgt.pairgt_handle(h, 0.0375)
    args = to_dev([p["src_points"] for p in raw], [p["tgt_points"] for p in raw], [p["rot"] for p in raw], [p["trans"] for p in raw])
    want = pairgt.pair_ground_truth(*args, 0.0375)
    assert int(want.n_src_hit.min()) > 0
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
