"""CPU: the float64 restatement of the ground-truth side outputs (tests/gt_util.py) is pinned to what the reference's own
get_node_correspondences / get_node_occlusion_score returned (tests/golden/gt_ref.npz, written by tests/golden/make_gt_golden.py), and
the seeded inputs of tests/test_gt_gpu.py satisfy the conditions under which those tests prove anything: nothing undecided on the
lattice inputs, at most 5 % undecided on the random ones."""
import os

import numpy as np
import pytest

import gt_util as U

HERE = os.path.dirname(os.path.abspath(__file__))
PAIR_KEYS = ("points", "nodes", "knn_idx", "knn_mask", "node_mask")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "gt_ref.npz"))


def _case(g, i):
    p = {f"{s}_{k}": g[f"{i}.{s}_{k}"] for s in ("tgt", "src") for k in PAIR_KEYS}
    p["rot"], p["trans"] = g[f"{i}.rot"], g[f"{i}.trans"]
    return p


@pytest.mark.parametrize("i", [0, 1, 2])
def test_reference_values_lie_inside_the_intervals(golden, i):
    p = _case(golden, i)
    civ, oiv = U.corr_intervals(p), U.occ_intervals(p)
    print(f"case {i}: band {civ['band']:.3e} (r^2 = {U.POS_RADIUS ** 2:.3e}), {oiv['band']:.3e} (thr^2 = {U.OCC_THR ** 2:.3e}); "
          f"undecided shares {U.undecided_shares(civ, oiv)}")
    U.check_corr(golden[f"{i}.corr_indices"], golden[f"{i}.corr_overlaps"], civ, f"case {i}")
    U.check_occ(golden[f"{i}.occ_tgt"], oiv, "tgt", f"case {i}")
    U.check_occ(golden[f"{i}.occ_src"], oiv, "src", f"case {i}")
    # the recorded kNN(1) distances of the padded clouds (pad rows included on both sides) against the brute-force float64 ones
    for side in ("tgt", "src"):
        got2, want2 = golden[f"{i}.dist_{side}"].astype(np.float64) ** 2, oiv[side + "_d2"]
        assert got2.shape == want2.shape
        assert np.all(np.abs(got2 - want2) <= oiv["band"] + 4 * np.spacing(want2.astype(np.float32)).astype(np.float64)), side
    if i == 0:
        assert civ["lo"].shape == (40, 37) and golden["0.corr_indices"].shape[0] > 100
    if i == 1:
        assert (~p["tgt_node_mask"]).sum() == 2 and (~p["src_node_mask"]).sum() == 3
        assert sorted(set(p["tgt_knn_mask"].sum(1)) & {1, 17, 63}) == [1, 17, 63]
        unmasked = U.corr_intervals(dict(p, tgt_node_mask=np.ones(12, bool), src_node_mask=np.ones(11, bool)))
        assert ((unmasked["lo"] > 0) & ~civ["live"]).sum() > 0      # the masks hide node pairs that do overlap
    if i == 2:
        assert golden["2.corr_indices"].shape[0] == 0 and (civ["hi"] == 0).all()


def _lattice_batches():
    yield "lattice", U.lattice_batch(), [True] * 3
    yield "ball", U.ball_batch(), [True] * 4
    for name in U.EDGES:
        pairs, exact = U.edge_batch(name)
        yield name, pairs, exact


def test_lattice_inputs_are_exact_in_fp32_and_have_nothing_undecided():
    for name, pairs, exact in _lattice_batches():
        for b, (p, ex) in enumerate(zip(pairs, exact)):
            civ, oiv = U.corr_intervals(p), U.occ_intervals(p)
            if not ex:
                continue
            assert U.is_exact(p) and civ["band"] == 0.0 and oiv["band"] == 0.0, (name, b)
            # no squared distance of the lattice comes closer to a threshold than 0.1 lattice steps
            for thr2 in (U.POS_RADIUS ** 2, U.OCC_THR ** 2):
                assert abs(thr2 / U.STEP ** 2 - round(thr2 / U.STEP ** 2)) > 0.1
            assert civ["undecided_point_pairs"] == 0 and U.undecided_shares(civ, oiv) == (0.0, 0.0), (name, b)
            assert np.array_equal(civ["lo"], civ["hi"]) and np.array_equal(oiv["tgt_lo"], oiv["tgt_hi"])


def test_random_inputs_leave_at_most_five_percent_undecided():
    total = np.zeros(4, np.int64)
    for b, p in enumerate(U.random_batch()):
        civ, oiv = U.corr_intervals(p), U.occ_intervals(p)
        may, must, und, nodes = U.undecided_counts(civ, oiv)
        print(f"random pair {b}: band {civ['band']:.3e}, undecided node pairs {may} of {must} listed, undecided scores {und} of {nodes} nodes")
        assert must >= 10, b      # the pair has something to list
        assert may <= 0.05 * must and und <= 0.05 * nodes, (b, may, must, und, nodes)
        total += (may, must, und, nodes)
    assert total[0] <= 0.05 * total[1] and total[2] <= 0.05 * total[3], total.tolist()


def test_the_edge_inputs_contain_their_edge():
    (p,), _ = U.edge_batch("node_masks")
    civ = U.corr_intervals(p)
    unmasked = U.corr_intervals(dict(p, tgt_node_mask=np.ones(12, bool), src_node_mask=np.ones(11, bool)))
    assert ((unmasked["lo"] > 0) & ~civ["live"]).sum() > 0
    (p,), _ = U.edge_batch("short_patches")
    for side in ("tgt", "src"):
        assert {1, 17, 63} <= set(p[side + "_knn_mask"].sum(1).tolist())
        assert (p[side + "_knn_idx"][~p[side + "_knn_mask"]] == p[side + "_points"].shape[0]).all()
    # pad_row: the transformed source pad row alone makes target points visible, and pad slots taken as valid would add hits
    (p,), _ = U.edge_batch("pad_row")
    oiv, civ = U.occ_intervals(p), U.corr_intervals(p)
    near_pad = ((U.f64(p["tgt_points"]) - U.f64(p["trans"])) ** 2).sum(1) < U.POS_RADIUS ** 2 / 4
    real = U._nearest_d2(U.f64(p["tgt_points"])[near_pad], U.f64(p["src_points"]) @ U.f64(p["rot"]).T + U.f64(p["trans"]))
    assert near_pad.sum() > 0 and (real > U.OCC_THR ** 2).any() and (oiv["tgt_d2"][:-1][near_pad] < U.OCC_THR ** 2).all()
    assert (U.f64(p["tgt_points"]) ** 2).sum(1).min() > 0.25           # an untransformed zero row is far from every target point
    as_valid = U.corr_intervals(dict(p, src_knn_mask=np.ones_like(p["src_knn_mask"])))
    assert not np.array_equal(as_valid["lo"], civ["lo"])
    pairs, _ = U.edge_batch("far_pair")
    assert (U.corr_intervals(pairs[1])["hi"] == 0).all() and (U.corr_intervals(pairs[0])["lo"] > 0).any()
    assert (U.occ_intervals(pairs[1])["tgt_hi"] == 0).all()
    (p,), _ = U.edge_batch("sphere_zero")
    assert U.sphere_pass_zero_overlap(p, U.corr_intervals(p)).sum() >= 5
    survivors = 0
    for p, steps in zip(U.ball_batch(), U.BALL_STEPS):
        civ = U.corr_intervals(p)
        survivors += int(U.sphere_pass(p).sum())
        assert civ["lo"].shape == (70, 70) and p["tgt_node_mask"].all()
        if steps == 6:
            assert (civ["lo"] == 1.0).all()
        else:       # neighbouring node pairs differ: many distinct values, zeros among them
            assert np.unique(civ["lo"]).size > 50 and (civ["lo"] == 0).any() and (civ["lo"] == 1.0).any()
    print("ball batch: node pairs that pass the sphere test by 1e-4:", survivors)
    assert survivors > 16384
