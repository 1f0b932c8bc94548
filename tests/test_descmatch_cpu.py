"""CPU: the ground the descriptor-matching GPU tests stand on -- the float64 restatement (tests/descmatch_util.py) against what the
reference's matching_descriptors / mutual_selection / get_inlier_ratio computed (tests/golden/descmatch_ref.npz), the torch-only
mutual_selection against the same file, and the new ABI."""
import os

import numpy as np
import torch

import descmatch_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "descmatch_ref.npz"))


def case(seed):
    return U.make_case(seed, 64, scale="unit" if seed % 2 == 0 else "x2")


def test_library_exports_the_descriptor_matching_symbols():
    import ctypes
    import __graft_entry__ as G
    from roitr_amd import _lib, descmatch
    lib = _lib.lib()
    names = G.declared_symbols()
    for n in ("roitr_desc_match_workspace_bytes", "roitr_desc_match_batch", "roitr_desc_match_select"):
        assert n in names and hasattr(lib, n), n
    lib.roitr_desc_match_workspace_bytes.restype = ctypes.c_size_t
    assert lib.roitr_desc_match_workspace_bytes(64, 5000 * 64, 5000 * 64) >= 2 * 5000 * 64 * 8
    assert lib.roitr_abi_version() == 4   # functions added, no struct changed
    assert descmatch.METRICS == {"dot": 0, "sqdist": 1} and descmatch.MODES == {"row": 0, "col": 1, "mutual": 2}


def test_float64_restatement_reproduces_the_reference():
    g = golden()
    for seed in range(6):
        c = case(seed)
        assert U.checksum(c) == str(g[f"checksum_{seed}"]), seed   # the regenerated inputs are the ones the reference saw
        s, t = c["src_desc"], c["tgt_desc"]
        for metric in (0, 1):   # the golden's cases are decided: exact comparison is meaningful
            u_row, u_col = U.undecided(U.scores_f64(s, t, metric), metric, *U.bounds(s, t, metric))
            assert u_row.sum() == 0 and u_col.sum() == 0, (seed, metric)
        d = U.match_f64(s, t, 1)
        for name, mode in (("row", "row"), ("col", "col"), ("union", "union"), ("mutual", "mutual")):
            assert np.array_equal(U.select(d["row_idx"], d["col_idx"], mode), g[f"md_{name}_{seed}"]), (seed, name)
        m = U.match_f64(s, t, 0)
        assert np.array_equal(U.select(m["row_idx"], m["col_idx"], "mutual"), g[f"ms_{seed}"]), seed
        ir = U.inlier_ratio_f64(c, 0.1)
        for k in ("wo", "w"):
            assert abs(ir[k][1] - float(g[f"ir_{k}_{seed}"])) <= 1e-6, (seed, k)
            assert ir[k][0].shape == g[f"dist_{k}_{seed}"].shape and np.abs(ir[k][0] - g[f"dist_{k}_{seed}"]).max() < 1e-4
        n_mutual = len(g[f"md_mutual_{seed}"])
        assert 190 <= n_mutual <= 240, n_mutual


def test_torch_mutual_selection_matches_the_reference():
    from roitr_amd.descmatch import mutual_selection
    g = golden()
    for seed in range(6):
        c = case(seed)
        sc = torch.from_numpy(c["src_desc"]) @ torch.from_numpy(c["tgt_desc"]).T
        for arg in (sc, sc.numpy(), sc[None]):
            sel = mutual_selection(arg)
            assert isinstance(sel, np.ndarray) and sel.dtype == np.bool_ and sel.shape == (1,) + tuple(sc.shape)
            assert np.array_equal(np.stack(np.nonzero(sel[0]), 1), g[f"ms_{seed}"]), seed
    ties = mutual_selection(np.zeros((3, 4), np.float32))   # the first maximum of every row and column: (0, 0) alone
    assert ties.sum() == 1 and ties[0, 0, 0]


def test_tie_rule_of_restatement_and_torch_mutual_selection_agree():
    """The hand-made tie case the GPU tests' restatement stands on, and the same case through descmatch.mutual_selection."""
    from roitr_amd.descmatch import mutual_selection
    s = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]], np.float32)
    t = np.array([[0, 1, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]], np.float32)
    for metric in (0, 1):
        r = U.match_f64(s, t, metric)
        assert list(r["row_idx"]) == [1, 1, 0] and list(r["col_idx"]) == [2, 0, 0]
        assert U.select(r["row_idx"], r["col_idx"], "mutual").tolist() == [[0, 1], [2, 0]]
        sel = mutual_selection(r["score"] if metric == 0 else -r["score"])[0]
        assert np.stack(np.nonzero(sel), 1).tolist() == [[0, 1], [2, 0]]
        assert U.select(r["row_idx"], r["col_idx"], "union").tolist() == [[0, 1], [0, 2], [1, 1], [2, 0]]
    e = U.match_f64(np.zeros((0, 4), np.float32), t, 0)
    assert len(e["row_idx"]) == 0 and list(e["col_idx"]) == [-1, -1, -1]
    assert U.select(e["row_idx"], e["col_idx"], "col").shape == (0, 2)


def test_descmatch_entry_points_refuse_host_tensors():
    import pytest
    from roitr_amd import _lib, descmatch
    z, o = torch.zeros(8, 8), torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(_lib.RoitrError):
        descmatch.match_batch(o, z, o, z)
    with pytest.raises(_lib.RoitrError):
        descmatch.select(o, o, torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32))
