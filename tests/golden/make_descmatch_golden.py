"""Writes tests/golden/descmatch_ref.npz: what the REFERENCE's lib/utils.py matching_descriptors (all four mode combinations) and
registration/benchmark_utils.py mutual_selection / get_inlier_ratio compute on the seeded cases of tests/descmatch_util.py
(seeds 0-5, N = 333, M = 301, D = 64; even seeds unit-normalised, odd seeds scaled by 2).

Per seed: `md_row_<s>`, `md_col_<s>`, `md_union_<s>`, `md_mutual_<s>` (the (n, 2) correspondences), `ms_<s>` (np.nonzero of
mutual_selection(src @ tgt^T), as (k, 2)), `ir_wo_<s>` / `ir_w_<s>` / `dist_wo_<s>` / `dist_w_<s>` (get_inlier_ratio) and
`checksum_<s>` of the generated inputs -- the inputs themselves are regenerated from the seed by the tests.  The script prints the
number of undecided rows and columns of every case (descmatch_util's rule): the committed seeds show 0, so index sets are compared
exactly.  The reference is imported with the stubs of make_golden.py; nothing of it is modified (np.bool, which it uses and
current numpy has dropped, is aliased here before the import).

    python tests/golden/make_descmatch_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402  (install_stubs, the reference's location)
import descmatch_util as U  # noqa: E402


def scale_of(seed):
    return "unit" if seed % 2 == 0 else "x2"


def main():
    make_golden.install_stubs()
    if not hasattr(np, "bool"):
        np.bool = bool
    for name in ("nibabel", "nibabel.quaternions"):   # registration/benchmark.py imports it for a function that is not called here
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    os.chdir(make_golden.REF)
    sys.path.insert(0, make_golden.REF)
    from lib.utils import matching_descriptors
    from registration.benchmark_utils import get_inlier_ratio, mutual_selection
    out = {}
    for seed in range(6):
        c = U.make_case(seed, 64, scale=scale_of(seed))
        s, t = c["src_desc"], c["tgt_desc"]
        for metric in (0, 1):
            sc = U.scores_f64(s, t, metric)
            u_row, u_col = U.undecided(sc, metric, *U.bounds(s, t, metric))
            print(f"seed {seed} metric {metric}: undecided rows {int(u_row.sum())}, columns {int(u_col.sum())}")
        out[f"md_row_{seed}"] = np.asarray(matching_descriptors(s, t, mutual=False, major="row"), np.int64)
        out[f"md_col_{seed}"] = np.asarray(matching_descriptors(s, t, mutual=False, major="col"), np.int64)
        out[f"md_union_{seed}"] = np.asarray(matching_descriptors(s, t, mutual=False, major=None), np.int64)
        out[f"md_mutual_{seed}"] = np.asarray(matching_descriptors(s, t, mutual=True), np.int64)
        sel = mutual_selection(torch.from_numpy(s) @ torch.from_numpy(t).T)[0]
        out[f"ms_{seed}"] = np.stack(np.nonzero(sel), 1).astype(np.int64)
        r = get_inlier_ratio(c["src_pcd"], c["tgt_pcd"], s, t, c["rot"], c["trans"], inlier_distance_threshold=0.1)
        for k in ("wo", "w"):
            out[f"ir_{k}_{seed}"] = np.float64(float(r[k]["inlier_ratio"]))
            out[f"dist_{k}_{seed}"] = np.asarray(r[k]["distance"], np.float32)
        print(f"seed {seed}: mutual {len(out[f'md_mutual_{seed}'])}, union {len(out[f'md_union_{seed}'])}, "
              f"IR wo {float(r['wo']['inlier_ratio']):.4f} w {float(r['w']['inlier_ratio']):.4f}")
        out[f"checksum_{seed}"] = np.array(U.checksum(c))
    np.savez_compressed(os.path.join(HERE, "descmatch_ref.npz"), **out)


if __name__ == "__main__":
    main()
