"""Writes tests/golden/nfmr_ref.npz: what the REFERENCE's registration/evaluate_fdmatch.py computes on the seeded cases of
tests/nfmr_util.py (seeds 0-5, distinct anchors: with repeated anchors np.argpartition's choice among equal distances is
implementation-defined and the reference's recall differs from any fixed tie rule by a few points per case).

Per seed: `recall_<s>` (compute_nrfmr), `flow_<s>` / `mask_<s>` (blend_anchor_motion on the metric points, the float64 restatement's
anchors and their motions, as float32) and `checksum_<s>` of the generated inputs -- the inputs themselves are regenerated from the
seed by the tests.  The reference is imported with the stubs of make_golden.py (open3d, pointops_cuda); nothing of it is modified.

    python tests/golden/make_nfmr_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402  (install_stubs, the reference's location)
import nfmr_util as U  # noqa: E402


def main():
    make_golden.install_stubs()
    os.chdir(make_golden.REF)            # evaluate_fdmatch.py appends the working directory to sys.path for `lib`
    from registration.evaluate_fdmatch import blend_anchor_motion, compute_nrfmr
    out = {}
    for seed in range(6):
        case = U.make_case(seed, True)
        data = dict(src_raw_pcd=torch.from_numpy(case["src_raw"]), src_pcd=torch.from_numpy(case["src_deformed"]),
                    tgt_pcd=torch.zeros(1, 3), src_corr_pts=torch.from_numpy(case["src_corr"]),
                    tgt_corr_pts=torch.from_numpy(case["tgt_corr"]), metric_index_list=torch.from_numpy(case["metric_index"]),
                    rot=torch.from_numpy(case["rot"]), trans=torch.from_numpy(case["trans"]).reshape(3, 1))
        recall = float(compute_nrfmr(data, recall_thr=U.THR))
        f64 = U.nfmr_f64(case)
        anchor = case["src_raw"][f64["anchor_idx"]]
        flow, mask = blend_anchor_motion(case["src_raw"][case["metric_index"]], anchor, case["tgt_corr"] - anchor, knn=3,
                                         search_radius=U.RADIUS)
        differing = abs(round(recall * 600) - f64["hits"])
        print(f"seed {seed}: reference recall {recall:.6f}, float64 restatement {f64['nfmr']:.6f} ({differing} of 600 differ), "
              f"ambiguous {int(U.ambiguous(case, f64).sum())}")
        out[f"recall_{seed}"] = np.float64(recall)
        out[f"flow_{seed}"] = np.asarray(flow, np.float32)
        out[f"mask_{seed}"] = np.asarray(mask, bool)
        out[f"checksum_{seed}"] = np.array(U.checksum(case))
    np.savez_compressed(os.path.join(HERE, "nfmr_ref.npz"), **out)


if __name__ == "__main__":
    main()
