"""Writes tests/golden/loss_ref.npz: what the REFERENCE's lib/loss.py OverallLoss computes (fp32 torch on the CPU) on the six seeded
cases of tests/loss_util.py.

Per case: `c_loss_<i>`, `f_loss_<i>`, `f_count_<i>` (the number of labels, from the reference's own square_distance in fp32) and
`checksum_<i>` of the generated inputs -- the inputs themselves are regenerated from the seed by the tests.  The reference is imported
with the stubs of make_golden.py (open3d, pointops_cuda); nothing of it is modified.  The script also prints the figures
tests/loss_util.py records: the relative deviation of the reference's fp32 values from the float64 restatement, and the share of
source points the decided-case rule masks.

    python tests/golden/make_loss_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402  (install_stubs, the reference's location)
import loss_util as U  # noqa: E402


class Cfg(dict):
    __getattr__ = dict.__getitem__


def main():
    make_golden.install_stubs()
    from lib.loss import OverallLoss
    from lib.utils import square_distance
    cfg = Cfg(coarse_loss_positive_margin=0.1, coarse_loss_negative_margin=1.4, coarse_loss_positive_optimal=0.1,
              coarse_loss_negative_optimal=1.4, coarse_loss_log_scale=24, coarse_loss_positive_overlap=0.1, coarse_loss_weight=1.0,
              fine_loss_positive_radius=U.RADIUS, fine_loss_weight=1.0, occ_loss_weight=0.0)
    loss_fn = OverallLoss(cfg)
    out, worst = {}, 0.0
    for i, raw in enumerate(U.golden_cases()):
        case = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in raw.items()}
        output_dict = dict(tgt_node_feats=case["tgt_feats"], src_node_feats=case["src_feats"], gt_node_corr_indices=case["gt_idx"],
                           gt_node_corr_overlaps=case["gt_overlaps"], tgt_node_corr_knn_points=case["tgt_pts"],
                           src_node_corr_knn_points=case["src_pts"], tgt_node_corr_knn_masks=case["tgt_masks"],
                           src_node_corr_knn_masks=case["src_masks"], matching_scores=case["scores"])
        data_dict = dict(rot=case["rot"][None], trans=case["trans"].reshape(1, 3, 1))
        with torch.no_grad():
            r = loss_fn(output_dict, data_dict)
            moved = torch.matmul(case["src_pts"], case["rot"].T) + case["trans"].reshape(1, 1, 3)
            gt = torch.lt(square_distance(case["tgt_pts"], moved), U.RADIUS ** 2) & case["tgt_masks"][:, :, None] & case["src_masks"][:, None, :]
            n_labels = int(gt.sum() + ((gt.sum(2) == 0) & case["tgt_masks"]).sum() + ((gt.sum(1) == 0) & case["src_masks"]).sum())
        c64, f64 = U.coarse_f64(raw), U.fine_f64(raw)
        undecided = dict(raw, src_masks=U.make_case(i, *U.GOLDEN_SIZES[i], decided=False)["src_masks"])
        share = U.decide(undecided)
        dev_c, dev_f = U.rel(r["c_loss"], c64["loss"]), U.rel(r["f_loss"], f64["loss"])
        worst = max(worst, dev_c, dev_f)
        print(f"case {i}: c_loss {float(r['c_loss']):.7f} (float64 {c64['loss']:.9f}, rel {dev_c:.2e})  f_loss {float(r['f_loss']):.7f} "
              f"(float64 {f64['loss']:.9f}, rel {dev_f:.2e})  labels {n_labels} (float64 {f64['count']})  masked share {share:.4f}  "
              f"E {U.fine_error_bound(raw):.2e}")
        assert n_labels == f64["count"], i
        out[f"c_loss_{i}"] = np.float32(r["c_loss"])
        out[f"f_loss_{i}"] = np.float32(r["f_loss"])
        out[f"f_count_{i}"] = np.int64(n_labels)
        out[f"checksum_{i}"] = np.array(U.checksum(raw))
    print(f"largest relative deviation of the reference's fp32 from float64: {worst:.3e}; 8 x = {8 * worst:.3e}")
    np.savez_compressed(os.path.join(HERE, "loss_ref.npz"), **out)


if __name__ == "__main__":
    main()
