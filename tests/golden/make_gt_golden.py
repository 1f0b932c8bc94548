"""Writes tests/golden/gt_ref.npz: what the REFERENCE's lib/utils.py get_node_correspondences and get_node_occlusion_score return
(fp32 torch on the CPU) on three small seeded cases of tests/gt_util.py:

  0  n_t = 40, n_s = 37 nodes, random rotation
  1  masked-out nodes and short patches (1, 17, 63 valid points)
  2  clouds 10 m apart: an empty correspondence list

Per case the inputs (`<i>.<key>` for every key of the pair dict) and `<i>.corr_indices`, `<i>.corr_overlaps`, `<i>.occ_tgt`,
`<i>.occ_src`, plus `<i>.dist_tgt` / `<i>.dist_src`: the nearest distances of the padded clouds through the reference's own knnquery
wrapper (whose native half is oracle/pointops_ref.c here, see make_golden.py).  The reference is imported with the stubs of
make_golden.py; nothing of it is modified.  tests/test_gt_cpu.py pins the float64 restatement to these values.

    python tests/golden/make_gt_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402  (install_stubs, the reference's location)
import gt_util as U  # noqa: E402


def cases():
    a = U.random_pair(301, 40, 37)
    b = U.random_pair(302, 12, 11, per_node=110)
    b["tgt_node_mask"][[1, 7]] = False
    b["src_node_mask"][[0, 4, 9]] = False
    U.shorten_patches(b)
    c = U.lattice_pair(303, 9, 14, src_shift=10.0)
    return [a, b, c]


def main():
    make_golden.install_stubs()
    from lib import utils as LU
    from cpp_wrappers.pointops.functions.pointops import knnquery
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x))   # noqa: E731
    out = {}
    for i, p in enumerate(cases()):
        src_pad = torch.cat([tt(p["src_points"]), torch.zeros(1, 3)], 0)
        tgt_pad = torch.cat([tt(p["tgt_points"]), torch.zeros(1, 3)], 0)
        ki = {s: tt(p[s + "_knn_idx"].astype(np.int64)) for s in ("tgt", "src")}
        km = {s: tt(p[s + "_knn_mask"]) for s in ("tgt", "src")}
        nm = {s: tt(p[s + "_node_mask"]) for s in ("tgt", "src")}
        rot, trans = tt(p["rot"]), tt(p["trans"].reshape(3, 1))
        with torch.no_grad():
            ci, co = LU.get_node_correspondences(tt(p["tgt_nodes"]), tt(p["src_nodes"]), LU.index_select(tgt_pad, ki["tgt"], 0),
                                                 LU.index_select(src_pad, ki["src"], 0), rot, trans, U.POS_RADIUS,
                                                 ref_masks=nm["tgt"], src_masks=nm["src"], ref_knn_masks=km["tgt"], src_knn_masks=km["src"])
            o_ref, o_src = LU.get_node_occlusion_score(ki["tgt"], ki["src"], tgt_pad, src_pad, rot, trans, ref_masks=nm["tgt"],
                                                       src_masks=nm["src"], ref_knn_masks=km["tgt"], src_knn_masks=km["src"],
                                                       overlap_thres=U.OCC_THR)
            moved = torch.matmul(src_pad, rot.T) + trans.T
            o_t, o_s = torch.tensor([tgt_pad.shape[0]], dtype=torch.int32), torch.tensor([moved.shape[0]], dtype=torch.int32)
            _, d_tgt = knnquery(1, moved, tgt_pad, o_s, o_t)
            _, d_src = knnquery(1, tgt_pad, moved, o_t, o_s)
        for k, v in p.items():
            out[f"{i}.{k}"] = v
        out[f"{i}.corr_indices"], out[f"{i}.corr_overlaps"] = ci.numpy().astype(np.int32), co.numpy()
        out[f"{i}.occ_tgt"], out[f"{i}.occ_src"] = o_ref.numpy(), o_src.numpy()
        out[f"{i}.dist_tgt"], out[f"{i}.dist_src"] = d_tgt.numpy().reshape(-1), d_src.numpy().reshape(-1)
        print(f"case {i}: nodes {p['tgt_nodes'].shape[0]} x {p['src_nodes'].shape[0]}, listed {ci.shape[0]}, "
              f"occ tgt mean {float(o_ref.mean()):.3f} src mean {float(o_src.mean()):.3f}")
    path = os.path.join(HERE, "gt_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f kB" % (os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
