"""GPU: scene.register_scene on four rigid copies of one 1024-point cloud with all six pairs: bit for bit the four calls made by hand
(match, lgr_handle, edge_information, pose_graph_batch), and independent of pairs_per_call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_util import build_model  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("poses", "pair_T", "inliers", "info", "uncertain", "init_poses", "line_weight", "pruned", "steps", "solves", "status", "objective",
        "lambda_out")


def test_register_scene_equals_the_calls_by_hand_and_ignores_pairs_per_call():
    import torch
    from roitr_amd import posegraph as PG, scene as S
    from roitr_amd.lgr import lgr_handle
    model = build_model("3DMatch", weights="selective")
    clouds, planted = S.rigid_copies(S.synthetic_scene(2, 1024)[1], 4, seed=3)
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    enc = model.encode_clouds(clouds)
    res = S.register_scene(model, enc, pairs, iterations=30)
    # by hand: one match call, then the three operators
    handle = model.launch_match(enc, pairs)
    model.finish_batch(handle)
    out = handle["out"]
    r = lgr_handle(handle, radius=0.1, min_rows=3, steps=5)
    e = PG.edge_information(out["pair_starts"], out["out_src_pts"], out["out_tgt_pts"], r["T"], radius=0.1)
    unc = torch.tensor([0 if j - i == 1 else 1 for i, j in pairs], dtype=torch.int32, device="cuda")
    init = torch.from_numpy(S.spanning_poses(4, pairs, r["T"].cpu().numpy(), r["inliers"].cpu().numpy())).float().cuda()
    mu = float(PG.line_process_weight(e["info"], unc, 0.05, 1.0))
    pg = PG.pose_graph_batch([0, 4], [0, 6], [p[0] for p in pairs], [p[1] for p in pairs], r["T"], e["info"], unc, init, mu=mu, iterations=30)
    hand = dict(pg, pair_T=r["T"], inliers=r["inliers"], info=e["info"], uncertain=unc, init_poses=init)
    inl, st = res["inliers"].cpu().numpy(), int(res["status"][0])
    X = res["poses"].cpu().numpy().astype(np.float64)
    true = np.stack([np.linalg.inv(planted[j]) @ planted[i] for i, j in pairs])
    X0 = res["init_poses"].cpu().numpy().astype(np.float64)
    for name, T in (("pair poses", res["pair_T"].cpu().numpy().astype(np.float64)),
                    ("spanning tree", np.stack([np.linalg.inv(X0[j]) @ X0[i] for i, j in pairs])),
                    ("scene poses", np.stack([np.linalg.inv(X[j]) @ X[i] for i, j in pairs]))):
        rre, rte = S.pose_errors(T, true)
        print(name, "RRE (deg)", np.round(rre, 3), "RTE", np.round(rte, 4))
        # the fragments are exact rigid copies: every stage must register every pair by the benchmark's own criterion (15 deg, 0.3 m);
        # a tree walked the wrong way round or poses in the wrong frame miss it by the planted 34 deg
        assert (rre < 15.0).all() and (rte < 0.3).all(), name
    print("inliers", inl, "mu", mu, "status", st, "steps", int(res["steps"][0]), "solves", int(res["solves"][0]),
          "line weights", res["line_weight"].cpu().numpy())
    assert res["mu"] == mu and (inl > 0).all() and not st & (PG.ONE_NODE | PG.NO_EDGES | PG.BAD_EDGE | PG.BAD_COUNTS)
    for k in KEYS:
        assert res[k].dtype == hand[k].dtype and torch.equal(res[k], hand[k]), k
    for per_call in (1, 4):
        other = S.register_scene(model, enc, pairs, iterations=30, pairs_per_call=per_call)
        for k in KEYS:
            assert torch.equal(res[k], other[k]), (per_call, k)
