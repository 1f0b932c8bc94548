"""Test-mode harness: the loop of lib/tester.py:19-69 (reference) on the MI355X engine.

Per pair it writes `{snapshot_dir}/{benchmark}/{idx}.pth` with exactly the keys the reference's tester saves
(lib/tester.py:56-69) so that registration/evaluate_registration_c2f.py can consume the files unchanged.
Differences by design: pairs are sharded over ranks by their GLOBAL index (pair i -> rank i mod W, the file name
keeps the global index -- the reference's DDP test mode would overwrite files), several
pairs go through the engine per forward (`pairs_per_forward`), and checkpoints load through the same
'module.'-stripping rule as lib/trainer.py:94-130.  At the end of the run ONE collective (shard.gather_result_records:
a gather of the per-pair records {pair id, #correspondences, IR, PIR, match scores}, packed into one fixed-size block per
rank, over RCCL) brings every rank's results to rank 0; `Tester.records` holds them there.  `test()` returns the per-rank
correspondence counts on rank 0 and None on every other rank (only rank 0 receives the records).
Every optional evaluation is a Stage (below); ONE more collective (merge_rows) merges their per-pair rows, and rank 0 reports from them once.
"""
import functools
import os

import torch

from . import _args as A
from .shard import assemble_block, gather_result_records, pairs_for_rank, slots_per_rank


DESC_INLIER_THRESHOLD = 0.1   # registration/benchmark_utils.py:80 get_inlier_ratio's default, whatever eval_acceptance_radius says
DESC_FMR_THRESHOLD = 0.05   # registration/evaluate_registration_c2f.py:109: a pair counts when its inlier ratio exceeds it
RECALL_RMSE = 0.2            # registration/benchmark.py:217 evaluate_registration: a pair is registered when p <= 0.2 ** 2
OVERLAP_BINS = (("overlap_ge_0.3", 0.3, float("inf")), ("overlap_0.1_0.3", 0.1, 0.3), ("overlap_lt_0.1", float("-inf"), 0.1))
SUCCESS_RRE, SUCCESS_RTE = 15.0, 0.3   # the pose-error success rule of the registration and the FPFH report (degrees, metres)
NONRIGID_BENCHMARKS = ("4DMatch", "4DLoMatch")
FILE_OUTPUTS = (("src_nodes", "src_nodes"), ("tgt_nodes", "tgt_nodes"), ("src_node_desc", "src_node_feats"), ("tgt_node_desc", "tgt_node_feats"),
                ("src_point_desc", "src_point_feats"), ("tgt_point_desc", "tgt_point_feats"), ("src_corr_pts", "src_corr_points"), ("tgt_corr_pts",
                "tgt_corr_points"), ("confidence", "corr_scores"), ("gt_tgt_node_occ",) * 2, ("gt_src_node_occ",) * 2)   # lib/tester.py:59-67: file, output
REPORT_ORDER = ("val", "eval", "descriptor", "registration", "fpfh", "refinement", "recall", "gt", "nonrigid")   # of the printed lines


def _offsets(clouds, device):
    """The reference's `offset` of a list of clouds: their cumulative ends, int32 on the device."""
    return A.cumulative([c.shape[0] for c in clouds], device)[1:]


_column = lambda rows, col: [v[col] for v in rows.values() if v[col] == v[col]]   # one column of {pair id: row} without its nan entries
_mean = lambda x, empty=float("nan"): sum(x) / len(x) if x else empty


def load_pretrain(model, path):
    """lib/trainer.py:94-130 `_load_pretrain`: state['state_dict'], 'module.' prefixes stripped, strict load."""
    state = torch.load(path, map_location="cpu")
    sd = state["state_dict"] if "state_dict" in state else state
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    model.load_state_dict(sd, strict=True)
    return model


def merge_rows(local, world):
    """{stage name: {pair id: row}} of this rank -> the same over the pairs of ALL ranks, on every rank, rank by rank: the one collective
    of a run besides the record gather.  Every rank takes part; a rank without rows for a stage contributes an empty dict."""
    if world == 1:
        return local
    parts = [None] * world
    torch.distributed.all_gather_object(parts, local)
    return {name: {k: v for part in parts for k, v in part[name].items()} for name in local}


class Forward:
    """One forward for the stages: GLOBAL pair ids, dataset items, the engine's pairs, its handle and outputs, the estimator's result `reg`,
    the current pose on the host `est` (the refinement replaces it), `file`: the keys the stages add to the pair files, one value per pair."""

    def __init__(self, ids, items, pairs, handle):
        self.ids, self.items, self.pairs, self.handle = ids, items, pairs, handle
        self.outs, self.reg, self.est, self.file = None, None, None, {}

    @functools.cached_property
    def gt_pose(self):   # (rot (b,3,3), trans (b,3)) of the pairs, stacked once, when the first stage asks
        return torch.stack([p["rot"].reshape(3, 3) for p in self.pairs]), torch.stack([p["trans"].reshape(3) for p in self.pairs])


class Stage:
    """One optional evaluation.  Its options are its attributes (__init__ validates them); run(fw) makes its call for one Forward (importing
    its module there, so a run without the option never loads it) and files this rank's rows under the GLOBAL pair ids; attributes() is what
    the Tester shows of them under its own names.  Rank 0, on the rows of ALL ranks: metrics(rows, base) gives the keys for the Tester's
    `publishes` dict (base: IR / PIR), lines(rows, that dict) the printed lines per REPORT_ORDER slot, both pure; finish(rows) writes files."""
    name, publishes = None, "metrics"

    def __init__(self, **options):
        vars(self).update(options, rows={})

    attributes = lambda self: {self.name: self.rows}
    metrics = lambda self, rows, base: {}
    lines = lambda self, rows, metrics: {}
    finish = lambda self, rows: None


class Nonrigid(Stage):
    """With evaluate on the 4DMatch / 4DLoMatch benchmark and items that carry `metric_index`, the NFMR of every pair is computed on the
    device (nonrigid.nfmr_handle; `kw` holds its keyword arguments) and `Tester.nonrigid` maps this rank's pair ids to (NFMR, number of
    metric points); it stays None otherwise."""
    name = "nonrigid"

    def run(self, fw):
        if not all("metric_index" in it for it in fw.items):
            return
        from .nonrigid import nfmr_handle
        nf = nfmr_handle(fw.handle, [it["metric_index"] for it in fw.items], **self.kw)
        for idx, r, m in zip(fw.ids, nf["nfmr"].cpu().tolist(), nf["n_metric"].cpu().tolist()):
            self.rows[idx] = (float(r), int(m))

    attributes = lambda self: {"nonrigid": self.rows or None}

    def lines(self, rows, metrics):
        v = list(rows.values())
        return {} if not v else {"nonrigid": [
            f"[roitr_amd] 4DMatch non-rigid evaluation over {len(v)} pairs: NFMR {sum(r[0] for r in v) / len(v):.4f} (recall threshold 0.04 m, "
            f"{sum(r[1] for r in v)} metric points), IR {metrics['IR']:.4f} at {self.radius:g} m"]}


class Losses(Stage):
    """validate: the reference's `val` report (lib/trainer.py:335-344: OverallLoss and Evaluator per pair under no_grad); implies evaluate.
    loss.loss_batch computes the losses of every pair on the device (two batched kernels per forward): `Tester.losses` maps this rank's
    pair ids to (loss, c_loss, f_loss, o_loss), and on rank 0 `Tester.validation` holds their means, PIR and IR over the pairs of ALL ranks
    plus `skipped`: the reference's AverageMeter turns a whole mean into nan on one nan pair (a pair without fine labels, or without a row
    and a column that have both a positive and a negative); here such pairs are left out of that key's mean and counted per key."""
    name, publishes, KEYS = "losses", "validation", ("loss", "c_loss", "f_loss", "o_loss")

    def run(self, fw):
        from .loss import loss_batch
        total, c_loss, f_loss, _, _ = loss_batch(fw.handle, self.config)
        rows = torch.stack([total, c_loss, f_loss, 0.0 * f_loss], 1).cpu().tolist()   # o_loss = 0 * f_loss (lib/loss.py:165)
        for idx, row in zip(fw.ids, rows):
            self.rows[idx] = tuple(float(x) for x in row)

    def metrics(self, rows, base):
        out = {"PIR": base["PIR"], "IR": base["IR"], "pairs": len(rows), "skipped": {"PIR": base["pairs_without_coarse"], "IR": 0}}
        for col, key in enumerate(self.KEYS):
            vals = _column(rows, col)
            out[key] = _mean(vals)
            out["skipped"][key] = len(rows) - len(vals)
        return out

    def lines(self, rows, v):
        return {"val": ["[roitr_amd] val over %d pairs: " % v["pairs"] + "  ".join(f"{k} {v[k]:.4f}" for k in self.KEYS + ("PIR", "IR")),
                        "[roitr_amd] val: pairs left out of a mean because their value is nan: " + ", ".join(f"{k} {n}" for k, n in v["skipped"].items())]}


class Descriptor(Stage):
    """descriptor_eval (with evaluate): the descriptor-level evaluation of registration/benchmark_utils.py get_inlier_ratio on the point
    descriptors of every pair (descmatch.descriptor_handle, one fused matching launch per forward): `Tester.descriptor` maps this rank's
    pair ids to (IR without the mutual check, IR with it, number of mutual matches) and `metrics` gains desc_IR_wo (mean over pairs),
    desc_IR_w (mean over the pairs that have mutual matches: the IR of an empty set is nan, handled as PIR is) and desc_FMR (share of
    pairs with IR without the mutual check above 0.05, evaluate_registration_c2f.py:109), over the pairs of ALL ranks, like IR / PIR.
    The inlier distance is get_inlier_ratio's default, 0.1 m, not the config's eval_acceptance_radius."""
    name = "descriptor"

    def run(self, fw):
        from .descmatch import descriptor_handle
        d = descriptor_handle(fw.handle, "point", DESC_INLIER_THRESHOLD)
        for idx, wo, w, nw in zip(fw.ids, d["ir_wo"].cpu().tolist(), d["ir_w"].cpu().tolist(), d["n_w"].cpu().tolist()):
            self.rows[idx] = (float(wo), float(w), int(nw))

    def metrics(self, rows, base):
        wo = _column(rows, 0)
        return {"desc_IR_wo": _mean(wo, 0.0), "desc_IR_w": _mean(_column(rows, 1), 0.0),
                "desc_FMR": _mean([float(x > DESC_FMR_THRESHOLD) for x in wo], 0.0)}

    def lines(self, rows, m):
        return {} if not rows else {"descriptor": [
            f"[roitr_amd] descriptor matching over {len(rows)} pairs: IR without mutual check {m['desc_IR_wo']:.4f}, with {m['desc_IR_w']:.4f} "
            f"({sum(r[2] for r in rows.values())} mutual matches), FMR at {DESC_FMR_THRESHOLD:g} {m['desc_FMR']:.4f}"]}


class Pose(Stage):
    """register: every pair's pose is estimated on the device and saved as `est_transform` in its file.  estimator: "ransac" (registration.
    register_handle, keyed on the GLOBAL pair id, so the poses do not depend on sharding or pairs_per_forward), "lgr" (lgr.lgr_handle: local-
    to-global registration on the matcher's patches: no random stream, so no keys), "compat" (compat.compat_handle: spatial-compatibility
    registration: no random stream and no patch structure either) or "fgr" (fgr.fgr_handle: fast global registration, one robust objective
    and no hypotheses; its optional tuple test is keyed on the GLOBAL pair id like RANSAC); `ransac` / `lgr` / `compat` / `fgr` hold their keyword arguments, everything
    downstream of the pose is the same code.  refine (implies register): None, or ICP from reg["T"] on the clouds the model saw: "point" /
    "plane" (icp.icp_handle: point-to-point, or point-to-plane on the target normals) or "gicp" (gicp.gicp_handle: generalized, plane-to-
    plane on the normals of both clouds; each module is imported in its own mode only); `icp` holds the keyword arguments, `epsilon` among
    them for "gicp".  The refined transform takes the place of the estimated one everywhere downstream.  `Tester.refinement` maps this rank's
    pair ids to (rre_before, rte_before, rre_after, rte_after, fitness, rmse, steps), `Tester.refinement_status` to the ICP status word and,
    with errors (the Tester's evaluate), `Tester.registration` to (RRE degrees, RTE metres, inliers).  A row is (registration row or None,
    refinement row + (status,) or None)."""
    name = "pose"

    def __init__(self, estimator, ransac, lgr, compat, refine, icp, errors, fgr=None):
        if refine not in (None, "point", "plane", "gicp"):
            raise ValueError("refine must be None, 'point', 'plane' or 'gicp'")
        if estimator not in ("ransac", "lgr", "compat", "fgr"):
            raise ValueError("estimator must be 'ransac', 'lgr', 'compat' or 'fgr'")
        super().__init__(estimator=estimator, kw={"ransac": ransac, "lgr": lgr, "compat": compat, "fgr": dict(fgr or {})}[estimator],
                         refine=refine, icp=icp, errors=errors)

    def run(self, fw):
        from .registration import pose_errors, register_handle
        if self.estimator == "lgr":
            from .lgr import lgr_handle
            fw.reg = lgr_handle(fw.handle, **self.kw)
        elif self.estimator == "compat":
            from .compat import compat_handle
            fw.reg = compat_handle(fw.handle, **self.kw)
        elif self.estimator == "fgr":
            from .fgr import fgr_handle
            fw.reg = fgr_handle(fw.handle, pair_keys=fw.ids, **self.kw)
        else:
            fw.reg = register_handle(fw.handle, pair_keys=fw.ids, **self.kw)
        fw.est = fw.reg["T"].cpu()
        refined = registered = [None] * len(fw.ids)
        if self.refine is not None:
            gt_pose = fw.gt_pose
            if self.refine == "gicp":
                from .gicp import gicp_handle
                ref = gicp_handle(fw.handle, fw.reg["T"], **self.icp)
            else:
                from .icp import icp_handle
                ref = icp_handle(fw.handle, fw.reg["T"], plane=self.refine == "plane", **self.icp)
            before, fw.est = pose_errors(fw.est, *gt_pose), ref["T"].cpu()
            after = pose_errors(fw.est, *gt_pose)
            cols = [x.cpu().tolist() for x in (*before, *after, ref["fitness"], ref["rmse"], ref["steps"], ref["status"])]
            refined = [tuple(float(c[k]) for c in cols[:6]) + (int(cols[6][k]), int(cols[7][k])) for k in range(len(fw.ids))]
        if self.errors:
            rre, rte = pose_errors(fw.est, *fw.gt_pose)
            registered = [(float(a), float(b), int(c)) for a, b, c in zip(rre, rte, fw.reg["inliers"].cpu().tolist())]
        self.rows.update(zip(fw.ids, zip(registered, refined)))
        fw.file["est_transform"] = fw.est

    def attributes(self):
        part = lambda on, pick: {k: pick(v) for k, v in self.rows.items()} if on else None
        return {"registration": part(self.errors, lambda v: v[0]), "refinement": part(self.refine is not None, lambda v: v[1][:7]),
                "refinement_status": part(self.refine is not None, lambda v: v[1][7])}

    def lines(self, rows, metrics):
        """Mean / median RRE and RTE and the success share; the same before and after the refinement, mean steps, pairs per status bit."""
        import numpy as np
        out = {}
        if rows and self.errors:
            rre, rte = np.array([v[0][0] for v in rows.values()]), np.array([v[0][1] for v in rows.values()])
            out["registration"] = [
                f"[roitr_amd] registration ({self.estimator}) over {len(rows)} pairs: RRE mean {rre.mean():.3f} deg, median "
                f"{np.median(rre):.3f} deg; RTE mean {rte.mean():.4f} m, median {np.median(rte):.4f} m",
                f"[roitr_amd] pairs with RRE < 15 deg and RTE < 0.3 m: {float(np.mean((rre < SUCCESS_RRE) & (rte < SUCCESS_RTE))):.4f} (a pose-error success "
                "rate, not the 3DMatch-protocol registration recall, which needs the benchmark's gt.info)"]
        if rows and self.refine is not None:
            from . import icp
            a = np.array([v[1][:7] for v in rows.values()], dtype=np.float64)
            bits = ", ".join(f"{name} {sum(1 for v in rows.values() if v[1][7] & bit)}" for name, bit in
                             (("converged", icp.CONVERGED), ("too few", icp.TOO_FEW), ("singular", icp.SINGULAR), ("empty", icp.EMPTY),
                              ("non-finite", icp.NONFINITE)))
            label = "generalized, plane-to-plane" if self.refine == "gicp" else f"point-to-{self.refine}"
            out["refinement"] = [
                f"[roitr_amd] ICP refinement ({label}) over {len(rows)} pairs: RRE mean {a[:, 0].mean():.3f} -> {a[:, 2].mean():.3f} deg, "
                f"median {np.median(a[:, 0]):.3f} -> {np.median(a[:, 2]):.3f} deg; RTE mean {a[:, 1].mean():.4f} -> {a[:, 3].mean():.4f} m, "
                f"median {np.median(a[:, 1]):.4f} -> {np.median(a[:, 3]):.4f} m; mean steps {a[:, 6].mean():.1f}; pairs: {bits}"]
        return out


class Fpfh(Stage):
    """fpfh_baseline: None, or a dict (radius, max_nn, mutual; defaults 0.125, 100, True) that switches on the learning-free baseline
    (fpfh.fpfh_handle) with evaluate and register: FPFH descriptors of the clouds and normals the model was fed, matched under the
    squared distance, their pose from the Pose stage's estimator with its keyword arguments ("ransac", keyed on the global pair id like
    the model's, "compat" or "fgr"; "lgr" needs the matcher's patches and is refused with a ValueError).  `Tester.fpfh` maps this rank's pair
    ids to (inlier ratio of the matches at get_inlier_ratio's 0.1 m, nan without matches; RRE degrees; RTE metres; number of matches)
    and on rank 0 `metrics` gains fpfh_ir (mean over the pairs that have matches), fpfh_rre, fpfh_rte (means) and fpfh_success (share
    of pairs with RRE < 15 degrees and RTE < 0.3 m), over the pairs of ALL ranks."""
    name = "fpfh"

    def __init__(self, options, pose):
        if options is not None and pose.estimator == "lgr":
            raise ValueError("the FPFH baseline has no patches: it runs with estimator 'ransac', 'compat' or 'fgr', not 'lgr'")
        super().__init__(options=options, pose=pose)

    def run(self, fw):
        from .fpfh import fpfh_handle
        from .registration import pose_errors
        kw = dict(self.options)
        mode = "mutual" if kw.pop("mutual", True) else "row"
        base = fpfh_handle(fw.handle, mode=mode, estimator=self.pose.estimator, pair_keys=fw.ids, estimator_kw=self.pose.kw,
                           inlier_distance_threshold=DESC_INLIER_THRESHOLD, **kw)
        rre, rte = pose_errors(base["reg"]["T"].cpu(), *fw.gt_pose)
        for k, (idx, ir, cnt) in enumerate(zip(fw.ids, base["ir"].cpu().tolist(), base["n_matches"].cpu().tolist())):
            self.rows[idx] = (float(ir), float(rre[k]), float(rte[k]), int(cnt))

    metrics = lambda self, rows, base: fpfh_metrics(rows)

    def lines(self, rows, m):
        return {"fpfh": [
            f"[roitr_amd] FPFH baseline ({self.pose.estimator}, radius {self.options.get('radius', 0.125):g} m, max_nn {self.options.get('max_nn', 100)}) "
            f"over {m['fpfh_pairs']} pairs: IR {m['fpfh_ir']:.4f}, RRE mean {m['fpfh_rre']:.3f} deg, RTE mean {m['fpfh_rte']:.4f} m, pairs with RRE "
            f"< 15 deg and RTE < 0.3 m: {m['fpfh_success']:.4f}"]}


class Recall(Stage):
    """recall: the 3DMatch-protocol registration recall on the run's own pairs; implies register and evaluate.  Per forward ONE batched
    pairgt.pairgt_handle call on the clouds the model saw gives every pair's overlap ratios and gt.info matrix at `overlap_radius`;
    `Tester.recall` maps this rank's pair ids to (overlap_src, overlap_tgt, p, success) with p = compute_transformation_err(inv(T_gt) @
    T_est, info) and success = p <= 0.2 ** 2 (p is nan for a pair without a source point within the radius: it has no information matrix).
    On rank 0 `metrics` gains RR / RR_pairs over the pairs of ALL ranks that have a p, the same per bin of overlap_src (RR_overlap_ge_0.3:
    the 3DMatch range, RR_overlap_0.1_0.3: 3DLoMatch, RR_overlap_lt_0.1, each with its _pairs count; nan for an empty bin) and
    pairs_without_overlap, the pairs left out.  Every pair's file additionally holds gt_overlap (2, float64: source side, target side) and
    gt_info (6,6 float64); `Tester.gt` keeps (T_gt, info, overlap_src, T_est) per pair id for write_gt, and with `gt_dir` rank 0 writes
    those files for the pairs of ALL ranks.  A row is the recall row + (the gt row,)."""
    name = "recall"

    def run(self, fw):
        import numpy as np
        from .pairgt import pairgt_handle
        gt = pairgt_handle(fw.handle, self.overlap_radius)
        ov = torch.stack([gt.overlap_src, gt.overlap_tgt], 1).cpu()
        info, hits = gt.info.cpu(), gt.n_src_hit.cpu().tolist()
        for k, idx in enumerate(fw.ids):
            T_gt = np.eye(4)
            T_gt[:3, :3] = fw.pairs[k]["rot"].reshape(3, 3).double().cpu().numpy()
            T_gt[:3, 3] = fw.pairs[k]["trans"].reshape(3).double().cpu().numpy()
            T_est = fw.est[k].double().numpy()
            p = recall_error(T_gt, T_est, info[k].numpy()) if hits[k] > 0 else float("nan")
            self.rows[idx] = (float(ov[k, 0]), float(ov[k, 1]), p, bool(p <= RECALL_RMSE ** 2), (T_gt, info[k].numpy(), float(ov[k, 0]), T_est))
        fw.file["gt_overlap"], fw.file["gt_info"] = [o.clone() for o in ov], [i.clone() for i in info]

    attributes = lambda self: {"recall": {k: v[:4] for k, v in self.rows.items()}, "gt": {k: v[4] for k, v in self.rows.items()}}
    metrics = lambda self, rows, base: recall_metrics(rows)

    def lines(self, rows, m):
        out = {"recall": [
            f"[roitr_amd] registration recall (RMSE <= {RECALL_RMSE:g} m, overlap radius {self.overlap_radius:g} m) {m['RR']:.4f} over {m['RR_pairs']} "
            f"pairs ({m['pairs_without_overlap']} without overlap left out); overlap >= 0.3: {m['RR_overlap_ge_0.3']:.4f} ({m['RR_overlap_ge_0.3_pairs']}), "
            f"0.1 .. 0.3: {m['RR_overlap_0.1_0.3']:.4f} ({m['RR_overlap_0.1_0.3_pairs']}), < 0.1: {m['RR_overlap_lt_0.1']:.4f} ({m['RR_overlap_lt_0.1_pairs']})"]}
        if self.gt_dir is not None:
            out["gt"] = [f"[roitr_amd] wrote gt.log, gt.info, gt_overlap.log and est.log for {len(rows)} pairs under {self.gt_dir}"]
        return out

    def finish(self, rows):
        if self.gt_dir is not None:
            write_gt(self.gt_dir, {k: v[4] for k, v in rows.items()})


class Tester:
    def __init__(self, config, model, dataset, snapshot_dir="snapshot", pairs_per_forward=8, rank=0, world=1, evaluate=False,
                 estimate_normals=False, view_point=(0.0, 0.0, 0.0), register=False, ransac=None, nonrigid=None, descriptor_eval=False,
                 validate=False, voxel_size=None, points_lim=None, subsample_seed=0, recall=False, overlap_radius=0.0375,
                 estimator="ransac", lgr=None, refine=None, icp=None, compat=None, fpfh_baseline=None, gt_dir=None, fgr=None,
                 outlier=None):
        """evaluate: also compute PIR / IR per pair on the device (lib/loss.py:169-213 Evaluator) and return their means.
        estimate_normals: ignore the dataset's normals and recompute them on the GPU from the points the way the
        reference's dataset code does (open3d estimate_normals(knn=33) + normal_redirect, dataset/tdmatch.py:120-127).
        voxel_size / points_lim / subsample_seed: raw scans in front of the model, on the device (prep.voxel_down_sample,
        prep.random_subsample; see _prepare).  With either one set the normals are always re-estimated on the new points (the dataset's
        normals no longer belong to them) and the features are rebuilt as ones.
        outlier: dict(method="statistical", nb_neighbors=20, std_ratio=2.0) or dict(method="radius", nb_points=16, radius=0.05): remove
        flying pixels and isolated points on the device after the voxel grid and before the cap (prep.remove_statistical_outlier /
        remove_radius_outlier; see _prepare); re-estimates the normals like the two options above.  Rank 0, after test(): the report
        starts with one line on the removed share per side.
        The other options are described with their stage: nonrigid (Nonrigid), validate (Losses), descriptor_eval (Descriptor), register /
        ransac / estimator / lgr / compat / fgr / refine / icp (Pose), fpfh_baseline (Fpfh), recall / overlap_radius / gt_dir (Recall).  `stages`
        holds the stages that are on, in running order; a stage that is off leaves None.  Rank 0, after test(): `report`, the printed lines."""
        self.config, self.model, self.dataset, self.snapshot_dir, self.pairs_per_forward = config, model, dataset, snapshot_dir, pairs_per_forward
        self.benchmark = config["benchmark"] if isinstance(config, dict) else config.benchmark
        self.rank, self.world, self.voxel_size, self.points_lim, self.subsample_seed = rank, world, voxel_size, points_lim, subsample_seed
        self.outlier = None if outlier is None else dict(outlier)
        if self.outlier is not None and self.outlier.get("method") not in ("statistical", "radius"):
            raise ValueError(f"outlier: method must be 'statistical' or 'radius', got {self.outlier.get('method')!r}")
        self.outlier_rows = {}   # GLOBAL pair id -> (source points in, kept, target points in, kept)
        self.estimate_normals = estimate_normals or voxel_size is not None or points_lim is not None or outlier is not None
        self.view_point = view_point
        recall = recall or gt_dir is not None
        self.evaluate = evaluate or validate or recall
        self.register = register or recall or refine is not None
        self.estimator, self.refine, self.fpfh_baseline = estimator, refine, None if fpfh_baseline is None else dict(fpfh_baseline)
        self.ransac, self.lgr, self.compat, self.icp = dict(ransac or {}), dict(lgr or {}), dict(compat or {}), dict(icp or {})
        self.fgr = dict(fgr or {})
        pose = Pose(estimator, self.ransac, self.lgr, self.compat, refine, self.icp, errors=self.evaluate, fgr=self.fgr)
        radius = float(config.get("eval_acceptance_radius", 0.1) if isinstance(config, dict) else getattr(config, "eval_acceptance_radius", 0.1))
        every = ((Nonrigid(kw=dict(nonrigid or {}), radius=radius), self.evaluate and self.benchmark in NONRIGID_BENCHMARKS),
                 (Losses(config=config), validate), (Descriptor(), descriptor_eval and self.evaluate), (pose, self.register),
                 (Fpfh(self.fpfh_baseline, pose), fpfh_baseline is not None and self.register and self.evaluate),
                 (Recall(overlap_radius=overlap_radius, gt_dir=gt_dir), recall))   # every stage validates its options, whether it is on or not
        for stage, on in every:
            vars(self).update(stage.attributes() if on else dict.fromkeys(stage.attributes()))
        self.stages = [stage for stage, on in every if on]
        self.validation = self.metrics = self.report = self.records = None   # rank 0 after test(); records: shard.GatheredRecords

    def _prepare(self, ids, items, device):
        """The reference's preparation of a raw scan, for all clouds of one forward: the voxel grid its 3DMatch files went through
        beforehand (one batched call for the source clouds, on `raw_src_pcd` with `src_points` as the attribute -- the identity for
        rigid items, the deformed cloud of 4DMatch as the per-voxel mean of the deformed points -- and one for the targets), then the
        outlier filter (one batched call for the sources, on `raw_src_pcd` with `src_points` carried along as the attribute, so a
        deformed cloud keeps the same rows, and one for the targets), then the
        `points_lim` cap of dataset/tdmatch.py:72-78 / dataset/fdmatch.py:49-56 (one batched call; cloud keys 2 * GLOBAL pair id and
        2 * id + 1, so the kept rows do not depend on sharding or pairs_per_forward; kept rows stay in input order where the reference
        keeps permutation order).  `metric_index` becomes unique(inverse[metric_index]) under the grid and the kept ones of its rows,
        renumbered, under the outlier filter and the cap (the reference leaves it pointing into the uncapped cloud)."""
        from .prep import random_subsample, voxel_down_sample
        k = len(items)
        raw = [it["raw_src_pcd"].float() for it in items]
        deformed = [it["src_points"].float() for it in items]
        tgt = [it["tgt_points"].float() for it in items]
        metric = [it["metric_index"].to(device).long() if torch.is_tensor(it.get("metric_index")) else None for it in items]
        if self.voxel_size is not None:
            off_in = _offsets(raw, device)
            rs = voxel_down_sample(torch.cat(raw), off_in, self.voxel_size, attr=torch.cat(deformed))
            rt = voxel_down_sample(torch.cat(tgt), _offsets(tgt, device), self.voxel_size)
            lo_in, lo_s, lo_t = [0] + off_in.tolist(), [0] + rs.offset.tolist(), [0] + rt.offset.tolist()
            for j in range(k):
                if metric[j] is not None:
                    metric[j] = torch.unique(rs.inverse[metric[j] + lo_in[j]].long()) - lo_s[j]
            raw = [rs.points[lo_s[j]:lo_s[j + 1]] for j in range(k)]
            deformed = [rs.attr[lo_s[j]:lo_s[j + 1]] for j in range(k)]
            tgt = [rt.points[lo_t[j]:lo_t[j + 1]] for j in range(k)]
        if self.outlier is not None:
            from . import prep
            kw = {key: v for key, v in self.outlier.items() if key != "method"}
            run = prep.remove_statistical_outlier if self.outlier["method"] == "statistical" else prep.remove_radius_outlier
            off_s, off_t = _offsets(raw, device), _offsets(tgt, device)
            rs = run(torch.cat(raw), off_s, attr=torch.cat(deformed), **kw)
            rt = run(torch.cat(tgt), off_t, **kw)
            lo_in, lo_s, lo_t = [0] + off_s.tolist(), [0] + rs.offset.tolist(), [0] + rt.offset.tolist()
            for j in range(k):
                self.outlier_rows[ids[j]] = (raw[j].shape[0], lo_s[j + 1] - lo_s[j], tgt[j].shape[0], lo_t[j + 1] - lo_t[j])
                if metric[j] is not None:   # the kept ones of its rows, renumbered, as under the cap
                    pos = torch.cumsum(rs.keep[lo_in[j]:lo_in[j + 1]].long(), 0) - 1
                    metric[j] = pos[metric[j]][rs.keep[lo_in[j]:lo_in[j + 1]][metric[j]]]
            raw = [rs.points[lo_s[j]:lo_s[j + 1]] for j in range(k)]
            deformed = [rs.attr[lo_s[j]:lo_s[j + 1]] for j in range(k)]
            tgt = [rt.points[lo_t[j]:lo_t[j + 1]] for j in range(k)]
        if self.points_lim is not None:
            off = _offsets(raw + tgt, device)
            idx, new_off = random_subsample(off, self.points_lim, self.subsample_seed, [2 * i for i in ids] + [2 * i + 1 for i in ids])
            idx, lo, cut = idx.long(), [0] + off.tolist(), [0] + new_off.tolist()
            for j in range(2 * k):
                kept = idx[cut[j]:cut[j + 1]] - lo[j]
                if j >= k:
                    tgt[j - k] = tgt[j - k][kept]
                    continue
                if metric[j] is not None:
                    pos = torch.full((raw[j].shape[0],), -1, dtype=torch.long, device=device)
                    pos[kept] = torch.arange(kept.shape[0], device=device)
                    m = pos[metric[j]]
                    metric[j] = m[m >= 0]
                raw[j], deformed[j] = raw[j][kept], deformed[j][kept]
        for j, it in enumerate(items):
            it["raw_src_pcd"], it["src_points"], it["tgt_points"] = raw[j], deformed[j], tgt[j]
            it["src_feats"] = torch.ones((raw[j].shape[0], 1), dtype=torch.float32, device=device)
            it["tgt_feats"] = torch.ones((tgt[j].shape[0], 1), dtype=torch.float32, device=device)
            if metric[j] is not None:
                it["metric_index"] = metric[j]

    def _load(self, ids, device):
        """The Forward of these pairs, launched: items on the device, prepared, with normals, and the engine call enqueued."""
        items = [{k: v.to(device) if torch.is_tensor(v) else v for k, v in self.dataset[i].items()} for i in ids]
        if self.voxel_size is not None or self.points_lim is not None or self.outlier is not None:
            self._prepare(ids, items, device)
        if self.estimate_normals:   # one batched call for all clouds of this forward
            from .prep import estimate_normals
            clouds = [it["raw_src_pcd"] for it in items] + [it["tgt_points"] for it in items]
            off = _offsets(clouds, device)
            nrm = estimate_normals(torch.cat(clouds).float(), off, 33, self.view_point)
            lo = [0] + off.tolist()
            for k, it in enumerate(items):
                it["src_normals"] = nrm[lo[k]:lo[k + 1]]
                it["tgt_normals"] = nrm[lo[len(items) + k]:lo[len(items) + k + 1]]
        pairs = [dict(src_pcd=it["src_points"].contiguous(), tgt_pcd=it["tgt_points"].contiguous(),
                      src_feats=it["src_feats"].contiguous(), tgt_feats=it["tgt_feats"].contiguous(),
                      src_normals=it["src_normals"].contiguous(), tgt_normals=it["tgt_normals"].contiguous(),
                      rot=it["rot"], trans=it["trans"], src_raw_pcd=it["raw_src_pcd"].contiguous()) for it in items]
        return Forward(ids, items, pairs, self.model.launch_batch(pairs))

    def _write(self, fw, out_dir):
        """One file per pair: the keys of lib/tester.py:56-69, then the ones the stages handed over."""
        for k, (idx, it, p, o) in enumerate(zip(fw.ids, fw.items, fw.pairs, fw.outs)):
            data = {key: p[key].cpu() for key in ("src_raw_pcd", "src_pcd", "tgt_pcd")}
            data.update((key, o[out].cpu()) for key, out in FILE_OUTPUTS)
            data["rot"], data["trans"] = p["rot"].cpu(), p["trans"].cpu()
            if self.benchmark in NONRIGID_BENCHMARKS and "metric_index" in it:
                data["metric_index_list"] = it["metric_index"].cpu() if torch.is_tensor(it["metric_index"]) else it["metric_index"]
            data.update((key, per_pair[k]) for key, per_pair in fw.file.items())
            torch.save(data, os.path.join(out_dir, f"{idx}.pth"))

    def test(self, limit=None):
        out_dir = os.path.join(self.snapshot_dir, str(self.benchmark))
        os.makedirs(out_dir, exist_ok=True)
        n = len(self.dataset) if limit is None else min(limit, len(self.dataset))
        mine = pairs_for_rank(n, self.rank, self.world)
        device = next(self.model.parameters()).device
        self.model.eval()
        evaluator = None
        if self.evaluate:
            from .evaluate import Evaluator
            evaluator = Evaluator(self.config)
        blocks = []   # packed result records of every batch (device)
        with torch.no_grad():
            batches = [mine[s:s + self.pairs_per_forward] for s in range(0, len(mine), self.pairs_per_forward)]
            nxt = self._load(batches[0], device) if batches else None
            for k in range(len(batches)):
                # the next batch is loaded and enqueued before this one is unpacked and written to disk
                fw = nxt
                nxt = self._load(batches[k + 1], device) if k + 1 < len(batches) else None
                fw.outs = self.model.finish_batch(fw.handle)
                aux = None
                if evaluator is not None:   # after finish_batch: an overfull 4DMatch call has been repeated into the handle
                    ir, pir, _, _ = evaluator.evaluate_batch(fw.handle)
                    aux = torch.stack([ir.float(), pir.float()], 1)
                blocks.append(self.model.batch_records(fw.handle, fw.ids, aux))
                for stage in self.stages:
                    stage.run(fw)
                self._write(fw, out_dir)
        for stage in self.stages:
            vars(self).update(stage.attributes())
        # ---- the two collectives of the run, every rank takes part: the records -> rank 0 (RCCL over xGMI), the stages' rows -> all
        per_pair = self.model.record_scores_per_pair()
        self.records = gather_result_records(assemble_block(blocks, slots_per_rank(n, self.world), per_pair, device),
                                             slots_per_rank(n, self.world), per_pair)
        local = {stage.name: stage.rows for stage in self.stages}
        if self.outlier is not None:
            local["outlier"] = self.outlier_rows
        merged = merge_rows(local, self.world)
        if self.records is None:     # ranks other than 0
            return None
        if self.records.truncated:
            import warnings
            warnings.warn(f"result records: the score pool of a rank was full, the scores of {len(self.records.truncated)} pair(s) were "
                          f"cut (first: {self.records.truncated[:8]}); raise config key record_scores_per_pair (now {per_pair}). "
                          "The .pth files on disk are complete.")
        counts = [sum(cnt for pid, cnt in self.records.n_scores.items() if pid % self.world == r) for r in range(self.world)]
        lines = {}
        if evaluator is not None:
            # PIR of a pair without coarse correspondences is the mean of an empty tensor = nan in the reference
            # (lib/loss.py:191): such pairs are left out of the PIR mean (and counted) instead of poisoning it or counting as 0
            irs = [a[0] for a in self.records.aux.values()]
            pirs = [a[1] for a in self.records.aux.values() if a[1] == a[1]]
            self.metrics = {"IR": sum(irs) / max(len(irs), 1), "PIR": sum(pirs) / max(len(pirs), 1), "pairs": len(irs),
                            "pairs_without_coarse": len(irs) - len(pirs)}
            lines["eval"] = [f"[roitr_amd] PIR {self.metrics['PIR']:.4f}  IR {self.metrics['IR']:.4f}  over {self.metrics['pairs']} pairs"]
        for stage in self.stages:
            found = stage.metrics(merged[stage.name], self.metrics)
            if found:
                setattr(self, stage.publishes, {**(getattr(self, stage.publishes) or {}), **found})
            lines.update(stage.lines(merged[stage.name], getattr(self, stage.publishes)))
            stage.finish(merged[stage.name])
        self.report = [line for slot in REPORT_ORDER for line in lines.get(slot, ())]
        if self.outlier is not None:
            self.outlier_rows = merged["outlier"]
            self.report.insert(0, outlier_line(self.outlier["method"], merged["outlier"]))
        return counts


def outlier_line(method, rows):
    """The one line of the outlier filter: the removed share per side over the pairs of all ranks."""
    s_in, s_kept, t_in, t_kept = (sum(r[c] for r in rows.values()) for c in range(4))
    return (f"[roitr_amd] outlier removal ({method}) over {len(rows)} pairs: removed {1 - s_kept / max(s_in, 1):.4f} of the source points "
            f"({s_in - s_kept} of {s_in}), {1 - t_kept / max(t_in, 1):.4f} of the target points ({t_in - t_kept} of {t_in})")


def fpfh_metrics(rows):
    """{pair id: (ir, rre, rte, matches)} -> the baseline's report: fpfh_ir over the pairs that have matches, mean fpfh_rre / fpfh_rte,
    fpfh_success = share of pairs with RRE < 15 degrees and RTE < 0.3 m (the registration report's pose-error success rate)."""
    v = [rows[k] for k in sorted(rows)]
    return {"fpfh_ir": _mean([r[0] for r in v if r[0] == r[0]]), "fpfh_rre": _mean([r[1] for r in v]), "fpfh_rte": _mean([r[2] for r in v]),
            "fpfh_success": _mean([1.0 if r[1] < SUCCESS_RRE and r[2] < SUCCESS_RTE else 0.0 for r in v]), "fpfh_pairs": len(v)}


def recall_error(T_gt, T_est, info):
    """registration/benchmark.py:260: p = computeTransformationErr(inv(T_gt) @ T_est, info), the value compared with 0.2 ** 2."""
    import numpy as np
    from .registration import compute_transformation_err
    return compute_transformation_err(np.linalg.inv(T_gt) @ T_est, info)


def recall_metrics(recall):
    """{pair id: (overlap_src, overlap_tgt, p, success, ...)} -> RR over the pairs that have a p, and per bin of overlap_src."""
    rows = [v for v in recall.values() if v[2] == v[2]]
    rate = lambda sel: sum(1 for v in sel if v[3]) / len(sel) if sel else float("nan")
    out = {"RR": rate(rows), "RR_pairs": len(rows), "pairs_without_overlap": len(recall) - len(rows)}
    for name, lo, hi in OVERLAP_BINS:
        sel = [v for v in rows if lo <= v[0] < hi]
        out["RR_" + name], out["RR_" + name + "_pairs"] = rate(sel), len(sel)
    return out


def write_gt(directory, gt):
    """gt.log, gt.info, gt_overlap.log and est.log for {pair id: (T_gt, info, overlap_src, T_est)} in the layouts
    registration.read_trajectory / read_trajectory_info read and the `i,j,ratio` lines of the reference's gt_overlap.log.  Pair id k is
    written as the fragment pair (k, k + 2) of k_max + 3 fragments: registration/benchmark.py only tests non-consecutive pairs.  It
    also marks the tested pairs by their POSITIVE index into gt.log (`gt_mask[i, j] = idx`, `> 0`), so whatever stands at index 0 is
    never tested: the first record of gt.log, gt.info and est.log is a filler, the consecutive pair (0, 1) with identity matrices,
    and every pair of the run is tested.  gt_overlap.log holds the run's pairs only."""
    import numpy as np
    from .registration import write_trajectory, write_trajectory_info
    os.makedirs(directory, exist_ok=True)
    ids = sorted(gt)
    n_frag = (ids[-1] + 3) if ids else 2
    meta = [(0, 1, n_frag)] + [(k, k + 2, n_frag) for k in ids]
    write_trajectory(np.stack([np.eye(4)] + [gt[k][0] for k in ids]), meta, os.path.join(directory, "gt.log"))
    write_trajectory_info(np.stack([np.eye(6)] + [gt[k][1] for k in ids]), meta, os.path.join(directory, "gt.info"))
    write_trajectory(np.stack([np.eye(4)] + [gt[k][3] for k in ids]), meta, os.path.join(directory, "est.log"))
    with open(os.path.join(directory, "gt_overlap.log"), "w") as f:
        for k in ids:
            f.write(f"{k},{k + 2},{gt[k][2]:.4f}\n")


class SyntheticPairs(torch.utils.data.Dataset):
    """Stand-in for dataset/tdmatch.py (no 3DMatch data in this image): seeded synthetic pairs with the same keys."""

    def __init__(self, n_pairs, n_points=5000, config=2, nonrigid=False):
        """nonrigid: 4DMatch-shaped pairs with a real deformation and `metric_index` (synthetic.make_nonrigid_pair; `config` is
        not used then, the generator has a config number of its own)."""
        self.n_pairs, self.n_points, self.config, self.nonrigid = n_pairs, n_points, config, nonrigid

    def __len__(self):
        return self.n_pairs

    def __getitem__(self, i):
        from .synthetic import make_nonrigid_pair, make_pair
        if self.nonrigid:
            return {k: torch.from_numpy(v) for k, v in make_nonrigid_pair(self.n_points, pair_index=i).items()}
        return {k: torch.from_numpy(v) for k, v in make_pair(self.n_points, config=self.config, pair_index=i).items()}
