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
"""
import os

import torch

from . import _args as A
from .shard import assemble_block, gather_result_records, pairs_for_rank, slots_per_rank


DESC_INLIER_THRESHOLD = 0.1   # registration/benchmark_utils.py:80 get_inlier_ratio's default, whatever eval_acceptance_radius says
DESC_FMR_THRESHOLD = 0.05   # registration/evaluate_registration_c2f.py:109: a pair counts when its inlier ratio exceeds it
RECALL_RMSE = 0.2            # registration/benchmark.py:217 evaluate_registration: a pair is registered when p <= 0.2 ** 2
OVERLAP_BINS = (("overlap_ge_0.3", 0.3, float("inf")), ("overlap_0.1_0.3", 0.1, 0.3), ("overlap_lt_0.1", float("-inf"), 0.1))


def _offsets(clouds, device):
    """The reference's `offset` of a list of clouds: their cumulative ends, int32 on the device."""
    return A.cumulative([c.shape[0] for c in clouds], device)[1:]


def load_pretrain(model, path):
    """lib/trainer.py:94-130 `_load_pretrain`: state['state_dict'], 'module.' prefixes stripped, strict load."""
    state = torch.load(path, map_location="cpu")
    sd = state["state_dict"] if "state_dict" in state else state
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    model.load_state_dict(sd, strict=True)
    return model


class Tester:
    def __init__(self, config, model, dataset, snapshot_dir="snapshot", pairs_per_forward=8, rank=0, world=1, evaluate=False,
                 estimate_normals=False, view_point=(0.0, 0.0, 0.0), register=False, ransac=None, nonrigid=None, descriptor_eval=False,
                 validate=False, voxel_size=None, points_lim=None, subsample_seed=0, recall=False, overlap_radius=0.0375,
                 estimator="ransac", lgr=None, refine=None, icp=None, compat=None, fpfh_baseline=None):
        """evaluate: also compute PIR / IR per pair on the device (lib/loss.py:169-213 Evaluator) and return their means.
        estimate_normals: ignore the dataset's normals and recompute them on the GPU from the points the way the
        reference's dataset code does (open3d estimate_normals(knn=33) + normal_redirect, dataset/tdmatch.py:120-127).
        register: also estimate every pair's pose on the device (registration.register_handle, keyed on the GLOBAL pair id, so the
        poses do not depend on sharding or pairs_per_forward; `ransac` holds its keyword arguments) and save it as `est_transform`
        in the pair's file.  With evaluate as well, `registration` maps this rank's pair ids to (RRE degrees, RTE metres, inliers).
        estimator: "ransac" (the default, as above) or "lgr": the pose comes from lgr.lgr_handle (local-to-global registration on the
        matcher's patches: no random stream, so no keys; `lgr` holds its keyword arguments) or "compat": the pose comes from
        compat.compat_handle (spatial-compatibility registration: no random stream and no patch structure either; `compat` holds its
        keyword arguments); everything downstream of the pose
        (est_transform, RRE / RTE, the inlier column, the recall rows) is the same code.
        With evaluate on the 4DMatch / 4DLoMatch benchmark and items that carry `metric_index`, the NFMR of every pair is computed
        on the device (nonrigid.nfmr_handle; `nonrigid` holds its keyword arguments) and `self.nonrigid` maps this rank's pair ids
        to (NFMR, number of metric points); it stays None otherwise.
        descriptor_eval (with evaluate): the descriptor-level evaluation of registration/benchmark_utils.py get_inlier_ratio on
        the point descriptors of every pair (descmatch.descriptor_handle, one fused matching launch per forward): `self.descriptor`
        maps this rank's pair ids to (IR without the mutual check, IR with it, number of mutual matches) and `metrics` gains
        desc_IR_wo (mean over pairs), desc_IR_w (mean over the pairs that have mutual matches: the IR of an empty set is nan, handled
        as PIR is) and desc_FMR (share of pairs with IR without the mutual check above 0.05, evaluate_registration_c2f.py:109),
        over the pairs of ALL ranks (one all_gather_object of the per-pair values when world > 1), like IR / PIR.  The inlier
        distance is get_inlier_ratio's default, 0.1 m, not the config's eval_acceptance_radius.  The result records and their
        format are untouched.
        validate: the reference's `val` report (lib/trainer.py:335-344: OverallLoss and Evaluator per pair under no_grad); implies
        evaluate.  The losses of every pair are computed on the device (loss.loss_batch, two batched kernels per forward):
        `self.losses` maps this rank's pair ids to (loss, c_loss, f_loss, o_loss), and on rank 0 `self.validation` holds the means of
        loss, c_loss, f_loss, o_loss, PIR and IR over the pairs of ALL ranks (one all_gather_object) plus `skipped`: the reference's
        AverageMeter turns a whole mean into nan on one nan pair (a pair without fine labels, or without a row and a column that
        have both a positive and a negative); here such pairs are left out of that key's mean and counted per key.
        voxel_size / points_lim / subsample_seed: raw scans in front of the model, on the device (prep.voxel_down_sample,
        prep.random_subsample; see _prepare).  With either one set the normals are always re-estimated on the new points (the dataset's
        normals no longer belong to them) and the features are rebuilt as ones.
        recall: the 3DMatch-protocol registration recall on the run's own pairs; implies register and evaluate.  Per forward ONE batched
        pairgt.pairgt_handle call on the clouds the model saw gives every pair's overlap ratios and gt.info matrix at `overlap_radius`;
        `self.recall` maps this rank's pair ids to (overlap_src, overlap_tgt, p, success) with p = compute_transformation_err(
        inv(T_gt) @ T_est, info) and success = p <= 0.2 ** 2 (p is nan for a pair without a source point within the radius: it has
        no information matrix).  On rank 0 `metrics` gains RR / RR_pairs over the pairs of ALL ranks that have a p, the same per
        overlap bin of overlap_src (RR_overlap_ge_0.3: the 3DMatch range, RR_overlap_0.1_0.3: 3DLoMatch, RR_overlap_lt_0.1, each
        with its _pairs count; nan for an empty bin) and pairs_without_overlap, the pairs left out.  Every pair's file additionally
        holds gt_overlap (2, float64: source side, target side) and gt_info (6,6 float64); `self.gt` keeps (T_gt, info,
        overlap_src, T_est) per pair id for write_gt.  With recall off, files, records and metrics are what they are without it.
        refine: None, "point" or "plane": after the estimator's pose, ICP on the clouds the model saw (icp.icp_handle from reg["T"],
        point-to-point or point-to-plane on the target normals; `icp` holds its keyword arguments); implies register.  The refined
        transform takes the place of the estimated one everywhere downstream (est_transform, `registration`, the recall rows), and
        `self.refinement` maps this rank's pair ids to (rre_before, rte_before, rre_after, rte_after, fitness, rmse, steps),
        `self.refinement_status` to the pair's ICP status word.  With refine=None nothing of it is imported or run.
        refine="gicp": the same with generalized ICP (gicp.gicp_handle: plane-to-plane on the normals of both clouds); `icp` then also
        carries `epsilon`.  The rows of `self.refinement` / `self.refinement_status` are the same; gicp.py is imported in this mode only.
        fpfh_baseline: None, or a dict (radius, max_nn, mutual; defaults 0.125, 100, True) that switches on the learning-free baseline
        (fpfh.fpfh_handle) with evaluate and register: FPFH descriptors of the clouds and normals the model was fed, matched under
        the squared distance, their pose from the selected estimator with its keyword arguments ("ransac", keyed on the global pair
        id like the model's, or "compat"; "lgr" needs the matcher's patches and is refused with a ValueError).  `self.fpfh` maps this
        rank's pair ids to (inlier ratio of the matches at get_inlier_ratio's 0.1 m, nan without matches; RRE degrees; RTE metres;
        number of matches) and on rank 0 `metrics` gains fpfh_ir (mean over the pairs that have matches), fpfh_rre, fpfh_rte (means)
        and fpfh_success (share of pairs with RRE < 15 degrees and RTE < 0.3 m), over the pairs of ALL ranks.  Files, records and
        every other metric are what they are without it."""
        self.config, self.model, self.dataset = config, model, dataset
        self.snapshot_dir = snapshot_dir
        self.pairs_per_forward = pairs_per_forward
        self.rank, self.world = rank, world
        self.voxel_size, self.points_lim, self.subsample_seed = voxel_size, points_lim, subsample_seed
        estimate_normals = estimate_normals or voxel_size is not None or points_lim is not None
        self.evaluate, self.estimate_normals, self.view_point = evaluate or validate, estimate_normals, view_point
        if refine not in (None, "point", "plane", "gicp"):
            raise ValueError("refine must be None, 'point', 'plane' or 'gicp'")
        register = register or recall or refine is not None
        self.evaluate = self.evaluate or recall
        if estimator not in ("ransac", "lgr", "compat"):
            raise ValueError("estimator must be 'ransac', 'lgr' or 'compat'")
        self.register, self.ransac = register, dict(ransac or {})
        self.estimator, self.lgr, self.compat = estimator, dict(lgr or {}), dict(compat or {})
        self.refine, self.icp = refine, dict(icp or {})
        if fpfh_baseline is not None and estimator == "lgr":
            raise ValueError("the FPFH baseline has no patches: it runs with estimator 'ransac' or 'compat', not 'lgr'")
        self.fpfh_baseline = None if fpfh_baseline is None else dict(fpfh_baseline)
        self.fpfh = {} if fpfh_baseline is not None and register and self.evaluate else None
        self.refinement = {} if refine is not None else None
        self.refinement_status = {} if refine is not None else None
        self.registration = {} if register and self.evaluate else None
        self.recall = {} if recall else None
        self.gt = {} if recall else None
        self.overlap_radius = overlap_radius
        self.nonrigid_kw = dict(nonrigid or {})
        self.nonrigid = None   # {global pair id: (nfmr, n_metric)} once a 4DMatch batch with metric_index has been evaluated
        self.descriptor = {} if descriptor_eval and self.evaluate else None
        self.losses = {} if validate else None
        self.validation = None
        self.metrics = None
        self.records = None   # rank 0 after test(): shard.GatheredRecords {pair id: match scores}

    def _all_ranks(self, per_pair):
        """A per-pair dict (or None: not collected) merged over all ranks; every rank takes part."""
        if per_pair is None or self.world == 1:
            return per_pair
        parts = [None] * self.world
        torch.distributed.all_gather_object(parts, per_pair)
        return {k: v for part in parts for k, v in part.items()}

    def _to_device(self, item, device):
        out = {}
        for k, v in item.items():
            out[k] = v.to(device) if torch.is_tensor(v) else v
        return out

    def _prepare(self, ids, items, device):
        """The reference's preparation of a raw scan, for all clouds of one forward: the voxel grid its 3DMatch files went through
        beforehand (one batched call for the source clouds, on `raw_src_pcd` with `src_points` as the attribute -- the identity for
        rigid items, the deformed cloud of 4DMatch as the per-voxel mean of the deformed points -- and one for the targets), then the
        `points_lim` cap of dataset/tdmatch.py:72-78 / dataset/fdmatch.py:49-56 (one batched call; cloud keys 2 * GLOBAL pair id and
        2 * id + 1, so the kept rows do not depend on sharding or pairs_per_forward; kept rows stay in input order where the reference
        keeps permutation order).  `metric_index` becomes unique(inverse[metric_index]) under the grid and the kept ones of its rows,
        renumbered, under the cap (the reference leaves it pointing into the uncapped cloud)."""
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

    def _recall_rows(self, handle, ids, pairs, est):
        """One pairgt call for the forward: fills self.recall / self.gt and returns per pair (gt_overlap, gt_info) for its file."""
        import numpy as np
        from .pairgt import pairgt_handle
        gt = pairgt_handle(handle, self.overlap_radius)
        ov = torch.stack([gt.overlap_src, gt.overlap_tgt], 1).cpu()
        info, hits = gt.info.cpu(), gt.n_src_hit.cpu().tolist()
        rows = []
        for k, idx in enumerate(ids):
            T_gt = np.eye(4)
            T_gt[:3, :3] = pairs[k]["rot"].reshape(3, 3).double().cpu().numpy()
            T_gt[:3, 3] = pairs[k]["trans"].reshape(3).double().cpu().numpy()
            T_est = est[k].double().numpy()
            p = recall_error(T_gt, T_est, info[k].numpy()) if hits[k] > 0 else float("nan")
            self.recall[idx] = (float(ov[k, 0]), float(ov[k, 1]), p, bool(p <= RECALL_RMSE ** 2))
            self.gt[idx] = (T_gt, info[k].numpy(), float(ov[k, 0]), T_est)
            rows.append((ov[k].clone(), info[k].clone()))
        return rows

    def test(self, limit=None):
        benchmark = self.config["benchmark"] if isinstance(self.config, dict) else self.config.benchmark
        out_dir = os.path.join(self.snapshot_dir, str(benchmark))
        os.makedirs(out_dir, exist_ok=True)
        n = len(self.dataset) if limit is None else min(limit, len(self.dataset))
        mine = pairs_for_rank(n, self.rank, self.world)
        device = next(self.model.parameters()).device
        self.model.eval()
        def load(s):
            ids = mine[s:s + self.pairs_per_forward]
            items = [self._to_device(self.dataset[i], device) for i in ids]
            if self.voxel_size is not None or self.points_lim is not None:
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
            return ids, items, pairs, self.model.launch_batch(pairs)

        evaluator = None
        if self.evaluate:
            from .evaluate import Evaluator
            evaluator = Evaluator(self.config)
        blocks = []   # packed result records of every batch (device)
        with torch.no_grad():
            starts = list(range(0, len(mine), self.pairs_per_forward))
            nxt = load(starts[0]) if starts else None
            for k in range(len(starts)):
                ids, items, pairs, handle = nxt
                # the next batch is loaded and enqueued before this one is unpacked and written to disk
                nxt = load(starts[k + 1]) if k + 1 < len(starts) else None
                outs = self.model.finish_batch(handle)
                aux = None
                if evaluator is not None:   # after finish_batch: an overfull 4DMatch call has been repeated into the handle
                    ir, pir, _, _ = evaluator.evaluate_batch(handle)
                    aux = torch.stack([ir.float(), pir.float()], 1)
                blocks.append(self.model.batch_records(handle, ids, aux))
                if evaluator is not None and benchmark in ("4DMatch", "4DLoMatch") and all("metric_index" in it for it in items):
                    from .nonrigid import nfmr_handle
                    nf = nfmr_handle(handle, [it["metric_index"] for it in items], **self.nonrigid_kw)
                    if self.nonrigid is None:
                        self.nonrigid = {}
                    for idx, r, m in zip(ids, nf["nfmr"].cpu().tolist(), nf["n_metric"].cpu().tolist()):
                        self.nonrigid[idx] = (float(r), int(m))
                if self.losses is not None:
                    from .loss import loss_batch
                    total, c_loss, f_loss, _, _ = loss_batch(handle, self.config)
                    rows = torch.stack([total, c_loss, f_loss, 0.0 * f_loss], 1).cpu().tolist()   # o_loss = 0 * f_loss (lib/loss.py:165)
                    for idx, row in zip(ids, rows):
                        self.losses[idx] = tuple(float(x) for x in row)
                if self.descriptor is not None:
                    from .descmatch import descriptor_handle
                    d = descriptor_handle(handle, "point", DESC_INLIER_THRESHOLD)
                    for idx, wo, w, nw in zip(ids, d["ir_wo"].cpu().tolist(), d["ir_w"].cpu().tolist(), d["n_w"].cpu().tolist()):
                        self.descriptor[idx] = (float(wo), float(w), int(nw))
                est = None
                if self.register:
                    from .registration import pose_errors, register_handle
                    if self.estimator == "lgr":
                        from .lgr import lgr_handle
                        reg = lgr_handle(handle, **self.lgr)
                    elif self.estimator == "compat":
                        from .compat import compat_handle
                        reg = compat_handle(handle, **self.compat)
                    else:
                        reg = register_handle(handle, pair_keys=ids, **self.ransac)
                    est = reg["T"].cpu()
                    if self.refine is not None or self.registration is not None:
                        gt_pose = (torch.stack([p["rot"].reshape(3, 3) for p in pairs]), torch.stack([p["trans"].reshape(3) for p in pairs]))
                    if self.refine is not None:
                        if self.refine == "gicp":
                            from .gicp import gicp_handle
                            ref = gicp_handle(handle, reg["T"], **self.icp)
                        else:
                            from .icp import icp_handle
                            ref = icp_handle(handle, reg["T"], plane=self.refine == "plane", **self.icp)
                        before, est = pose_errors(est, *gt_pose), ref["T"].cpu()
                        after = pose_errors(est, *gt_pose)
                        cols = [x.cpu().tolist() for x in (*before, *after, ref["fitness"], ref["rmse"], ref["steps"], ref["status"])]
                        for k, idx in enumerate(ids):
                            self.refinement[idx] = tuple(float(c[k]) for c in cols[:6]) + (int(cols[6][k]),)
                            self.refinement_status[idx] = int(cols[7][k])
                    if self.registration is not None:
                        rre, rte = pose_errors(est, *gt_pose)
                        inl = reg["inliers"].cpu().tolist()
                        for k, idx in enumerate(ids):
                            self.registration[idx] = (float(rre[k]), float(rte[k]), int(inl[k]))
                if self.fpfh is not None:
                    from .fpfh import fpfh_handle
                    from .registration import pose_errors
                    kw = dict(self.fpfh_baseline)
                    mode = "mutual" if kw.pop("mutual", True) else "row"
                    base = fpfh_handle(handle, mode=mode, estimator=self.estimator, pair_keys=ids,
                                       estimator_kw=self.compat if self.estimator == "compat" else self.ransac,
                                       inlier_distance_threshold=DESC_INLIER_THRESHOLD, **kw)
                    rre, rte = pose_errors(base["reg"]["T"].cpu(), torch.stack([p["rot"].reshape(3, 3) for p in pairs]),
                                           torch.stack([p["trans"].reshape(3) for p in pairs]))
                    for k, (idx, ir, cnt) in enumerate(zip(ids, base["ir"].cpu().tolist(), base["n_matches"].cpu().tolist())):
                        self.fpfh[idx] = (float(ir), float(rre[k]), float(rte[k]), int(cnt))
                gt_rows = None
                if self.recall is not None:
                    gt_rows = self._recall_rows(handle, ids, pairs, est)
                for k_pair, (idx, it, p, o) in enumerate(zip(ids, items, pairs, outs)):
                    data = dict()  # lib/tester.py:56-69
                    data["src_raw_pcd"] = p["src_raw_pcd"].cpu()
                    data["src_pcd"], data["tgt_pcd"] = p["src_pcd"].cpu(), p["tgt_pcd"].cpu()
                    data["src_nodes"], data["tgt_nodes"] = o["src_nodes"].cpu(), o["tgt_nodes"].cpu()
                    data["src_node_desc"], data["tgt_node_desc"] = o["src_node_feats"].cpu(), o["tgt_node_feats"].cpu()
                    data["src_point_desc"], data["tgt_point_desc"] = o["src_point_feats"].cpu(), o["tgt_point_feats"].cpu()
                    data["src_corr_pts"], data["tgt_corr_pts"] = o["src_corr_points"].cpu(), o["tgt_corr_points"].cpu()
                    data["confidence"] = o["corr_scores"].cpu()
                    data["gt_tgt_node_occ"] = o["gt_tgt_node_occ"].cpu()
                    data["gt_src_node_occ"] = o["gt_src_node_occ"].cpu()
                    data["rot"], data["trans"] = p["rot"].cpu(), p["trans"].cpu()
                    if benchmark in ("4DMatch", "4DLoMatch") and "metric_index" in it:
                        data["metric_index_list"] = it["metric_index"].cpu() if torch.is_tensor(it["metric_index"]) else it["metric_index"]
                    if est is not None:
                        data["est_transform"] = est[k_pair]
                    if gt_rows is not None:
                        data["gt_overlap"], data["gt_info"] = gt_rows[k_pair]
                    torch.save(data, os.path.join(out_dir, f"{idx}.pth"))
        # ---- the one collective of the run: every rank's records -> rank 0 (RCCL over xGMI under torch.distributed.run)
        per_pair = self.model.record_scores_per_pair()
        self.records = gather_result_records(assemble_block(blocks, slots_per_rank(n, self.world), per_pair, device),
                                             slots_per_rank(n, self.world), per_pair)
        # every rank takes part: IR / PIR below cover all ranks, so must these
        desc_all, losses_all, recall_all = self._all_ranks(self.descriptor), self._all_ranks(self.losses), self._all_ranks(self.recall)
        fpfh_all = self._all_ranks(self.fpfh)
        if self.records is None:     # ranks other than 0
            return None
        if self.records.truncated:
            import warnings
            warnings.warn(f"result records: the score pool of a rank was full, the scores of {len(self.records.truncated)} pair(s) were "
                          f"cut (first: {self.records.truncated[:8]}); raise config key record_scores_per_pair (now {per_pair}). "
                          "The .pth files on disk are complete.")
        counts = [0] * self.world
        for pid, cnt in self.records.n_scores.items():
            counts[pid % self.world] += cnt
        if evaluator is not None:
            # PIR of a pair without coarse correspondences is the mean of an empty tensor = nan in the reference
            # (lib/loss.py:191): such pairs are left out of the PIR mean (and counted) instead of poisoning it or counting as 0
            irs = [a[0] for a in self.records.aux.values()]
            pirs = [a[1] for a in self.records.aux.values() if a[1] == a[1]]
            self.metrics = {"IR": sum(irs) / max(len(irs), 1), "PIR": sum(pirs) / max(len(pirs), 1), "pairs": len(irs),
                            "pairs_without_coarse": len(irs) - len(pirs)}
            if self.descriptor is not None:
                wo = [v[0] for v in desc_all.values() if v[0] == v[0]]
                w = [v[1] for v in desc_all.values() if v[1] == v[1]]
                self.metrics.update(desc_IR_wo=sum(wo) / max(len(wo), 1), desc_IR_w=sum(w) / max(len(w), 1),
                                    desc_FMR=sum(1 for x in wo if x > DESC_FMR_THRESHOLD) / max(len(wo), 1))
            if recall_all is not None:
                self.metrics.update(recall_metrics(recall_all))
            if fpfh_all is not None:
                self.metrics.update(fpfh_metrics(fpfh_all))
            if losses_all is not None:
                self.validation = {"PIR": self.metrics["PIR"], "IR": self.metrics["IR"], "pairs": len(losses_all),
                                   "skipped": {"PIR": self.metrics["pairs_without_coarse"], "IR": 0}}
                for col, key in enumerate(("loss", "c_loss", "f_loss", "o_loss")):
                    vals = [v[col] for v in losses_all.values() if v[col] == v[col]]
                    self.validation[key] = sum(vals) / len(vals) if vals else float("nan")
                    self.validation["skipped"][key] = len(losses_all) - len(vals)
        return counts


def fpfh_metrics(rows):
    """{pair id: (ir, rre, rte, matches)} -> the baseline's report: fpfh_ir over the pairs that have matches, mean fpfh_rre / fpfh_rte,
    fpfh_success = share of pairs with RRE < 15 degrees and RTE < 0.3 m (main.py's pose-error success rate)."""
    v = [rows[k] for k in sorted(rows)]
    ir = [r[0] for r in v if r[0] == r[0]]
    mean = lambda x: sum(x) / len(x) if x else float("nan")
    return {"fpfh_ir": mean(ir), "fpfh_rre": mean([r[1] for r in v]), "fpfh_rte": mean([r[2] for r in v]),
            "fpfh_success": mean([1.0 if r[1] < 15.0 and r[2] < 0.3 else 0.0 for r in v]), "fpfh_pairs": len(v)}


def recall_error(T_gt, T_est, info):
    """registration/benchmark.py:260: p = computeTransformationErr(inv(T_gt) @ T_est, info), the value compared with 0.2 ** 2."""
    import numpy as np
    from .registration import compute_transformation_err
    return compute_transformation_err(np.linalg.inv(T_gt) @ T_est, info)


def recall_metrics(recall):
    """{pair id: (overlap_src, overlap_tgt, p, success)} -> RR over the pairs that have a p, and per bin of overlap_src."""
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
