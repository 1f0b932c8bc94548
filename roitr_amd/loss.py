"""Validation losses on the GPU: the forward values of lib/loss.py:8-166.

`loss_batch` computes c_loss, f_loss and their weighted sum for every pair of a RIGA_v2.launch_batch() handle with the two batched
entry points of csrc/loss.hip (rules in include/roitr_engine.h), on the engine's output buffers in place and without a host round
trip.  `WeightedCircleLoss`, `CoarseMatchingLoss`, `FineMatchingLoss` and `OverallLoss` keep the reference's names, config keys and
signatures and run the same kernels with one pair; `weighted_circle_loss` is the dense general-mask form in torch (a cold path).
Everything runs under no_grad: there is no backward.

Differences from the reference, by design: the fine loss measures point distances as fp32 differences, not by the
|a|^2 + |b|^2 - 2ab expansion (a label can differ where |d^2 - r^2| lies inside that form's rounding error); sums run in a fixed order
(partly in float64), so a value differs from torch's in the last bits and does not depend on the batch.
"""
import numpy as np
import torch

from . import _args as A
from . import _lib as L
from .riga import handle_poses, handle_starts

FINE_EMPTY, COARSE_EMPTY, BAD_OFFSETS, BAD_INDEX = 1, 2, 4, 8

DEFAULTS = dict(coarse_loss_positive_margin=0.1, coarse_loss_negative_margin=1.4, coarse_loss_positive_optimal=0.1,
                coarse_loss_negative_optimal=1.4, coarse_loss_log_scale=24, coarse_loss_positive_overlap=0.1, coarse_loss_weight=1.0,
                fine_loss_positive_radius=0.05, fine_loss_weight=1.0, occ_loss_weight=0.0)


def _cfg(cfg, key):
    v = cfg.get(key) if isinstance(cfg, dict) else getattr(cfg, key, None)
    return DEFAULTS[key] if v is None else v


def _ints(values, dev):
    return torch.tensor(np.asarray(values, np.int32), device=dev)


@torch.no_grad()
def fine_loss_batch(first_slot, patch_count, tgt_knn_pts, src_knn_pts, tgt_knn_masks, src_knn_masks, matching_scores, rot, trans,
                    positive_radius=0.05):
    """FineMatchingLoss.forward (lib/loss.py:119-143) of every pair of a batch.  Pair b owns patch slots [first_slot[b], first_slot[b]
    + patch_count[b]) of the per-patch arrays ((slots, L, 3) points, (slots, L) masks, (slots, L+1, L+1) scores); rot (B,3,3),
    trans (B,3).  Device tensors.  Returns (f_loss, f_sum, f_count, status), each (B,); a pair without labels has f_loss NaN and
    FINE_EMPTY in its status."""
    i32, f32 = torch.int32, torch.float32
    first_slot, patch_count = A.dev(first_slot, i32, "first_slot").reshape(-1), A.dev(patch_count, i32, "patch_count").reshape(-1)
    B = int(first_slot.numel())
    scores = A.dev(matching_scores, f32, "matching_scores")
    slots, Lp = int(scores.shape[0]), int(scores.shape[-1]) - 1
    if scores.dim() != 3 or scores.shape[1] != scores.shape[2] or patch_count.numel() != B:
        raise L.RoitrError(f"fine_loss_batch: matching_scores {tuple(scores.shape)}, {B} first slots, {patch_count.numel()} counts")
    tp, sp = A.dev(tgt_knn_pts, f32, "tgt_knn_pts"), A.dev(src_knn_pts, f32, "src_knn_pts")
    tm, sm = A.dev(tgt_knn_masks, i32, "tgt_knn_masks"), A.dev(src_knn_masks, i32, "src_knn_masks")
    if tuple(tp.shape) != (slots, Lp, 3) or tp.shape != sp.shape or tuple(tm.shape) != (slots, Lp) or tm.shape != sm.shape:
        raise L.RoitrError(f"fine_loss_batch: points {tuple(tp.shape)} / {tuple(sp.shape)} and masks {tuple(tm.shape)} / {tuple(sm.shape)} "
                           f"do not match scores {tuple(scores.shape)}")
    rot, trans = A.poses(rot, trans, B)
    dev = scores.device
    f_sum, f_loss = torch.empty((B,), dtype=f32, device=dev), torch.empty((B,), dtype=f32, device=dev)
    f_count, status = torch.empty((B,), dtype=i32, device=dev), torch.empty((B,), dtype=i32, device=dev)
    lib = L.lib()
    nbytes = int(lib.roitr_fine_loss_workspace_bytes(slots))
    ws = A.workspace(nbytes, dev)
    L.check(lib.roitr_fine_loss_batch(B, slots, first_slot.data_ptr(), patch_count.data_ptr(), Lp, tp.data_ptr(), sp.data_ptr(),
                                      tm.data_ptr(), sm.data_ptr(), scores.data_ptr(), rot.data_ptr(), trans.data_ptr(),
                                      float(positive_radius), f_sum.data_ptr(), f_count.data_ptr(), f_loss.data_ptr(), status.data_ptr(),
                                      ws.data_ptr(), nbytes, L.stream_ptr().value), "fine_loss_batch")
    return f_loss, f_sum, f_count, status


@torch.no_grad()
def coarse_loss_batch(tgt_feats, tgt_first, tgt_count, src_feats, src_first, src_count, max_t, max_s, gt_idx, gt_overlaps, gt_count,
                      positive_margin=0.1, negative_margin=1.4, positive_optimal=0.1, negative_optimal=1.4, log_scale=24.0,
                      positive_overlap=0.1):
    """CoarseMatchingLoss.forward (lib/loss.py:88-111 over weighted_circle_loss) of every pair of a batch.  Pair b owns rows
    [tgt_first[b], tgt_first[b] + tgt_count[b]) of tgt_feats and likewise of src_feats (at most max_t / max_s rows; both may be the
    same tensor); gt_idx (B, cap, 2) [tgt node, src node], gt_overlaps (B, cap), gt_count (B,).  Device tensors.
    Returns (c_loss, status), each (B,)."""
    i32, f32 = torch.int32, torch.float32
    tf, sf = A.dev(tgt_feats, f32, "tgt_feats"), A.dev(src_feats, f32, "src_feats")
    if tf.dim() != 2 or sf.dim() != 2 or tf.shape[1] != sf.shape[1]:
        raise L.RoitrError(f"coarse_loss_batch: descriptors {tuple(tf.shape)} / {tuple(sf.shape)}")
    t0, tc = A.dev(tgt_first, i32, "tgt_first").reshape(-1), A.dev(tgt_count, i32, "tgt_count").reshape(-1)
    s0, sc = A.dev(src_first, i32, "src_first").reshape(-1), A.dev(src_count, i32, "src_count").reshape(-1)
    B = int(t0.numel())
    gi, go, gc = A.dev(gt_idx, i32, "gt_idx"), A.dev(gt_overlaps, f32, "gt_overlaps"), A.dev(gt_count, i32, "gt_count").reshape(-1)
    if not (tc.numel() == s0.numel() == sc.numel() == gc.numel() == B) or gi.dim() != 3 or tuple(gi.shape) != (B, go.shape[-1], 2) or go.shape[0] != B:
        raise L.RoitrError(f"coarse_loss_batch: {B} pairs, gt_idx {tuple(gi.shape)}, gt_overlaps {tuple(go.shape)}")
    dev = tf.device
    c_loss, status = torch.empty((B,), dtype=f32, device=dev), torch.empty((B,), dtype=i32, device=dev)
    lib = L.lib()
    nbytes = int(lib.roitr_coarse_loss_workspace_bytes(B, int(max_t), int(max_s)))
    ws = A.workspace(nbytes, dev)
    L.check(lib.roitr_coarse_loss_batch(B, int(tf.shape[1]), tf.data_ptr(), int(tf.shape[0]), t0.data_ptr(), tc.data_ptr(), sf.data_ptr(),
                                        int(sf.shape[0]), s0.data_ptr(), sc.data_ptr(), int(max_t), int(max_s), int(go.shape[1]),
                                        gi.data_ptr(), go.data_ptr(), gc.data_ptr(), float(positive_margin), float(negative_margin),
                                        float(positive_optimal), float(negative_optimal), float(log_scale), float(positive_overlap),
                                        c_loss.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr().value),
            "coarse_loss_batch")
    return c_loss, status


def _circle_kw(cfg):
    return dict(positive_margin=_cfg(cfg, "coarse_loss_positive_margin"), negative_margin=_cfg(cfg, "coarse_loss_negative_margin"),
                positive_optimal=_cfg(cfg, "coarse_loss_positive_optimal"), negative_optimal=_cfg(cfg, "coarse_loss_negative_optimal"),
                log_scale=_cfg(cfg, "coarse_loss_log_scale"), positive_overlap=_cfg(cfg, "coarse_loss_positive_overlap"))


def _raise_on_bad(status, what):
    """The one host round trip of the single-pair forms (loss_batch leaves the status to its caller)."""
    bad = int(status.max().item()) if status.numel() else 0
    if bad & BAD_OFFSETS:
        raise L.RoitrError(f"{what}: a row or slot range leaves its buffer")
    if bad & BAD_INDEX:
        raise L.RoitrError(f"{what}: a ground-truth node index lies outside its cloud")


@torch.no_grad()
def loss_batch(handle, cfg):
    """OverallLoss of every pair of a RIGA_v2.launch_batch() handle, after finish_batch(handle) (an overfull 4DMatch call has been
    repeated into the handle by then), in the strided and the compacted patch layout alike.  Needs rot / trans in the pairs.
    Returns device tensors (loss, c_loss, f_loss, f_count, status), each (B,): loss = coarse_loss_weight * c_loss + fine_loss_weight *
    f_loss; status holds FINE_EMPTY / COARSE_EMPTY where a loss is NaN (the reference's mean of an empty selection)."""
    out, B, P, n4 = handle["out"], handle["B"], handle["P"], handle["n4"]
    rot, trans = handle_poses(handle, "loss_batch")
    n_corr = out["n_corr"]
    if "loss_index" not in handle:   # host-known layout of the call, built once per handle
        s, t = handle_starts(handle, "node")
        handle["loss_index"] = (t[:-1], t[1:] - t[:-1], s[:-1], s[1:] - s[:-1], _ints(np.arange(B) * P, n_corr.device))
    tgt_first, tgt_count, src_first, src_count, strided_first = handle["loss_index"]
    if handle["compacted"]:   # the selected patches of all pairs back to back (roitr_patch_offsets)
        first = torch.cumsum(n_corr, 0, dtype=torch.int32) - n_corr
        count = n_corr
    else:                     # patch p of pair b at slot b * P + p
        first = strided_first
        count = n_corr.clamp(max=P)
    f_loss, _, f_count, f_status = fine_loss_batch(first, count, out["tgt_knn_pts"], out["src_knn_pts"], out["tgt_knn_masks"],
                                                   out["src_knn_masks"], out["matching_scores"], rot, trans,
                                                   _cfg(cfg, "fine_loss_positive_radius"))
    c_loss, c_status = coarse_loss_batch(out["node_feats"], tgt_first, tgt_count, out["node_feats"], src_first, src_count, max(n4[B:]),
                                         max(n4[:B]), out["gt_corr_idx"], out["gt_corr_overlaps"], out["gt_corr_count"],
                                         **_circle_kw(cfg))
    loss = float(_cfg(cfg, "coarse_loss_weight")) * c_loss + float(_cfg(cfg, "fine_loss_weight")) * f_loss
    return loss, c_loss, f_loss, f_count, f_status | c_status


@torch.no_grad()
def weighted_circle_loss(pos_masks, neg_masks, feat_dists, pos_margin, neg_margin, pos_optimal, neg_optimal, log_scale, pos_scales=None,
                         neg_scales=None):
    """lib/loss.py:8-49 for arbitrary masks and scales, in torch on the tensors' device (the general form; CoarseMatchingLoss runs
    the kernel)."""
    row_masks = (pos_masks.sum(-1) > 0) & (neg_masks.sum(-1) > 0)
    col_masks = (pos_masks.sum(-2) > 0) & (neg_masks.sum(-2) > 0)
    pos_weights = torch.clamp_min(feat_dists - 1e5 * (~pos_masks).float() - pos_optimal, 0.0)
    if pos_scales is not None:
        pos_weights = pos_weights * pos_scales
    neg_weights = torch.clamp_min(neg_optimal - (feat_dists + 1e5 * (~neg_masks).float()), 0.0)
    if neg_scales is not None:
        neg_weights = neg_weights * neg_scales
    pos_term = log_scale * (feat_dists - pos_margin) * pos_weights
    neg_term = log_scale * (neg_margin - feat_dists) * neg_weights
    loss_row = torch.nn.functional.softplus(torch.logsumexp(pos_term, dim=-1) + torch.logsumexp(neg_term, dim=-1)) / log_scale
    loss_col = torch.nn.functional.softplus(torch.logsumexp(pos_term, dim=-2) + torch.logsumexp(neg_term, dim=-2)) / log_scale
    return (loss_row[row_masks].mean() + loss_col[col_masks].mean()) / 2


class WeightedCircleLoss(torch.nn.Module):
    def __init__(self, pos_margin, neg_margin, pos_optimal, neg_optimal, log_scale):
        super().__init__()
        self.pos_margin, self.neg_margin = pos_margin, neg_margin
        self.pos_optimal, self.neg_optimal = pos_optimal, neg_optimal
        self.log_scale = log_scale

    def forward(self, pos_masks, neg_masks, feat_dists, pos_scales=None, neg_scales=None):
        return weighted_circle_loss(pos_masks, neg_masks, feat_dists, self.pos_margin, self.neg_margin, self.pos_optimal, self.neg_optimal,
                                    self.log_scale, pos_scales=pos_scales, neg_scales=neg_scales)


class CoarseMatchingLoss(torch.nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.weighted_circle_loss = WeightedCircleLoss(*(_cfg(cfg, "coarse_loss_" + k) for k in
                                                         ("positive_margin", "negative_margin", "positive_optimal", "negative_optimal",
                                                          "log_scale")))
        self.positive_overlap = _cfg(cfg, "coarse_loss_positive_overlap")

    @torch.no_grad()
    def forward(self, output_dict):
        """lib/loss.py:88-111 on one pair's output dict: the batched kernel with one pair."""
        tgt, src = output_dict["tgt_node_feats"], output_dict["src_node_feats"]
        dev = tgt.device
        gi = output_dict["gt_node_corr_indices"].to(torch.int32).reshape(1, -1, 2)
        go = output_dict["gt_node_corr_overlaps"].reshape(1, -1)
        w = self.weighted_circle_loss
        c_loss, status = coarse_loss_batch(tgt, _ints([0], dev), _ints([tgt.shape[0]], dev), src, _ints([0], dev), _ints([src.shape[0]], dev),
                                           int(tgt.shape[0]), int(src.shape[0]), gi, go, _ints([gi.shape[1]], dev), w.pos_margin,
                                           w.neg_margin, w.pos_optimal, w.neg_optimal, w.log_scale, self.positive_overlap)
        _raise_on_bad(status, "CoarseMatchingLoss")
        return c_loss[0]


class FineMatchingLoss(torch.nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.positive_radius = _cfg(cfg, "fine_loss_positive_radius")

    @torch.no_grad()
    def forward(self, output_dict, data_dict):
        """lib/loss.py:119-143 on one pair's output dict: the batched kernel with one pair."""
        rot, trans = data_dict["rot"], data_dict["trans"]
        if rot.dim() == 3:
            rot, trans = rot[0], trans[0]
        scores = output_dict["matching_scores"]
        dev = scores.device
        f_loss, _, _, status = fine_loss_batch(_ints([0], dev), _ints([scores.shape[0]], dev), output_dict["tgt_node_corr_knn_points"],
                                               output_dict["src_node_corr_knn_points"], output_dict["tgt_node_corr_knn_masks"],
                                               output_dict["src_node_corr_knn_masks"], scores, rot.reshape(1, 3, 3), trans.reshape(1, 3),
                                               self.positive_radius)
        _raise_on_bad(status, "FineMatchingLoss")
        return f_loss[0]


class OverallLoss(torch.nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.coarse_loss = CoarseMatchingLoss(cfg)
        self.fine_loss = FineMatchingLoss(cfg)
        self.weight_coarse_loss = float(_cfg(cfg, "coarse_loss_weight"))
        self.weight_fine_loss = float(_cfg(cfg, "fine_loss_weight"))
        self.weight_occ_loss = float(_cfg(cfg, "occ_loss_weight"))

    def forward(self, output_dict, data_dict):
        coarse_loss = self.coarse_loss(output_dict)
        fine_loss = self.fine_loss(output_dict, data_dict)
        loss = self.weight_coarse_loss * coarse_loss + self.weight_fine_loss * fine_loss
        return {"loss": loss, "c_loss": coarse_loss, "f_loss": fine_loss, "o_loss": 0. * fine_loss}
