"""Times the validation losses (loss.loss_batch: the batched kernels of csrc/loss.hip) against the baseline a
user has without them: a straight torch port of lib/loss.py's two formulas, pair by pair, on the same device buffers.  Device events
around the whole call, the median of 20 after 5 warm-up calls.  The buffers are seeded stand-ins with the engine's shapes (a
launch_batch handle holds nothing else that loss_batch reads), so no forward has to run.

Cases: 3DMatch (512 pairs x 256 patches, L = 64, strided slots), 4DMatch (64 pairs, ~1000 selected patches each, compacted slots),
single (one pair).  Printed per case: ms, GB/s on the algorithmic bytes (every live matching_scores entry, point and mask once, the
node descriptors and the ground-truth lists once) and that rate's share of the MI355X's 8 TB/s.

    python scripts/bench_loss.py [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_GBS = 8000.0   # HBM3E peak of the MI355X, as in README.md
CASES = [("3DMatch", 512, 256, False), ("4DMatch", 64, 1000, True), ("single", 1, 256, False)]
N_TGT, N_SRC, D, L, N_GT = 78, 125, 256, 64, 300


def timed(fn, warmup=5, reps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def make_handle(B, per_pair, compacted, seed):
    """A finished launch_batch handle's worth of buffers: what loss_batch reads, nothing else."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = lambda *s: torch.rand(s, device="cuda", generator=g)
    if compacted:
        n_corr = (per_pair * (0.5 + u(B))).to(torch.int32)
        P = N_TGT * N_SRC
    else:
        n_corr = torch.full((B,), per_pair, dtype=torch.int32, device="cuda")
        n_corr[B // 2] = per_pair // 2   # one pair with dead slots
        P = per_pair
    S = int(n_corr.sum()) if compacted else B * P
    centre = 0.4 * u(S, 1, 3) - 0.2
    tgt = centre + 0.16 * u(S, L, 3) - 0.08
    src = tgt[:, torch.randperm(L, device="cuda", generator=g)] + 0.06 * u(S, L, 3) - 0.03   # rot = identity, trans = 0
    feats = torch.nn.functional.normalize(u(B * (N_TGT + N_SRC), D) - 0.5, dim=1)
    cap = N_TGT * N_SRC
    n_gt = N_GT
    flat = torch.stack([torch.randperm(cap, device="cuda", generator=g)[:n_gt].sort().values for _ in range(B)])
    gt_idx = torch.zeros((B, cap, 2), dtype=torch.int32, device="cuda")
    gt_idx[:, :n_gt, 0], gt_idx[:, :n_gt, 1] = flat // N_SRC, flat % N_SRC
    gt_ov = torch.zeros((B, cap), device="cuda")
    gt_ov[:, :n_gt] = u(B, n_gt)
    out = dict(n_corr=n_corr, tgt_knn_pts=tgt, src_knn_pts=src, tgt_knn_masks=(u(S, L) < 0.85).to(torch.int32),
               src_knn_masks=(u(S, L) < 0.85).to(torch.int32), matching_scores=-12.0 * u(S, L + 1, L + 1) - 0.05, node_feats=feats,
               gt_corr_idx=gt_idx, gt_corr_overlaps=gt_ov, gt_corr_count=torch.full((B,), n_gt, dtype=torch.int32, device="cuda"))
    rot = torch.eye(3, device="cuda").repeat(B, 1, 1)
    trans = torch.zeros((B, 3), device="cuda")
    keep = (None, None, None, None, rot, trans)
    live = int(n_corr.sum())
    nbytes = live * ((L + 1) ** 2 * 4 + 2 * L * 16) + feats.numel() * 4 + B * n_gt * 12
    return dict(out=out, B=B, P=P, slots=S, compacted=compacted, n4=[N_SRC] * B + [N_TGT] * B, have_gt=True, keep=keep), nbytes


def torch_port(h, cfg):
    """lib/loss.py:88-143 in torch, pair by pair, on the handle's buffers: what a user would write today."""
    from roitr_amd.loss import DEFAULTS, weighted_circle_loss
    out, B, P = h["out"], h["B"], h["P"]
    n_corr = out["n_corr"].tolist()   # the host round trip such a port needs
    r2 = DEFAULTS["fine_loss_positive_radius"] ** 2
    res = []
    p0 = 0
    for b in range(B):
        nc = n_corr[b]
        lo = p0 if h["compacted"] else b * P
        p0 += nc
        t, s = out["tgt_knn_pts"][lo:lo + nc], out["src_knn_pts"][lo:lo + nc] @ h["keep"][4][b].T + h["keep"][5][b]
        tm, sm = out["tgt_knn_masks"][lo:lo + nc].bool(), out["src_knn_masks"][lo:lo + nc].bool()
        scores = out["matching_scores"][lo:lo + nc]
        d = (-2.0 * t @ s.transpose(1, 2) + (t ** 2).sum(-1)[:, :, None] + (s ** 2).sum(-1)[:, None, :]).clamp_min(1e-12)
        gt = (d < r2) & tm[:, :, None] & sm[:, None, :]
        labels = torch.zeros_like(scores, dtype=torch.bool)
        labels[:, :-1, :-1] = gt
        labels[:, :-1, -1] = (gt.sum(2) == 0) & tm
        labels[:, -1, :-1] = (gt.sum(1) == 0) & sm
        f_loss = -scores[labels].mean()
        ft = out["node_feats"][B * N_SRC + b * N_TGT:B * N_SRC + (b + 1) * N_TGT]
        fs = out["node_feats"][b * N_SRC:(b + 1) * N_SRC]
        fd = torch.sqrt((-2.0 * ft @ fs.T + (ft ** 2).sum(-1)[:, None] + (fs ** 2).sum(-1)[None, :]).clamp_min(1e-12))
        ov = torch.zeros_like(fd)
        gi = out["gt_corr_idx"][b, :N_GT].long()
        ov[gi[:, 0], gi[:, 1]] = out["gt_corr_overlaps"][b, :N_GT]
        pos, neg = ov > DEFAULTS["coarse_loss_positive_overlap"], ov == 0
        c_loss = weighted_circle_loss(pos, neg, fd, 0.1, 1.4, 0.1, 1.4, 24, torch.sqrt(ov * pos))
        res.append((c_loss, f_loss))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from roitr_amd.loss import DEFAULTS, loss_batch
    rows = []
    for name, B, per_pair, compacted in CASES:
        h, nbytes = make_handle(B, per_pair, compacted, seed=B)
        kernel = lambda: loss_batch(h, DEFAULTS)
        port = lambda: torch_port(h, DEFAULTS)
        got, want = kernel(), port()
        c_ref, f_ref = torch.stack([w[0] for w in want]), torch.stack([w[1] for w in want])
        dev_c = float(((got[1] - c_ref).abs() / c_ref.abs()).nan_to_num(0).max())
        dev_f = float(((got[2] - f_ref).abs() / f_ref.abs()).nan_to_num(0).max())
        ms_k, ms_p = timed(kernel), timed(port)
        row = dict(case=name, pairs=B, patches=int(h["out"]["n_corr"].sum()), kernel_ms=ms_k, torch_port_ms=ms_p, speedup=ms_p / ms_k,
                   algorithmic_bytes=nbytes, kernel_gbs=nbytes / ms_k / 1e6, hbm_fraction=nbytes / ms_k / 1e6 / PEAK_GBS,
                   max_rel_dev_c_loss=dev_c, max_rel_dev_f_loss=dev_f)
        rows.append(row)
        print(f"{name:8s} {B:4d} pairs {row['patches']:7d} patches: loss_batch {ms_k:8.3f} ms  {row['kernel_gbs']:8.1f} GB/s "
              f"({row['hbm_fraction']:.3f} of {PEAK_GBS / 1000:g} TB/s)   torch port {ms_p:9.3f} ms   x{row['speedup']:.1f}   "
              f"largest relative difference to the port: c_loss {dev_c:.1e}, f_loss {dev_f:.1e}")
        del h
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
