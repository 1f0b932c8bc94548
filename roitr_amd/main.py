"""`python -m roitr_amd.main <config.yaml> [--pretrain ckpt.pth] [--synthetic N_PAIRS] [--n-points N]`

Test-mode entry mirroring main.py:16-139 of the reference for `mode: test`: load the flattened YAML config,
build the model, load the checkpoint, run the tester.  Under torch.distributed.run every rank takes its share of
the pairs (one process per GPU, RCCL for the final gather)."""
import argparse
import os

import torch

from .config import Config, load_config
from .riga import create_model, state_dict_layout
from .tester import SyntheticPairs, Tester, load_pretrain


def parser():
    """The command line of `python -m roitr_amd.main`."""
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--pretrain", default=None)
    ap.add_argument("--closed-form-weights", action="store_true",
                    help="ignore any checkpoint and fill the model with the deterministic closed-form weights of roitr_amd/weights.py "
                         "(parity / benchmark runs without a released checkpoint)")
    ap.add_argument("--synthetic", type=int, default=8, help="number of synthetic pairs (no datasets ship with this repo)")
    ap.add_argument("--n-points", type=int, default=5000)
    ap.add_argument("--snapshot-dir", default="snapshot")
    ap.add_argument("--pairs-per-forward", type=int, default=8)
    ap.add_argument("--evaluate", action="store_true", help="report mean PIR / IR (lib/loss.py Evaluator) computed on the device")
    ap.add_argument("--estimate-normals", action="store_true", help="recompute the normals on the GPU (open3d knn=33 + normal_redirect)")
    ap.add_argument("--register", action="store_true",
                    help="estimate every pair's pose on the GPU (--estimator: correspondence RANSAC, registration.py, local-to-global "
                         "registration, lgr.py, spatial-compatibility registration, compat.py, or fast global registration, fgr.py) and save "
                         "it as est_transform")
    ap.add_argument("--nonrigid", action="store_true",
                    help="synthetic 4DMatch-shaped pairs with a real deformation and metric points (synthetic.make_nonrigid_pair); "
                         "with --evaluate on a 4DMatch config the mean NFMR is reported (nonrigid.py)")
    ap.add_argument("--descriptor-eval", action="store_true",
                    help="with --evaluate: the descriptor-level inlier ratio without / with the mutual check and the feature-matching "
                         "recall at 0.05, from the point descriptors of every pair (descmatch.py)")
    ap.add_argument("--validate", action="store_true",
                    help="the reference's `val` report: mean loss, c_loss, f_loss, o_loss (lib/loss.py OverallLoss, computed on the device "
                         "by loss.py), PIR and IR over all pairs; implies --evaluate")
    ap.add_argument("--voxel-size", type=float, default=None,
                    help="voxel-grid downsample every cloud on the GPU first (metres; 0.025 is what the 3DMatch files went through); the "
                         "normals are then re-estimated on the new points")
    ap.add_argument("--points-lim", type=int, default=None,
                    help="cap every cloud at N points, uniform without replacement, on the GPU (the reference's points_lim / max_points)")
    ap.add_argument("--remove-outliers", choices=("statistical", "radius"), default=None,
                    help="remove flying pixels and isolated points on the GPU after the voxel grid and before the cap (prep.py): the "
                         "statistical filter (mean distance to --outlier-nn neighbours against the cloud's mean + --outlier-std sigma) or "
                         "the radius filter (more than --outlier-points points within --outlier-radius); the normals are then re-estimated")
    ap.add_argument("--outlier-nn", type=int, default=20, help="statistical filter: neighbours per point, the point included (2 .. 100)")
    ap.add_argument("--outlier-std", type=float, default=2.0, help="statistical filter: the threshold in standard deviations")
    ap.add_argument("--outlier-points", type=int, default=16, help="radius filter: a point stays with more than N points within the radius")
    ap.add_argument("--outlier-radius", type=float, default=0.05, help="radius filter: the radius (metres)")
    ap.add_argument("--subsample-seed", type=int, default=0, help="seed of the cap's counter-based stream")
    ap.add_argument("--recall", action="store_true",
                    help="the 3DMatch-protocol registration recall on the run's own pairs: overlap ratios and gt.info matrices computed "
                         "on the GPU (pairgt.py), RR overall and per overlap bin; implies --register and --evaluate")
    ap.add_argument("--overlap-radius", type=float, default=0.0375, help="radius of the ground-truth overlap / information matrix (metres)")
    ap.add_argument("--write-gt", default=None, metavar="DIR",
                    help="write gt.log, gt.info, gt_overlap.log and est.log for the run's pairs into DIR (the reference's benchmark() reads "
                         "them); pair k is the fragment pair (k, k + 2) behind one filler record, because the reference never tests the "
                         "record at index 0; implies --recall")
    ap.add_argument("--ransac-iterations", type=int, default=50000)
    ap.add_argument("--ransac-points", type=int, default=1000, help="correspondences drawn per pair (probability ~ confidence)")
    ap.add_argument("--estimator", choices=("ransac", "lgr", "compat", "fgr"), default="ransac",
                    help="pose estimator of --register: correspondence RANSAC, RANSAC-free local-to-global registration on the "
                         "matcher's patches, spatial-compatibility registration on the correspondences alone (both deterministic, "
                         "no random stream), or fast global registration: one robust objective, no hypotheses")
    ap.add_argument("--lgr-radius", type=float, default=0.1, help="acceptance radius of the lgr estimator (metres)")
    ap.add_argument("--lgr-steps", type=int, default=5, help="global reweighted solves of the lgr estimator")
    ap.add_argument("--compat-dist", type=float, default=0.1,
                    help="compat estimator: two correspondences are compatible when their point distances differ by less (metres)")
    ap.add_argument("--compat-seeds", type=int, default=64, help="compat estimator: hypotheses per pair (seeds by degree)")
    ap.add_argument("--compat-k", type=int, default=20, help="compat estimator: rows of a seed's consensus set")
    ap.add_argument("--fgr-max-dist", type=float, default=0.1, help="fgr estimator: the final scale of the robust cost (metres)")
    ap.add_argument("--fgr-iterations", type=int, default=128, help="fgr estimator: Gauss-Newton steps (1 .. 1024)")
    ap.add_argument("--fgr-tuples", type=int, default=0,
                    help="fgr estimator: triples drawn per pair for the tuple test (0: none), keyed on the global pair id")
    ap.add_argument("--refine", choices=("none", "point", "plane", "gicp"), default="none",
                    help="refine the estimated pose by ICP on the dense clouds (icp.py): point-to-point, or point-to-plane on the target "
                         "normals; gicp: generalized ICP, plane-to-plane on the normals of both clouds (gicp.py); implies --register")
    ap.add_argument("--icp-distance", type=float, default=0.05, help="maximum correspondence distance of the refinement (metres)")
    ap.add_argument("--icp-iterations", type=int, default=30)
    ap.add_argument("--gicp-epsilon", type=float, default=1e-3,
                    help="--refine gicp: the covariance eigenvalue along a point's normal, in [1e-6, 1] (1: isotropic points)")
    ap.add_argument("--fpfh-baseline", action="store_true",
                    help="with --evaluate and --register: also run the learning-free baseline on the same pairs (fpfh.py): FPFH "
                         "descriptors, mutual matches under the squared distance, the pose from --estimator (ransac, compat or fgr)")
    ap.add_argument("--fpfh-radius", type=float, default=0.125, help="FPFH neighbourhood radius (metres)")
    ap.add_argument("--fpfh-max-nn", type=int, default=100, help="FPFH neighbourhood size: the point and at most N - 1 neighbours (2 .. 100)")
    return ap


def outlier_options(args):
    """The Tester's `outlier` argument of the parsed command line (None: off)."""
    if args.remove_outliers == "statistical":
        return dict(method="statistical", nb_neighbors=args.outlier_nn, std_ratio=args.outlier_std)
    if args.remove_outliers == "radius":
        return dict(method="radius", nb_points=args.outlier_points, radius=args.outlier_radius)
    return None


def main():
    args = parser().parse_args()
    config = Config(load_config(args.config))
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group("nccl")
    model = create_model(config).cuda()
    ckpt = None if args.closed_form_weights else (args.pretrain or config.get("pretrain"))
    if ckpt:
        if not os.path.exists(ckpt):   # lib/trainer.py:128-130 _load_pretrain: raise ValueError('no checkpoint found')
            raise ValueError(f"=> no checkpoint found at '{ckpt}' (pass --closed-form-weights to run without one)")
        load_pretrain(model, ckpt)
    else:
        from .weights import closed_form_param
        sd = model.state_dict()
        for k, shape, kind in state_dict_layout(model.factor, model.architecture):
            if kind == "param":
                sd[k].copy_(torch.from_numpy(closed_form_param(k, tuple(shape))))
        print("[roitr_amd] no checkpoint given: using closed-form weights (roitr_amd/weights.py)")
    tester = Tester(config, model, SyntheticPairs(args.synthetic, args.n_points, nonrigid=args.nonrigid), args.snapshot_dir,
                    args.pairs_per_forward, rank, world, evaluate=args.evaluate, estimate_normals=args.estimate_normals,
                    register=args.register, ransac=dict(iterations=args.ransac_iterations, n_points=args.ransac_points),
                    descriptor_eval=args.descriptor_eval, validate=args.validate, voxel_size=args.voxel_size, points_lim=args.points_lim,
                    subsample_seed=args.subsample_seed, recall=args.recall, overlap_radius=args.overlap_radius, estimator=args.estimator,
                    lgr=dict(radius=args.lgr_radius, steps=args.lgr_steps), refine=None if args.refine == "none" else args.refine,
                    compat=dict(compat_dist=args.compat_dist, max_seeds=args.compat_seeds, k=args.compat_k),
                    fgr=dict(max_dist=args.fgr_max_dist, iterations=args.fgr_iterations, tuples=args.fgr_tuples),
                    icp=dict(max_dist=args.icp_distance, iterations=args.icp_iterations, **(dict(epsilon=args.gicp_epsilon) if args.refine == "gicp" else {})),
                    fpfh_baseline=dict(radius=args.fpfh_radius, max_nn=args.fpfh_max_nn) if args.fpfh_baseline else None, gt_dir=args.write_gt,
                    outlier=outlier_options(args))
    counts = tester.test()
    if rank == 0:
        print(*tester.report, f"[roitr_amd] wrote {args.synthetic} result files under {args.snapshot_dir}/{config.benchmark}; "
              f"correspondences per rank: {counts}", sep="\n")
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
