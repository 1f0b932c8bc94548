"""Register a pair list over a set of clouds with every cloud encoded once.

The 3DMatch / 3DLoMatch protocol registers every overlapping pair of a scene's fragments (each fragment takes part in ~7 pairs), loop
closure matches one cloud against dozens: `match_pairs` runs the per-cloud half of the model once per cloud
(RIGA_v2.encode_clouds) and the pair half once per pair (RIGA_v2.launch_match), in calls of `pairs_per_call` with two calls in flight.

    python -m roitr_amd.scene --clouds 16 --points 5000            # all pairs i < j of 16 synthetic clouds, pairs/s
"""
import argparse
import collections
import time


def chunk_pairs(pairs, pairs_per_call):
    """The pair list cut into calls: consecutive slices of at most pairs_per_call pairs, in list order."""
    n = int(pairs_per_call)
    if n < 1:
        raise ValueError(f"pairs_per_call must be >= 1, got {pairs_per_call}")
    pairs = list(pairs)
    return [pairs[i:i + n] for i in range(0, len(pairs), n)]


def match_pairs(model, clouds, pairs, pairs_per_call=512, clouds_per_call=128):
    """Yield (pair, result) for every (src_index, tgt_index) of `pairs`, in list order.  `clouds`: the list of cloud dicts
    RIGA_v2.encode_clouds takes (encoded here, once) or an EncodedClouds made earlier.  Two match calls are kept in flight: call s + 1
    is queued before the host waits for call s, so the device does not idle while the results of s are unpacked."""
    calls = chunk_pairs(pairs, pairs_per_call)
    if not calls:
        return
    enc = clouds if hasattr(clouds, "table") else model.encode_clouds(clouds, clouds_per_call=clouds_per_call)
    flight = collections.deque()
    for call in calls:
        flight.append((call, model.launch_match(enc, call)))
        if len(flight) == 2:
            done, handle = flight.popleft()
            yield from zip(done, model.finish_batch(handle))
    while flight:
        done, handle = flight.popleft()
        yield from zip(done, model.finish_batch(handle))


def synthetic_scene(n_clouds, n_points, config=2):
    """Cloud dicts on the device: the sources and targets of synthetic.make_pair(n_points, config, pair_index = i, normals='field')."""
    import numpy as np
    import torch
    from .synthetic import make_pair
    clouds = []
    for i in range((n_clouds + 1) // 2):
        p = make_pair(n_points, config=config, pair_index=i, normals="field")
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        clouds.append(dict(points=dev(p["raw_src_pcd"]), points_out=dev(p["src_points"]), normals=dev(p["src_normals"]), feats=dev(p["src_feats"])))
        clouds.append(dict(points=dev(p["tgt_points"]), normals=dev(p["tgt_normals"]), feats=dev(p["tgt_feats"])))
    return clouds[:n_clouds]


def main(argv=None):
    import torch
    from .harness import build_model
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clouds", type=int, default=16)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--pairs-per-call", type=int, default=512)
    args = ap.parse_args(argv)
    model = build_model("3DMatch", weights="selective")
    clouds = synthetic_scene(args.clouds, args.points)
    pairs = [(i, j) for i in range(args.clouds) for j in range(i + 1, args.clouds)]
    with torch.no_grad():
        for _ in range(2):   # the first pass sizes the engine's scratch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n_corr = sum(int(res["corr_scores"].shape[0]) for _, res in match_pairs(model, clouds, pairs, args.pairs_per_call))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
    print(f"{len(pairs)} pairs over {args.clouds} clouds of {args.points} points: {len(pairs) / dt:.0f} pairs/s "
          f"(encode included), {n_corr} correspondences")


if __name__ == "__main__":
    main()
