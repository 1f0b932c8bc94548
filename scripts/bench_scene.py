"""Times a pair list that shares clouds, forwarded pair by pair against encoded once and matched.

Workload: 64 clouds of N = 5000 -- sources and targets of make_pair(5000, config=2, pair_index=i, normals="field"), i < 32 -- under the
selective closed-form weights; the pair list is all 2016 pairs i < j, in calls of 512.  Two arms in one process, alternating:

  (a) forward   RIGA_v2.launch_batch / finish_batch over the list: every call encodes its 1024 cloud slots again;
  (b) cached    RIGA_v2.encode_clouds once (part of the arm's time), then launch_match / finish_batch over the list.

Both arms keep two calls in flight.  Before anything is timed the first call of both arms is compared BITWISE, pair by pair and key by
key: a number from a wrong result is never written.  Device events around every arm and around single 512-pair calls; medians with
min - max over --runs repeats after --warmup.  The acceptance of the issue is checked and recorded, not assumed: a match call and arm (b)
as a whole both faster than the forward's in the same run, by more than arm (a)'s own min - max spread.

    python scripts/bench_scene.py [--runs 9] [--warmup 3] [--out profiles/scene_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_scene.py --only match --runs 3 --out DIR/trace_run.json
    python scripts/bench_scene.py --kernel-stats DIR/.../*_kernel_stats.csv --out profiles/scene_bench.json     # adds the kernels' shares
    python scripts/forward_ab.py --parent PARENT_TREE --out profiles/scene_forward_ab.json   # the existing path: dumps identical, headline in the parent's band
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("src_points", "tgt_points", "src_nodes", "tgt_nodes", "src_point_feats", "tgt_point_feats", "src_node_feats", "tgt_node_feats",
        "src_node_corr_indices", "tgt_node_corr_indices", "src_node_corr_knn_points", "tgt_node_corr_knn_points",
        "src_node_corr_knn_masks", "tgt_node_corr_knn_masks", "matching_scores", "tgt_corr_points", "src_corr_points", "corr_scores",
        "_src_node_knn_indices", "_tgt_node_knn_indices", "_node_corr_scores")
NEW_KERNELS = ("cache_gather_nodes_kernel", "cache_patch_gather_kernel")


def stats(ms):
    return dict(ms=round(float(np.median(ms)), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), runs=len(ms))


def forward_pair(clouds, s, t):
    cs, ct = clouds[s], clouds[t]
    return dict(src_pcd=cs["points"], src_raw_pcd=cs["points"], src_normals=cs["normals"], src_feats=cs["feats"],
                tgt_pcd=ct["points"], tgt_normals=ct["normals"], tgt_feats=ct["feats"])


def in_flight(launch, finish, calls, sink):
    """Every call launched, two in flight, every result handed to `sink`."""
    prev = None
    for call in calls:
        h = launch(call)
        if prev is not None:
            sink(finish(prev))
        prev = h
    sink(finish(prev))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def kernel_shares(path, match_call_ms):
    """The two new kernels in a rocprofv3 --kernel-trace --stats run of `--only match` (one encode, then match calls of 512 pairs, one
    launch of each kernel per call): ms per launch, and that as a share of the event-timed match call of the untraced run.  The
    trace's own total also holds the encode and the model set-up, so the share of it is given for what it is."""
    rows = list(csv.DictReader(open(path)))
    name = next(k for k in rows[0] if k.lower() in ("name", "kernelname", "kernel_name"))
    dur = next(k for k in rows[0] if k.lower() in ("totaldurationns", "total_duration_ns", "totaldurationns "))
    total = sum(float(r[dur]) for r in rows)
    out = {"kernel_time_ms_in_trace": round(total / 1e6, 3)}
    for kn in NEW_KERNELS:
        ns = sum(float(r[dur]) for r in rows if kn in r[name])
        calls = sum(int(r.get("Calls", 0) or 0) for r in rows if kn in r[name])
        per = ns / 1e6 / max(1, calls)
        out[kn] = dict(ms_per_launch=round(per, 4), launches=calls, share_of_match_call=round(per / match_call_ms, 5) if match_call_ms else None,
                       share_of_all_kernel_time_in_trace=round(ns / total, 5))
    top = sorted(rows, key=lambda r: -float(r[dur]))[:6]
    out["top_kernels"] = [dict(name=r[name][:80], share=round(float(r[dur]) / total, 4)) for r in top]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3, help="untimed passes over everything the timed window runs (arenas and the allocator's pools grow in the first ones)")
    ap.add_argument("--clouds", type=int, default=64)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--pairs-per-call", type=int, default=512)
    ap.add_argument("--only", choices=("match",), default=None, help="encode once, then match calls alone (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *_kernel_stats.csv of an --only match run: adds the new kernels' shares to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_bench.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        result = json.load(open(args.out))
        result["match_call_kernel_trace"] = kernel_shares(args.kernel_stats, result.get("ms_per_call_of_512", {}).get("match", {}).get("ms"))
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result["match_call_kernel_trace"]))
        return
    assert args.runs >= (5 if args.only is None else 1), "each arm runs at least 5 times"
    from roitr_amd.harness import build_model
    from roitr_amd.scene import chunk_pairs, synthetic_scene
    torch.cuda.set_device(0)
    model = build_model("3DMatch", weights="selective")
    clouds = [dict(c) for c in synthetic_scene(args.clouds, args.points)]
    for c in clouds:
        c.pop("points_out", None)          # every cloud is a target somewhere: one coordinate set, as the forward has for targets
    pairs = [(i, j) for i in range(args.clouds) for j in range(i + 1, args.clouds)]
    calls = chunk_pairs(pairs, args.pairs_per_call)
    fwd_calls = [[forward_pair(clouds, s, t) for s, t in call] for call in calls]
    n_sink = [0]

    def sink(results):
        n_sink[0] += sum(int(r["corr_scores"].shape[0]) for r in results[:1])   # touch a result; the unpacking itself is in the arm

    def arm_forward():
        in_flight(lambda c: model.launch_batch(c, want_gt=False), model.finish_batch, fwd_calls, sink)

    def arm_cached():
        enc = model.encode_clouds(clouds)
        in_flight(lambda c: model.launch_match(enc, c), model.finish_batch, calls, sink)
        return enc

    with torch.no_grad():
        enc = model.encode_clouds(clouds)
        if args.only == "match":
            for _ in range(args.runs):
                in_flight(lambda c: model.launch_match(enc, c), model.finish_batch, calls[:1], sink)
            torch.cuda.synchronize()
            json.dump(dict(only="match", runs=args.runs, pairs=len(calls[0])), open(args.out, "w"))
            return
        # ---- the correctness guard: the first call of both arms, bitwise
        fwd = model.forward_batch(fwd_calls[0], want_gt=False)
        got = model.match_batch(enc, calls[0])
        for j, (a, b) in enumerate(zip(got, fwd)):
            for k in KEYS:
                assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (j, calls[0][j], k)
        n_corr = [int(r["corr_scores"].shape[0]) for r in fwd]
        assert min(n_corr) > 0, "a pair of the first call has no correspondences: the guard compares nothing there"
        guard = dict(pairs_compared=len(got), keys=len(KEYS), bitwise_equal=True, correspondences_min=min(n_corr), correspondences_mean=round(float(np.mean(n_corr)), 1))
        print(json.dumps(guard), flush=True)
        del fwd, got
        # ---- warm-up of every shape the timed window uses, then the arms alternating
        for _ in range(args.warmup):   # every call the timed window makes, the single calls and the encode included
            arm_forward()
            arm_cached()
            model.finish_batch(model.launch_batch(fwd_calls[0], want_gt=False))
            model.finish_batch(model.launch_match(enc, calls[0]))
            model.encode_clouds(clouds)
        ms = {k: [] for k in ("forward_list", "cached_list", "forward_call", "match_call", "encode")}
        for _ in range(args.runs):
            ms["forward_list"].append(timed(arm_forward)[0])
            ms["cached_list"].append(timed(arm_cached)[0])
            ms["forward_call"].append(timed(lambda: model.finish_batch(model.launch_batch(fwd_calls[0], want_gt=False)))[0])
            ms["match_call"].append(timed(lambda: model.finish_batch(model.launch_match(enc, calls[0])))[0])
            ms["encode"].append(timed(lambda: model.encode_clouds(clouds))[0])
    st = {k: stats(v) for k, v in ms.items()}
    spread_list = st["forward_list"]["ms_max"] - st["forward_list"]["ms_min"]
    spread_call = st["forward_call"]["ms_max"] - st["forward_call"]["ms_min"]
    accept = dict(
        match_call_faster_than_forward_call_by_more_than_its_spread=bool(st["forward_call"]["ms"] - st["match_call"]["ms"] > spread_call),
        cached_list_faster_than_forward_list_by_more_than_its_spread=bool(st["forward_list"]["ms"] - st["cached_list"]["ms"] > spread_list),
        forward_call_spread_ms=round(spread_call, 3), forward_list_spread_ms=round(spread_list, 3))
    result = dict(metric="encode_once_match_many", device=torch.cuda.get_device_name(0), clouds=args.clouds, points=args.points, pairs=len(pairs),
                  pairs_per_call=args.pairs_per_call, calls=[len(c) for c in calls], runs=args.runs, warmup=args.warmup,
                  timing="device events around each arm / call, host unpacking of the results included; arms alternate in one process",
                  guard=guard,
                  ms_per_call_of_512=dict(forward=st["forward_call"], match=st["match_call"],
                                          forward_over_match=round(st["forward_call"]["ms"] / st["match_call"]["ms"], 2)),
                  encode_ms=st["encode"], list_ms=dict(forward=st["forward_list"], cached_with_encode=st["cached_list"],
                                                      forward_over_cached=round(st["forward_list"]["ms"] / st["cached_list"]["ms"], 2)),
                  pairs_per_s=dict(forward=round(1e3 * len(pairs) / st["forward_list"]["ms"], 1), cached_with_encode=round(1e3 * len(pairs) / st["cached_list"]["ms"], 1)),
                  cache_bytes_per_cloud=int(enc.nbytes // len(enc)), cache_bytes=int(enc.nbytes),
                  estimate_before_measuring="a match call roughly a third of a forward call (published phase times: 14.6 + 11.5 ms of 81.5 ms, less geo_table's 5.7 ms)",
                  acceptance=accept)
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    assert all(v for k, v in accept.items() if k.endswith("spread")), accept


if __name__ == "__main__":
    main()
