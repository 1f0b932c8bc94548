"""The existing forward path of two built trees (a parent checkout and this one) side by side: `bench.py --dump-outputs` of both,
every dumped file compared byte for byte, and the headline of both in alternating runs, each a process of its own under its own time
limit.  Written for changes that must leave the forward as it is: the record says whether the files are
identical and whether the tree's headline lies inside the band the parent's own runs span.

    python scripts/forward_ab.py --parent ../parent [--branch .] [--rounds 3] [--steps 20] [--warmup 5] [--out profiles/scene_forward_ab.json]

The first run that fails or runs into its time limit ends the script: nothing is started after it."""
import argparse
import filecmp
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(tree, steps, warmup, dump, limit):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)] + (["--dump-outputs", dump] if dump else [])
    r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"bench.py failed in {tree} with status {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="a built checkout of the parent commit")
    ap.add_argument("--branch", default=ROOT)
    ap.add_argument("--rounds", type=int, default=3, help="runs per tree, alternating parent, branch, parent, ...")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=280, help="seconds per bench.py process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_forward_ab.json"))
    args = ap.parse_args()
    trees = {"parent": os.path.abspath(args.parent), "branch": os.path.abspath(args.branch)}
    values = {k: [] for k in trees}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(args.rounds):
            for name, tree in trees.items():
                dump = os.path.join(tmp, name) if r == 0 else None   # the first run of each tree also dumps its last step's results
                line = bench(tree, args.steps, args.warmup, dump, args.limit)
                values[name].append(line["value"])
                print(name, r, line["value"], line.get("unit"), flush=True)
        files = {k: sorted(os.listdir(os.path.join(tmp, k))) for k in trees}
        differing = [f for f in files["parent"] if f not in files["branch"] or
                     not filecmp.cmp(os.path.join(tmp, "parent", f), os.path.join(tmp, "branch", f), shallow=False)]
        identical = files["parent"] == files["branch"] and not differing and len(files["parent"]) > 0
    med = lambda v: sorted(v)[len(v) // 2]
    lo, hi = min(values["parent"]), max(values["parent"])
    result = dict(what="bench.py --gpus 1 --steps %d --warmup %d from the parent commit and from this tree, alternating, one process per run" % (args.steps, args.warmup),
                  dump_outputs=dict(files=len(files["parent"]), identical=bool(identical), differing=differing),
                  headline_pairs_per_s=dict(parent=values["parent"], branch=values["branch"], parent_median=med(values["parent"]), branch_median=med(values["branch"]),
                                            branch_over_parent=round(med(values["branch"]) / med(values["parent"]), 4),
                                            parent_band=[lo, hi], parent_spread_rel=round((hi - lo) / med(values["parent"]), 4),
                                            branch_median_not_below_parent_band=bool(med(values["branch"]) >= lo)))
    print(json.dumps(result), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not identical:
        raise SystemExit("the dumped outputs differ: " + ", ".join(differing[:8]))


if __name__ == "__main__":
    main()
