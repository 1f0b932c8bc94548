"""A/B of the test-mode command line between two trees (a parent checkout and a branch, both built):

    python scripts/tester_ab.py --parent ../parent --branch . [--out profiles/tester_stages_refactor.txt] [--timing 5]

Every `python -m roitr_amd.main` line of README.md runs from both trees at --synthetic 4 --n-points 2000 (plus one line with every
option on and one where the point cap bites), each run a process of its own under its own time limit.  Compared: stdout line by line
(only the snapshot directory is masked), every .pth file key by key (same keys in the same order, torch.equal, nan-aware) and the
--write-gt files byte by byte.  With two visible devices the same runs are repeated under torch.distributed.run with two ranks.
--timing N: the wall time of one everything-on run of 64 pairs x 5000 points, parent and branch alternating, N runs each.
The first run that fails, differs in its exit status or runs into its time limit ends the script: nothing is started after it."""
import argparse
import os
import re
import shlex
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERYTHING = ("roitr_amd/configs/tdmatch_test.yaml --closed-form-weights --estimator compat --refine plane --recall --descriptor-eval "
              "--validate --fpfh-baseline --write-gt snapshot/gt")
EXTRA = (EVERYTHING, "roitr_amd/configs/tdmatch_test.yaml --closed-form-weights --evaluate --voxel-size 0.05 --points-lim 1000")


def readme_lines():
    """The option lines of README.md's `python -m roitr_amd.main` examples, without their comments, sizes and output places."""
    out = []
    for line in open(os.path.join(ROOT, "README.md")):
        if line.startswith("python -m roitr_amd.main "):
            out.append(line.split("#")[0].split("roitr_amd.main ", 1)[1].strip())
    return out


def command(options, out_dir, pairs, points, ranks):
    args = shlex.split(re.sub(r"--(synthetic|n-points) \S+", "", options))
    if "--write-gt" in args:
        args[args.index("--write-gt") + 1] = os.path.join(out_dir, "gt")
    launch = ["-m", "roitr_amd.main"] if ranks == 1 else ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}",
                                                          "--master-addr", "127.0.0.1", "--master-port", "29541", "-m", "roitr_amd.main"]
    return [sys.executable] + launch + args + ["--synthetic", str(pairs), "--n-points", str(points), "--snapshot-dir", out_dir]


def run(tree, options, out_dir, pairs, points, ranks, limit):
    """(stdout lines with the snapshot directory masked, seconds) of one run from `tree`; ends the script if the run does not end well."""
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    t0 = time.perf_counter()
    try:
        r = subprocess.run(command(options, out_dir, pairs, points, ranks), cwd=tree, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"STOP: no end within {limit} s: {tree}: {options}")
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit(f"STOP: exit status {r.returncode}: {tree}: {options}\n{r.stderr[-3000:]}")
    return [line.replace(out_dir, "<snapshot>") for line in r.stdout.splitlines()], dt


def same_value(a, b):
    import torch
    if torch.is_tensor(a) and torch.is_tensor(b):
        if a.dtype != b.dtype or a.shape != b.shape:
            return False
        return torch.equal(a, b) or (a.is_floating_point() and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num()))
    return type(a) is type(b) and a == b


def compare_files(dir_a, dir_b):
    """Differences between the result files of two runs, as strings; the number of files and keys compared."""
    import torch
    diffs, n_files, n_keys = [], 0, 0
    walk = lambda d: sorted(os.path.relpath(os.path.join(p, f), d) for p, _, fs in os.walk(d) for f in fs)
    if walk(dir_a) != walk(dir_b):
        return [f"file lists differ: {walk(dir_a)} != {walk(dir_b)}"], 0, 0
    for rel in walk(dir_a):
        n_files += 1
        if not rel.endswith(".pth"):
            if open(os.path.join(dir_a, rel), "rb").read() != open(os.path.join(dir_b, rel), "rb").read():
                diffs.append(f"{rel}: bytes differ")
            continue
        a, b = torch.load(os.path.join(dir_a, rel)), torch.load(os.path.join(dir_b, rel))
        if list(a) != list(b):
            diffs.append(f"{rel}: keys {list(a)} != {list(b)}")
            continue
        n_keys += len(a)
        diffs += [f"{rel}: {k} differs" for k in a if not same_value(a[k], b[k])]
    return diffs, n_files, n_keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--branch", default=ROOT)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--timing", type=int, default=0, help="timed everything-on runs per tree (0: none)")
    ap.add_argument("--limit", type=float, default=180.0, help="time limit of one run, seconds")
    ap.add_argument("--skip-ab", action="store_true", help="only the timing")
    args = ap.parse_args()
    trees = {"parent": os.path.abspath(args.parent), "branch": os.path.abspath(args.branch)}
    devices = int(subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True,
                                 timeout=120).stdout.strip() or 0)
    report = [f"tester A/B, parent against branch, {devices} visible device(s); every line below ran at --synthetic 4 --n-points 2000"]

    def say(line):
        report.append(line)
        print(line, flush=True)
        if args.out:
            open(args.out, "w").write("\n".join(report) + "\n")

    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for ranks in ([] if args.skip_ab else [1, 2] if devices >= 2 else [1]):
            for n, options in enumerate(readme_lines() + list(EXTRA)):
                got = {}
                for name, tree in trees.items():
                    out_dir = os.path.join(tmp, f"r{ranks}_{n}_{name}")
                    got[name] = run(tree, options, out_dir, 4, 2000, ranks, args.limit) + (out_dir,)
                (la, ta, da), (lb, tb, db) = got["parent"], got["branch"]
                diffs, n_files, n_keys = compare_files(da, db)
                lines = [f"stdout line {i}: {x!r} != {y!r}" for i, (x, y) in enumerate(zip(la, lb)) if x != y]
                if len(la) != len(lb):
                    lines.append(f"stdout: {len(la)} lines != {len(lb)} lines")
                bad += bool(diffs or lines)
                say(f"[{ranks} rank(s)] {options}\n    stdout: {len(la)} lines, {'identical' if not lines else 'DIFFERENT'}; files: {n_files} "
                    f"({n_keys} keys), {'identical' if not diffs else 'DIFFERENT'}; wall {ta:.1f} s / {tb:.1f} s")
                for d in lines + diffs:
                    say("    " + d)
                shutil.rmtree(da), shutil.rmtree(db)
        if devices < 2 and not args.skip_ab:
            say("two ranks: NOT RUN, this machine shows fewer than two devices")
        if args.timing:
            times = {"parent": [], "branch": []}
            for k in range(args.timing):
                for name, tree in trees.items():
                    times[name].append(run(tree, EVERYTHING, os.path.join(tmp, f"t{k}_{name}"), 64, 5000, 1, 4 * args.limit)[1])
                    shutil.rmtree(os.path.join(tmp, f"t{k}_{name}"))
                    print(f"timing run {k} {name}: {times[name][-1]:.2f} s", flush=True)
            p, b = times["parent"], times["branch"]
            say(f"timing, everything on, 64 pairs x 5000 points, wall seconds of the whole process, parent and branch alternating:\n"
                f"    parent {' '.join(f'{x:.2f}' for x in p)}  median {statistics.median(p):.2f}  range {min(p):.2f} .. {max(p):.2f}\n"
                f"    branch {' '.join(f'{x:.2f}' for x in b)}  median {statistics.median(b):.2f}  range {min(b):.2f} .. {max(b):.2f}\n"
                f"    branch median not above the parent's range: {statistics.median(b) <= max(p)}")
    if not args.skip_ab:
        say(f"result: {'ALL IDENTICAL' if not bad else f'{bad} run(s) DIFFER'}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
