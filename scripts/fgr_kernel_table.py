"""profiles/fgr_kernels.csv from the kernel trace of `rocprofv3 --kernel-trace --stats -d DIR -o fgr --output-format csv -- python
scripts/bench_fgr.py --steps 3 --warmup 1 --only fgr --out DIR/bench.json`: the two FGR kernels per shape (the grid tells the number
of pairs) and kind of call.  The trace does not carry a kernel's arguments, so the solve launches of the 512-pair set, which
bench_fgr.py also runs at iterations 1 and 32, are told apart by their duration (below 100 us, below 600 us, above: the three differ by
more than a factor of 3), and a tuple launch with more than one block per pair is the one that draws.

    python scripts/fgr_kernel_table.py DIR/fgr_kernel_trace.csv [profiles/fgr_kernels.csv]
"""
import collections
import csv
import sys

SHAPES = {1: "1x1000", 64: "64x10000", 512: "512x1000"}


def table(trace):
    rows = collections.defaultdict(list)
    for r in csv.DictReader(open(trace)):
        name = r["Kernel_Name"]
        if "fgr_" not in name:
            continue
        blocks, pairs = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Grid_Size_Y"])
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "fgr_solve_kernel" in name:
            kernel, pairs = "fgr_solve_kernel", blocks
            call = "iterations 128" if pairs != 512 or us >= 600 else "iterations 1" if us < 100 else "iterations 32"
        else:
            kernel, call = "fgr_tuple_kernel", "tuples 131072" if blocks > 1 else "tuples 0"
        rows[(SHAPES.get(pairs, str(pairs)), kernel, call)].append(us)
    return rows


def main():
    out = sys.argv[2] if len(sys.argv) > 2 else "profiles/fgr_kernels.csv"
    with open(out, "w") as f:
        f.write("shape,kernel,call,calls,avg_us,min_us,max_us\n")
        for (shape, kernel, call), v in sorted(table(sys.argv[1]).items()):
            f.write(f"{shape},{kernel},{call},{len(v)},{sum(v) / len(v):.1f},{min(v):.1f},{max(v):.1f}\n")


if __name__ == "__main__":
    main()
