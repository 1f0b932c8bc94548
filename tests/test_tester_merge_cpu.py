"""CPU, world_size 2 over gloo (the launcher of test_shard_cpu.py): tester.merge_rows, the one collective of a Tester run besides the
record gather.  Two ranks hold disjoint pair ids for two stages and rank 1 holds nothing for a third; both end with the same merged
dicts, rank by rank, and neither waits for the other."""
import textwrap

import test_shard_cpu as shard_cpu

WORKER = textwrap.dedent("""
    import os, sys, json
    sys.path.insert(0, %r)
    import torch.distributed as dist
    from roitr_amd.shard import pairs_for_rank
    from roitr_amd.tester import merge_rows
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    mine = pairs_for_rank(5, rank, world)                                   # rank 0: 0, 2, 4; rank 1: 1, 3
    local = {"descriptor": {i: (0.5 * i, float("nan") if i == 3 else 0.25 * i, i) for i in mine},
             "pose": {i: ((1.0 + i, 0.1 * i, 10 * i), None) for i in mine},
             "nonrigid": {i: (0.125 * i, 7) for i in mine} if rank == 0 else {}}       # rank 1 has no rows for this stage
    merged = merge_rows(local, world)
    out = {"rank": rank, "names": list(merged), "ids": {name: list(rows) for name, rows in merged.items()},
           "rows": {name: {str(k): repr(v) for k, v in rows.items()} for name, rows in merged.items()}}
    open(os.path.join(os.environ["RESULT_DIR"], f"rank{rank}.json"), "w").write(json.dumps(out))
    dist.destroy_process_group()
""") % shard_cpu.ROOT


def test_two_process_merge_gloo(tmp_path):
    script = tmp_path / "merge_worker.py"
    script.write_text(WORKER)
    by_rank = shard_cpu._torchrun(script, 29535)           # a rank that hung would run into the launcher's time limit
    a, b = by_rank[0], by_rank[1]
    assert a["names"] == b["names"] == ["descriptor", "pose", "nonrigid"]
    assert a["ids"] == b["ids"] == {"descriptor": [0, 2, 4, 1, 3], "pose": [0, 2, 4, 1, 3], "nonrigid": [0, 2, 4]}   # rank by rank
    assert a["rows"] == b["rows"]
    assert a["rows"]["descriptor"]["3"] == "(1.5, nan, 3)" and a["rows"]["pose"]["4"] == "((5.0, 0.4, 40), None)"
    assert a["rows"]["nonrigid"] == {"0": "(0.0, 7)", "2": "(0.25, 7)", "4": "(0.5, 7)"}


def test_one_process_merge_is_the_identity():
    from roitr_amd.tester import merge_rows
    local = {"descriptor": {0: (0.5, 0.25, 3)}, "nonrigid": {}}
    assert merge_rows(local, 1) is local
