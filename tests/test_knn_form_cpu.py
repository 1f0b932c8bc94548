"""roitr_knn_form (include/roitr_pointops.h): the kernel form roitr_knnquery_ex / roitr_knn_within give a call, the list width of its
kernel template and the query sort, or the status the call is refused with.  The launcher dispatches through the same host function
(knn_plan, csrc/pointops_knn.hip), so what is pinned here is what runs.  Host code that follows no pointer: needs the built library,
no GPU.

The table is the one of DESIGN.md ("Forms of the kNN").  test_form_of_every_gpu_case takes the shapes of tests/test_knn_fused_gpu.py
from that module's own tables, so a later change of a threshold cannot silently move one of its cases to another kernel."""
import os
import re

import pytest

import knn_util as U
import test_knn_fused_gpu as G
from knn_util import ERR_ARG, FORM, ROOT, SORT, branch, knn_form

NONE, S4096, SMAX = SORT["NONE"], SORT["4096"], SORT["MAX"]


def test_form_names():
    assert FORM == {"NOTHING": 0, "BRUTE": 1, "LANE_BRUTE": 2, "LANE": 3, "PREFILTER": 4, "WITHIN": 5, "CELL": 6, "GRIDSEL": 7}
    assert SORT == {"NONE": 0, "4096": 1, "MAX": 2} and U.OUT == {"IDX": 1, "DIST2": 2, "GROUP": 4, "PPF": 8}


def test_design_table_lists_every_form():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = text[text.index("**Forms of the kNN.**"):]
    table = table[:table.index("\n\n", table.index("| form |"))]
    assert re.findall(r"^\| (\w+) \| (\d+) \|", table, re.M) == [(name, str(value)) for name, value in sorted(FORM.items(), key=lambda kv: kv[1])]


GPU = vars(G)   # the shape tables of the GPU module (importing it starts nothing on a GPU)


@pytest.mark.parametrize("case", G.CASES, ids=[f"{i}-{c[0]}" for i, c in enumerate(G.CASES)])
def test_form_of_every_gpu_case(case):
    name, use_grid, sizes, take, ns, _, _ = case
    n, m, b = sum(sizes), sum(take) if take else sum(sizes), len(sizes)
    assert branch(b, n, m, ns, use_grid, take is None) == name                      # the engine's call: group_idx + ppf
    assert knn_form(b, n, m, ns, use_grid, take is None, "idgp") == knn_form(b, n, m, ns, use_grid, take is None, "gp")


def test_the_other_gpu_cases():
    r8, rlb = sum(GPU["R8"]), sum(GPU["RLB"])
    assert knn_form(8, r8, r8, 2, True, True, "gp") == ("LANE", 4, NONE)            # test_knn_fused_one_column
    assert knn_form(256, rlb, rlb, 1, False, True, "id") == ("LANE_BRUTE", 2, NONE)  # test_knn_lane_brute_nsample_1
    # test_knn_ppf_without_group_idx: lane_emit reads the neighbours back from group_idx, so a lane-sized shape goes to a wave form
    assert knn_form(8, r8, r8, 17, True, True, "p") == ("CELL", 0, NONE)
    assert knn_form(256, rlb, rlb, 17, False, True, "p") == ("BRUTE", 1, NONE)
    assert knn_form(8, r8, r8, 17, True, True, "gp") == ("LANE", 18, NONE)
    assert knn_form(256, rlb, rlb, 17, False, True, "gp") == ("LANE_BRUTE", 18, NONE)
    assert knn_form(8, r8, 8 * 1100, 17, True, False, "p") == ("GRIDSEL", 0, NONE)   # ... and its queries are not sorted


def test_engine_call_pattern_cases():
    """test_knn_engine_call_pattern: 8 clouds of ~5000 / 1250 / 312 points per level, the level's self query (nsample 9, 17, 17) and the
    TransitionDown query of the next level's points (nsample 17); a grid at levels 0 and 1."""
    sizes = [U.ragged(8, 5000)]
    for _ in range(3):
        sizes.append([s // 4 for s in sizes[-1]])
    self_forms = (("PREFILTER", 10, NONE), ("LANE", 18, NONE), ("BRUTE", 1, NONE))
    td_forms = (("LANE", 18, S4096), ("GRIDSEL", 0, NONE), ("BRUTE", 1, NONE))
    for level in range(3):
        n, m, use_grid = sum(sizes[level]), sum(sizes[level + 1]), level < 2
        assert use_grid == (n > 768 * 8)
        assert knn_form(8, n, n, (9, 17, 17)[level], use_grid, True, "gp") == self_forms[level], level
        assert knn_form(8, n, m, 17, use_grid, False, "gp") == td_forms[level], level


def test_query_count_switch_points():
    for m, want in ((8191, "CELL"), (8192, "LANE")):                                # a lane per query from 8192 queries on a grid
        assert knn_form(4, m, m, 17, True, True)[0] == want
    assert knn_form(4, 20000, 8191, 17, True, False) == ("GRIDSEL", 0, NONE)
    assert knn_form(4, 20000, 8192, 17, True, False) == ("LANE", 18, S4096)
    for m, want in ((65535, ("BRUTE", 1, NONE)), (65536, ("LANE_BRUTE", 18, NONE))):  # ... from 65536 without one
        assert knn_form(256, m, m, 17, False, True) == want
        assert knn_form(256, 70000, m, 17, False, False) == want


def test_width_switch_points():
    """nsample + 1 against the list widths 2, 4, 10, 18, 34 of both lane families; from 35 the selection kernels (or the wave list)."""
    for need, width in ((2, 2), (3, 4), (4, 4), (5, 10), (10, 10), (11, 18), (18, 18), (19, 34), (34, 34)):
        ns = need - 1
        grid_form = "PREFILTER" if 5 <= need <= 10 else "LANE"
        assert knn_form(8, 10000, 10000, ns, True, True) == (grid_form, width, NONE), need
        assert knn_form(8, 20000, 10000, ns, True, False) == (grid_form, width, S4096), need
        assert knn_form(256, 70000, 70000, ns, False, True) == ("LANE_BRUTE", width, NONE), need
    assert knn_form(8, 10000, 10000, 34, True, True) == ("CELL", 0, NONE)           # nsample + 1 = 35
    assert knn_form(8, 20000, 10000, 34, True, False) == ("GRIDSEL", 0, S4096)      # the sort goes by the query count alone
    assert knn_form(256, 70000, 70000, 34, False, True) == ("BRUTE", 1, NONE)
    for ns, nr in ((63, 1), (64, 2), (100, 2)):                                     # the wave list: one register up to 64 entries
        assert knn_form(2, 550, 550, ns, False, True) == ("BRUTE", nr, NONE)


def test_cell_form_switch_points():
    for m in (3000, 10000):
        assert knn_form(2, m, m, 65, True, True) == ("CELL", 0, NONE)               # nsample - 1 = 64
        assert knn_form(2, m, m, 66, True, True) == ("GRIDSEL", 0, NONE)
        assert knn_form(2, m, m, 100, True, True) == ("GRIDSEL", 0, NONE)
    assert knn_form(2, 3000, 3000, 17, True, True) == ("CELL", 0, NONE)             # self ...
    assert knn_form(2, 3000, 3000, 17, True, False) == ("GRIDSEL", 0, NONE)         # ... or a subset of as many queries


@pytest.mark.parametrize("b", [1, 2, 8])
def test_query_sort_switch_point(b):
    """n = 6144 b: the cell cap of the grid the reference clouds were built with (the rule of roitr_knn_build_grid_ex)."""
    assert knn_form(b, 6144 * b, 9000, 17, True, False) == ("LANE", 18, S4096)
    assert knn_form(b, 6144 * b + 1, 9000, 17, True, False) == ("LANE", 18, SMAX)
    assert knn_form(b, 9000, 9000, 17, True, True) == ("LANE", 18, NONE)            # self queries come in the grid's own order


def test_legacy_entry_is_brute_only():
    """b == 0 (knnquery_cuda_launcher: no cloud count, no grid): the two forms without a grid."""
    for ns in (1, 9, 33, 64, 100):
        assert knn_form(0, 0, 5000, ns, False, False, "id") == ("BRUTE", 1 if ns + 1 <= 64 else 2, NONE)
    assert knn_form(0, 0, 65536, 9, False, False, "id") == ("LANE_BRUTE", 10, NONE)
    assert knn_form(0, 0, 65536, 64, False, False, "id") == ("BRUTE", 2, NONE)


def test_finite_cap():
    """roitr_knn_within: nsample 1, dist2 only, a finite cap."""
    assert knn_form(8, 20000, 10000, 1, True, False, "d", capped=True) == ("WITHIN", 0, S4096)
    assert knn_form(8, 10000, 10000, 1, True, True, "d", capped=True) == ("WITHIN", 0, NONE)
    assert knn_form(8, 20000, 10000, 1, True, False, "d") == ("LANE", 2, S4096)     # the same outputs, exact
    assert knn_form(8, 20000, 10000, 1, True, False, "id", capped=True) == ("LANE", 2, S4096)
    assert knn_form(8, 20000, 8191, 1, True, False, "d", capped=True) == ("GRIDSEL", 0, NONE)
    assert knn_form(8, 20000, 70000, 1, False, False, "d", capped=True) == ("LANE_BRUTE", 2, NONE)
    assert knn_form(8, 20000, 5000, 1, False, False, "d", capped=True) == ("BRUTE", 1, NONE)
    for ns in (4, 9):                                                               # the prefilter's radius rule is for the exact k
        assert knn_form(8, 10000, 10000, ns, True, True, "id", capped=True) == ("LANE", 10, NONE)
        assert knn_form(8, 10000, 10000, ns, True, True, "id") == ("PREFILTER", 10, NONE)


def test_nothing_to_do():
    for m in (0, -1):
        assert knn_form(8, 10000, m, 9, True, False) == ("NOTHING", 0, NONE)
        assert knn_form(8, 10000, m, 0, True, False, normals=False) == ("NOTHING", 0, NONE)   # as the launcher: before any refusal


@pytest.mark.parametrize("use_grid", [True, False])
def test_refusals(use_grid):
    for ns in (0, -1, 101):
        assert knn_form(8, 10000, 10000, ns, use_grid, True) == -ERR_ARG
    assert knn_form(8, 10000, 10000, 100, use_grid, True)[0] in ("GRIDSEL", "BRUTE")
    assert knn_form(8, 10000, 10000, 9, use_grid, True, "gp", normals=False) == -ERR_ARG
    assert knn_form(8, 10000, 10000, 9, use_grid, True, "p", normals=False) == -ERR_ARG
    assert knn_form(8, 10000, 10000, 9, use_grid, True, "idg", normals=False)[0] in ("PREFILTER", "BRUTE")
