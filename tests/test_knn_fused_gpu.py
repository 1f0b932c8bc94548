"""The fused outputs of the kNN (group_idx, ppf) in every kernel form of roitr_knnquery_ex, asked for the way the engine asks.

issue_geometry_chain (engine.cpp) never takes idx / dist2: it takes group_idx (columns 1.. of the row) and the fused PPF, with query
normals from another array than the reference normals, from a grid built once per level (m_capacity = the level above) and queried
several times out of one workspace.  Four pieces of pointops_knn.hip write a result row -- write_rows (wave-per-query kernels), the
cell kernel's own epilogue, lane_emit (lane-per-query kernels; reads group_idx back from global memory for the PPF) and write_rows<2>
behind the replay heap (every query with equal distances among its best nsample + 1) -- and every row comes from one of them.

Reference: oracle.pointops_cpu.knnquery_raw for the indices (group_idx == idx[:, 1:] bit for bit), a float64 restatement of
calc_ppf_gpu on the oracle's indices for the PPF (knn_util.ppf_ref), bounds of test_ppf_against_float64: |d| within 1e-6 max(1, |d|),
angles / pi within 5e-7 where the float64 angle lies in (1e-3, 1 - 1e-3), 2e-4 elsewhere.  Every case makes the engine's call
(group_idx + ppf only) and the call with all four outputs from the same workspace: same group_idx and ppf bits, idx / dist2 equal to
the oracle.  Outputs are pre-filled with NaN / -1 and followed by guard elements (knn_util.Grid.query).  Measured on MI355X over all
cases of this module: |d| within 1.9e-7 max(1, |d|), angles / pi within 1.3e-7 (generic or not) -- what an fp32 numpy evaluation of
the same formula gives on the same inputs (1.8e-7, 1.3e-7): the bounds set for ppf.hip hold for the fused epilogues as they stand.

Dispatch branch of knnquery_impl -> the shape that reaches it here -> the epilogue behind it (uniform clouds | lattice, dup clouds:
nearly every query tied, so the rows come from knn_replay_kernel's write_rows<2>):

  knn_brute_kernel<1>             no grid, clouds [300, 77, 5] (5 < nsample: fill slots), nsample 9, 17          write_rows<1>
  knn_brute_kernel<2>             no grid, [400, 150], nsample 65, 100                                           write_rows<2>
  knn_lane_brute_kernel<4/10/18/34>  no grid, >= 65536 queries: 256 clouds x ~260 self, nsample 3 / 9 / 17 / 33; one cloud of
                                  1100 points (several staging chunks); 352 x ~250 references, 190 of each as queries  lane_emit
  knn_lane_kernel<4>              grid, 8 x ~1250 self, nsample 3 (and 2: one output column)                     lane_emit
  knn_prefilter_kernel<10,40> + knn_lane_kernel<10> on its retry list
                                  grid, 8 x ~1250 self / 1100 of each as queries, nsample 9, 5                   lane_emit (both)
  knn_lane_kernel<18>, <34>       grid, 8 x ~1250 self / 1100 of each as queries, nsample 17, 33                 lane_emit
  sort_queries_kernel<4096>       every subset case above on a grid (n <= 6144 b)
  sort_queries_kernel<GRID_MAX_CELLS>  grid, 2 x ~9000 references (n > 6144 b), 4100 of each as queries, nsample 17  lane_emit
  knn_cell_kernel + knn_gridsel_kernel on its retry list
                                  grid, self, < 8192 queries: [3000], [700, 3100], nsample 9, 17, 65             the cell kernel's
                                                                                                epilogue, write_rows (retries)
                                  (uniform clouds of these sizes fill no retry list -- ROITR_KNN_STATS counted 0 of 27200 queries;
                                  the `clustered` clouds hand 7716 of 13600 over, of which the selection kernel passes the densest
                                  on to the replay; the prefilter hands 212 of 75056 uniform queries to its ring kernel)
  knn_gridsel_kernel alone        grid, references [5000], 1250 of them as queries, nsample 17; self [2000], nsample 100  write_rows
  ppf without group_idx           lane-sized shapes fall back to the wave kernels (lane_ok: !ppf || group_idx)   write_rows

  knn_lane_brute_kernel<2>        no grid, 256 x ~260 self, nsample 1: idx and dist2 only (group_idx has no columns)  lane_emit

Every form of roitr_knn_form (the rule the launcher dispatches through; tests/test_knn_form_cpu.py pins the form of every case here
by its shape) is reached: the kernels that could not be -- a wave-per-query grid kernel and 66- / 101-slot lane lists -- are gone.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import knn_util as U  # noqa: E402
from oracle import pointops_cpu as O  # noqa: E402  (checker only)
from test_pointops_gpu import cloud  # noqa: E402

ERR_ARG = 1   # common.h ROITR_ERR_ARG


KINDS = ("uniform", "lattice", "dup", "clustered")


def make_cloud(rng, n, kind):
    """cloud() of test_pointops_gpu.py, and `clustered`: half of the points uniform in the box, half in one cube of a twentieth of its
    side -- generic points (no ties) whose cells hold far more than the mean: the cell kernel hands those queries to its retry list."""
    if kind != "clustered":
        return cloud(rng, n, kind)
    p = (rng.random((n, 3)) * 2).astype(np.float32)
    p[n // 2:] = (rng.random(3) * 1.8 + rng.random((n - n // 2, 3)) * 0.1).astype(np.float32)
    return p


def make_inputs(seed, sizes, kind, take=None, axis_quarter=False):
    """Reference clouds with normals and a query set: the reference points themselves (take None) or take[c] random points of cloud c
    in index order, as a separate array (the TransitionDown form).  The query normals are an array of their own whose values differ
    from the reference normals at the same point: a kernel that reads the wrong array or the wrong row fails."""
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([make_cloud(rng, n, kind) for n in sizes])
    off = np.cumsum(sizes).astype(np.int32)
    r_nrm = U.unit_normals(rng, xyz.shape[0], axis_quarter)
    if take is None:
        sel, q_xyz, q_off = None, xyz, off
    else:
        sel = U.subset(rng, sizes, take)
        q_xyz, q_off = np.ascontiguousarray(xyz[sel]), np.cumsum(take).astype(np.int32)
    q_nrm = U.unit_normals(rng, q_xyz.shape[0], axis_quarter)
    return dict(xyz=xyz, off=off, r_nrm=r_nrm, sel=sel, q_xyz=q_xyz, q_off=q_off, q_nrm=q_nrm)


def reference(inp, nsample, kind):
    """Oracle indices and distances, the float64 PPF on them, and the conditions that keep a case on the epilogue it is meant for
    (asserted from the reference alone)."""
    ridx, rd2 = O.knnquery_raw(nsample, inp["xyz"], inp["q_xyz"], inp["off"], inp["q_off"], threads=8)
    ref = U.ppf_ref(inp["q_xyz"], inp["q_nrm"], inp["xyz"], inp["r_nrm"], ridx[:, 1:])
    tied = U.tied_fraction(rd2, nsample)
    if kind in ("uniform", "clustered"):
        assert tied < 0.10, tied                         # the kernel's own epilogue writes the rows
        assert U.generic_angles(ref).mean() >= 0.90
        if inp["sel"] is not None:                       # column 0 of a TransitionDown row is the point itself
            assert np.array_equal(ridx[:, 0], inp["sel"]) and not rd2[:, 0].any()
    if kind == "lattice":
        assert tied > 0.90, tied                         # the replay's write_rows<2> writes them
    return ridx, rd2, ref


def check_engine_form(g, q, nsample, ridx, rd2, ref, what):
    """The engine's call (group_idx + ppf) and the call with all four outputs, from one workspace."""
    a = g.query(nsample, q, "gp")
    assert np.array_equal(a.group, ridx[:, 1:]), f"{what}: group_idx rows {np.unique(np.nonzero(a.group != ridx[:, 1:])[0])[:10]}"
    U.assert_ppf(a.ppf, ref, what)
    f = g.query(nsample, q, "idgp")
    assert np.array_equal(f.dist2, rd2), f"{what}: dist2 rows {np.unique(np.nonzero(f.dist2 != rd2)[0])[:10]}"
    assert np.array_equal(f.idx, ridx), f"{what}: idx rows {np.unique(np.nonzero(f.idx != ridx)[0])[:10]}"
    assert np.array_equal(f.group, a.group), what
    assert np.array_equal(U.bits(f.ppf), U.bits(a.ppf)), f"{what}: ppf bits differ between the two output sets"
    return a


R8 = U.ragged(8, 1250)
T8 = [1100] * 8                      # >= 8192 queries: the lane kernels
RLB = U.ragged(256, 261)             # >= 65536 queries without a grid
RLB_BIG = RLB[:5] + [1100] + RLB[6:]  # one cloud of several staging chunks (the chunk is the mean cloud rounded up to 64)
RSUB, TSUB = U.ragged(352, 250), [190] * 352
R9K, T9K = U.ragged(2, 9000), [4100] * 2

# (branch, use_grid, sizes, take, nsample, kind, a quarter of the normals exactly +-z)
CASES = [
    ("brute<1>", False, [300, 77, 5], None, 9, "uniform", True),
    ("brute<1>", False, [300, 77, 5], None, 17, "uniform", False),
    ("brute<1>", False, [300, 77, 5], None, 17, "lattice", False),
    ("brute<1>", False, [300, 77, 5], None, 9, "dup", False),
    ("brute<2>", False, [400, 150], None, 65, "uniform", True),
    ("brute<2>", False, [400, 150], None, 100, "uniform", False),
    ("brute<2>", False, [400, 150], None, 65, "lattice", False),
    ("brute<2>", False, [400, 150], None, 100, "dup", False),
    ("lane_brute<4>", False, RLB, None, 3, "uniform", False),
    ("lane_brute<10>", False, RLB, None, 9, "uniform", True),
    ("lane_brute<10>", False, RLB_BIG, None, 9, "uniform", False),
    ("lane_brute<18>", False, RLB, None, 17, "uniform", False),
    ("lane_brute<34>", False, RLB, None, 33, "uniform", False),
    ("lane_brute<18>", False, RSUB, TSUB, 17, "uniform", False),
    ("lane_brute<4>", False, RLB, None, 3, "lattice", False),
    ("lane_brute<34>", False, RLB, None, 33, "lattice", False),
    ("lane_brute<18>", False, RSUB, TSUB, 17, "lattice", False),
    ("lane_brute<10>", False, RLB, None, 9, "dup", False),
    ("lane<4>", True, R8, None, 3, "uniform", True),
    ("lane<4>", True, R8, None, 3, "lattice", False),
    ("lane<4>", True, R8, None, 3, "dup", False),
    ("prefilter<10,40>+lane<10>", True, R8, None, 9, "uniform", True),
    ("prefilter<10,40>+lane<10>", True, R8, None, 5, "uniform", False),
    ("prefilter<10,40>+lane<10> sort<4096>", True, R8, T8, 9, "uniform", False),
    ("prefilter<10,40>+lane<10> sort<4096>", True, R8, T8, 5, "uniform", False),
    ("prefilter<10,40>+lane<10>", True, R8, None, 9, "lattice", False),
    ("prefilter<10,40>+lane<10> sort<4096>", True, R8, T8, 9, "lattice", False),
    ("prefilter<10,40>+lane<10>", True, R8, None, 5, "dup", False),
    ("lane<18>", True, R8, None, 17, "uniform", True),
    ("lane<34>", True, R8, None, 33, "uniform", True),
    ("lane<18> sort<4096>", True, R8, T8, 17, "uniform", False),
    ("lane<34> sort<4096>", True, R8, T8, 33, "uniform", False),
    ("lane<18>", True, R8, None, 17, "lattice", False),
    ("lane<34> sort<4096>", True, R8, T8, 33, "lattice", False),
    ("lane<18> sort<4096>", True, R8, T8, 17, "dup", False),
    ("lane<18> sort<max>", True, R9K, T9K, 17, "uniform", True),
    ("lane<18> sort<max>", True, R9K, T9K, 17, "lattice", False),
    ("cell+gridsel", True, [3000], None, 9, "uniform", True),
    ("cell+gridsel", True, [3000], None, 65, "uniform", False),
    ("cell+gridsel", True, [700, 3100], None, 17, "uniform", False),
    ("cell+gridsel", True, [700, 3100], None, 65, "uniform", False),
    ("cell+gridsel", True, [700, 3100], None, 17, "lattice", False),
    ("cell+gridsel", True, [3000], None, 65, "lattice", False),
    ("cell+gridsel", True, [3000], None, 9, "dup", False),
    ("cell+gridsel", True, [3000], None, 17, "clustered", False),
    ("cell+gridsel", True, [700, 3100], None, 65, "clustered", False),
    ("gridsel", True, [5000], [1250], 17, "uniform", True),
    ("gridsel", True, [2000], None, 100, "uniform", False),
    ("gridsel", True, [5000], [1250], 17, "lattice", False),
]


def _case_id(c):
    name, _, sizes, take, ns, kind, axis = c
    shape = f"{len(sizes)}x{sizes[0]}" if len(sizes) > 3 else "-".join(map(str, sizes))
    name = name.translate(str.maketrans(" ,+", "___", "<>"))
    return f"{name}-{shape}{'-sub' if take else ''}-k{ns}-{kind}{'-z' if axis else ''}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_knn_fused_branch(case):
    name, use_grid, sizes, take, ns, kind, axis = case
    n, m, b = sum(sizes), sum(take) if take else sum(sizes), len(sizes)
    assert U.branch(b, n, m, ns, use_grid, take is None) == name
    inp = make_inputs(1000 * KINDS.index(kind) + 13 * ns + n + 7 * m + int(use_grid), sizes, kind, take, axis)
    ridx, rd2, ref = reference(inp, ns, kind)
    # grids of the engine's 6 points per cell; the cell kernel's larger k at what pointops._knn builds for it
    g = U.Grid(inp["xyz"], inp["off"], inp["r_nrm"], m_capacity=m, use_grid=use_grid, occupancy=max(6.0, 0.4 * (ns + 1) if ns + 1 >= 35 else 0.0))
    q = g.queries(None if take is None else inp["q_xyz"], inp["q_off"], inp["q_nrm"])
    check_engine_form(g, q, ns, ridx, rd2, ref, _case_id(case))


@pytest.mark.parametrize("level", [0, 1, 2])
def test_knn_engine_call_pattern(level):
    """One level of issue_geometry_chain: the level's grid is built once, carved for the query count of the level above (not the
    count of any query made from it), then serves the level's self query (K + 1), the next level's TransitionDown query and the
    self query again.  All three equal the oracle; the third equals the first bit for bit: the workspace's tie list, retry list
    and query-order regions leak nothing from one query into the next.  Level 2 (8 x ~312) has no grid, like the engine's."""
    rng = np.random.default_rng(500 + level)
    sizes = [U.ragged(8, 5000)]
    for _ in range(3):
        sizes.append([s // 4 for s in sizes[-1]])
    xyz = np.concatenate([cloud(rng, s, "uniform") for s in sizes[0]])
    for lv in range(level):                       # random subsets instead of FPS picks
        xyz = xyz[U.subset(rng, sizes[lv], sizes[lv + 1])]
    cur, nxt = sizes[level], sizes[level + 1]
    off, noff = np.cumsum(cur).astype(np.int32), np.cumsum(nxt).astype(np.int32)
    sel = U.subset(rng, cur, nxt)
    t_xyz = np.ascontiguousarray(xyz[sel])
    r_nrm, s_nrm, t_nrm = (U.unit_normals(rng, k) for k in (xyz.shape[0], xyz.shape[0], t_xyz.shape[0]))
    ks, kt = (8, 16, 16)[level] + 1, 16 + 1
    use_grid = xyz.shape[0] > 768 * 8
    assert use_grid == (level < 2)
    m_capacity = sum(sizes[max(level - 1, 0)])
    assert U.branch(8, sum(cur), sum(cur), ks, use_grid, True) == ("prefilter<10,40>+lane<10>", "lane<18>", "brute<1>")[level]
    assert U.branch(8, sum(cur), sum(nxt), kt, use_grid, False) == ("lane<18> sort<4096>", "gridsel", "brute<1>")[level]
    s_idx, s_d2 = O.knnquery_raw(ks, xyz, xyz, off, off, threads=8)
    t_idx, t_d2 = O.knnquery_raw(kt, xyz, t_xyz, off, noff, threads=8)
    assert np.array_equal(t_idx[:, 0], sel)
    s_ref = U.ppf_ref(xyz, s_nrm, xyz, r_nrm, s_idx[:, 1:])
    t_ref = U.ppf_ref(t_xyz, t_nrm, xyz, r_nrm, t_idx[:, 1:])
    g = U.Grid(xyz, off, r_nrm, m_capacity=m_capacity, use_grid=use_grid, occupancy=6.0)
    q_self, q_td = g.queries(None, None, s_nrm), g.queries(t_xyz, noff, t_nrm)
    first = g.query(ks, q_self, "gp")
    td = g.query(kt, q_td, "gp")
    again = g.query(ks, q_self, "gp")
    assert np.array_equal(first.group, s_idx[:, 1:])
    U.assert_ppf(first.ppf, s_ref, f"level {level} self")
    assert np.array_equal(td.group, t_idx[:, 1:])
    U.assert_ppf(td.ppf, t_ref, f"level {level} TransitionDown")
    assert np.array_equal(again.group, first.group) and np.array_equal(U.bits(again.ppf), U.bits(first.ppf))


@pytest.mark.parametrize("sizes", [[1250, 1247, 900], [9000, 8997, 700]], ids=["cap4096", "capmax"])
def test_knn_sorted_points(sizes):
    """roitr_knn_sorted_points: the row order the fused local blocks take.  n float4 (x, y, z, index as bits): every cloud owns
    its own contiguous range, in cloud order, holding a permutation of the cloud's indices, each with its own coordinates."""
    from roitr_amd import _lib as L
    rng = np.random.default_rng(sum(sizes))
    xyz = np.concatenate([cloud(rng, s, "uniform") for s in sizes])
    off = np.cumsum(sizes).astype(np.int32)
    n, b = xyz.shape[0], len(sizes)
    assert (n <= 6144 * b) == (sizes[0] == 1250)      # both forms of grid_build_kernel
    g = U.Grid(xyz, off, None, m_capacity=n + 37, use_grid=True, occupancy=6.0)
    lib = L.bind(["roitr_knn_sorted_points"])
    at = lib.roitr_knn_sorted_points(b, n, n + 37, L.ptr(g.ws)) - g.ws.data_ptr()
    assert 0 <= at and at + 16 * n <= g.ws.numel()
    torch.cuda.synchronize()
    pts = g.ws[at:at + 16 * n].clone().view(torch.float32).cpu().numpy().reshape(n, 4)
    w = pts[:, 3].copy().view(np.int32)
    for c in range(b):
        lo, hi = (0 if c == 0 else int(off[c - 1])), int(off[c])
        assert np.array_equal(np.sort(w[lo:hi]), np.arange(lo, hi, dtype=np.int32)), c
    assert np.array_equal(U.bits(pts[:, :3]), U.bits(xyz[w]))


def test_knn_fused_one_column():
    """nsample = 2 on a lane-kernel shape: one output column."""
    inp = make_inputs(2, R8, "uniform")
    assert U.branch(8, sum(R8), sum(R8), 2, True, True) == "lane<4>"
    ridx, rd2, ref = reference(inp, 2, "uniform")
    g = U.Grid(inp["xyz"], inp["off"], inp["r_nrm"], m_capacity=sum(R8))
    a = check_engine_form(g, g.queries(None, None, inp["q_nrm"]), 2, ridx, rd2, ref, "nsample 2")
    assert a.group.shape == (sum(R8), 1) and a.ppf.shape == (sum(R8), 1, 4)


def test_knn_lane_brute_nsample_1():
    """nsample = 1 without a grid at >= 65536 queries: the width-2 lane list, idx and dist2 against the oracle bit for bit."""
    n = sum(RLB)
    assert U.knn_form(256, n, n, 1, False, True, "id") == ("LANE_BRUTE", 2, U.SORT["NONE"])
    inp = make_inputs(1, RLB, "uniform")
    ridx, rd2 = O.knnquery_raw(1, inp["xyz"], inp["q_xyz"], inp["off"], inp["q_off"], threads=8)
    g = U.Grid(inp["xyz"], inp["off"], None, m_capacity=n, use_grid=False)
    r = g.query(1, g.queries(None, None, None), "id")
    assert np.array_equal(r.dist2, rd2), f"dist2 rows {np.nonzero(r.dist2 != rd2)[0][:10]}"
    assert np.array_equal(r.idx, ridx), f"idx rows {np.nonzero(r.idx != ridx)[0][:10]}"


def test_knn_ppf_without_normals_is_refused():
    """ppf without reference or query normals: ROITR_ERR_ARG, nothing launched, nothing written."""
    inp = make_inputs(3, [300, 77], "uniform")
    g = U.Grid(inp["xyz"], inp["off"], inp["r_nrm"], m_capacity=377, use_grid=False)
    for q, ref_normals in ((g.queries(None, None, None), True), (g.queries(None, None, inp["q_nrm"]), False)):
        r = g.query(9, q, "idgp", ref_normals=ref_normals, check=False)
        assert r.status == ERR_ARG
        assert (r.idx == -1).all() and (r.group == -1).all() and np.isnan(r.dist2).all() and np.isnan(r.ppf).all()


@pytest.mark.parametrize("use_grid", [True, False])
def test_knn_ppf_without_group_idx(use_grid):
    """ppf with group_idx NULL on a lane-sized shape: lane_emit reads the neighbours back from group_idx, so the host falls back to
    a wave kernel there (lane_ok: !ppf || group_idx) -- the PPF is the same."""
    sizes = R8 if use_grid else RLB
    n = sum(sizes)
    assert U.branch(8 if use_grid else 256, n, n, 17, use_grid, True, ppf=True, group=False) == ("cell+gridsel" if use_grid else "brute<1>")
    inp = make_inputs(4 + use_grid, sizes, "uniform")
    ridx, rd2, ref = reference(inp, 17, "uniform")
    g = U.Grid(inp["xyz"], inp["off"], inp["r_nrm"], m_capacity=n, use_grid=use_grid)
    alone = g.query(17, g.queries(None, None, inp["q_nrm"]), "p")
    assert alone.group is None
    U.assert_ppf(alone.ppf, ref, "ppf alone")
