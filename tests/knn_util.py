"""Helpers of tests/test_knn_fused_gpu.py: inputs shaped like the engine's kNN calls, a float64 restatement of calc_ppf_gpu, and a
direct caller of roitr_knn_build_grid_ex / roitr_knnquery_ex that chooses which outputs are NULL.

Everything above `class Grid` is numpy only, but for knn_form / branch, which ask the built library (no GPU)."""
import os
import re

import numpy as np

GUARD = 64                               # elements behind every output buffer that a call must leave alone
KNN_FILL = np.float32(1e10)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1


def _header(prefix):
    text = open(os.path.join(ROOT, "include", "roitr_pointops.h")).read()
    return {name: int(value) for name, value in re.findall(r"#define %s(\w+) (\d+)" % prefix, text)}


FORM = _header("ROITR_KNN_(?!OUT_|SORT_)")          # NOTHING .. GRIDSEL
OUT = _header("ROITR_KNN_OUT_")                     # IDX, DIST2, GROUP, PPF
SORT = _header("ROITR_KNN_SORT_")                   # NONE, 4096, MAX
FORM_NAME = {v: k for k, v in FORM.items()}
_FORMAT = {"BRUTE": "brute<%d>", "LANE_BRUTE": "lane_brute<%d>", "LANE": "lane<%d>", "PREFILTER": "prefilter<%d,40>+lane<%d>", "WITHIN": "within",
           "CELL": "cell+gridsel", "GRIDSEL": "gridsel", "NOTHING": "nothing"}


def knn_form(b, n, m, nsample, use_grid, self_query, want="idgp", normals=True, capped=False):
    """roitr_knn_form for a call with the outputs `want` (letters of "idgp"): (form name, list width, sort form), or the negative status.
    Host code that follows no pointer: needs the built library, no GPU."""
    from roitr_amd import _lib as L
    outputs = sum(OUT[k] for c, k in zip("idgp", ("IDX", "DIST2", "GROUP", "PPF")) if c in want)
    v = L.lib().roitr_knn_form(b, n, m, nsample, int(self_query), outputs, int(normals), int(use_grid), int(capped))
    return v if v < 0 else (FORM_NAME[v & 0xff], (v >> 8) & 0xff, v >> 16)


def branch(b, n, m, nsample, use_grid, self_query, ppf=True, group=True):
    """The kernel roitr_knnquery_ex gives a call (by shape alone), as the name the GPU tests use: what roitr_knn_form -- the rule the
    launcher dispatches through -- says; where the queries are counting-sorted first, the sort's form is appended."""
    form, width, sort = knn_form(b, n, m, nsample, use_grid, self_query, ("g" if group else "") + ("p" if ppf else ""))
    name = _FORMAT[form]
    name = name % ((width,) * name.count("%d"))
    return name + {SORT["NONE"]: "", SORT["4096"]: " sort<4096>", SORT["MAX"]: " sort<max>"}[sort]


def ragged(n_clouds, n):
    return [n - 3 * (i % 4) for i in range(n_clouds)]


def unit_normals(rng, n, axis_quarter=False):
    """Random unit vectors (fp32); axis_quarter: a quarter of them exactly +z or -z."""
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v = v.astype(np.float32)
    if axis_quarter:
        pick = rng.random(n) < 0.25
        v[pick] = 0.0
        v[pick, 2] = np.where(rng.random(int(pick.sum())) < 0.5, 1.0, -1.0)
    return v


def subset(rng, sizes, take):
    """Global indices of `take[c]` random points of every cloud, in index order (the TransitionDown form: FPS picks are
    reference points; random ones here)."""
    sel, start = [], 0
    for n, t in zip(sizes, take):
        sel.append(start + np.sort(rng.choice(n, size=t, replace=False)))
        start += n
    return np.concatenate(sel).astype(np.int64)


def ppf_ref(q_xyz, q_nrm, r_xyz, r_nrm, idx, dtype=np.float64):
    """lib/utils.py:358-389 calc_ppf_gpu on the neighbours idx (m, k) of every query: (m, k, 4) = |d|, angle(n1, d) / pi,
    angle(n2, d) / pi, angle(n1, n2) / pi with d = neighbour - query and angle(a, b) = atan2(|a x b|, a . b).  dtype float64: the
    reference; float32: what plain fp32 arithmetic makes of the same formula (the yardstick for an fp32 kernel's error)."""
    idx = idx.astype(np.int64)
    d = r_xyz.astype(dtype)[idx] - q_xyz.astype(dtype)[:, None, :]
    n2 = r_nrm.astype(dtype)[idx]
    n1 = np.broadcast_to(q_nrm.astype(dtype)[:, None, :], d.shape)

    def ang(a, b):
        return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1)) / dtype(np.pi)

    return np.stack([np.linalg.norm(d, axis=-1), ang(n1, d), ang(n2, d), ang(n1, n2)], -1)


def generic_angles(ref):
    """Angle entries of a float64 PPF whose operands are not within 1e-3 (of pi) of parallel or anti-parallel."""
    a = ref[..., 1:]
    return (a > 1e-3) & (a < 1 - 1e-3)


def ppf_errors(got, ref):
    """(max |d| error over max(1, |d|), max error of the generic angles, max error of all angles) against the float64 reference."""
    e_d = np.abs(got[..., 0] - ref[..., 0]) / np.maximum(1.0, np.abs(ref[..., 0]))
    e_a = np.abs(got[..., 1:].astype(np.float64) - ref[..., 1:])
    gen = generic_angles(ref)
    return float(e_d.max()), float(e_a[gen].max()) if gen.any() else 0.0, float(e_a.max())


def assert_ppf(got, ref, what=""):
    """The bounds of test_ppf_against_float64 (set on MI355X for ppf.hip, which shares roitr_ppf4 with the fused epilogues)."""
    assert got.shape == ref.shape and got.dtype == np.float32, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).any(-1).sum())} ppf entries not finite (never written?)"
    e_d, e_gen, e_all = ppf_errors(got, ref)
    print(f"{what}: |d| {e_d:.3g}  generic angles {e_gen:.3g}  all angles {e_all:.3g}")
    assert e_d <= 1e-6, (what, e_d)
    assert e_gen <= 5e-7, (what, e_gen)
    assert e_all <= 2e-4, (what, e_all)


def tied_fraction(d2, nsample):
    """Share of the queries with two equal distances among their first nsample oracle entries (fill slots do not count)."""
    d = d2[:, :nsample]
    return float(((d[:, 1:] == d[:, :-1]) & (d[:, 1:] < KNN_FILL)).any(1).mean())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- device side
class Result:
    """Outputs of one roitr_knnquery_ex call as numpy arrays (None where the pointer was NULL) and its status."""
    def __init__(self, status, idx, dist2, group, ppf):
        self.status, self.idx, self.dist2, self.group, self.ppf = status, idx, dist2, group, ppf


class Grid:
    """A reference cloud set on the device with its kNN workspace, carved for m_capacity queries.  With use_grid the grid is built
    once, here (roitr_knn_build_grid_ex at the target occupancy); any number of query() calls then share the workspace, as the
    engine's levels do."""

    def __init__(self, xyz, off, normals, m_capacity, use_grid=True, occupancy=6.0):
        import ctypes
        import torch
        from roitr_amd import _lib as L
        self.L, self.lib = L, L.lib()
        self.b, self.n, self.m_capacity, self.use_grid = len(off), xyz.shape[0], int(m_capacity), bool(use_grid)
        self.xyz, self.off = self._dev(xyz, np.float32), self._dev(off, np.int32)
        self.normals = None if normals is None else self._dev(normals, np.float32)
        self.ws = torch.empty(self.lib.roitr_knn_workspace_bytes(self.b, self.n, self.m_capacity), dtype=torch.uint8, device="cuda")
        if use_grid:
            L.check(self.lib.roitr_knn_build_grid_ex(self.b, self.n, self.m_capacity, L.ptr(self.xyz), L.ptr(self.off), L.ptr(self.ws),
                                                     ctypes.c_float(occupancy), L.stream_ptr()), "knn_build_grid")

    @staticmethod
    def _dev(a, dtype):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()

    def queries(self, xyz=None, off=None, normals=None):
        """Device arrays of a query set.  xyz None: the reference points themselves -- the SAME device arrays, which is how
        roitr_knnquery_ex recognises a self query -- with query normals of their own all the same."""
        nrm = None if normals is None else self._dev(normals, np.float32)
        if xyz is None:
            return (self.xyz, self.off, nrm)
        return (self._dev(xyz, np.float32), self._dev(off, np.int32), nrm)

    def query(self, nsample, q, want="gp", ref_normals=True, check=True):
        """One roitr_knnquery_ex call from this workspace.  want: the outputs that are not NULL, letters of "idgp" (idx, dist2,
        group_idx, ppf).  Every output buffer is filled with a sentinel first (NaN / -1: the engine hands these kernels
        uninitialised arena memory) and carries GUARD sentinel elements behind its end: no sentinel may survive inside, none may
        be overwritten behind."""
        import torch
        L = self.L
        q_xyz, q_off, q_nrm = q
        m, k = q_xyz.shape[0], nsample - 1
        assert m <= self.m_capacity
        shapes = {"i": (m, nsample), "d": (m, nsample), "g": (m, k), "p": (m, k, 4)}
        buf = {}
        for c in want:
            numel = int(np.prod(shapes[c])) + GUARD
            buf[c] = torch.full((numel,), -1, dtype=torch.int32, device="cuda") if c in "ig" else \
                torch.full((numel,), float("nan"), dtype=torch.float32, device="cuda")
        status = self.lib.roitr_knnquery_ex(self.b, self.n, m, int(nsample), L.ptr(self.xyz), L.ptr(q_xyz), L.ptr(self.off), L.ptr(q_off),
                                            L.ptr(buf.get("i")), L.ptr(buf.get("d")), L.ptr(buf.get("g")), L.ptr(buf.get("p")),
                                            L.ptr(self.normals if ref_normals else None), L.ptr(q_nrm),
                                            1 if self.use_grid else 0, self.m_capacity, L.ptr(self.ws), L.stream_ptr())
        torch.cuda.synchronize()
        if check:
            L.check(status, "knnquery")
        out = {}
        for c in "idgp":
            if c not in buf:
                out[c] = None
                continue
            a = buf[c].cpu().numpy()
            body, guard = a[:-GUARD], a[-GUARD:]
            assert (guard == -1).all() if c in "ig" else np.isnan(guard).all(), f"output '{c}': written behind its end"
            if check:
                left = int((body == -1).sum()) if c in "ig" else int(np.isnan(body).sum())
                assert left == 0, f"output '{c}': {left} of {body.size} elements never written"
            out[c] = body.reshape(shapes[c])
        return Result(status, out["i"], out["d"], out["g"], out["p"])
