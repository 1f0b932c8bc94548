"""Input preparation in front of the model, on the GPU.

Mirrors the reference's dataset code: `pcd.estimate_normals(search_param=o3d.geometry.KDTreeSearchParamKNN(knn=33))`
followed by `normal_redirect(points, normals, view_point)` (dataset/tdmatch.py:120-127, dataset/fdmatch.py:83-90,
dataset/common.py:312-320).  Open3D (0.13.0, requirements.txt:64) is not part of the reference tree; its algorithm is
restated in csrc/prep.hip.  No CPU fallback.

In front of the normals, for raw scans (csrc/voxel.hip): `voxel_down_sample` (the 2.5 cm voxel grid the
reference's 3DMatch files went through beforehand; Open3D's voxel_down_sample restated, with a DEFINED output order) and
`random_subsample` (the `points_lim` cap of dataset/tdmatch.py:72-78 and dataset/fdmatch.py:49-56 as a distribution).
"""
import collections
import ctypes

import torch

from . import _args as A
from . import _lib as L
from .pointops import GRID_MIN_POINTS


def _vp(view_point):
    v = [float(x) for x in (view_point if view_point is not None else (0.0, 0.0, 0.0))]
    return (ctypes.c_float * 3)(*v)


def estimate_normals(xyz, offset, knn=33, view_point=(0.0, 0.0, 0.0), use_grid=None):
    """xyz (n,3) fp32 device tensor of b concatenated clouds, offset (b) cumulative int32 -> normals (n,3) fp32.

    view_point=None keeps the unoriented PCA direction (Open3D's sign is arbitrary); otherwise the result equals
    normal_redirect(points, open3d_normals, view_point)."""
    xyz = A.dev(xyz, torch.float32, "estimate_normals")
    offset = offset.to(torch.int32).contiguous()
    n, b = int(xyz.shape[0]), int(offset.shape[0])
    out = torch.empty((n, 3), dtype=torch.float32, device=xyz.device)
    if n == 0:
        return out
    if use_grid is None:
        use_grid = n > GRID_MIN_POINTS * b
    lib = L.lib()
    ws = torch.empty(lib.roitr_normals_workspace_bytes(b, n, int(knn)), dtype=torch.uint8, device=xyz.device)
    vp = _vp(view_point) if view_point is not None else None
    L.check(lib.roitr_estimate_normals(b, n, L.ptr(xyz), L.ptr(offset), int(knn), 1 if use_grid else 0, vp, L.ptr(out), L.ptr(ws),
                                       L.stream_ptr()), "estimate_normals")
    return out


def normal_redirect(points, normals, view_point):
    """dataset/common.py:312-320: make the normals point towards the view point."""
    points, normals = A.dev(points, torch.float32, "normal_redirect"), normals.contiguous().float()
    out = torch.empty_like(normals)
    L.check(L.lib().roitr_normal_redirect(int(points.shape[0]), L.ptr(points), L.ptr(normals), _vp(view_point), L.ptr(out), L.stream_ptr()),
            "normal_redirect")
    return out


VoxelResult = collections.namedtuple("VoxelResult", "points offset attr inverse counts status")
VOXEL_STATUS_RANGE, VOXEL_STATUS_NONFINITE = 1, 2


def voxel_down_sample(xyz, offset, voxel_size, attr=None, strict=True):
    """Voxel-grid downsampling of b concatenated clouds: xyz (n,3) fp32 device tensor, offset (b) cumulative int32.

    Per cloud, in float64 on the fp32 inputs: vmb = min_bound - voxel_size / 2, ijk = floor((p - vmb) / voxel_size); one output point
    per occupied voxel, the sum of its points in input order over their count, rounded once to fp32 (Open3D's voxel_down_sample
    restated; parity with the original is unpinned).  Open3D leaves the output order to a hash map; here clouds keep their order and
    the voxels of a cloud ascend in (ix, iy, iz).  Returns VoxelResult:
      points (m,3), offset (b) cumulative int32, attr (m,c) per-voxel means of `attr` (n,c) or None, inverse (n) int32 output row of
      every input point (Open3D's `_and_trace`), counts (m) int32 points per voxel, status (b) int32 per cloud: bit 1 = an axis needs
      a voxel index above 65535, bit 2 = a non-finite coordinate; such a cloud yields no voxels and inverse = -1.
    strict: raise RoitrError naming the first cloud with a status bit.  One host read (the total, to slice the capacity buffers; the
    status words travel with it)."""
    xyz = A.dev(xyz, torch.float32, "voxel_down_sample")
    offset = offset.to(device=xyz.device, dtype=torch.int32).contiguous()
    n, b = int(xyz.shape[0]), int(offset.shape[0])
    c = 0
    if attr is not None:
        c = int(attr[0].numel()) if n else int(torch.Size(attr.shape[1:]).numel())
        attr = attr.to(xyz.device).contiguous().float().reshape(n, c)
    dev = xyz.device
    out_xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    out_attr = torch.empty((n, c), dtype=torch.float32, device=dev) if attr is not None else None
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    inverse = torch.empty((n,), dtype=torch.int32, device=dev)
    tail = torch.empty((2 * b,), dtype=torch.int32, device=dev)   # new_offset, status: one host read for both
    new_offset, status = tail[:b], tail[b:]
    lib = L.lib()
    ws = torch.empty(lib.roitr_voxel_workspace_bytes(b, n, c), dtype=torch.uint8, device=dev)
    L.check(lib.roitr_voxel_downsample(b, n, L.ptr(xyz), L.ptr(offset), ctypes.c_double(float(voxel_size)), c, L.ptr(attr), L.ptr(out_xyz),
                                       L.ptr(new_offset), L.ptr(counts), L.ptr(inverse), L.ptr(out_attr), L.ptr(status), L.ptr(ws),
                                       L.stream_ptr()), "voxel_down_sample")
    host = tail.cpu()
    if strict and bool(host[b:].any()):
        k = int(torch.nonzero(host[b:])[0])
        what = [w for bit, w in ((VOXEL_STATUS_RANGE, "an axis needs a voxel index above 65535 (voxel_size too small for its extent)"),
                                 (VOXEL_STATUS_NONFINITE, "a non-finite coordinate")) if int(host[b + k]) & bit]
        raise L.RoitrError(f"voxel_down_sample: cloud {k}: " + " and ".join(what))
    m = int(host[b - 1])
    return VoxelResult(out_xyz[:m], new_offset, out_attr[:m] if out_attr is not None else None, inverse, counts[:m], status)


OutlierResult = collections.namedtuple("OutlierResult", "points offset attr index keep status mean_dist stats counts")
OUTLIER_STATUS_NONFINITE = 1
_outlier = L.binder(("roitr_outlier_workspace_bytes", "roitr_remove_statistical_outlier", "roitr_remove_radius_outlier"))


def _outlier_groups(lib, sizes, k, max_bytes):
    """Consecutive groups [g0, g1) of clouds whose workspace stays under max_bytes; a single larger cloud goes alone."""
    groups, g0, rows = [], 0, 0
    for c, s in enumerate(sizes):
        if c > g0 and int(lib.roitr_outlier_workspace_bytes(c + 1 - g0, rows + s, k)) > max_bytes:
            groups.append((g0, c))
            g0, rows = c, 0
        rows += s
    return groups + [(g0, len(sizes))]


def _outlier_run(what, xyz, offset, attr, k, max_bytes, call, optional):
    """The part the two filters share: the buffers, the groups, the calls, ONE host read (new_offset and status of every group), the
    slices.  optional: (mean_dist, stats, counts) as the caller allocated them, or None.
    call(lib, b, n, xyz, offset, keep, index, new_offset, status, rows (lo, hi), clouds (g0, g1), ws, nbytes) -> status code, for one group."""
    xyz = A.points(xyz, what)
    dev = xyz.device
    offset = offset.to(device=dev, dtype=torch.int32).contiguous()
    n, b = int(xyz.shape[0]), int(offset.shape[0])
    if attr is not None:
        attr = attr.to(dev)
        if int(attr.shape[0]) != n:
            raise L.RoitrError(f"{what}: attr must have one row per point")
    lib = _outlier()
    keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    index = torch.empty((n,), dtype=torch.int32, device=dev)
    tail = torch.zeros((2 * b,), dtype=torch.int32, device=dev)   # new_offset, status: one host read for both
    new_offset, status = tail[:b], tail[b:]
    groups, bounds = [(0, b)], [0, n]
    if b > 1 and int(lib.roitr_outlier_workspace_bytes(b, n, k)) > max_bytes:
        ends = [0] + offset.cpu().tolist()   # only a call that has to be split reads the offsets first
        groups = _outlier_groups(lib, [ends[c + 1] - ends[c] for c in range(b)], k, max_bytes)
        bounds = ends
    for g0, g1 in groups:
        lo, hi = (0, n) if len(groups) == 1 else (bounds[g0], bounds[g1])
        if g1 == g0:
            continue
        off = offset[g0:g1] if lo == 0 else (offset[g0:g1] - lo).contiguous()
        nbytes = int(lib.roitr_outlier_workspace_bytes(g1 - g0, hi - lo, k))
        ws = A.workspace(nbytes, dev)
        L.check(call(lib, g1 - g0, hi - lo, xyz[lo:hi], off, keep[lo:hi], index[lo:hi], new_offset[g0:g1], status[g0:g1], (lo, hi), (g0, g1),
                     ws, nbytes), what)
    host = tail.cpu()
    if len(groups) > 1:   # group-local rows and counts -> the call's
        parts, offs, total = [], [], 0
        for g0, g1 in groups:
            m = int(host[g1 - 1]) if g1 > g0 else 0
            parts.append(index[bounds[g0]:bounds[g0] + m] + bounds[g0])
            offs.append(new_offset[g0:g1] + total)
            total += m
        index, new_offset = torch.cat(parts), torch.cat(offs)
    else:
        index = index[:int(host[b - 1]) if b else 0]
    rows = index.long()
    return OutlierResult(xyz[rows], new_offset, attr[rows] if attr is not None else None, index, keep.bool(), status, *optional)


def remove_statistical_outlier(xyz, offset, nb_neighbors=20, std_ratio=2.0, attr=None, return_stats=False, max_workspace_bytes=1 << 30):
    """Open3D's remove_statistical_outlier restated (include/roitr_pointops.h above roitr_remove_statistical_outlier is the definition;
    parity with the original is unpinned): xyz (n,3) fp32 device tensor of b concatenated clouds, offset (b) cumulative int32.

    mean_i = the mean distance of point i to the nb_neighbors entries of its kNN row (itself included); a point is kept iff
    0 < mean_i < cloud_mean + std_ratio * std over its own cloud.  Returns OutlierResult: points (m,3), offset (b) cumulative int32,
    attr (m,c) the kept rows of `attr` or None, index (m) int32 the kept global rows, ascending, keep (n) bool, status (b) int32 (bit 1 =
    a non-finite coordinate: the cloud keeps nothing), and with return_stats mean_dist (n) float64 and stats (b,3) float64 = cloud_mean,
    std, thr (None otherwise; counts is the radius filter's).
    The clouds are processed in consecutive groups whose workspace (n * nb_neighbors * 4 bytes of kNN rows dominate) stays under
    max_workspace_bytes; a single larger cloud goes alone.  The results do not depend on the split.  One host read (the totals; a call
    that has to be split reads the offsets first)."""
    k, ratio = int(nb_neighbors), float(std_ratio)
    n, b = int(xyz.shape[0]), int(offset.shape[0])
    mean = stats = None
    if return_stats and torch.is_tensor(xyz) and xyz.is_cuda:
        mean = torch.zeros((n,), dtype=torch.float64, device=xyz.device)
        stats = torch.zeros((b, 3), dtype=torch.float64, device=xyz.device)

    def call(lib, gb, gn, gx, goff, keep, index, new_offset, status, rows, clouds, ws, nbytes):
        return lib.roitr_remove_statistical_outlier(gb, gn, L.ptr(gx), L.ptr(goff), k, ratio, L.ptr(keep), L.ptr(index), L.ptr(new_offset),
                                                    L.ptr(status), L.ptr(mean[rows[0]:rows[1]] if mean is not None else None),
                                                    L.ptr(stats[clouds[0]:clouds[1]] if stats is not None else None), L.ptr(ws), nbytes,
                                                    L.stream_ptr())
    return _outlier_run("remove_statistical_outlier", xyz, offset, attr, k, int(max_workspace_bytes), call, (mean, stats, None))


def remove_radius_outlier(xyz, offset, nb_points=16, radius=0.05, attr=None, return_counts=False):
    """Open3D's remove_radius_outlier restated (defined in include/roitr_pointops.h): a point is kept iff more than nb_points points of
    its own cloud, itself included, lie strictly within `radius` of it (float64 on the fp32 coordinates).  Arguments and result as
    remove_statistical_outlier; return_counts adds counts (n) int32, the points within the radius (without it a query stops counting
    at nb_points + 1).  One host read."""
    n = int(xyz.shape[0])
    counts = torch.zeros((n,), dtype=torch.int32, device=xyz.device) if return_counts and torch.is_tensor(xyz) and xyz.is_cuda else None

    def call(lib, gb, gn, gx, goff, keep, index, new_offset, status, rows, clouds, ws, nbytes):
        return lib.roitr_remove_radius_outlier(gb, gn, L.ptr(gx), L.ptr(goff), float(radius), int(nb_points), L.ptr(keep), L.ptr(index),
                                               L.ptr(new_offset), L.ptr(status), L.ptr(counts), L.ptr(ws), nbytes, L.stream_ptr())
    return _outlier_run("remove_radius_outlier", xyz, offset, attr, 0, 1 << 62, call, (None, None, counts))


def random_subsample(offset, limit, seed=0, cloud_keys=None):
    """The point cap: offset (b) cumulative int32 device tensor -> (idx, new_offset).

    A cloud with more than `limit` points keeps `limit` of them, uniform without replacement: point j of a cloud with key k draws
    u = splitmix64(seed ^ DOMAIN ^ splitmix64(k << 32 | j)) >> 16 and the points of smallest (u, j) stay; a smaller cloud keeps all.
    idx: the kept GLOBAL rows (int32), ascending -- the reference's np.random.permutation(n)[:points_lim] keeps permutation order and
    its stream cannot be reproduced on a device; the distribution of the kept set is the same.  cloud_keys (b ints): k per cloud
    (default: the cloud's position); the selection depends on (seed, k, cloud size, limit) only, not on the rest of the call."""
    offset = A.dev(offset, torch.int32, "random_subsample")
    dev = offset.device
    b = int(offset.shape[0])
    keys = None
    if cloud_keys is not None:
        keys = torch.as_tensor(cloud_keys).to(device=dev, dtype=torch.int32).contiguous()
        if int(keys.shape[0]) != b:
            raise L.RoitrError("random_subsample: one cloud key per cloud")
    host = offset.cpu()
    n = int(host[-1]) if b else 0
    idx = torch.empty((n,), dtype=torch.int32, device=dev)
    new_offset = torch.empty((b,), dtype=torch.int32, device=dev)
    lib = L.lib()
    ws = torch.empty(lib.roitr_subsample_workspace_bytes(b, n), dtype=torch.uint8, device=dev)
    L.check(lib.roitr_random_subsample(b, n, L.ptr(offset), int(limit), ctypes.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), L.ptr(keys),
                                       L.ptr(idx), L.ptr(new_offset), L.ptr(ws), L.stream_ptr()), "random_subsample")
    sizes = torch.diff(host, prepend=host.new_zeros(1)).clamp(max=int(limit))   # the total follows from the sizes: no second read
    return idx[:int(sizes.sum())], new_offset
