"""float64 numpy restatement of roitr_amd.prep.voxel_down_sample and random_subsample (test infrastructure).

Voxels: Open3D's voxel_down_sample from its published algorithm, with the output order this project defines (clouds in input order,
voxels ascending in (ix, iy, iz)).  np.unique on packed keys, then np.bincount(inverse, weights=...) per channel: bincount adds
sequentially in input order (np.add.reduceat does not), which is the summation order the library promises.
Cap: the counter-based stream in wrapping uint64 (roitr_amd/weights.py::_splitmix64), the `limit` smallest (u, j) per cloud."""
import numpy as np

from roitr_amd.weights import _splitmix64

AXIS_MAX = 65535
STATUS_RANGE, STATUS_NONFINITE = 1, 2
SUB_DOMAIN = np.uint64(0xE7037ED1A0B428DB)


def _mean32(inverse, weights, counts):
    return (np.bincount(inverse, weights=weights.astype(np.float64), minlength=len(counts)) / counts).astype(np.float32)


def voxel_cloud(p, voxel_size, attr=None):
    """One cloud (n,3) fp32 -> (points, attr, inverse, counts, status)."""
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    n = len(p)
    c = 0 if attr is None else int(np.prod(np.shape(attr)[1:]))
    empty = (np.zeros((0, 3), np.float32), None if attr is None else np.zeros((0, c), np.float32), np.full(n, -1, np.int32),
             np.zeros(0, np.int32))
    if n == 0:
        return empty + (0,)
    if not np.isfinite(p).all():
        return empty + (STATUS_NONFINITE,)
    vs = np.float64(voxel_size)
    vmb = p.min(0).astype(np.float64) - vs * 0.5
    with np.errstate(over="ignore"):
        ijk = np.floor((p.astype(np.float64) - vmb) / vs)
    if not ((ijk >= 0) & (ijk <= AXIS_MAX)).all():
        return empty + (STATUS_RANGE,)
    ijk = ijk.astype(np.uint64)
    key = (ijk[:, 0] << np.uint64(32)) | (ijk[:, 1] << np.uint64(16)) | ijk[:, 2]
    _, inverse, counts = np.unique(key, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    pts = np.stack([_mean32(inverse, p[:, a], counts) for a in range(3)], 1)
    out_attr = None
    if attr is not None:
        a32 = np.ascontiguousarray(attr, np.float32).reshape(n, c)
        out_attr = np.stack([_mean32(inverse, a32[:, k], counts) for k in range(c)], 1) if c else np.zeros((len(counts), 0), np.float32)
    return pts, out_attr, inverse.astype(np.int32), counts.astype(np.int32), 0


def voxel_batch(xyz, offset, voxel_size, attr=None):
    """Concatenated clouds -> dict(points, offset, attr, inverse, counts, status), inverse in global output rows."""
    lo, pts, atts, inv, cnt, status, new_off, total = 0, [], [], [], [], [], [], 0
    for hi in [int(x) for x in offset]:
        p, a, i, k, s = voxel_cloud(xyz[lo:hi], voxel_size, None if attr is None else attr[lo:hi])
        pts.append(p); atts.append(a); cnt.append(k); status.append(s)
        inv.append(np.where(i >= 0, i + total, -1).astype(np.int32))
        total += len(p)
        new_off.append(total)
        lo = hi
    return dict(points=np.concatenate(pts) if pts else np.zeros((0, 3), np.float32),
                offset=np.array(new_off, np.int32), attr=None if attr is None else np.concatenate(atts),
                inverse=np.concatenate(inv) if inv else np.zeros(0, np.int32), counts=np.concatenate(cnt) if cnt else np.zeros(0, np.int32),
                status=np.array(status, np.int32))


def subsample_u(n, key, seed):
    """u of points 0 .. n-1 of a cloud with key `key`: 48-bit integers (uint64)."""
    ctr = (np.uint64(key) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    return _splitmix64(np.uint64(seed) ^ SUB_DOMAIN ^ _splitmix64(ctr)) >> np.uint64(16)


def subsample_cloud(n, limit, key, seed):
    """Cloud-local kept rows, ascending."""
    if n <= limit:
        return np.arange(n, dtype=np.int32)
    order = np.lexsort((np.arange(n), subsample_u(n, key, seed)))   # by u, ties by j
    return np.sort(order[:limit]).astype(np.int32)


def subsample_batch(offset, limit, seed=0, cloud_keys=None):
    lo, idx, new_off = 0, [], []
    for c, hi in enumerate(int(x) for x in offset):
        k = c if cloud_keys is None else int(cloud_keys[c])
        idx.append(subsample_cloud(hi - lo, limit, k, seed) + lo)
        new_off.append((new_off[-1] if new_off else 0) + len(idx[-1]))
        lo = hi
    return (np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32)), np.array(new_off, np.int32)
