"""float64 numpy restatement of the pair ground truth (csrc/pairgt.hip, include/roitr_pointops.h): the same operations in the same
order on the fp32 inputs, brute force over all (i, j).  numpy evaluates every ufunc on its own, so nothing here is fused."""
import numpy as np

STATUS_NONFINITE, STATUS_EMPTY, STATUS_OVERFLOW = 1, 2, 4


def move(p, R, t, inverse=False):
    """forward: ((R[c][0] px + R[c][1] py) + R[c][2] pz) + t[c];  inverse: d = p - t, (R[0][c] dx + R[1][c] dy) + R[2][c] dz."""
    p = np.asarray(p, np.float32).astype(np.float64).reshape(-1, 3)
    R = np.asarray(R, np.float32).astype(np.float64).reshape(3, 3)
    t = np.asarray(t, np.float32).astype(np.float64).reshape(3)
    out = np.empty_like(p)
    if not inverse:
        for c in range(3):
            out[:, c] = ((R[c, 0] * p[:, 0] + R[c, 1] * p[:, 1]) + R[c, 2] * p[:, 2]) + t[c]
    else:
        d = p - t
        for c in range(3):
            out[:, c] = (R[0, c] * d[:, 0] + R[1, c] * d[:, 1]) + R[2, c] * d[:, 2]
    return out


def sqdist(pm, q):
    """((px - qx)^2 + (py - qy)^2) + (pz - qz)^2 for all (i, j), float64."""
    q = np.asarray(q, np.float32).astype(np.float64).reshape(-1, 3)
    dx, dy, dz = (pm[:, None, c] - q[None, :, c] for c in range(3))
    return (dx * dx + dy * dy) + dz * dz


def info_matrix(p):
    """sum of G^T G over the rows of p (float64), G = [ I3 | -2 [p]x ]: the gt.info layout, translation block first."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    G = np.zeros((p.shape[0], 3, 6))
    G[:, 0, 0] = G[:, 1, 1] = G[:, 2, 2] = 1.0
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    # -2 [p]x = -2 [[0, -z, y], [z, 0, -x], [-y, x, 0]]
    G[:, 0, 4], G[:, 0, 5] = 2 * z, -2 * y
    G[:, 1, 3], G[:, 1, 5] = -2 * z, 2 * x
    G[:, 2, 3], G[:, 2, 4] = 2 * y, -2 * x
    return np.einsum("nki,nkj->ij", G, G)


def info_abs_terms(p):
    """per entry, the sum of the absolute values of the terms the entry adds up (the scale of its rounding error)."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    G = np.zeros((p.shape[0], 3, 6))
    G[:, 0, 0] = G[:, 1, 1] = G[:, 2, 2] = 1.0
    x, y, z = np.abs(p[:, 0]), np.abs(p[:, 1]), np.abs(p[:, 2])
    G[:, 0, 4], G[:, 0, 5] = 2 * z, 2 * y
    G[:, 1, 3], G[:, 1, 5] = 2 * z, 2 * x
    G[:, 2, 3], G[:, 2, 4] = 2 * y, 2 * x
    return np.einsum("nki,nkj->ij", G, G)


def pair_status(src, tgt, R, t):
    s = 0
    if not (np.isfinite(src).all() and np.isfinite(tgt).all() and np.isfinite(np.asarray(R, np.float32)).all()
            and np.isfinite(np.asarray(t, np.float32)).all()):
        s |= STATUS_NONFINITE
    if len(src) == 0 or len(tgt) == 0:
        s |= STATUS_EMPTY
    return s


def pair_brute(src, tgt, R, t, radius, K=None, inverse=False):
    """One pair: dict(count, nn_idx, nn_dist2, n_hit, overlap, info, corr (rows (i, j), ascending i then (d2, j), first K per i),
    status).  inverse: `src` are the queries moved by R^T (q - t), `tgt` the searched cloud (the target-side overlap)."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    n = len(src)
    status = pair_status(src, tgt, R, t)
    out = dict(count=np.zeros(n, np.int32), nn_idx=np.full(n, -1, np.int32), nn_dist2=np.full(n, np.inf), n_hit=0,
               overlap=float("nan"), info=np.zeros((6, 6)), corr=np.zeros((0, 2), np.int32), status=status, d2=None)
    if status:
        return out
    r = np.float64(np.float32(radius))
    d2 = sqdist(move(src, R, t, inverse), tgt)
    within = d2 < r * r
    out["d2"] = d2
    out["count"] = within.sum(1).astype(np.int32)
    rows = []
    for i in range(n):
        js = np.nonzero(within[i])[0]
        if len(js) == 0:
            continue
        js = js[np.lexsort((js, d2[i, js]))]
        out["nn_idx"][i], out["nn_dist2"][i] = js[0], d2[i, js[0]]
        if K is not None:
            js = js[:K]
        rows.append(np.stack([np.full(len(js), i), js], 1))
    hit = out["count"] > 0
    out["n_hit"] = int(hit.sum())
    out["overlap"] = out["n_hit"] / n
    out["info"] = info_matrix(src[hit].astype(np.float64))
    if rows:
        out["corr"] = np.concatenate(rows).astype(np.int32)
    return out


def batch_brute(srcs, tgts, Rs, ts, radius, K=None, inverse=False):
    """A ragged batch (lists of clouds): the concatenated per-point outputs, the per-pair ones stacked, corr with corr_offset."""
    res = [pair_brute(s, t, R, tr, radius, K, inverse) for s, t, R, tr in zip(srcs, tgts, Rs, ts)]
    cat = lambda k, dt: np.concatenate([r[k] for r in res]).astype(dt) if res else np.zeros(0, dt)
    return dict(count=cat("count", np.int32), nn_idx=cat("nn_idx", np.int32), nn_dist2=cat("nn_dist2", np.float64),
                n_hit=np.array([r["n_hit"] for r in res], np.int32), overlap=np.array([r["overlap"] for r in res], np.float64),
                info=np.stack([r["info"] for r in res]), corr=np.concatenate([r["corr"] for r in res]).astype(np.int32).reshape(-1, 2),
                corr_offset=np.cumsum([len(r["corr"]) for r in res]).astype(np.int32),
                status=np.array([r["status"] for r in res], np.int32), pairs=res)


def rodrigues(w):
    """rotation matrix of a rotation vector (float64)."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def random_rigid(rng, angle=None, shift=1.0):
    w = rng.normal(size=3)
    w *= (rng.uniform(0.2, 3.0) if angle is None else angle) / np.linalg.norm(w)
    return rodrigues(w).astype(np.float32), (rng.normal(size=3) * shift).astype(np.float32)
