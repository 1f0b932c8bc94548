"""out and ebar of roitr_mha for every case of tests/test_geo_attn_gpu.py (CASES: every kernel form, both sides of every threshold), on the
case's launch window at a fixed seed, saved to one .npz: run it on two builds, then `--compare a.npz b.npz` (no GPU) lists the keys and
fails unless every one is bitwise equal.

    python scripts/dump_mha.py out.npz
    python scripts/dump_mha.py --compare parent.npz branch.npz

The package and the test module are taken from the tree the script lies in, so a copy of the script in another commit's tree dumps that
commit; only the case table and the input builder (Setup, window) of the test module are used, the launch is ops.multi_head_attention.
Rows outside the window keep the NaN they were filled with and are compared too.  profiles/mha_refactor.txt records the comparison made
when the dispatch became one plan."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch

    import test_geo_attn_gpu as T
    from roitr_amd import ops
    out = {}
    for n, (case_id, _, C, heads, sizes, cross, e, diag) in enumerate(T.CASES):
        for packed in (True, False):
            S = T.Setup(C, heads, sizes, cross, e, diag, packed=packed, seed=n)
            q_row0, q_rows = T.window(S.T)
            o = torch.full((S.T, C), float("nan"), device="cuda")
            eb = torch.full((S.T, heads, C), float("nan"), device="cuda") if S.E is not None else None
            kw = dict(E=S.E, eoff=S.eoff, qt=S.qt, bp=S.bp) if S.E is not None else {}
            ops.multi_head_attention(S.q, S.k, S.v, S.offset, S.cloud_of_row, S.nk_max, heads=heads, partner=S.partner_t, q_row0=q_row0,
                                     q_rows=q_rows, out=o, ebar=eb, **kw)
            torch.cuda.synchronize()
            name = f"{case_id}/{'packed' if packed else 'dense'}"
            out[name + "/out"] = o.cpu().numpy()
            if eb is not None:
                out[name + "/ebar"] = eb.cpu().numpy()
    # an array above 1 MiB is kept as the SHA-256 of its bytes behind its dtype and shape (equal digests = equal bits)
    kept = {}
    for k, a in out.items():
        a = np.ascontiguousarray(a)
        kept[k] = a if a.nbytes <= 1 << 20 else np.frombuffer(f"{a.dtype}{a.shape}".encode() + hashlib.sha256(a.tobytes()).digest(), np.uint8)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **kept)
    print(len(kept), "arrays ->", path)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    keys = sorted(set(a.files) & set(b.files))
    for k in keys:   # the bits, not the values: -0 is not +0, and a NaN only equals the same NaN
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
            bad.append(k)
    print(f"{len(keys) - len(set(bad) & set(keys))} of {len(keys)} keys bitwise equal")
    if bad:
        sys.exit("NOT EQUAL or missing on one side: " + ", ".join(bad))


if __name__ == "__main__":
    compare(*sys.argv[2:4]) if sys.argv[1] == "--compare" else dump(sys.argv[1])
