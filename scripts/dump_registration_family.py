"""Every tensor lgr_batch, compat_batch, icp_batch (both modes) and gicp_batch return on the seeded fixtures of their GPU tests, saved
to one .npz: run it on two builds, then `--compare a.npz b.npz` (no GPU) lists the keys and fails unless every one is bitwise equal.

    python scripts/dump_registration_family.py out.npz
    python scripts/dump_registration_family.py --compare parent.npz branch.npz

The package and the tests are taken from the tree the script lies in, so a copy of another commit's tree dumps that commit.
profiles/registration_family_refactor.txt records the comparison made when the shared stages were carved out."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import compat_util as CU
    import lgr_util as LU
    import test_compat_gpu as TC
    import test_gicp_gpu as TG
    import test_icp_gpu as TI
    import test_lgr_gpu as TL
    out = {}

    def put(prefix, result):
        for k, v in result.items():
            for i, x in enumerate(v if isinstance(v, list) else [v]):   # "nn" is a list of per-pair arrays
                out[f"{prefix}/{k}" + (f"/{i}" if isinstance(v, list) else "")] = np.asarray(x)

    for name in TL.CASES:
        put(f"lgr/{name}", TL.run([LU.fixture(name)]))
    put("lgr/ragged", TL.run([None if n is None else LU.fixture(n) for n in TL.RAGGED]))
    for name in TC.CASES:
        data, kw = CU.fixture(name)
        put(f"compat/{name}", TC.run([data], **kw))
    put("compat/ragged", TC.run([None if n is None else CU.fixture(n)[0] for n in TC.RAGGED]))

    names = ("room_a", "room_b", "n255", "n256", "n257")
    none = np.zeros((0, 3), np.float32)
    for plane in (False, True):
        mode = "plane" if plane else "point"
        for name in names:
            put(f"icp_{mode}/{name}", TI.run([TI.pair_of(name)], plane))
        a, c = TI.pair_of("room_a"), TI.pair_of("n257")     # the batch of test_icp_gpu.test_ragged_batch
        nan, far = dict(c, src=c["src"].copy()), dict(c, T0=c["T0"].copy())
        nan["src"][5, 2] = np.nan
        far["T0"][:3, 3] += 50.0
        put(f"icp_{mode}/ragged", TI.run([a, dict(a, src=none), dict(a, tgt=none, normals=none), nan, far, c], plane))
    for name in names:
        put(f"gicp/{name}", TG.run([TG.pair_of(name)]))
    a, c = TG.pair_of("room_a"), TG.pair_of("n257")         # the batch of test_gicp_gpu.test_ragged_batch
    far = dict(c, T0=c["T0"].copy())
    far["T0"][:3, 3] += 50.0
    put("gicp/ragged", TG.run([a, far, dict(a, src=none, src_normals=none), c]))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print(len(out), "tensors ->", path)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    per_op, bad = {}, sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        equal = a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")
        n = per_op.setdefault(k.split("/")[0], [0, 0])
        n[0] += 1
        n[1] += equal
        if not equal:
            bad.append(k)
    for op, (n, eq) in per_op.items():
        print(f"{op}: {eq} of {n} keys bitwise equal")
    if bad:
        sys.exit("NOT EQUAL or missing on one side: " + ", ".join(bad))


if __name__ == "__main__":
    compare(*sys.argv[2:4]) if sys.argv[1] == "--compare" else dump(sys.argv[1])
