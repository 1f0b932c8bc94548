"""CPU: the C-ABI library loads and exports every symbol the headers declare (no compute calls); the signatures roitr_amd/_lib.py
reads from include/*.h for the evaluation and preparation entry points; the host-only *_workspace_bytes() values."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_library_exports_declared_symbols():
    import __graft_entry__ as G
    from roitr_amd import _lib
    lib = _lib.lib()
    names = G.declared_symbols()
    assert len(names) >= 50
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.roitr_abi_version() == 4   # bumped with every struct change of include/*.h (round 6: batch_live, the compacted patch layout; RoitrLocalBlock::w*_h)
    # the reference's own launcher names are present verbatim (cpp_wrappers/pointops/src/*/*_cuda_kernel.h)
    for n in ("furthestsampling_cuda_launcher", "knnquery_cuda_launcher", "grouping_forward_cuda_launcher",
              "grouping_backward_cuda_launcher", "interpolation_forward_cuda_launcher", "interpolation_backward_cuda_launcher",
              "subtraction_forward_cuda_launcher", "subtraction_backward_cuda_launcher", "aggregation_forward_cuda_launcher",
              "aggregation_backward_cuda_launcher"):
        assert hasattr(lib, n), n


def test_level_sizes_and_workspace_queries_are_host_only():
    from roitr_amd import _lib
    lib = _lib.lib()
    out = (ctypes.c_int * 4)()
    lib.roitr_level_sizes(5000, out)
    assert list(out) == [5000, 1250, 312, 78]       # model/model.py:59-62 floor rule
    lib.roitr_knn_workspace_bytes.restype = ctypes.c_size_t
    assert lib.roitr_knn_workspace_bytes(2, 10000, 10000) > 10000 * 16


def test_product_has_no_cpu_fallback():
    import pytest
    import torch
    from roitr_amd import _lib, pointops
    x = torch.zeros(8, 3)
    o = torch.tensor([8], dtype=torch.int32)
    with pytest.raises(_lib.RoitrError):
        pointops.furthestsampling(x, o, torch.tensor([2], dtype=torch.int32))
    with pytest.raises(_lib.RoitrError):
        pointops.knnquery(3, x, x, o, o)


def test_product_never_imports_the_oracle():
    import re
    pkg = os.path.join(ROOT, "roitr_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                text = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, re.M), f
                assert "liboracle" not in text and "pointops_cpu" not in text and "roitr_ref" not in text, f


def _header_struct(name):
    """[(field, ctypes type)] of `typedef struct <name> { ... }` in include/roitr_engine.h (scalars int / long / float / size_t and
    pointers only)."""
    import re
    text = open(os.path.join(ROOT, "include", "roitr_engine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    scalars = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(?:unsigned\s+)?([A-Za-z_][A-Za-z0-9_]*)\s*(.*)$", decl, re.S)
        base, rest = m.group(1), m.group(2)
        for item in rest.split(","):
            item = item.strip()
            if item.startswith("*"):
                fields.append((item.lstrip("* ").strip(), ctypes.c_void_p))
            else:
                fields.append((item, scalars[base]))
    return fields


def test_ctypes_mirrors_match_the_header():
    """The ctypes structures of roitr_amd/ops.py, field by field (name, type, order, hence offsets) against include/roitr_engine.h."""
    from roitr_amd import ops
    for mirror, name in ((ops._NodeCorr, "RoitrNodeCorr"), (ops._OT, "RoitrOT"), (ops._Fine, "RoitrFine"), (ops._Coarse, "RoitrCoarse"),
                         (ops._LocalAttn, "RoitrLocalAttn")):
        want = _header_struct(name)
        got = [(f[0], f[1]) for f in mirror._fields_]
        assert got == want, (name, [(a, b) for a, b in zip(got, want) if a != b], len(got), len(want))


I, F, D, P, SZ = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t


def header_parameter_counts():
    """{name: number of parameters} by counting the commas of every prototype: independent of the parser under test."""
    counts = {}
    for h in ("roitr_pointops.h", "roitr_engine.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        for name, params in re.findall(r"\b(\w+)\s*\(([^()]*)\)\s*;", text):
            counts[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return counts


def test_bound_signatures_follow_the_headers():
    from roitr_amd import _lib
    lib, counts = _lib.lib(), header_parameter_counts()
    assert len(_lib.BOUND) == len(set(_lib.BOUND)) == 35
    for name in _lib.BOUND:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == counts[name], name
        assert fn.restype is (SZ if name.endswith("_workspace_bytes") else I), name
    # three signatures written out by hand: the parser itself
    assert lib.roitr_pairgt_workspace_bytes.argtypes == [I, I, I, ctypes.c_longlong]
    assert lib.roitr_voxel_downsample.argtypes == [I, I, P, P, D, I] + [P] * 9
    rc = lib.roitr_ransac_correspondences.argtypes
    assert rc[15] is ctypes.c_uint64 and ctypes.sizeof(rc[15]) == 8 and rc[15](-1).value == 2 ** 64 - 1
    assert rc == [I, P, I, P, P, P, P, I, I, I, F, F, I, I, I, ctypes.c_uint64, I, P, SZ] + [P] * 7
    # the timed path converts its own arguments: nothing of it is declared here
    assert lib.roitr_engine_forward.argtypes is None and lib.roitr_knnquery_ex.argtypes is None


def test_every_prototype_resolves():
    """No prototype of the two headers has a type the parser does not know (it raises KeyError on one), and none is missed."""
    from roitr_amd import _lib
    protos, counts = _lib.header_prototypes(), header_parameter_counts()
    assert set(protos) == set(counts) and len(protos) >= 110
    assert all(len(protos[n][1]) == counts[n] for n in counts)


# (arguments, bytes) of the build before this layer existed: a small call and one of batch size each
WORKSPACE_BYTES = {
    "roitr_registration_workspace_bytes": [((1, 37, 1000, 0), 2304), ((8, 40000, 50000, 0), 1625088)],
    "roitr_nfmr_workspace_bytes": [((1, 5, 7), 512), ((8, 30000, 20000), 720384)],
    "roitr_desc_match_workspace_bytes": [((1, 33, 65), 2304), ((8, 40000, 41000), 972544)],
    "roitr_fine_loss_workspace_bytes": [((3,), 512), ((2048,), 16384)],
    "roitr_coarse_loss_workspace_bytes": [((1, 5, 7), 1536), ((8, 197, 203), 2585600)],
    "roitr_voxel_workspace_bytes": [((1, 100, 0), 10752), ((16, 500000, 3), 14632448)],
    "roitr_subsample_workspace_bytes": [((1, 100), 10752), ((16, 500000), 14632448)],
    "roitr_pairgt_workspace_bytes": [((1, 50, 60, 1024), 81664), ((8, 40000, 41000, 1280000), 17833472)],
}


@pytest.mark.parametrize("name", sorted(WORKSPACE_BYTES))
def test_workspace_sizes_are_unchanged(name):
    from roitr_amd import _lib
    fn = getattr(_lib.lib(), name)
    for args, nbytes in WORKSPACE_BYTES[name]:
        assert fn(*args) == nbytes, (name, args)
