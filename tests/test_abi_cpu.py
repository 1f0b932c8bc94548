"""CPU: the C-ABI library loads and exports every symbol the headers declare (no compute calls); the struct classes roitr_amd/_lib.py
makes from include/*.h against the C compiler's layout of the same headers; the signatures it reads from them for the evaluation and
preparation entry points and for everything roitr_amd/ops.py calls; the host-only *_workspace_bytes() values."""
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


MIRRORS = {"ops": dict(_Gemm="RoitrGemm", _LocalAttn="RoitrLocalAttn", _LocalAttnFold="RoitrLocalAttnFold", _LocalBlock="RoitrLocalBlock",
                      _LocalTd="RoitrLocalTd", _LocalFirst="RoitrLocalFirst", _Mha="RoitrMha", _Coarse="RoitrCoarse", _OT="RoitrOT",
                      _Fine="RoitrFine", _NodeCorr="RoitrNodeCorr"),
           "riga": dict(_CConfig="RoitrEngineConfig", _CForwardIO="RoitrForwardIO")}


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof and every offsetof of all 14 structs of include/*.h, as the C compiler lays them out from the headers themselves, against
    the ctypes classes roitr_amd/_lib.py makes from its own reading of the headers (the classes ops.py, riga.py and the tests use)."""
    import importlib
    import subprocess
    from roitr_amd import _lib as L
    from roitr_amd.build import HIPCC
    structs = L.header_structs()
    assert len(structs) == 14 and sum(len(f) for f in structs.values()) == 321   # ABI 4: a field the reader drops can hide in padding
    for module, names in MIRRORS.items():
        for attr, name in names.items():
            assert getattr(importlib.import_module("roitr_amd." + module), attr) is L.struct(name), (module, attr)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "roitr_pointops.h"', '#include "roitr_engine.h"', 'int main(void) {']
    for name, fields in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in fields]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["return 0; }", ""]))
    subprocess.run([HIPCC, "-x", "c", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)   # no compiler: an error
    want = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    got = {}
    for name, fields in structs.items():
        got[name] = str(ctypes.sizeof(L.struct(name)))
        got.update({f"{name}.{f}": str(getattr(L.struct(name), f).offset) for f, _ in fields})
    assert len(want) == 14 + 321 and got == want, sorted(set(got.items()) ^ set(want.items()))


def test_struct_reader_against_hand_written_fields():
    from roitr_amd import _lib as L
    structs = L.header_structs()
    assert structs["RoitrOT"] == [("pairs", I), ("num_corr", I), ("limit", I), ("num_iter", I), ("n_corr", P), ("scores", P),
                                  ("row_masks", P), ("col_masks", P), ("alpha", P), ("out", P), ("pair_off", P), ("slots", I)]
    cfg = structs["RoitrEngineConfig"]
    assert [(n, t) for n, t in cfg if n != "geo_is_cross"] == [
        ("factor", I), ("num_corr", I), ("point_limit", I), ("fine_topk", I), ("fine_mutual", I), ("fine_use_global_score", I),
        ("fine_conf", F), ("n_geo_layers", I), ("matching_radius", F), ("adaptive_coarse", I), ("occlusion_radius", F),
        ("operand_dtype", I)]
    name, arr = cfg[8]
    assert name == "geo_is_cross" and arr._type_ is I and arr._length_ == 16 and len(cfg) == 13
    # the other forms a field takes: size_t, long, double, `unsigned char*`; a type the table does not know is an error, not a gap
    assert L._fields("size_t n; long a, b; double d; unsigned char* flags; const long* eoff") == [
        ("n", SZ), ("a", ctypes.c_long), ("b", ctypes.c_long), ("d", D), ("flags", P), ("eoff", P)]
    with pytest.raises(KeyError):
        L._fields("int a; short b")
    # every struct a prototype takes has been read
    text = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("roitr_pointops.h", "roitr_engine.h"))
    taken = set(re.findall(r"const\s+(Roitr\w+)\s*\*", text))
    assert len(taken) >= 13 and taken <= set(structs), taken - set(structs)


def test_ops_entry_points_are_bound_from_the_headers():
    """Every entry point roitr_amd/ops.py calls has its restype / argtypes from the header: no call site converts by hand."""
    from roitr_amd import ops
    source = open(os.path.join(ROOT, "roitr_amd", "ops.py")).read()
    called = set(re.findall(r"\.(roitr_\w+)\(", source))
    assert len(called) >= 40 and "roitr_gemm" in called and "roitr_add_layernorm" in called
    lib, counts = ops._lib(), header_parameter_counts()
    headers = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("roitr_pointops.h", "roitr_engine.h"))
    sized = set(re.findall(r"^size_t\s+(\w+)\s*\(", headers, re.M))
    assert {"roitr_coarse_scratch_floats", "roitr_geo_table_floats"} <= sized & called
    assert called - set(counts) == {"roitr_local_block_dbg"}   # the tuning hook no header declares: (struct pointer, int, stream)
    for name in called & set(counts):
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == counts[name], name
        assert fn.restype is (SZ if name in sized else I), name
    for word in ("ctypes.c_long(", "c_float(", ".restype =", "ctypes.Structure"):
        assert word not in source, word


def test_structs_and_ops_import_without_the_library(monkeypatch, tmp_path):
    import importlib
    from roitr_amd import _lib as L, ops
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "missing.so"))
    monkeypatch.setattr(L, "_lib", None)
    assert ctypes.sizeof(L.struct.__wrapped__("RoitrGemm")) == ctypes.sizeof(L.struct("RoitrGemm")) > 0
    ops = importlib.reload(ops)
    assert ops._Gemm is L.struct("RoitrGemm")
    with pytest.raises(L.RoitrError):     # nothing above asked for the library: asking does
        ops._lib()


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
