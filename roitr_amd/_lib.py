"""ctypes binding of libroitr_hip.so (the C-ABI boundary, include/*.h).

There is no CPU fallback anywhere in this package: if the HIP library is missing or fails to load,
importing an operator raises.  (The CPU restatement lives under oracle/ and is test-only.)

Struct layouts (struct()) and prototypes (BOUND, bind(), binder()) are read from include/*.h by one reader, _headers(); nothing of them
is typed a second time in Python.  tests/test_abi_cpu.py holds every struct's sizeof / offsetof against the C compiler.  The calls of
the timed path (riga, pointops) are left undeclared and convert their own arguments.
"""
import ctypes
import functools
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libroitr_hip.so")
_lib = None


class RoitrError(RuntimeError):
    pass


# The entry points of the evaluation and preparation modules (registration, nonrigid, descmatch, loss, pairgt, prep, evaluate): their
# restype / argtypes are read from the prototypes of include/*.h at load, so a call cannot disagree with the header about a type.
# (The calls of the timed path -- pointops, riga -- convert their arguments themselves.)  The last two lines: the row-wise layers and
# the positional fold behind the operator wrappers of ops.py; ops.py binds the rest of what it calls itself (binder()).
BOUND = ("roitr_registration_workspace_bytes roitr_ransac_correspondences roitr_ransac_samples roitr_weighted_procrustes "
         "roitr_nfmr_workspace_bytes roitr_nfmr_batch roitr_blend_anchor_motion "
         "roitr_desc_match_workspace_bytes roitr_desc_match_batch roitr_desc_match_select "
         "roitr_fine_loss_workspace_bytes roitr_fine_loss_batch roitr_coarse_loss_workspace_bytes roitr_coarse_loss_batch "
         "roitr_pairgt_workspace_bytes roitr_pairgt_stats roitr_pairgt_correspondences "
         "roitr_normals_workspace_bytes roitr_estimate_normals roitr_normal_redirect "
         "roitr_voxel_workspace_bytes roitr_voxel_downsample roitr_subsample_workspace_bytes roitr_random_subsample "
         "roitr_inlier_counts roitr_coarse_hits "
         "roitr_build_pfold roitr_add_layernorm roitr_l2_normalize roitr_segment_mean roitr_interp3_add "
         "roitr_gather_rows roitr_compose_idx roitr_transpose roitr_add_vectors").split()
_CTYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "long": ctypes.c_long,
           "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_uint64, "unsigned int": ctypes.c_uint,
           "unsigned": ctypes.c_uint, "roitr_stream_t": ctypes.c_void_p, "void": None}


def _ctype(decl, named):
    """ctypes type of a C parameter, field or return declaration; any pointer is a c_void_p, `x[n]` of a parameter included (struct fields
    come here without their `[n]`).  named: the last word may be the name."""
    if "*" in decl or "[" in decl:
        return ctypes.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if named and len(words) > 1 and " ".join(words) not in _CTYPES:
        words.pop()
    return _CTYPES[" ".join(words)]   # KeyError: a type this table does not know


def _fields(body):
    """[(field, ctypes type)] of a struct body: `int M, N, K;`, `const float* A;`, `int geo_is_cross[16];`."""
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = [item.strip() for item in decl.split(",")]
        base, first = re.fullmatch(r"(.*?)([\*\s]*\b\w+\s*(?:\[\d+\])?)", first, re.S).groups()   # the type words | the first declarator
        for item in [first] + more:
            stars, name, count = re.fullmatch(r"([\*\s]*)(\w+)\s*(?:\[(\d+)\])?", item).groups()
            ct = _ctype(f"{base} {stars} {name}", True)
            fields.append((name, ct * int(count) if count else ct))
    return fields


HEADERS = ("roitr_pointops.h", "roitr_engine.h")
ENCODE_HEADER = "roitr_encode.h"   # part 3 of the ABI (encode once, match many): read by the same reader, listed on its own


@functools.lru_cache(maxsize=None)
def _headers(names=HEADERS):
    """(structs, prototypes) of the named headers of include/ (default: roitr_pointops.h and roitr_engine.h): the one reader of the
    headers."""
    structs, protos = {}, {}
    for h in names:
        text = open(os.path.join(os.path.dirname(_HERE), "include", h)).read()
        text = re.sub(r"/\*.*?\*/|//[^\n]*|^\s*#[^\n]*|extern \"C\" \{", "", text, flags=re.S | re.M)
        for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;", text):
            structs[name] = _fields(body)
        while re.search(r"\{[^{}]*\}", text):   # struct bodies
            text = re.sub(r"\{[^{}]*\}", "", text)
        for ret, name, params in re.findall(r"([\w\s\*]+?)\b(\w+)\s*\(([^()]*)\)\s*;", text):
            params = [p.strip() for p in params.split(",") if p.strip() not in ("", "void")]
            protos[name] = (_ctype(ret.strip(), False), [_ctype(p, True) for p in params])
    return structs, protos


def header_structs():
    """{struct name: [(field, ctypes type), ...]} of every `typedef struct X { ... } X;` of the two headers."""
    return _headers()[0]


def header_prototypes():
    """{function name: (restype, [argtypes])} of every prototype of the two headers."""
    return _headers()[1]


def encode_header():
    """(structs, prototypes) of include/roitr_encode.h, as header_structs() / header_prototypes() give them for the other two."""
    return _headers((ENCODE_HEADER,))


@functools.lru_cache(maxsize=None)
def _abi():
    """(structs, prototypes) of all three headers in one table each: what struct() and the binders look names up in."""
    return tuple({**a, **b} for a, b in zip(_headers(), encode_header()))


@functools.lru_cache(maxsize=None)
def struct(name):
    """The ctypes.Structure of a struct of the headers (needs the header only, not the library)."""
    return type(name, (ctypes.Structure,), {"_fields_": _abi()[0][name]})


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RoitrError(
                f"{LIB_PATH} is missing: build it with `python -m roitr_amd.build` "
                "(hipcc --offload-arch=gfx950).  roitr_amd has no CPU fallback.")
        # torch first: the library must bind to the HIP runtime torch brings along.  Loaded before torch, it pulls in the system
        # libamdhip64 and the process ends up with two runtimes -- the engine then sees "no ROCm-capable device" (build() followed by
        # smoke() in one process did exactly that).  torch is the package's device-memory / stream plumbing anyway.
        import torch  # noqa: F401
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.roitr_last_error.restype = ctypes.c_char_p
        _lib.roitr_knn_workspace_bytes.restype = ctypes.c_size_t
        _lib.roitr_geo_table_floats.restype = ctypes.c_size_t
        for name in ("roitr_engine_create",):
            if hasattr(_lib, name):
                getattr(_lib, name).restype = ctypes.c_void_p
        _assign(_lib, BOUND)
    return _lib


def _assign(handle, names):
    protos = _abi()[1]
    for name in names:
        getattr(handle, name).restype, getattr(handle, name).argtypes = protos[name]


def bind(names):
    """restype / argtypes from the header for a module's own entry points (those not listed in BOUND); returns the library."""
    handle = lib()
    _assign(handle, names)
    return handle


def binder(names):
    """A function that returns the library with `names` bound from the header; it binds on its first call (binding parses the headers)."""
    return functools.lru_cache(maxsize=None)(lambda: bind(names))


def check(status, what=""):
    if status != 0:
        raise RoitrError(f"{what} failed with status {status}: {lib().roitr_last_error().decode()}")


def ptr(t):
    """Device pointer of a torch tensor (or None -> NULL).  A host tensor is an error, not a fallback: every entry point of the
    library dereferences its pointers on the device."""
    if t is None:
        return ctypes.c_void_p(0)
    if not t.is_cuda:
        raise RoitrError("roitr_amd needs ROCm device tensors (no CPU fallback): got a tensor on " + str(t.device))
    return ctypes.c_void_p(t.data_ptr())


def host_ptr(t):
    """Pointer of a HOST tensor, for the few host-side entry points (roitr_geo_table_build)."""
    if t.is_cuda:
        raise RoitrError("host_ptr: expected a CPU tensor")
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def c_float(x):
    """A by-value float argument (ctypes would otherwise pass a Python float as a double)."""
    return ctypes.c_float(float(x))
