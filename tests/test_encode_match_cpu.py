"""CPU: the host side of encode once / match many (include/roitr_encode.h, roitr_amd/riga.py, roitr_amd/scene.py): the new structs
as roitr_amd/_lib.py reads them against the C compiler's layout of the header, the host-only size query of the cloud cache against the
documented per-cloud terms, the cloud-table arithmetic with 64-bit embedding offsets, and the pair chunking of scene.match_pairs."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_STRUCTS = ("RoitrCloudSeg", "RoitrCloudTable", "RoitrEncodeIO", "RoitrMatchIO", "RoitrCacheGather", "RoitrCachePatch")


def test_new_struct_layouts_match_the_compiler(tmp_path):
    """sizeof and every offsetof of the structs of include/roitr_encode.h as the C compiler lays them out from the header itself,
    against the ctypes classes roitr_amd/_lib.py makes from its own reading of it (the mechanism of
    test_abi_cpu.py::test_struct_layouts_match_the_compiler); riga.py uses those classes and declares none of its own."""
    from roitr_amd import _lib as L, riga
    from roitr_amd.build import HIPCC
    structs, protos = L.encode_header()
    assert tuple(structs) == NEW_STRUCTS and sum(len(f) for f in structs.values()) == 5 + 13 + 14 + 21 + 12 + 17
    assert set(protos) == {"roitr_engine_encode_bytes", "roitr_engine_encode", "roitr_engine_match", "roitr_cache_gather_nodes",
                           "roitr_cache_patch_gather"}
    for attr, name in dict(_CCloudSeg="RoitrCloudSeg", _CCloudTable="RoitrCloudTable", _CEncodeIO="RoitrEncodeIO", _CMatchIO="RoitrMatchIO").items():
        assert getattr(riga, attr) is L.struct(name), attr
    assert "ctypes.Structure" not in open(os.path.join(ROOT, "roitr_amd", "riga.py")).read()
    # the two headers of before still read as they did: the new structs live in a header of their own
    assert len(L.header_structs()) == 14 and not set(L.header_structs()) & set(structs)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "roitr_encode.h"', 'int main(void) {']
    for name, fields in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in fields]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["return 0; }", ""]))
    subprocess.run([HIPCC, "-x", "c", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)
    want = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    got = {}
    for name, fields in structs.items():
        got[name] = str(ctypes.sizeof(L.struct(name)))
        got.update({f"{name}.{f}": str(getattr(L.struct(name), f).offset) for f, _ in fields})
    assert len(want) == 6 + 82 and got == want, sorted(set(got.items()) ^ set(want.items()))
    # the 64-bit field is 64 bits, and the ABI version did not move
    assert L.struct("RoitrCloudSeg").emb0.size == 8 and ctypes.sizeof(L.struct("RoitrCloudSeg")) == 24
    assert L.lib().roitr_abi_version() == 4


def documented_bytes(n_points, C, Lm):
    """The per-cloud terms of include/roitr_encode.h, written out once more: 4 * (3 n + C n + 3 n4 + n4 + 2 L n4 + C n4 + C n4^2)."""
    total = 0
    for n in n_points:
        n4 = n // 4 // 4 // 4
        total += 4 * (3 * n + C * n + 3 * n4 + n4 + 2 * Lm * n4 + C * n4 + C * n4 * n4)
    return total


def test_size_query_is_host_only_and_sums_the_documented_terms():
    from roitr_amd import riga
    lib = riga._cache_lib()
    assert lib.roitr_engine_encode_bytes.restype is ctypes.c_size_t
    for sizes, C, Lm in (([5000], 256, 64), ([1024, 1024, 1500, 2300, 5000, 5000], 256, 64), ([8000, 300], 512, 32)):
        arr = (ctypes.c_int * len(sizes))(*sizes)
        per = (ctypes.c_size_t * 8)()
        total = lib.roitr_engine_encode_bytes(len(sizes), arr, C, Lm, per)   # no device is touched: this test runs without one
        assert total == documented_bytes(sizes, C, Lm) == sum(per)
        assert (list(per), total) == riga.cache_bytes(sizes, C, Lm)
        assert lib.roitr_engine_encode_bytes(len(sizes), arr, C, Lm, None) == total
    assert documented_bytes([5000], 256, 64) == 11531072            # "about 11.5 MB per cloud at N = 5000 in fp32"
    small = (ctypes.c_int * 2)(5000, 255)
    assert lib.roitr_engine_encode_bytes(2, small, 256, 64, None) == 0   # a cloud below 256 points (4 superpoints) is refused
    assert lib.roitr_engine_encode_bytes(0, small, 256, 64, None) == 0


def test_cloud_table_arithmetic_keeps_64_bit_embedding_offsets():
    from roitr_amd import riga
    C = 256
    seg = riga.cloud_segments([5000] * 600)            # 600 clouds of 78 nodes
    assert all(s.n_nodes == 78 and s.n_points == 5000 for s in seg)
    for c in (0, 1, 299, 599):
        assert (seg[c].pt_row0, seg[c].node_row0, seg[c].emb0) == (5000 * c, 78 * c, 78 * 78 * c)
    end = seg[599].emb0 + 78 * 78                      # entries of C floats
    assert end == 600 * 6084 and end * C * 4 == 3738009600 > 2 ** 31     # the cache's E: byte offsets past 2^31 (and past 2^31 floats below)
    # ragged sizes: every segment starts where the one before ends
    sizes = [1024, 1500, 2300, 5000, 257, 4999]
    seg = riga.cloud_segments(sizes)
    pt = nd = emb = 0
    for s, n in zip(seg, sizes):
        n4 = n // 64
        assert (s.pt_row0, s.n_points, s.node_row0, s.n_nodes, s.emb0) == (pt, n, nd, n4, emb)
        pt, nd, emb = pt + n, nd + n4, emb + n4 * n4
    # enough clouds for the ELEMENT offset (floats) to pass 2^31 as well: the field holds it, an int32 would not
    seg = riga.cloud_segments([5000] * 1500)
    assert seg[1499].emb0 * C == 1499 * 6084 * 256 > 2 ** 31
    assert ctypes.c_int(seg[1499].emb0 * C).value != seg[1499].emb0 * C


class StubModel:
    """Records the order of the calls scene.match_pairs makes."""

    def __init__(self):
        self.log, self.live = [], 0

    def encode_clouds(self, clouds, clouds_per_call=128):
        self.log.append(("encode", len(clouds), clouds_per_call))
        return type("Enc", (), {"table": None, "n": len(clouds)})()

    def launch_match(self, enc, pairs):
        self.live += 1
        assert self.live <= 2                      # never more than two calls in flight
        self.log.append(("launch", list(pairs)))
        return list(pairs)

    def finish_batch(self, handle):
        self.live -= 1
        self.log.append(("finish", handle))
        return [("result", p) for p in handle]


def test_match_pairs_chunks_in_order_with_two_calls_in_flight():
    from roitr_amd import scene
    pairs = [(i, j) for i in range(5) for j in range(i + 1, 5)]          # 10 pairs
    assert scene.chunk_pairs(pairs, 4) == [pairs[0:4], pairs[4:8], pairs[8:10]]
    assert scene.chunk_pairs(pairs, 10) == [pairs] and scene.chunk_pairs(pairs, 512) == [pairs] and scene.chunk_pairs([], 4) == []
    with pytest.raises(ValueError):
        scene.chunk_pairs(pairs, 0)
    m = StubModel()
    got = list(scene.match_pairs(m, ["c"] * 5, pairs, pairs_per_call=4))
    assert got == [(p, ("result", p)) for p in pairs]                     # list order, one result per pair
    kinds = [e[0] for e in m.log]
    assert kinds == ["encode", "launch", "launch", "finish", "launch", "finish", "finish"]   # encoded once; call s + 1 queued before s is awaited
    assert m.log[0] == ("encode", 5, 128)
    assert [e[1] for e in m.log if e[0] == "launch"] == scene.chunk_pairs(pairs, 4)
    # an empty list encodes nothing; an encoded cache is taken as it is
    m = StubModel()
    assert list(scene.match_pairs(m, ["c"] * 5, [], pairs_per_call=4)) == [] and m.log == []
    enc = m.encode_clouds(["c"] * 3)
    assert len(list(scene.match_pairs(m, enc, [(0, 1), (1, 2)], pairs_per_call=1))) == 2
    assert [e[0] for e in m.log].count("encode") == 1
