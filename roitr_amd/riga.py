"""Host-side mirror of the reference's model API for the inference path.

`create_model(config)` / `RIGA_v2(config)` follow model/RIGA_v2.py:11-181 (reference): the same
constructor config keys, the same `forward(src_pcd, tgt_pcd, src_feats, tgt_feats,
src_normals, tgt_normals, rot, trans, src_raw_pcd)` signature and the same output dict keys
(model/RIGA_v2.py:70-173), and -- so that the released checkpoints load unchanged through a strict
`load_state_dict` (lib/trainer.py:94-130) -- the same 522-entry state_dict layout.

The module tree below only HOLDS parameters; all arithmetic happens in libroitr_hip.so through the
engine (csrc/engine.cpp).  There is no PyTorch compute path and no CPU fallback.
"""
import ctypes
import math
import time

import numpy as np
import torch
import torch.nn as nn

from . import _args as A
from . import _lib as L


# ----------------------------------------------------------------------------------------------
# state_dict layout (names follow the reference module tree: model/model.py:146-184,
# model/transformer/ppftransformer.py:202-225, geotransformer.py:62-92, geoattention.py, RIGA_v2.py:14-53)
# ----------------------------------------------------------------------------------------------
def _linear(prefix, out, inp):
    return [(prefix + ".weight", (out, inp), "param"), (prefix + ".bias", (out,), "param")]


def _norm(prefix, c):
    return [(prefix + ".weight", (c,), "param"), (prefix + ".bias", (c,), "param")]


def _local_transformer(prefix, inp, hidden, out):
    ent = [(prefix + ".embedding.embedding.div_term", (hidden // 2,), "buffer")]
    ent += _linear(prefix + ".embedding.proj", hidden, 4)
    ent += _linear(prefix + ".in_proj", hidden, inp)
    for n in ("proj_q", "proj_k", "proj_v", "proj_p", "proj_vp"):
        ent += _linear(prefix + ".transformer.attention." + n, hidden, hidden)
    ent += _linear(prefix + ".transformer.linear", hidden, hidden)
    ent += _norm(prefix + ".transformer.norm", hidden)
    ent += _linear(prefix + ".out_proj", out, hidden)
    return ent


def _ffn(prefix, c):
    return _linear(prefix + ".expand", 2 * c, c) + _linear(prefix + ".squeeze", c, 2 * c) + _norm(prefix + ".norm", c)


def state_dict_layout(factor=1, architecture=("self", "cross", "self", "cross", "self", "cross"), blocks=(2, 3, 3, 3)):
    """[(key, shape, 'param'|'buffer')] in the reference's registration order."""
    f = factor
    planes = [64 * f, 128 * f, 256 * f, 256 * f]
    ent = []
    inp = 1
    for lvl in range(4):
        pl = planes[lvl]
        hid = min(pl, 256 * f)
        e = f"backbone.enc{lvl + 1}"
        ent += _local_transformer(e + ".0.transformer", inp, hid, pl)
        for b in range(1, blocks[lvl]):
            ent += _local_transformer(f"{e}.{b}.transformer.transformer", pl, hid, pl)
            ent += _norm(f"{e}.{b}.bn2", pl)
        inp = pl
    for lvl in (3, 2, 1, 0):
        pl = planes[lvl]
        hid = min(pl, 256 * f)
        d = f"backbone.dec{lvl + 1}"
        if lvl == 3:
            ent += _linear(d + ".0.linear1.0", pl, 2 * pl) + _norm(d + ".0.linear1.1", pl)
            ent += _linear(d + ".0.linear2.0", pl, pl)
        else:
            ent += _linear(d + ".0.linear1.0", pl, pl) + _norm(d + ".0.linear1.1", pl)
            ent += _linear(d + ".0.linear2.0", pl, planes[lvl + 1]) + _norm(d + ".0.linear2.1", pl)
        ent += _local_transformer(d + ".1.transformer.transformer", pl, hid, pl)
        ent += _norm(d + ".1.bn2", pl)
    c = 256 * f
    g = "backbone.global_transformer"
    ent += [(g + ".embedding.embedding.div_term", (c // 2,), "buffer")]
    ent += _linear(g + ".embedding.proj_d", c, c) + _linear(g + ".embedding.proj_a", c, c)
    ent += _linear(g + ".in_proj", c, c)
    for i, kind in enumerate(architecture):
        lp = f"{g}.transformer.layers.{i}"
        at = lp + ".attention.attention"
        names = ("proj_q", "proj_k", "proj_v", "proj_p", "proj_vp") if kind == "self" else ("proj_q", "proj_k", "proj_v")
        for n in names:
            ent += _linear(f"{at}.{n}", c, c)
        ent += _linear(lp + ".attention.linear", c, c) + _norm(lp + ".attention.norm", c)
        if kind == "self":
            ent += _linear(lp + ".attention.pos_linear", c, c) + _norm(lp + ".attention.pos_norm", c)
        ent += _ffn(lp + ".output", c)
        if kind == "self":
            ent += _ffn(lp + ".pos_proj", c)
    ent += _linear(g + ".out_proj", c, c)
    ent += _linear("backbone.occ_proj", 1, c)
    ent += [("OT.alpha", (), "param")]
    ent += _linear("coarse_proj", c, c)
    ent += _linear("fine_proj", c, 64 * f)
    ent += [("optimal_transport.alpha", (), "param")]
    return ent


def div_term(d_model):
    """SinusoidalPositionalEmbedding buffer, positional_encoding.py:43-45, in float32 like torch."""
    idx = torch.arange(0, d_model, 2).float()
    return torch.exp(idx * (-np.log(10000.0) / d_model))


class _Holder(nn.Module):
    """Bare container: gives the parameters their reference names."""


def _attach(root, key, tensor, kind):
    parts = key.split(".")
    mod = root
    for p in parts[:-1]:
        if p not in mod._modules:
            mod.add_module(p, _Holder())
        mod = mod._modules[p]
    if kind == "param":
        mod.register_parameter(parts[-1], nn.Parameter(tensor, requires_grad=False))
    else:
        mod.register_buffer(parts[-1], tensor)


_CConfig = L.struct("RoitrEngineConfig")
_CForwardIO = L.struct("RoitrForwardIO")
# encode once, match many (include/roitr_encode.h)
_CCloudSeg = L.struct("RoitrCloudSeg")
_CCloudTable = L.struct("RoitrCloudTable")
_CEncodeIO = L.struct("RoitrEncodeIO")
_CMatchIO = L.struct("RoitrMatchIO")
_cache_lib = L.binder(["roitr_engine_encode_bytes", "roitr_engine_encode", "roitr_engine_match"])
CACHE_ARRAYS = ("points", "point_feats", "node_xyz", "node_masks", "node_knn_idx", "node_knn_mask", "node_geo", "embedding")


def cloud_segments(n_points):
    """The RoitrCloudSeg entries of clouds of n_points[c] points cached back to back (a ctypes array, host): first point row and
    count, first node row and count (n4 = n // 64 by the floor rule of level_sizes) and the first entry of the cloud's n4 x n4 block
    of E -- in entries of C floats, a 64-bit count: 600 clouds of 5000 points are 3.65 million entries, 3.7 GB of fp32 at C = 256."""
    seg = (_CCloudSeg * len(n_points))()
    pt = nd = emb = 0
    for c, n in enumerate(n_points):
        n4 = RIGA_v2.level_sizes(int(n))[3]
        seg[c].pt_row0, seg[c].n_points, seg[c].node_row0, seg[c].n_nodes, seg[c].emb0 = pt, int(n), nd, n4, emb
        pt, nd, emb = pt + int(n), nd + n4, emb + n4 * n4
    return seg


def cache_bytes(n_points, channels, limit):
    """Bytes of the eight cache arrays (CACHE_ARRAYS order) for these clouds and their sum: the documented per-cloud terms
    4 * (3 n, C n, 3 n4, n4, L n4, L n4, C n4, C n4^2), in Python (roitr_engine_encode_bytes is the library's own count)."""
    per = [0] * 8
    for n in n_points:
        n4 = RIGA_v2.level_sizes(int(n))[3]
        for i, t in enumerate((3 * n, channels * n, 3 * n4, n4, limit * n4, limit * n4, channels * n4, channels * n4 * n4)):
            per[i] += 4 * int(t)
    return per, sum(per)


class EncodedClouds:
    """The cloud cache of RIGA_v2.encode_clouds: the eight arrays (`arrays`, CACHE_ARRAYS), the cloud table on the host (`seg`) and
    on the device, the host copies of the counts, and the weight signature of the model at encode time."""

    def __init__(self, arrays, n_points, channels, limit, signature, engine):
        self.arrays, self.n_points, self.channels, self.limit = arrays, [int(n) for n in n_points], channels, limit
        self.n4 = [RIGA_v2.level_sizes(n)[3] for n in self.n_points]
        self.seg = cloud_segments(self.n_points)
        dev = arrays["points"].device
        # uploaded from pinned memory on the current stream: nothing here waits for the GPU (the pinned copy lives as long as the cache)
        self._seg_pin = torch.frombuffer(bytearray(bytes(self.seg)), dtype=torch.uint8).pin_memory()
        self.seg_dev = self._seg_pin.to(dev, non_blocking=True)
        self.signature, self.engine = signature, engine
        t = _CCloudTable()
        t.n_clouds, t.channels, t.limit = len(self.n_points), channels, limit
        for k in CACHE_ARRAYS:
            setattr(t, k, L.ptr(arrays[k]))
        t.seg = ctypes.cast(self.seg, ctypes.c_void_p)
        t.seg_dev = L.ptr(self.seg_dev)
        self.table = t
        self.nbytes = sum(a.numel() * a.element_size() for a in arrays.values())

    def __len__(self):
        return len(self.n_points)

    def cloud(self, c):
        """Views of cloud c's rows in the cache arrays (the embedding as (n4, n4, C))."""
        s, n4 = self.seg[c], self.n4[c]
        out = {k: self.arrays[k][s.pt_row0:s.pt_row0 + s.n_points] for k in ("points", "point_feats")}
        out.update({k: self.arrays[k][s.node_row0:s.node_row0 + n4] for k in ("node_xyz", "node_masks", "node_knn_idx", "node_knn_mask", "node_geo")})
        out["embedding"] = self.arrays["embedding"][s.emb0:s.emb0 + n4 * n4].view(n4, n4, self.channels)
        return out


def _cfg_get(config, key, default=None):
    if isinstance(config, dict):
        return config.get(key, default)
    return getattr(config, key, default)


class LazyDict(dict):
    """Output dict whose dtype conversions (int32 -> int64 indices, int32 -> bool masks; the reference's dtypes)
    run only when a key is read: the tester reads 10 of the 22 keys (lib/tester.py:59-65)."""

    def __getitem__(self, k):
        v = dict.__getitem__(self, k)
        if callable(v):
            v = v()
            dict.__setitem__(self, k, v)
        return v

    def get(self, k, default=None):
        return self[k] if k in self else default

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]


class RIGA_v2(nn.Module):
    """The RoITr pipeline (model/RIGA_v2.py:11-175) on the MI355X engine."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.benchmark = _cfg_get(config, "benchmark")
        self.with_cross_pos_embed = _cfg_get(config, "with_cross_pos_embed", True)
        self.factor = 1 if self.benchmark in ("3DMatch", "3DLoMatch") else 2
        self.architecture = list(_cfg_get(config, "transformer_architecture"))
        self.mode = _cfg_get(config, "mode", "test")
        self.point_per_patch = int(_cfg_get(config, "point_per_patch", 64))
        self.matching_radius = float(_cfg_get(config, "matching_radius", 0.05))
        self.num_est_coarse_corr = int(_cfg_get(config, "num_est_coarse_corr", 256))
        self.fine_topk = int(_cfg_get(config, "fine_matching_topk", 3))
        self.fine_mutual = bool(_cfg_get(config, "fine_matching_mutual", True))
        self.fine_conf = float(_cfg_get(config, "fine_matching_confidence_threshold", 0.05))
        self.fine_use_dustbin = bool(_cfg_get(config, "fine_matching_use_dustbin", False))
        self.fine_use_global_score = bool(_cfg_get(config, "fine_matching_use_global_score", False))
        # not a reference key: 'f32' (default, the reference's arithmetic), 'bf16' (bf16 operand storage of the dense layers) or 'f32x3'
        # (fp32 like 'f32'; the K >= 256 linear layers multiply on the bf16 matrix cores by a three-way operand split, csrc/gemm_x3.hip)
        self.operand_dtype = str(_cfg_get(config, "operand_dtype", "f32"))
        if self.operand_dtype not in ("f32", "bf16", "f32x3"):
            raise ValueError(f"operand_dtype must be 'f32', 'bf16' or 'f32x3', got {self.operand_dtype!r}")
        # not a reference key (4DMatch only): AVERAGE number of patch slots per pair a call's per-patch buffers are sized for.  The adaptive
        # matching may select every node pair (n4max^2 = 15 625 per pair at N = 8000: 33 KB of tail buffers each); the reference runs the
        # tail on the selected ones only (RIGA_v2.py:126-152), so does the engine (compacted patch list).  A call that selects more than
        # B x this many is repeated once with the exact number (finish_batch): results never depend on the value.
        self.patch_slots_per_pair = int(_cfg_get(config, "patch_slots_per_pair", 2048))
        if self.fine_use_dustbin:
            raise NotImplementedError("fine_matching_use_dustbin=True is not on the reference's test configs")
        for key, shape, kind in state_dict_layout(self.factor, self.architecture):
            if kind == "buffer":
                t = div_term(shape[0] * 2)
            elif len(shape) == 2:  # nn.Linear default init range, deterministic content comes from load_state_dict
                t = torch.empty(shape).uniform_(-1.0 / math.sqrt(shape[1]), 1.0 / math.sqrt(shape[1]))
            elif len(shape) == 1:
                t = torch.ones(shape) if key.endswith(".weight") else torch.zeros(shape)
            else:
                t = torch.tensor(1.0)
            _attach(self, key, t, kind)
        self._engine = None
        # host-side milliseconds spent inside launch_batch (packing, allocation, the engine call's ~350 launches) and inside finish_batch
        # AFTER the device has answered (per-pair unpacking); bench.py reports them per step (host share at 8 ranks)
        self.host_ms = {"launch": 0.0, "unpack": 0.0, "calls": 0}
        # launch_batch default: True = the pairs handed to it are complete device tensors with nothing pending on the current
        # stream (a resident pool, a loader that synchronised its copies) -- see launch_batch(inputs_resident=...)
        self.inputs_resident = False
        self.weights_frozen = False      # True: skip the per-forward "did a weight change" check (see _ensure_engine)
        self._pack_stream = None
        self._engine_sig = None
        self._holders = []

    # ---------------------------------------------------------------- engine plumbing
    def _make_engine(self):
        lib = L.lib()
        cfg = _CConfig()
        cfg.factor = self.factor
        cfg.num_corr = self.num_est_coarse_corr
        cfg.point_limit = self.point_per_patch
        cfg.fine_topk = self.fine_topk
        cfg.fine_mutual = int(self.fine_mutual)
        cfg.fine_use_global_score = int(self.fine_use_global_score)
        cfg.fine_conf = self.fine_conf
        cfg.n_geo_layers = len(self.architecture)
        for i, a in enumerate(self.architecture):
            cfg.geo_is_cross[i] = 0 if a == "self" else 1
        cfg.matching_radius = self.matching_radius
        cfg.adaptive_coarse = 0 if self.factor == 1 else 1
        cfg.occlusion_radius = 0.0375
        cfg.operand_dtype = {"f32": 0, "bf16": 1, "f32x3": 2}[self.operand_dtype]
        lib.roitr_engine_create.restype = ctypes.c_void_p
        h = lib.roitr_engine_create(ctypes.byref(cfg))
        if not h:
            raise L.RoitrError("roitr_engine_create failed")
        return ctypes.c_void_p(h)

    def sync_engine(self):
        """(Re)register every parameter's device pointer with the engine and rebuild the derived weights."""
        lib = L.lib()
        if self._engine is None:
            self._engine = self._make_engine()
            self._engine_token = object()   # what a cloud cache remembers of its engine (an address could be reused by a later one)
        for k, v in self.state_dict(keep_vars=True).items():
            if not v.is_cuda:
                raise L.RoitrError(f"parameter {k} is not on a ROCm device: call model.cuda() (no CPU fallback)")
            if v.dtype != torch.float32 or not v.is_contiguous():
                raise L.RoitrError(f"parameter {k} must be contiguous float32")
            L.check(lib.roitr_engine_set_param(self._engine, k.encode(), L.ptr(v), ctypes.c_long(v.numel())), "set_param")
        L.check(lib.roitr_engine_finalize(self._engine, L.stream_ptr()), "engine_finalize")
        self._holders = list(self.modules())       # the holder tree is fixed after construction; its tensors may be replaced or updated
        self._engine_sig = self._weights_signature()

    def _weights_signature(self):
        """(address, version) of every parameter / buffer, read through the holder modules' own dicts: in-place updates
        (load_state_dict, an optimizer step), .cuda() / .to() and a replaced Parameter object all change it.  This runs in front
        of every forward: walking state_dict() instead (prefix strings, hooks, 409 modules) cost ~0.5 ms of the 2.3 ms a
        one-pair call takes on the host."""
        return [(t.data_ptr(), t._version) for m in self._holders for d in (m._parameters, m._buffers) for t in d.values() if t is not None]

    def _ensure_engine(self):
        # weights_frozen: the caller states that no parameter changes until it says so (an inference loop): the 0.3 ms signature walk in
        # front of every forward is skipped -- it is a sixth of the host's time in a one-pair call; sync_engine() re-registers explicitly
        if self._engine is None or (not self.weights_frozen and self._weights_signature() != self._engine_sig):
            self.sync_engine()

    def set_tap(self, name, tensor):
        self._ensure_engine()
        self._taps = getattr(self, "_taps", {})
        self._taps[name] = tensor
        L.lib().roitr_engine_set_tap(self._engine, name.encode(), L.ptr(tensor))

    def set_inject(self, name, tensor):
        self._ensure_engine()
        self._injects = getattr(self, "_injects", {})
        self._injects[name] = tensor
        L.lib().roitr_engine_set_inject(self._engine, name.encode(), L.ptr(tensor))

    def set_phase_overlap(self, on=1):
        """Global transformer + coarse front on the engine's branch stream beside the decoder: 1 (default) for calls large enough for it to
        pay, 2 for every call, 0 never (the same launches on the main stream).  The results are the same bytes in every mode."""
        self._ensure_engine()
        L.check(L.lib().roitr_engine_set_phase_overlap(self._engine, ctypes.c_int(int(on))), "set_phase_overlap")

    def set_ln256_min_rows(self, rows=-1):
        """Rows per launch from which the 256-wide fp32 Linear + LayerNorm layers run as one launch (csrc/gemm_ln256.hip): 0 never, < 0 the
        built-in default.  The results are the same bytes either way (for the tests)."""
        self._ensure_engine()
        L.check(L.lib().roitr_engine_set_ln256_min_rows(self._engine, ctypes.c_int(int(rows))), "set_ln256_min_rows")

    def scratch_info(self):
        """Diagnostics of the engine's scratch: capacities and fills of the main and the branch arena in bytes, and whether the last forward
        queued its branch (global transformer + coarse front) on the engine's branch stream."""
        self._ensure_engine()
        out = (ctypes.c_long * 5)()
        L.check(L.lib().roitr_engine_scratch_info(self._engine, out), "scratch_info")
        return {"main_cap": out[0], "main_peak": out[1], "branch_cap": out[2], "branch_fill": out[3], "on_branch_stream": bool(out[4])}

    PROF_CLASSES = {"fps_kernel": 0, "knn_query_kernel": 1, "grid_build_kernel": 2, "knn_replay_kernel": 3, "phase.geometry": 4,
                    "phase.encoder": 5, "phase.global_transformer": 6, "phase.decoder": 7, "phase.matching": 8,
                    "phase.forward": 9, "ot_kernel": 10, "local_attn_kernel": 11, "gemm_kernel.mfma_roofed": 12, "mha_kernel": 13,
                    "geo_embed_kernel": 14, "geo_table_kernel": 15, "geo_embed_reference_flops": 16, "local_block_kernel": 17,
                    "gemm_kernel.hbm_roofed": 18}

    @staticmethod
    def profile_reset(enable=True):
        """HIP-event instrumentation of the dominant kernels (csrc/prof.cpp); off by default."""
        lib = L.lib()
        lib.roitr_prof_enable(1 if enable else 0)
        lib.roitr_prof_reset()

    @classmethod
    def profile_read(cls, kernels_only=True):
        lib = L.lib()
        out = {}
        for name, cid in cls.PROF_CLASSES.items():
            ms, n, by = ctypes.c_double(0), ctypes.c_long(0), ctypes.c_double(0)
            lib.roitr_prof_read(cid, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(by))
            aux = ctypes.c_double(0)
            lib.roitr_prof_read_aux(cid, ctypes.byref(aux))
            if n.value and (not kernels_only or not name.startswith("phase.")):
                # bytes: algorithmic HBM bytes (FLOPs for gemm_kernel / geo_embed_kernel / the phases); aux: algorithmic HBM bytes
                # of the MFMA classes and of every instrumented launch inside a phase (csrc/prof.cpp)
                out[name] = {"ms": ms.value, "launches": n.value, "bytes": by.value, "aux": aux.value}
        # the GEMM family as one entry (what rounds 1-4 reported) next to its two halves: launches whose roof is the matrix pipe and
        # launches whose roof is HBM (algorithmic FLOPs per algorithmic byte below the machine balance, csrc/prof.cpp)
        parts = [out[k] for k in ("gemm_kernel.mfma_roofed", "gemm_kernel.hbm_roofed") if k in out]
        if parts:
            out["gemm_kernel"] = {f: sum(p[f] for p in parts) for f in ("ms", "launches", "bytes", "aux")}
        lib.roitr_prof_enable(0)
        return out

    def geo_table_info(self):
        """The function table the engine evaluates the geometric embedding from (csrc/geo_table.hip), or None when the GEMM form is
        in use: {interval, n_int_d, n_int_a, fit_d, amp_d, fit_a, amp_a, rel_d, rel_a, lds_bytes} (fit = float64 |polynomial - function|
        on 64 probe points per interval, rel = the largest per-channel error over that channel's amplitude: the acceptance gate)."""
        self._ensure_engine()
        info = (ctypes.c_double * 9)()
        if not L.lib().roitr_engine_geo_table_info(self._engine, info):
            return None
        keys = ("interval", "n_int_d", "n_int_a", "fit_d", "amp_d", "fit_a", "amp_a", "rel_d", "rel_a")
        out = dict(zip(keys, list(info)))
        out["lds_bytes"] = int((out["n_int_d"] + out["n_int_a"]) * 8 * 64 * 4)   # per workgroup: one 64-channel slice of the table
        return out

    def __del__(self):
        try:
            if self._engine is not None:
                L.lib().roitr_engine_destroy(self._engine)
        except Exception:
            pass

    # ---------------------------------------------------------------- forward
    @staticmethod
    def level_sizes(n):
        return [n, n // 4, n // 4 // 4, n // 4 // 4 // 4]

    def forward_batch(self, pairs, want_gt=True, graph=False):
        """pairs: list of dicts with the forward() arguments as keys.  Returns a list of output dicts.

        All B pairs go through the engine in ONE batched pass (clouds laid out src_0..src_{B-1},
        tgt_0..tgt_{B-1}); the only host synchronisation is the final read of the correspondence count."""
        return self.finish_batch(self.launch_batch(pairs, want_gt, graph=graph))

    GRAPH_RING = 3   # persistent io buffer sets per shape in graph mode

    @staticmethod
    def _have_gt(pairs, want_gt):
        """The ground-truth side outputs need rot AND trans for EVERY pair of the batch; a mixed batch is an error
        (the engine computes them for all pairs of a call or for none)."""
        if not want_gt:
            return False
        flags = [p.get("rot") is not None and p.get("trans") is not None for p in pairs]
        if any(flags) and not all(flags):
            missing = [i for i, f in enumerate(flags) if not f]
            raise L.RoitrError(f"pairs {missing} of this batch have no rot/trans while others do: pass want_gt=False or give "
                               "every pair its ground-truth transform")
        return all(flags)

    def _patch_geometry(self, B, n4, patch_slots=None):
        """(P, slots): coarse-list slots per pair, and patch slots of the whole call.  3DMatch: P = num_est_coarse_corr, slots = B * P
        (strided: patch p of pair b at slot b * P + p).  4DMatch: P = n4max^2 bounds the coarse lists only, the per-patch buffers
        hold the selected patches of all pairs back to back in `slots` slots (RoitrForwardIO::patch_slots)."""
        if self.factor == 1:
            P = self.num_est_coarse_corr
            return P, B * P
        n4max = max(n4)
        P = n4max * n4max
        slots = B * min(P, self.patch_slots_per_pair) if patch_slots is None else int(patch_slots)
        return P, max(1, min(slots, B * P))

    def _alloc_outputs(self, dev, B, T, n4, have_gt, patch_slots=None):
        f32, i32 = torch.float32, torch.int32
        T4, n4max = sum(n4), max(n4)
        C = 256 * self.factor
        P, S = self._patch_geometry(B, n4, patch_slots)
        Lm = self.point_per_patch
        cap = S * Lm * self.fine_topk * (1 if self.fine_mutual else 2)   # row top-k OR column top-k when not mutual
        z = lambda shape, dt=f32: torch.empty(shape, dtype=dt, device=dev)  # every buffer is fully written by the engine (dead patch slots are never read)
        out = dict(node_xyz=z((T4, 3)), node_feats=z((T4, C)), point_feats=z((T, C)), node_masks=z((T4,), i32),
                   node_knn_idx=z((T4, Lm), i32), node_knn_mask=z((T4, Lm), i32), tgt_corr=z((B, P), i32), src_corr=z((B, P), i32),
                   corr_scores=z((B, P)), n_corr=z((B,), i32), tgt_knn_pts=z((S, Lm, 3)), src_knn_pts=z((S, Lm, 3)),
                   tgt_knn_masks=z((S, Lm), i32), src_knn_masks=z((S, Lm), i32), matching_scores=z((S, Lm + 1, Lm + 1)),
                   out_tgt_pts=z((cap, 3)), out_src_pts=z((cap, 3)), out_scores=z((cap,)), out_patch=z((cap,), i32),
                   fine_offsets=z((S,), i32), n_out=z((1,), i32), pair_starts=z((B + 1,), i32))
        if have_gt:
            out.update(gt_node_occ=z((T4,)), gt_corr_idx=z((B, n4max * n4max, 2), i32), gt_corr_overlaps=z((B, n4max * n4max)),
                       gt_corr_count=z((B,), i32))
        return out, P, S

    def launch_batch(self, pairs, want_gt=True, graph=False, inputs_resident=None, patch_slots=None):
        """Enqueue the batched forward on the current stream and return a handle for finish_batch().  Nothing here waits
        for the GPU: a caller may launch batch s+1 before finishing batch s, so the device never idles while the host
        unpacks results (outputs are per-call tensors, the engine's scratch arena is re-used in stream order).

        graph=True: the forward of a repeated shape is replayed as ONE HIP graph launch (roitr_engine_forward_graph)
        instead of ~800 kernel launches -- what makes the one-pair-per-call mode fast.  The inputs are copied into, and the
        results live in, persistent buffers that are re-used every GRAPH_RING-th call of the same shape: consume a
        result before launching GRAPH_RING more batches of that shape.

        inputs_resident (default: self.inputs_resident): the caller states that the tensors of `pairs` are complete -- no copy
        or kernel producing them is still pending on the current stream.  The inputs are then packed on a side stream and the
        engine starts this forward's first sampling level beside the previous forward instead of behind it
        (RoitrForwardIO::inputs_ready; one pair per call with two calls in flight: 3.23 -> 2.33 ms per pair).  Same results."""
        self._ensure_engine()
        if graph:
            return self._launch_graph(pairs, want_gt)
        t_host = time.perf_counter()
        dev = pairs[0]["src_pcd"].device
        B = len(pairs)
        f32 = torch.float32
        n_src = [int(p["src_raw_pcd"].shape[0]) for p in pairs]
        n_tgt = [int(p["tgt_pcd"].shape[0]) for p in pairs]
        n_all = n_src + n_tgt
        T = sum(n_all)
        have_gt = self._have_gt(pairs, want_gt)
        cat = lambda ks, kt: torch.cat([p[ks].to(f32) for p in pairs] + [p[kt].to(f32) for p in pairs], 0).contiguous()

        def pack_inputs():
            rot = trans = None
            if have_gt:
                rot = torch.stack([p["rot"].reshape(3, 3).to(f32) for p in pairs]).contiguous()
                trans = torch.stack([p["trans"].reshape(3).to(f32) for p in pairs]).contiguous()
            return (cat("src_raw_pcd", "tgt_pcd"), cat("src_pcd", "tgt_pcd"), cat("src_normals", "tgt_normals"), cat("src_feats", "tgt_feats"),
                    rot, trans)

        ready = None
        if self.inputs_resident if inputs_resident is None else inputs_resident:
            # the pairs are complete device tensors already (nothing pending on the current stream): pack them on a stream of their
            # own and hand the engine an event, so the first sampling level of this forward starts beside the previous forward
            # instead of behind it on the current stream (RoitrForwardIO::inputs_ready)
            if self._pack_stream is None:
                self._pack_stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(self._pack_stream):
                geom, pout, nrm, feats, rot, trans = pack_inputs()
                ready = torch.cuda.Event()
                ready.record()
            # allocated under the pack stream, read by the forward on the current stream (and the engine's geometry stream, which is
            # joined into it): tell the caching allocator, so that a handle dropped before finish_batch cannot hand these blocks to the
            # next pack while the forward still reads them
            for t_ in (geom, pout, nrm, feats, rot, trans):
                if t_ is not None:
                    t_.record_stream(torch.cuda.current_stream())
        else:
            geom, pout, nrm, feats, rot, trans = pack_inputs()
        n4 = [self.level_sizes(n)[3] for n in n_all]
        out, P, slots = self._alloc_outputs(dev, B, T, n4, have_gt, patch_slots)
        io = _CForwardIO()
        io.pairs = B
        arr = (ctypes.c_int * (2 * B))(*n_all)
        io.n_points = ctypes.cast(arr, ctypes.c_void_p)
        io.points_geom, io.normals, io.feats, io.points_out = L.ptr(geom), L.ptr(nrm), L.ptr(feats), L.ptr(pout)
        io.rot, io.trans = L.ptr(rot), L.ptr(trans)
        io.inputs_ready = ready.cuda_event if ready is not None else None
        io.patch_slots = slots if self.factor != 1 else 0
        for k, v in out.items():
            setattr(io, k, L.ptr(v))
        L.check(L.lib().roitr_engine_forward(self._engine, ctypes.byref(io), L.stream_ptr()), "engine_forward")
        # one D2H transfer for all the counts: [first output row of every pair | total | n_corr per pair | gt counts],
        # queued behind this forward only (an event, not a stream sync, is waited on in finish_batch)
        parts = [out["pair_starts"], out["n_corr"]] + ([out["gt_corr_count"]] if have_gt else [])
        meta_dev = torch.cat(parts)
        meta_host = torch.empty(meta_dev.shape, dtype=meta_dev.dtype, pin_memory=True)
        meta_host.copy_(meta_dev, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        keep = (geom, pout, nrm, feats, rot, trans, arr, meta_dev, ready)   # inputs stay alive until the forward has run
        self.host_ms["launch"] += 1e3 * (time.perf_counter() - t_host)
        self.host_ms["calls"] += 1
        return dict(pairs=pairs, out=out, B=B, P=P, slots=slots, compacted=self.factor != 1, n_all=n_all, n4=n4, have_gt=have_gt, meta_host=meta_host, done=done, keep=keep,
                    relaunch=dict(want_gt=want_gt, inputs_resident=inputs_resident))

    def _launch_graph(self, pairs, want_gt):
        dev = pairs[0]["src_pcd"].device
        B = len(pairs)
        f32, i32 = torch.float32, torch.int32
        n_all = [int(p["src_raw_pcd"].shape[0]) for p in pairs] + [int(p["tgt_pcd"].shape[0]) for p in pairs]
        have_gt = self._have_gt(pairs, want_gt)
        key = (tuple(n_all), have_gt)
        if not hasattr(self, "_graph_slots"):
            self._graph_slots, self._graph_stream = {}, torch.cuda.Stream()
        ring = self._graph_slots.setdefault(key, {"pos": 0, "slots": []})
        T = sum(n_all)
        n4 = [self.level_sizes(n)[3] for n in n_all]
        P, slots = self._patch_geometry(B, n4)
        if len(ring["slots"]) < self.GRAPH_RING:
            z = lambda shape, dt=f32: torch.empty(shape, dtype=dt, device=dev)
            out, P, slots = self._alloc_outputs(dev, B, T, n4, have_gt)
            n_meta = (B + 1) + B + (B if have_gt else 0)
            slot = dict(geom=z((T, 3)), pout=z((T, 3)), nrm=z((T, 3)), feats=z((T, 1)), rot=z((B, 3, 3)) if have_gt else None,
                        trans=z((B, 3)) if have_gt else None, out=out, meta_dev=z((n_meta,), i32),
                        meta_host=torch.empty((n_meta,), dtype=i32, pin_memory=True), arr=(ctypes.c_int * (2 * B))(*n_all))
            io = _CForwardIO()
            io.pairs = B
            io.n_points = ctypes.cast(slot["arr"], ctypes.c_void_p)
            io.points_geom, io.normals, io.feats, io.points_out = L.ptr(slot["geom"]), L.ptr(slot["nrm"]), L.ptr(slot["feats"]), L.ptr(slot["pout"])
            io.rot, io.trans = L.ptr(slot["rot"]), L.ptr(slot["trans"])
            io.patch_slots = slots if self.factor != 1 else 0
            for k, v in out.items():
                setattr(io, k, L.ptr(v))
            slot["io"] = io
            ring["slots"].append(slot)
            slot_i = len(ring["slots"]) - 1
        else:
            slot_i = ring["pos"] % self.GRAPH_RING
        ring["pos"] += 1
        slot = ring["slots"][slot_i]
        out = slot["out"]
        gs = self._graph_stream
        gs.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(gs):
            cat = lambda ks, kt, dst: torch.cat([p[ks].to(f32) for p in pairs] + [p[kt].to(f32) for p in pairs], 0, out=dst)
            cat("src_raw_pcd", "tgt_pcd", slot["geom"]); cat("src_pcd", "tgt_pcd", slot["pout"])
            cat("src_normals", "tgt_normals", slot["nrm"]); cat("src_feats", "tgt_feats", slot["feats"])
            if have_gt:
                torch.stack([p["rot"].reshape(3, 3).to(f32) for p in pairs], out=slot["rot"])
                torch.stack([p["trans"].reshape(3).to(f32) for p in pairs], out=slot["trans"])
            L.check(L.lib().roitr_engine_forward_graph(self._engine, ctypes.byref(slot["io"]), L.stream_ptr()), "engine_forward_graph")
            parts = [out["pair_starts"], out["n_corr"]] + ([out["gt_corr_count"]] if have_gt else [])
            torch.cat(parts, out=slot["meta_dev"])
            slot["meta_host"].copy_(slot["meta_dev"], non_blocking=True)
            done = torch.cuda.Event()
            done.record()
        # the replay ran on the private capture stream: order every later use of the engine's shared scratch arena and of
        # these output slots (a plain launch_batch, evaluate_batch, user code on the current stream) behind it
        torch.cuda.current_stream().wait_stream(gs)
        keep = (slot["geom"], slot["pout"], slot["nrm"], slot["feats"], slot["rot"], slot["trans"], slot["arr"], slot["meta_dev"])
        return dict(pairs=pairs, out=out, B=B, P=P, slots=slots, compacted=self.factor != 1, n_all=n_all, n4=n4, have_gt=have_gt, meta_host=slot["meta_host"], done=done, keep=keep,
                    relaunch=dict(want_gt=want_gt, inputs_resident=False))

    def max_scores_per_pair(self):
        """Exact upper bound of the correspondences one pair can emit under the 3DMatch settings (mutual top-k fine matching on
        num_est_coarse_corr patches); the adaptive 4DMatch matching may select every node pair, so it has no such bound."""
        from .shard import max_scores_per_pair
        return max_scores_per_pair(self.num_est_coarse_corr, self.point_per_patch, self.fine_topk, self.fine_mutual)

    def record_scores_per_pair(self):
        """AVERAGE score capacity per pair of the rank's result-record block (shard.py; config key `record_scores_per_pair`)."""
        from .shard import DEFAULT_SCORES_PER_PAIR
        return int(_cfg_get(self.config, "record_scores_per_pair", DEFAULT_SCORES_PER_PAIR))

    def batch_records(self, handle, pair_ids, aux=None):
        """The result records (shard.RecordBatch) of a FINISHED batch: headers + one contiguous slice of the engine's scores."""
        from .shard import pack_records
        return pack_records(pair_ids, handle["starts"], handle["out"]["out_scores"], aux)

    def graph_count(self):
        """Forwards currently held as instantiated HIP graphs."""
        return int(L.lib().roitr_engine_graph_count(self._engine)) if self._engine is not None else 0

    def finish_batch(self, h):
        """Wait for the forward of launch_batch() -- or the match of launch_match() -- and unpack it per pair (the one host
        synchronisation of the path)."""
        if "enc" in h:
            return self._finish_match(h)
        pairs, out, B, P, n_all, n4, have_gt = h["pairs"], h["out"], h["B"], h["P"], h["n_all"], h["n4"], h["have_gt"]
        h["done"].synchronize()
        t_host = time.perf_counter()
        meta = h["meta_host"].tolist()
        starts, n_corr, gt_cnt = meta[:B + 1], meta[B + 1:2 * B + 1], meta[2 * B + 1:]
        if self.factor == 1:
            p_off = [b * P for b in range(B + 1)]                 # strided patch slots
        else:
            p_off = np.concatenate([[0], np.cumsum(n_corr)]).tolist()   # the selected patches of all pairs back to back (roitr_patch_offsets)
            if p_off[B] > h["slots"]:
                # more patches selected than the call's buffers hold (the engine cut the tail of the list): the same call once more with
                # exactly the slots it needs -- the counts are known now.  Results never depend on patch_slots_per_pair.
                import warnings
                warnings.warn(f"adaptive matching selected {p_off[B]} patches in a call sized for {h['slots']} "
                              f"(patch_slots_per_pair = {self.patch_slots_per_pair}): repeating the call with {p_off[B]} slots")
                again = self.launch_batch(pairs, patch_slots=p_off[B], **h["relaunch"])
                res = self.finish_batch(again)
                h.update(out=again["out"], starts=again["starts"], slots=again["slots"], keep=again["keep"])
                return res
        h["starts"] = starts   # row offsets of every pair in out_scores (+ total): shard.pack_records reads them
        o_pts = np.cumsum([0] + n_all)
        o_nod = np.cumsum([0] + n4)
        results = []
        for b in range(B):
            sc, tc = b, B + b
            nc = n_corr[b]
            r = LazyDict()
            r["src_points"] = pairs[b]["src_pcd"]
            r["tgt_points"] = pairs[b]["tgt_pcd"]
            r["src_nodes"] = out["node_xyz"][o_nod[sc]:o_nod[sc + 1]]
            r["tgt_nodes"] = out["node_xyz"][o_nod[tc]:o_nod[tc + 1]]
            r["src_point_feats"] = out["point_feats"][o_pts[sc]:o_pts[sc + 1]]
            r["tgt_point_feats"] = out["point_feats"][o_pts[tc]:o_pts[tc + 1]]
            r["src_node_feats"] = out["node_feats"][o_nod[sc]:o_nod[sc + 1]]
            r["tgt_node_feats"] = out["node_feats"][o_nod[tc]:o_nod[tc + 1]]
            if have_gt:
                r["gt_node_corr_indices"] = lambda b=b: out["gt_corr_idx"][b, :gt_cnt[b]].long()
                r["gt_node_corr_overlaps"] = out["gt_corr_overlaps"][b, :gt_cnt[b]]
                r["gt_tgt_node_occ"] = out["gt_node_occ"][o_nod[tc]:o_nod[tc + 1]]
                r["gt_src_node_occ"] = out["gt_node_occ"][o_nod[sc]:o_nod[sc + 1]]
            else:
                r["gt_node_corr_indices"] = r["gt_node_corr_overlaps"] = r["gt_tgt_node_occ"] = r["gt_src_node_occ"] = None
            r["src_node_corr_indices"] = lambda b=b, nc=nc: out["src_corr"][b, :nc].long()
            r["tgt_node_corr_indices"] = lambda b=b, nc=nc: out["tgt_corr"][b, :nc].long()
            p0 = p_off[b]
            r["src_node_corr_knn_points"] = out["src_knn_pts"][p0:p0 + nc]
            r["tgt_node_corr_knn_points"] = out["tgt_knn_pts"][p0:p0 + nc]
            r["src_node_corr_knn_masks"] = lambda p0=p0, nc=nc: out["src_knn_masks"][p0:p0 + nc].bool()
            r["tgt_node_corr_knn_masks"] = lambda p0=p0, nc=nc: out["tgt_knn_masks"][p0:p0 + nc].bool()
            r["matching_scores"] = out["matching_scores"][p0:p0 + nc]
            s, e = starts[b], starts[b + 1]
            r["tgt_corr_points"] = out["out_tgt_pts"][s:e]
            r["src_corr_points"] = out["out_src_pts"][s:e]
            r["corr_scores"] = out["out_scores"][s:e]
            # extras (not in the reference dict): partition and coarse scores, handy for evaluation
            r["_node_corr_scores"] = out["corr_scores"][b, :nc]
            r["_src_node_knn_indices"] = out["node_knn_idx"][o_nod[sc]:o_nod[sc + 1]]
            r["_tgt_node_knn_indices"] = out["node_knn_idx"][o_nod[tc]:o_nod[tc + 1]]
            r["_src_node_knn_masks"] = lambda sc=sc: out["node_knn_mask"][o_nod[sc]:o_nod[sc + 1]].bool()
            r["_tgt_node_knn_masks"] = lambda tc=tc: out["node_knn_mask"][o_nod[tc]:o_nod[tc + 1]].bool()
            r["_src_node_masks"] = lambda sc=sc: out["node_masks"][o_nod[sc]:o_nod[sc + 1]].bool()
            r["_tgt_node_masks"] = lambda tc=tc: out["node_masks"][o_nod[tc]:o_nod[tc + 1]].bool()
            results.append(r)
        self.host_ms["unpack"] += 1e3 * (time.perf_counter() - t_host)
        return results

    # ---------------------------------------------------------------- encode once, match many (include/roitr_encode.h)
    def encode_clouds(self, clouds, clouds_per_call=128):
        """Run the per-cloud half of the forward once per cloud: `clouds` is a list of dicts with `points` (n,3), `normals` (n,3),
        `feats` (n,1) and optionally `points_out` (n,3: the coordinates the correspondences are reported in; default `points`).
        Returns the EncodedClouds that launch_match / match_batch take, filled by ceil(len / clouds_per_call) engine calls queued on
        the current stream (nothing here waits for the GPU).  The cache belongs to this model's weights as they are now."""
        self._ensure_engine()
        if not clouds:
            raise L.RoitrError("encode_clouds needs at least one cloud")
        lib = _cache_lib()
        dev = clouds[0]["points"].device
        f32, i32 = torch.float32, torch.int32
        C, Lm = 256 * self.factor, self.point_per_patch
        n_all = [int(c["points"].shape[0]) for c in clouds]
        arr = (ctypes.c_int * len(n_all))(*n_all)
        per = (ctypes.c_size_t * 8)()
        total = lib.roitr_engine_encode_bytes(len(n_all), arr, C, Lm, per)
        if total == 0:
            raise L.RoitrError("encode_clouds: a cloud is smaller than the model accepts (256 points = 4 superpoints)")
        n4 = [self.level_sizes(n)[3] for n in n_all]
        T, T4, etot = sum(n_all), sum(n4), sum(k * k for k in n4)
        z = lambda shape, dt=f32: torch.empty(shape, dtype=dt, device=dev)
        arrays = dict(points=z((T, 3)), point_feats=z((T, C)), node_xyz=z((T4, 3)), node_masks=z((T4,), i32), node_knn_idx=z((T4, Lm), i32),
                      node_knn_mask=z((T4, Lm), i32), node_geo=z((T4, C)), embedding=z((etot, C)))
        assert [a.numel() * a.element_size() for a in arrays.values()] == list(per)
        enc = EncodedClouds(arrays, n_all, C, Lm, self._engine_sig, self._engine_token)   # (_ensure_engine has just brought the signature up to date)
        for c0 in range(0, len(clouds), max(1, int(clouds_per_call))):
            part = clouds[c0:c0 + max(1, int(clouds_per_call))]
            cat = lambda k: torch.cat([c[k].to(f32) for c in part], 0).contiguous()
            geom, nrm, feats = cat("points"), cat("normals"), cat("feats")
            pout = torch.cat([c.get("points_out", c["points"]).to(f32) for c in part], 0).contiguous()
            s0 = enc.seg[c0]
            io = _CEncodeIO()
            io.clouds = len(part)
            io.n_points = ctypes.c_void_p(ctypes.addressof(arr) + 4 * c0)
            io.points_geom, io.normals, io.feats, io.points_out = L.ptr(geom), L.ptr(nrm), L.ptr(feats), L.ptr(pout)
            for k in CACHE_ARRAYS:
                row0 = s0.pt_row0 if k in ("points", "point_feats") else s0.emb0 if k == "embedding" else s0.node_row0
                setattr(io, k, L.ptr(arrays[k][row0:]))
            L.check(lib.roitr_engine_encode(self._engine, ctypes.byref(io), L.stream_ptr()), "engine_encode")
        return enc

    def _check_cache(self, enc):
        if not isinstance(enc, EncodedClouds):
            raise L.RoitrError("expected the EncodedClouds of encode_clouds()")
        if enc.engine is not self._engine_token:
            raise L.RoitrError("stale cloud cache: it was encoded by another engine")
        # after _ensure_engine the engine's signature IS the model's (with weights_frozen the caller vouches for it): no second walk
        if enc.signature != self._engine_sig:
            raise L.RoitrError("stale cloud cache: the model's weights changed since encode_clouds(): encode again")

    def _match_io(self, enc, src, tgt, out):
        """The RoitrMatchIO of pairs (src[b], tgt[b]) with the output tensors of `out` (absent = NULL) and what keeps its host arrays alive."""
        io = _CMatchIO()
        io.pairs = len(src)
        a_src, a_tgt = (ctypes.c_int * max(1, len(src)))(*src), (ctypes.c_int * max(1, len(tgt)))(*tgt)
        io.src_cloud, io.tgt_cloud = ctypes.cast(a_src, ctypes.c_void_p), ctypes.cast(a_tgt, ctypes.c_void_p)
        for k, v in out.items():
            setattr(io, k, L.ptr(v))
        return io, (a_src, a_tgt)

    def launch_match(self, enc, pairs, want_node_xyz=False):
        """Enqueue the pair half of the forward for `pairs` = [(src_index, tgt_index), ...] over the cached clouds of `enc` on the
        current stream and return a handle for finish_batch().  Like launch_batch it does not wait for the GPU.  A cloud may appear in
        any number of pairs, on either side; (a, a) is allowed.  want_node_xyz: also copy the node coordinates into the call layout
        (handle["out"]["node_xyz"]; the results' *_nodes are views into the cache either way)."""
        self._ensure_engine()
        self._check_cache(enc)
        t_host = time.perf_counter()
        pairs = [(int(s), int(t)) for s, t in pairs]
        B = len(pairs)
        if B == 0:
            return dict(enc=enc, match_pairs=[], B=0)
        bad = [p for p in pairs if not (0 <= p[0] < len(enc) and 0 <= p[1] < len(enc))]
        if bad:
            raise L.RoitrError(f"launch_match: cloud index outside the table of {len(enc)} clouds: {bad[:4]}")
        dev = enc.arrays["points"].device
        f32, i32 = torch.float32, torch.int32
        src, tgt = [p[0] for p in pairs], [p[1] for p in pairs]
        slots = src + tgt
        n4 = [enc.n4[c] for c in slots]
        T4, C, Lm = sum(n4), enc.channels, enc.limit
        P, S = self._patch_geometry(B, n4)
        cap = S * Lm * self.fine_topk * (1 if self.fine_mutual else 2)
        z = lambda shape, dt=f32: torch.empty(shape, dtype=dt, device=dev)
        out = dict(node_feats=z((T4, C)), tgt_corr=z((B, P), i32), src_corr=z((B, P), i32), corr_scores=z((B, P)), n_corr=z((B,), i32),
                   tgt_knn_pts=z((S, Lm, 3)), src_knn_pts=z((S, Lm, 3)), tgt_knn_masks=z((S, Lm), i32), src_knn_masks=z((S, Lm), i32),
                   matching_scores=z((S, Lm + 1, Lm + 1)), out_tgt_pts=z((cap, 3)), out_src_pts=z((cap, 3)), out_scores=z((cap,)),
                   out_patch=z((cap,), i32), fine_offsets=z((S,), i32), n_out=z((1,), i32), pair_starts=z((B + 1,), i32))
        if want_node_xyz:
            out["node_xyz"] = z((T4, 3))
        io, keep = self._match_io(enc, src, tgt, out)
        L.check(_cache_lib().roitr_engine_match(self._engine, ctypes.byref(enc.table), ctypes.byref(io), L.stream_ptr()), "engine_match")
        meta_dev = torch.cat([out["pair_starts"], out["n_corr"]])
        meta_host = torch.empty(meta_dev.shape, dtype=meta_dev.dtype, pin_memory=True)
        meta_host.copy_(meta_dev, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self.host_ms["launch"] += 1e3 * (time.perf_counter() - t_host)
        self.host_ms["calls"] += 1
        return dict(enc=enc, match_pairs=pairs, out=out, B=B, P=P, slots=S, compacted=False, n4=n4, have_gt=False, meta_host=meta_host,
                    done=done, keep=(keep, meta_dev))

    def match_batch(self, enc, pairs, want_node_xyz=False):
        """launch_match + finish_batch: the results of `pairs` over the cached clouds, one LazyDict per pair with the keys of a forward
        with want_gt=False."""
        return self.finish_batch(self.launch_match(enc, pairs, want_node_xyz=want_node_xyz))

    def _finish_match(self, h):
        if h["B"] == 0:
            return []
        enc, pairs, out, B, P, n4 = h["enc"], h["match_pairs"], h["out"], h["B"], h["P"], h["n4"]
        h["done"].synchronize()
        t_host = time.perf_counter()
        meta = h["meta_host"].tolist()
        starts, n_corr = meta[:B + 1], meta[B + 1:2 * B + 1]
        h["starts"] = starts
        o_nod = np.cumsum([0] + n4)
        A_ = enc.arrays
        results = []
        for b, (cs, ct) in enumerate(pairs):
            ss, st_ = enc.seg[cs], enc.seg[ct]
            nc, p0 = n_corr[b], b * P
            rows = lambda k, s, node: A_[k][s.node_row0:s.node_row0 + s.n_nodes] if node else A_[k][s.pt_row0:s.pt_row0 + s.n_points]
            r = LazyDict()
            # cloud-level entries: views into the cache
            r["src_points"], r["tgt_points"] = rows("points", ss, False), rows("points", st_, False)
            r["src_nodes"], r["tgt_nodes"] = rows("node_xyz", ss, True), rows("node_xyz", st_, True)
            r["src_point_feats"], r["tgt_point_feats"] = rows("point_feats", ss, False), rows("point_feats", st_, False)
            r["src_node_feats"] = out["node_feats"][o_nod[b]:o_nod[b + 1]]
            r["tgt_node_feats"] = out["node_feats"][o_nod[B + b]:o_nod[B + b + 1]]
            r["gt_node_corr_indices"] = r["gt_node_corr_overlaps"] = r["gt_tgt_node_occ"] = r["gt_src_node_occ"] = None
            r["src_node_corr_indices"] = lambda b=b, nc=nc: out["src_corr"][b, :nc].long()
            r["tgt_node_corr_indices"] = lambda b=b, nc=nc: out["tgt_corr"][b, :nc].long()
            r["src_node_corr_knn_points"] = out["src_knn_pts"][p0:p0 + nc]
            r["tgt_node_corr_knn_points"] = out["tgt_knn_pts"][p0:p0 + nc]
            r["src_node_corr_knn_masks"] = lambda p0=p0, nc=nc: out["src_knn_masks"][p0:p0 + nc].bool()
            r["tgt_node_corr_knn_masks"] = lambda p0=p0, nc=nc: out["tgt_knn_masks"][p0:p0 + nc].bool()
            r["matching_scores"] = out["matching_scores"][p0:p0 + nc]
            s, e = starts[b], starts[b + 1]
            r["tgt_corr_points"] = out["out_tgt_pts"][s:e]
            r["src_corr_points"] = out["out_src_pts"][s:e]
            r["corr_scores"] = out["out_scores"][s:e]
            r["_node_corr_scores"] = out["corr_scores"][b, :nc]
            r["_src_node_knn_indices"], r["_tgt_node_knn_indices"] = rows("node_knn_idx", ss, True), rows("node_knn_idx", st_, True)
            r["_src_node_knn_masks"] = lambda ss=ss: rows("node_knn_mask", ss, True).bool()
            r["_tgt_node_knn_masks"] = lambda st_=st_: rows("node_knn_mask", st_, True).bool()
            r["_src_node_masks"] = lambda ss=ss: rows("node_masks", ss, True).bool()
            r["_tgt_node_masks"] = lambda st_=st_: rows("node_masks", st_, True).bool()
            results.append(r)
        self.host_ms["unpack"] += 1e3 * (time.perf_counter() - t_host)
        return results

    def forward(self, src_pcd, tgt_pcd, src_feats, tgt_feats, src_normals, tgt_normals, rot, trans, src_raw_pcd):
        """model/RIGA_v2.py:58 -- one pair, same argument order, same output keys."""
        pair = dict(src_pcd=src_pcd, tgt_pcd=tgt_pcd, src_feats=src_feats, tgt_feats=tgt_feats, src_normals=src_normals,
                    tgt_normals=tgt_normals, rot=rot, trans=trans, src_raw_pcd=src_raw_pcd)
        return self.forward_batch([pair])[0]


# ---- what the evaluation operators read of a launch_batch() handle.  `keep` is read at call time: finish_batch replaces it when it
# repeats an overfull call, while the sizes (n_all, n4) the cached starts are built from are those of the pairs and stay.
def _forward_handle(handle, who):
    """The evaluation operators read clouds laid out src_0 .. src_{B-1}, tgt_0 .. tgt_{B-1}; a match handle's clouds are rows of the
    cloud cache, anywhere and shared between pairs."""
    if "enc" in handle:
        raise L.RoitrError(f"{who}: this is a launch_match() handle: its clouds are rows of the cloud cache, not the contiguous "
                           "src / tgt layout of a launch_batch() handle (read the per-pair results of finish_batch instead)")


def handle_poses(handle, who):
    """rot (B,3,3) / trans (B,3) fp32 device tensors of a handle's pairs, as the engine was given them."""
    _forward_handle(handle, who)
    if not handle["have_gt"]:
        raise L.RoitrError(f"{who} needs ground-truth transforms (rot / trans) in the pairs")
    return handle["keep"][4], handle["keep"][5]


def handle_starts(handle, which):
    """(src_starts, tgt_starts) of a handle's "point" rows (point_feats, the clouds the model was fed) or "node" rows (node_feats,
    node_xyz), which hold src_0 .. src_{B-1}, tgt_0 .. tgt_{B-1}: source pair b owns rows [src_starts[b], src_starts[b + 1]), its target
    [tgt_starts[b], tgt_starts[b + 1]); both (B + 1) int32 on the device, uploaded once per handle."""
    _forward_handle(handle, "handle_starts")
    if which not in ("point", "node"):
        raise L.RoitrError(f"which must be 'point' or 'node', got {which!r}")
    B = handle["B"]
    if which + "_starts" not in handle:
        handle[which + "_starts"] = A.cumulative(handle["n_all" if which == "point" else "n4"], handle["out"]["n_corr"].device)
    o = handle[which + "_starts"]
    return o[:B + 1], o[B:]


def handle_layout(handle, which):
    """(rows, src_starts, tgt_starts): handle_starts and the coordinates of those rows, the clouds the model was fed (src_pcd then
    tgt_pcd) for "point", node_xyz for "node"."""
    _forward_handle(handle, "handle_layout")
    src_starts, tgt_starts = handle_starts(handle, which)
    rows = handle["keep"][1] if which == "point" else handle["out"]["node_xyz"]
    return rows[:sum(handle["n_all" if which == "point" else "n4"])], src_starts, tgt_starts


def handle_normals(handle):
    """The normals the model was fed for the "point" rows of handle_layout (src_normals then tgt_normals), (rows, 3) fp32."""
    _forward_handle(handle, "handle_normals")
    return handle["keep"][2][:sum(handle["n_all"])]


def create_model(config):
    """model/RIGA_v2.py:178."""
    return RIGA_v2(config)
