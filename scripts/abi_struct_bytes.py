#!/usr/bin/env python3
"""Host only, no GPU and no library: the argument structs the wrappers of roitr_amd/ops.py hand to the library, byte for byte against the
constructions ops.py had while its structs were built positionally from hand-written ctypes mirrors (restated below).

The wrappers themselves run, on CPU tensors, with the library replaced by a recorder and L.ptr by a counter: the n-th pointer a
wrapper takes is 0x1000 * n, None is NULL.  The restatement draws from the same counter in the order the earlier code took its
pointers, so a pointer that lands in another field, a scalar in another slot or a field that is no longer zero changes the bytes.

    python scripts/abi_struct_bytes.py > profiles/abi_structs_refactor.txt
"""
import ctypes
import itertools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roitr_amd import _lib as L, ops  # noqa: E402

CALLS = []   # (entry point, bytes of every struct argument) in call order
P = None     # the pointer counter of the construction under way


class Recorder:
    def __getattr__(self, name):
        def call(*args):
            CALLS.append((name, [bytes(a._obj) for a in args if isinstance(getattr(a, "_obj", None), ctypes.Structure)]))
            return {"roitr_coarse_scratch_floats": 96, "roitr_local_td_supported": 1}.get(name, 0)
        return call


def restart():
    global P
    count = itertools.count(1)
    P = lambda present=True: 0x1000 * next(count) if present else 0
    del CALLS[:]


L.ptr = lambda t: ctypes.c_void_p(P(t is not None))
L.stream_ptr = lambda: ctypes.c_void_p(0)
ops._lib = Recorder


def by_name(cls, fields):
    a = cls()
    for k, v in fields:
        setattr(a, k, v)
    return a


# ---------------------------------------------------------------------------------------------- the earlier constructions
def old_gemm(M, N, K, ldw, bias, alpha=1.0, relu=0, flags=0, ln=None, addend=False, cat=None, interp=False, x3=0):
    """linear() (ln None) / linear_layernorm() (ln = (res, res_idx, post present, relu, eps))"""
    head = (M, N, K, P(), 0, K, 0, 0, P(), K, 0, 0, P(bias), alpha, relu, P(), N, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    if ln is None:
        g = ops._Gemm(*head)
    else:
        g = ops._Gemm(*head, P(), P(), P(ln[0]), P(ln[1]), P(ln[2]), ln[3], ln[4])
    g.bf16 = flags
    if addend:
        g.A2 = P()
    if cat is not None:   # (width of x_cat, row gather present)
        g.A_cat, g.lda_cat, g.k_cat = P(), cat[0], K
        g.K = K + cat[0]
        if cat[1]:
            g.a_cat_idx = P()
    g.ldw = ldw
    if interp:
        g.ip_feat, g.ip_idx, g.ip_dist2 = P(), P(), P()
    if x3:
        P(), P()   # roitr_split_bf16x3(weight, pieces)
        g.W, g.bf16, g.w_piece = P(), 8, x3
    return g


def old_coarse(C, num_corr, dual, nr, ns, stride):
    return ops._Coarse(1, C, num_corr, dual, nr, ns, P(), P(), P(), P(), stride, P(), P(), P(), P(), 0, 0, 0)


def old_adaptive(C, na, nb, stride):
    old_gemm(na, nb, C, C, False)   # xy = linear(src_feats, tgt_feats)
    return ops._Coarse(1, C, na * nb, 0, na, nb, P(), P(), P(), P(), stride, P(), P(), P(), P(), P(), 0, nb)


def old_ot(B, M, num_iter):
    return ops._OT(1, B, M, num_iter, P(), P(), P(), P(), P(), P())


def old_fine(B, Lm, k, mutual, conf, gs):
    return ops._Fine(1, B, Lm, k, mutual, conf, P(), P(), P(), P(), P(), P(), P(gs), P(), P(), P(), P(), P(), P(), P(), 0, B * Lm * Lm)


def old_node_corr(pairs, limit, max_nodes, radius, mat_stride, n_nodes):
    return ops._NodeCorr(pairs, limit, max_nodes, radius, P(), P(), P(), P(), P(), P(), P(), P(), P(), P(), mat_stride, P(), P(), P(),
                         n_nodes, P(), P())


def old_fold(M, I, H, no):
    return by_name(ops._LocalAttnFold, [("M", M), ("in_dim", I), ("H", H), ("x", P()), ("ldx", I), ("q", P()), ("ldq", H), ("qt", P())] +
                   [(k, P()) for k in ("group_idx", "ppf", "wpe", "wvpe", "bvpe")] +
                   [("scale", 1.0 / float(H // 4) ** 0.5), ("xbar", P()), ("vpart", P()), ("node_order", P(no))])


def old_attn(M, K, H, heads, lds, ldo, bf16, folded, no, scale=None):
    return by_name(ops._LocalAttn, [("M", M), ("K", K), ("H", H), ("heads", heads), ("q", P()), ("ldq", lds[0]), ("k", P()), ("ldk", lds[1]),
                                    ("v", P()), ("ldv", lds[2])] + [(k, P()) for k in ("group_idx", "ppf", "wvpe", "bvpe")] +
                   [("scale", 1.0 / float(H // heads) ** 0.5 if scale is None else scale), ("out", P()), ("ldo", ldo), ("node_order", P(no)),
                    ("bf16", bf16), ("wpe", P(folded)), ("bpe", P(folded))])


TD_W = ("wqqt", "bqqt", "wv", "bv", "wpe", "wvpe", "bvpe", "wcat", "bcat", "norm_w", "norm_b", "wout", "bout")
BLOCK_W = ("wq", "bq", "wpe", "bpe", "wvpe", "bvpe", "wcat", "bcat", "norm_w", "norm_b", "wout", "bout", "bn2_w", "bn2_b")
FIRST_W = ("head_consts", "G", "zero_bias", "norm_w", "norm_b", "wout", "bout")


def old_td(M, I, H, no):
    return by_name(ops._LocalTd, [("M", M), ("in_dim", I), ("H", H)] + [(k, P()) for k in ("x", "node_idx", "group_idx", "ppf")] +
                   [("node_order", P(no))] + [(k, P()) for k in TD_W] + [("scale", 1.0 / float(H // 4) ** 0.5), ("eps", 1e-5), ("out", P())])


def old_block(M, K, H, no, kv_bf16, weights_bf16):
    return by_name(ops._LocalBlock, [("M", M), ("K", K), ("H", H)] + [(k, P()) for k in ("x", "kv", "group_idx", "ppf")] +
                   [("node_order", P(no))] + [(k, P()) for k in BLOCK_W] +
                   [("scale", 1.0 / float(H // 4) ** 0.5), ("eps", 1e-5), ("out", P()), ("kv_bf16", kv_bf16)] +
                   ([(k, P()) for k in ("wq_h", "wcat_h", "wout_h")] if weights_bf16 else []))


def old_first(M, K, no):
    return by_name(ops._LocalFirst, [("M", M), ("K", K)] + [(k, P()) for k in ("x", "group_idx", "ppf")] + [("node_order", P(no))] +
                   [(k, P()) for k in FIRST_W] + [("scale", 0.25), ("eps", 1e-5), ("out", P())])


def old_mha(q_row0, q_rows, C, heads, lds, partner, nk_max, ldo, E):
    a = by_name(ops._Mha, [("q_row0", q_row0), ("q_rows", q_rows), ("C", C), ("heads", heads), ("q", P()), ("ldq", lds[0]), ("k", P()),
                           ("ldk", lds[1]), ("v", P()), ("ldv", lds[2]), ("offset", P()), ("cloud_of_row", P()), ("partner", P(partner)),
                           ("scale", 1.0 / float(C // heads) ** 0.5), ("nk_max", nk_max), ("out", P()), ("ldo", ldo)])
    if E is not None:
        for k in ("E", "eoff", "qt", "bp", "ebar"):
            setattr(a, k, P())
        a.e_bf16 = int(E)
    return a


# ---------------------------------------------------------------------------------------------- the cases
def f(*shape):
    return torch.rand(shape)


def i(*shape):
    return torch.zeros(shape, dtype=torch.int64)


def weights(names, shapes):
    return {k: f(*shapes.get(k, shapes["*"])) for k in names}


def cases():
    M, N, K, R = 40, 64, 96, 24
    x, w, b, gam, bet = f(M, K), f(N, K), f(N), f(N), f(N)
    yield "linear", lambda: ops.linear(x, w), lambda: old_gemm(M, N, K, K, False)
    yield "linear bias relu alpha", lambda: ops.linear(x, w, b, relu=True, alpha=0.5), lambda: old_gemm(M, N, K, K, True, 0.5, 1)
    yield "linear bf16 out_bf16", lambda: ops.linear(x, w, b, bf16=True, out_bf16=True), lambda: old_gemm(M, N, K, K, True, flags=1 | 4)
    yield "linear bf16 x", lambda: ops.linear(x.bfloat16(), w, bf16=True), lambda: old_gemm(M, N, K, K, False, flags=1 | 2)
    wc = f(N, K + 32)
    yield ("linear x_cat x_cat_idx addend", lambda: ops.linear(x, wc, b, x_cat=f(R, 32), x_cat_idx=i(M), addend=f(M, K)),
           lambda: old_gemm(M, N, K, K + 32, True, addend=True, cat=(32, True)))
    yield "linear x3", lambda: ops.linear(x, w, x3=True), lambda: old_gemm(M, N, K, K, False, x3=N * K)
    yield ("linear_layernorm", lambda: ops.linear_layernorm(x, w, b, gam, bet),
           lambda: old_gemm(M, N, K, K, True, ln=(False, False, False, 0, 1e-5)))
    yield ("linear_layernorm res res_idx post relu eps", lambda: ops.linear_layernorm(x, w, None, gam, bet, f(R, N), i(M), f(M, N), True, 1e-3),
           lambda: old_gemm(M, N, K, K, False, ln=(True, True, True, 1, 1e-3)))
    yield ("linear_layernorm bf16 x_cat interp x3",
           lambda: ops.linear_layernorm(x, wc, b, gam, bet, x_cat=f(M, 32), interp=(f(R, N), i(M, 3), f(M, 3)), x3=True),
           lambda: old_gemm(M, N, K, K + 32, True, ln=(False, False, False, 0, 1e-5), cat=(32, False), interp=True, x3=N * (K + 32)))
    nr, ns, C = 7, 5, 32
    fr, fs, mr, ms = f(nr, C), f(ns, C), torch.ones(nr, dtype=torch.bool), torch.ones(ns, dtype=torch.bool)
    yield "coarse_matching", lambda: ops.coarse_matching(fr, fs, mr, ms, 20, True), lambda: old_coarse(C, 20, 1, nr, ns, 96)
    yield "coarse_matching single norm", lambda: ops.coarse_matching(fr, fs, mr, ms, 9, False), lambda: old_coarse(C, 9, 0, nr, ns, 96)
    yield "adaptive_superpoint_matching", lambda: ops.adaptive_superpoint_matching(fs, fr, ms, mr, 4, 0.5), lambda: old_adaptive(C, ns, nr, 96)
    B, Lm = 3, 64
    masks = torch.ones((B, Lm), dtype=torch.bool)
    yield "optimal_transport", lambda: ops.optimal_transport(f(B, Lm, Lm), masks, masks, 0.25, 17), lambda: old_ot(B, Lm, 17)
    pts, ot = f(B, Lm, 3), f(B, Lm + 1, Lm + 1)
    yield ("fine_matching", lambda: ops.fine_matching(pts, pts, masks, masks, ot, 3, True, 0.05),
           lambda: old_fine(B, Lm, 3, 1, 0.05, False))
    yield ("fine_matching global_scores not mutual", lambda: ops.fine_matching(pts, pts, masks, masks, ot, 2, False, 0.1, f(B)),
           lambda: old_fine(B, Lm, 2, 0, 0.1, True))
    n_nodes, lim = 11, 8
    yield ("node_correspondences",
           lambda: ops.node_correspondences(f(n_nodes, 3), torch.tensor([3, 5, 8, 11]), i(n_nodes), f(50, 3), torch.tensor([10, 20, 35, 50]),
                                            i(n_nodes, lim), i(n_nodes, lim), f(2, 3, 3), f(2, 3), 0.1),
           lambda: old_node_corr(2, lim, 3, 0.1, 9, n_nodes))
    yield ("node_correspondences max_nodes mat_stride",
           lambda: ops.node_correspondences(f(n_nodes, 3), torch.tensor([3, 5, 8, 11]), i(n_nodes), f(50, 3), torch.tensor([10, 20, 35, 50]),
                                            i(n_nodes, lim), i(n_nodes, lim), f(2, 3, 3), f(2, 3), 0.2, max_nodes=4, mat_stride=32),
           lambda: old_node_corr(2, lim, 4, 0.2, 32, n_nodes))
    # built field by field before and after: the same assignments on the class read from the header
    Mn, I, H = 12, 64, 128
    g16, ppf = i(Mn, 16), f(Mn, 16, 4)
    for no in (None, f(Mn, 4)):
        tag = "" if no is None else " node_order"
        yield ("local_attention_fold" + tag, lambda no=no: ops.local_attention_fold(f(30, I), f(Mn, H), f(Mn, 4, I), g16, ppf, f(H, 4), f(H, 4), f(H), no),
               lambda no=no: old_fold(Mn, I, H, no is not None))
        yield ("local_td" + tag, lambda no=no: ops.local_td(f(30, I), i(Mn), g16, ppf, weights(TD_W, {"*": (H,), "wout": (H, H)}), no),
               lambda no=no: old_td(Mn, I, H, no is not None))
        yield ("local_first" + tag, lambda no=no: ops.local_first(f(Mn), i(Mn, 8), f(Mn, 8, 4), weights(FIRST_W, {"*": (64,)}), no),
               lambda no=no: old_first(Mn, 8, no is not None))
    bw = {"*": (H,), "wq": (H, H), "wcat": (H, 2 * H), "wout": (H, H)}
    yield ("local_block", lambda: ops.local_block(f(Mn, H), f(Mn, 2 * H), g16, ppf, weights(BLOCK_W, bw)), lambda: old_block(Mn, 16, H, False, 0, False))
    yield ("local_block bf16 kv and weights node_order",
           lambda: ops.local_block(f(Mn, H), f(Mn, 2 * H).bfloat16(), g16, ppf, weights(BLOCK_W, bw), f(Mn, 4), bf16_weights=True),
           lambda: old_block(Mn, 16, H, True, 1, True))
    qkv = f(30, 3 * H + 20)
    yield ("local_attention folded q columns", lambda: ops.local_attention(qkv[:, :H + 20], qkv[:, H + 20:2 * H + 20], qkv[:, 2 * H + 20:], g16, ppf, f(H, 4), f(H)),
           lambda: old_attn(Mn, 16, H, 4, [3 * H + 20] * 3, H, 0, False, False))
    yield ("local_attention bf16 wpe bpe node_order out ld*",
           lambda: ops.local_attention(f(30, H).bfloat16(), f(30, H).bfloat16(), f(30, H).bfloat16(), i(Mn, 8), f(Mn, 8, 4), f(H, 4), f(H), f(H, 4), f(H),
                                       ldq=H, ldk=2 * H, ldv=3 * H, ldo=7, bf16=True, node_order=f(Mn, 4), out=torch.empty((Mn, H + 8), dtype=torch.bfloat16)[:, :H],
                                       heads=8, scale=0.5),
           lambda: old_attn(Mn, 8, H, 8, [H, 2 * H, 3 * H], 7, 3, True, True, 0.5))
    T, Cg = 20, 256
    q3 = f(T, 3 * Cg)
    off, cor = torch.tensor([8, 20], dtype=torch.int32), torch.zeros(T, dtype=torch.int32)
    yield ("multi_head_attention", lambda: ops.multi_head_attention(q3[:, :Cg], q3[:, Cg:2 * Cg], q3[:, 2 * Cg:], off, cor, 12),
           lambda: old_mha(0, T, Cg, 4, [3 * Cg] * 3, False, 12, Cg, None))
    yield ("multi_head_attention partner E bf16 row range",
           lambda: ops.multi_head_attention(f(T, Cg), f(T, Cg), f(T, Cg), off, cor, 12, partner=torch.tensor([1, 0], dtype=torch.int32),
                                            E=f(208, Cg).bfloat16(), eoff=i(2), qt=f(T, 4, Cg), bp=f(Cg), q_row0=8, q_rows=12),
           lambda: old_mha(8, 12, Cg, 4, [Cg] * 3, True, 12, Cg, True))


def main():
    total = 0
    for name, new, old in cases():
        restart()
        new()
        got = [s for _, structs in CALLS for s in structs][-1]   # the wrapper's own struct: the last one handed over
        entry = CALLS[-1][0]
        restart()
        want = bytes(old())
        assert got == want, (name, [k for k in range(len(want)) if got[k:k + 1] != want[k:k + 1]])
        total += 1
        print(f"{name:55s} {entry:28s} {len(want):4d} bytes identical")
    print(f"{total} constructions, all identical")


if __name__ == "__main__":
    main()
