"""Operator-level mirrors of the reference's lib/utils.py hot-path helpers, backed by HIP kernels.

Each function cites the reference function it stands for.  ROCm device tensors only.
"""
import ctypes

import torch

from . import _lib as L

# The library with every entry point this file calls declared from the header (the row-wise layers and roitr_build_pfold are in L.BOUND):
# a Python int / float is converted to the prototype's `long rows`, `size_t`, by-value `float eps` by ctypes, not by the call site.
# (roitr_local_block_dbg, the tuning hook of local_block, is exported but in no header: a struct pointer, an int and the stream.)
_lib = L.binder("""roitr_calc_ppf roitr_point_to_node_partition roitr_coarse_scratch_floats roitr_coarse_matching roitr_adaptive_matching
    roitr_optimal_transport roitr_fine_matching roitr_split_bf16x3 roitr_gemm roitr_add_layernorm_interp roitr_geo_table_floats
    roitr_geo_table_build roitr_geo_embed_table roitr_geo_embed_bf16 roitr_split3_bf16 roitr_geo_embed_split roitr_geo_embed
    roitr_local_attention_fold roitr_local_attention roitr_local_td_supported roitr_local_td roitr_local_block
    roitr_local_first roitr_local_weights_prepare roitr_local_weights_release roitr_local_weights_count
    roitr_local_weights_reorder_host roitr_mha roitr_mha_form roitr_geo_indices roitr_build_padded_clouds roitr_node_occlusion_score
    roitr_node_correspondences""".split())

# The argument structs of include/roitr_engine.h: fields in header order, everything not set is 0 / NULL.
_Coarse = L.struct("RoitrCoarse")
_OT = L.struct("RoitrOT")
_Fine = L.struct("RoitrFine")
_Gemm = L.struct("RoitrGemm")
_LocalAttnFold = L.struct("RoitrLocalAttnFold")
_LocalAttn = L.struct("RoitrLocalAttn")
_LocalTd = L.struct("RoitrLocalTd")
_LocalBlock = L.struct("RoitrLocalBlock")
_LocalFirst = L.struct("RoitrLocalFirst")
_Mha = L.struct("RoitrMha")
_NodeCorr = L.struct("RoitrNodeCorr")


def _c(t):
    """float32 and contiguous, or None"""
    return None if t is None else t.contiguous().float()


def _i32c(t):
    """int32 and contiguous, or None"""
    return None if t is None else t.to(torch.int32).contiguous()


def calc_ppf(points, point_normals, ref_points, ref_normals, group_idx):
    """lib/utils.py:358-389 calc_ppf_gpu(points, point_normals, ref_points[group_idx], ref_normals[group_idx]).

    The reference takes pre-gathered (m,k,3) patches; gathering is fused here, so the caller passes the
    un-gathered reference cloud and the (m,k) indices instead.  Returns (m,k,4) float32."""
    m, k = group_idx.shape
    out = torch.empty((m, k, 4), dtype=torch.float32, device=points.device)
    grp = _i32c(group_idx)
    L.check(_lib().roitr_calc_ppf(m, k, L.ptr(points.contiguous()), L.ptr(point_normals.contiguous()),
                                   L.ptr(ref_points.contiguous()), L.ptr(ref_normals.contiguous()), L.ptr(grp), L.ptr(out),
                                   L.stream_ptr()), "calc_ppf")
    return out


def calc_ppf_gpu(points, point_normals, patches, patch_normals):
    """Signature-compatible with lib/utils.py:358 (pre-gathered patches (m,k,3))."""
    m, k, _ = patches.shape
    grp = torch.arange(m * k, dtype=torch.int32, device=points.device).view(m, k)
    return calc_ppf(points, point_normals, patches.reshape(-1, 3), patch_normals.reshape(-1, 3), grp)


# ------------------------------------------------------------------------------------------------
# Matching-tail operators (single pair / single batch of patches), thin ctypes fronts of the batched kernels.
# ------------------------------------------------------------------------------------------------
def point_to_node_partition(points, nodes, point_limit):
    """lib/utils.py:428-471 -> (point_to_node (N,) i64, node_masks (M,) bool, node_knn_indices (M,K) i64, node_knn_masks bool)"""
    dev = points.device
    N, M = points.shape[0], nodes.shape[0]
    i32 = torch.int32
    po = torch.tensor([N], dtype=i32, device=dev)
    no = torch.tensor([M], dtype=i32, device=dev)
    con = torch.zeros(M, dtype=i32, device=dev)
    p2n = torch.zeros(N, dtype=i32, device=dev)
    p2nd = torch.zeros(N, dtype=torch.float32, device=dev)
    nm = torch.zeros(M, dtype=i32, device=dev)
    kidx = torch.zeros((M, point_limit), dtype=i32, device=dev)
    kmask = torch.zeros((M, point_limit), dtype=i32, device=dev)
    L.check(_lib().roitr_point_to_node_partition(1, N, M, L.ptr(points.contiguous()), L.ptr(po), L.ptr(nodes.contiguous()), L.ptr(no),
                                                  L.ptr(con), int(point_limit), L.ptr(p2n), L.ptr(p2nd), L.ptr(nm), L.ptr(kidx),
                                                  L.ptr(kmask), L.stream_ptr()), "point_to_node_partition")
    return p2n.long(), nm.bool(), kidx.long(), kmask.bool()


def coarse_matching(ref_feats, src_feats, ref_masks, src_masks, num_correspondences=256, dual_normalization=True):
    """model/modules.py:141-178 CoarseMatching.forward -> (ref_corr_indices, src_corr_indices, corr_scores)"""
    dev = ref_feats.device
    nr, ns = ref_feats.shape[0], src_feats.shape[0]
    lib = _lib()
    feats = _c(torch.cat([src_feats, ref_feats], 0))   # cloud order: [src, tgt(=ref)]
    masks = _i32c(torch.cat([src_masks, ref_masks], 0))
    off = torch.tensor([ns, ns + nr], dtype=torch.int32, device=dev)
    stride = lib.roitr_coarse_scratch_floats(nr, ns)
    scratch = torch.empty(stride, dtype=torch.float32, device=dev)
    P = int(num_correspondences)
    tc = torch.zeros(P, dtype=torch.int32, device=dev)
    sc = torch.zeros(P, dtype=torch.int32, device=dev)
    cs = torch.zeros(P, dtype=torch.float32, device=dev)
    nc = torch.zeros(1, dtype=torch.int32, device=dev)
    a = _Coarse(pairs=1, C=feats.shape[1], num_corr=P, dual_norm=int(dual_normalization), max_ref=nr, max_src=ns, feats=L.ptr(feats),
                node_offset=L.ptr(off), node_masks=L.ptr(masks), scratch=L.ptr(scratch), scratch_stride=stride, tgt_corr=L.ptr(tc),
                src_corr=L.ptr(sc), corr_scores=L.ptr(cs), n_corr=L.ptr(nc))
    L.check(lib.roitr_coarse_matching(ctypes.byref(a), L.stream_ptr()), "coarse_matching")
    n = int(nc.item())
    return tc[:n].long(), sc[:n].long(), cs[:n]


def optimal_transport(scores, row_masks, col_masks, alpha, num_iter=100):
    """model/modules.py:28-68 LearnableLogOptimalTransport.forward: (B,64,64) -> (B,65,65)"""
    dev = scores.device
    B, M, N = scores.shape
    out = torch.zeros((B, M + 1, N + 1), dtype=torch.float32, device=dev)
    nc = torch.tensor([B], dtype=torch.int32, device=dev)
    al = torch.as_tensor(alpha, dtype=torch.float32, device=dev).reshape(1).contiguous()
    sc, rm, cm = _c(scores), _i32c(row_masks), _i32c(col_masks)   # named: temporaries must outlive the launch
    a = _OT(pairs=1, num_corr=B, limit=M, num_iter=int(num_iter), n_corr=L.ptr(nc), scores=L.ptr(sc), row_masks=L.ptr(rm),
            col_masks=L.ptr(cm), alpha=L.ptr(al), out=L.ptr(out))
    L.check(_lib().roitr_optimal_transport(ctypes.byref(a), L.stream_ptr()), "optimal_transport")
    return out


def fine_matching(ref_knn_points, src_knn_points, ref_knn_masks, src_knn_masks, matching_scores, k, mutual=True,
                  confidence_threshold=0.05, global_scores=None):
    """model/modules.py:288-324 FineMatching.forward (use_dustbin=False).  matching_scores: the (B,65,65) OT output
    (its dustbin row/column are dropped inside, RIGA_v2.py:159-160) -> (ref_corr_points, src_corr_points, corr_scores)"""
    dev = matching_scores.device
    B, Lp1, _ = matching_scores.shape
    Lm = Lp1 - 1
    i32 = torch.int32
    cap = B * Lm * Lm
    nc = torch.tensor([B], dtype=i32, device=dev)
    flags = torch.zeros(B * Lm * Lm, dtype=torch.uint8, device=dev)
    counts = torch.zeros(B, dtype=i32, device=dev)
    offs = torch.zeros(B, dtype=i32, device=dev)
    n_out = torch.zeros(1, dtype=i32, device=dev)
    o_r = torch.zeros((cap, 3), dtype=torch.float32, device=dev)
    o_c = torch.zeros((cap, 3), dtype=torch.float32, device=dev)
    o_s = torch.zeros(cap, dtype=torch.float32, device=dev)
    rm, cm = _i32c(ref_knn_masks), _i32c(src_knn_masks)
    rp, cp = _c(ref_knn_points), _c(src_knn_points)
    ms, gs = _c(matching_scores), _c(global_scores)
    a = _Fine(pairs=1, num_corr=B, limit=Lm, k=int(k), mutual=int(mutual), conf=float(confidence_threshold), n_corr=L.ptr(nc), ot=L.ptr(ms),
              row_masks=L.ptr(rm), col_masks=L.ptr(cm), row_pts=L.ptr(rp), col_pts=L.ptr(cp), global_scores=L.ptr(gs), flags=L.ptr(flags),
              counts=L.ptr(counts), offsets=L.ptr(offs), n_out=L.ptr(n_out), out_row_pts=L.ptr(o_r), out_col_pts=L.ptr(o_c),
              out_scores=L.ptr(o_s), out_cap=cap)
    L.check(_lib().roitr_fine_matching(ctypes.byref(a), L.stream_ptr()), "fine_matching")
    n = int(n_out.item())
    return o_r[:n], o_c[:n], o_s[:n]


BF16_W, BF16_A, BF16_C, BF16_X3 = 1, 2, 4, 8   # RoitrGemm::bf16 flags (include/roitr_engine.h)


def split_bf16x3(weight):
    """roitr_split_bf16x3: (N, K) fp32 -> (3, N, K) bf16 with weight == pieces.float().sum(0) exactly (csrc/gemm_x3.hip)."""
    w = _c(weight)
    out = torch.empty((3,) + tuple(w.shape), dtype=torch.bfloat16, device=w.device)
    L.check(_lib().roitr_split_bf16x3(w.numel(), L.ptr(w), L.ptr(out), w.numel(), L.stream_ptr()), "split_bf16x3")
    return out


def _bf16_flags(bf16, x, weight, out_bf16):
    """bf16 operand mode of the GEMM: the weight is stored bf16, x is rounded while staged unless it already is a bfloat16
    tensor, the output is stored bf16 on request.  Returns (x, weight, flags)."""
    if not bf16:
        return _c(x), _c(weight), 0
    flags = BF16_W | (BF16_C if out_bf16 else 0)
    w = weight.contiguous().to(torch.bfloat16)
    if x.dtype == torch.bfloat16:
        return x.contiguous(), w, flags | BF16_A
    return _c(x), w, flags


def _k_cat(g, x, x_cat, keep, x_cat_idx=None, addend=None):
    """RoitrGemm::A_cat: the product reads [x | x_cat] along K without the concatenation ever existing (fp32 fast path only).
    x_cat_idx: row gather of x_cat alone (RoitrGemm::a_cat_idx); addend: RoitrGemm::A2, added to the x part."""
    if addend is not None:
        ad = _c(addend)
        keep.append(ad)
        g.A2 = L.ptr(ad)
    if x_cat is None:
        return
    xc = _c(x_cat)
    keep.append(xc)
    g.A_cat, g.lda_cat, g.k_cat = L.ptr(xc), xc.shape[1], x.shape[1]
    g.K = x.shape[1] + xc.shape[1]
    if x_cat_idx is not None:
        ix = _i32c(x_cat_idx)
        keep.append(ix)
        g.a_cat_idx = L.ptr(ix)


def _x3(g, weight, keep):
    """RoitrGemm::bf16 = ROITR_BF16_X3: the weight as its three bf16 pieces (csrc/gemm_x3.hip)."""
    w3 = split_bf16x3(weight)
    keep.append(w3)
    g.W, g.bf16, g.w_piece = L.ptr(w3), BF16_X3, weight.numel()


def _gemm(x, weight, bias, out, flags, **fields):
    """RoitrGemm of out = x @ weight.T + bias in one batch of dense rows, plus `fields`."""
    (M, K), N = x.shape, weight.shape[0]
    return _Gemm(M=M, N=N, K=K, A=L.ptr(x), lda=K, W=L.ptr(weight), ldw=weight.shape[1], bias=L.ptr(bias), C=L.ptr(out), ldc=N, batch=1,
                 bf16=flags, **fields)


def linear(x, weight, bias=None, relu=False, alpha=1.0, bf16=False, out_bf16=False, x_cat=None, x_cat_idx=None, addend=None, x3=False):
    """act(alpha * x @ weight.T + bias): the kernel behind every nn.Linear of the path.  Default: the fp32 MFMA GEMM.
    bf16=True: the bf16-operand kernel (csrc/gemm_bf16.hip; weights stored bf16, fp32 accumulate); x may be a bfloat16
    tensor (stored-bf16 activation), out_bf16 stores the result in bf16.  x_cat: a second operand block, the product is
    [x | x_cat] @ weight.T (the K-concatenated A of the folded block transformers)."""
    x, weight, flags = _bf16_flags(bf16, x, weight, out_bf16)
    out = torch.empty((x.shape[0], weight.shape[0]), dtype=torch.bfloat16 if flags & BF16_C else torch.float32, device=x.device)
    b = _c(bias)
    g = _gemm(x, weight, b, out, flags, alpha=float(alpha), relu=int(relu))
    keep = []
    _k_cat(g, x, x_cat, keep, x_cat_idx, addend)
    if x3:   # fp32 in, fp32 out, products on the bf16 matrix cores by the three-way split (csrc/gemm_x3.hip)
        _x3(g, weight, keep)
    L.check(_lib().roitr_gemm(ctypes.byref(g), L.stream_ptr()), "gemm")
    return out


def linear_layernorm(x, weight, bias, gamma, beta, res=None, res_idx=None, post=None, relu=False, eps=1e-5, bf16=False, out_bf16=False,
                     x_cat=None, interp=None, x_cat_idx=None, addend=None, x3=False):
    """[relu](LayerNorm(x @ weight.T + bias + res[res_idx]) * gamma + beta + post) in ONE launch (64 / 128 / 256 output
    channels): the nn.Linear -> (+ residual) -> nn.LayerNorm call sites of attention.py:319, model/model.py:89-97,138-140.
    bf16 / out_bf16 as in linear().  interp = (feat (R, N), idx (M, 3) int32, dist2 (M, 3)): TransitionUp's three-nearest-neighbour
    interpolation (pointops.py:168-182) of the rows of `feat`, added after the activation (fp32 kernel only)."""
    x, weight, flags = _bf16_flags(bf16, x, weight, out_bf16)
    out = torch.empty((x.shape[0], weight.shape[0]), dtype=torch.bfloat16 if flags & BF16_C else torch.float32, device=x.device)
    b, gm, bt, rs, ri, po = _c(bias), _c(gamma), _c(beta), _c(res), _i32c(res_idx), _c(post)
    g = _gemm(x, weight, b, out, flags, alpha=1.0, ln_relu=int(relu), ln_eps=float(eps))
    g.ln_gamma, g.ln_beta, g.ln_res, g.ln_res_idx, g.ln_post = L.ptr(gm), L.ptr(bt), L.ptr(rs), L.ptr(ri), L.ptr(po)
    keep = []
    _k_cat(g, x, x_cat, keep, x_cat_idx, addend)
    if interp is not None:
        keep += [_c(interp[0]), _i32c(interp[1]), _c(interp[2])]
        g.ip_feat, g.ip_idx, g.ip_dist2 = L.ptr(keep[-3]), L.ptr(keep[-2]), L.ptr(keep[-1])
    if x3:
        _x3(g, weight, keep)
    L.check(_lib().roitr_gemm(ctypes.byref(g), L.stream_ptr()), "gemm+layernorm")
    return out


def add_layernorm_interp(x, gamma, beta, feat, idx, dist2, res=None, res_idx=None, relu=False, eps=1e-5):
    """[relu](LayerNorm(x + res[res_idx]) * gamma + beta) + three-nearest-neighbour interpolation of the rows of `feat`
    (roitr_add_layernorm_interp: the two-launch twin of linear_layernorm(..., interp=...))."""
    x, gm, bt, rs, ri, ft, ix, d2 = _c(x), _c(gamma), _c(beta), _c(res), _i32c(res_idx), _c(feat), _i32c(idx), _c(dist2)
    M, C = x.shape
    out = torch.empty_like(x)
    L.check(_lib().roitr_add_layernorm_interp(M, C, L.ptr(x), L.ptr(rs), L.ptr(ri), L.ptr(gm), L.ptr(bt), int(relu), float(eps),
                                               L.ptr(ft), L.ptr(ix), L.ptr(d2), L.ptr(out), L.stream_ptr()), "add_layernorm_interp")
    return out


def adaptive_superpoint_matching(src_feats, tgt_feats, src_masks, tgt_masks, min_num_correspondences=128, similarity_threshold=0.75):
    """model/modules.py:81-124 AdaptiveSuperPointMatching.forward (argument names as in the reference: the FIRST set
    indexes the first returned index list).  Returns (src_corr_indices, tgt_corr_indices, corr_scores)."""
    dev = src_feats.device
    na, nb = src_feats.shape[0], tgt_feats.shape[0]
    lib = _lib()
    xy = linear(src_feats, tgt_feats)                       # (na, nb) feature dot products
    feats = _c(torch.cat([tgt_feats, src_feats], 0))      # engine cloud order: [second set, first set]
    masks = _i32c(torch.cat([tgt_masks, src_masks], 0))
    off = torch.tensor([nb, nb + na], dtype=torch.int32, device=dev)
    stride = lib.roitr_coarse_scratch_floats(na, nb)
    scratch = torch.empty(stride, dtype=torch.float32, device=dev)
    cap = na * nb
    ia = torch.zeros(cap, dtype=torch.int32, device=dev)
    ib = torch.zeros(cap, dtype=torch.int32, device=dev)
    sc = torch.zeros(cap, dtype=torch.float32, device=dev)
    nc = torch.zeros(1, dtype=torch.int32, device=dev)
    a = _Coarse(pairs=1, C=feats.shape[1], num_corr=cap, max_ref=na, max_src=nb, feats=L.ptr(feats), node_offset=L.ptr(off),
                node_masks=L.ptr(masks), scratch=L.ptr(scratch), scratch_stride=stride, tgt_corr=L.ptr(ia), src_corr=L.ptr(ib),
                corr_scores=L.ptr(sc), n_corr=L.ptr(nc), xy=L.ptr(xy), xy_ld=nb)
    L.check(lib.roitr_adaptive_matching(ctypes.byref(a), int(min_num_correspondences), float(similarity_threshold),
                                        L.stream_ptr()), "adaptive_matching")
    n = int(nc.item())
    return ia[:n].long(), ib[:n].long(), sc[:n]


def geo_table_build(div_term, w_d, b_d, w_a, b_a, interval=2.0, d_range=48.0, a_range=12.0):
    """Host fit of the function table of the geometric embedding (csrc/geo_table.hip): returns (table on the weights' device,
    n_int_d, n_int_a, fit) with fit = [fit error d, amplitude d, fit error a, amplitude a, largest per-channel relative error d, a]
    measured in float64 on 64 probe points per interval."""
    import math
    C = int(w_d.shape[0])
    nd, na = int(math.ceil(d_range / interval)), int(math.floor(a_range / interval)) + 1
    lib = _lib()
    div_h, wd_h, bd_h, wa_h, ba_h = (_c(t.detach().cpu()) for t in (div_term, w_d, b_d, w_a, b_a))
    table = torch.empty(int(lib.roitr_geo_table_floats(C, nd, na)), dtype=torch.float32)
    fit = (ctypes.c_double * 6)()
    hp = L.host_ptr
    L.check(lib.roitr_geo_table_build(C, hp(div_h), hp(wd_h), hp(bd_h), hp(wa_h), hp(ba_h), float(interval), nd, na,
                                      hp(table), fit), "geo_table_build")
    return table.to(w_d.device), nd, na, list(fit)


def geo_embed_table(d_idx, a_idx, table, interval, n_int_d, n_int_a, div_term, w_d, b_d, w_a, b_a, out_bf16=False):
    """The embedding of geo_embed() evaluated from the function table; values outside the table are evaluated directly."""
    rows, k = int(a_idx.shape[0]), int(a_idx.shape[1])
    C = int(w_d.shape[0])
    d_idx, a_idx, table, div_term, w_d, b_d, w_a, b_a = map(_c, (d_idx, a_idx, table, div_term, w_d, b_d, w_a, b_a))
    out = torch.empty((rows, C), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=d_idx.device)
    L.check(_lib().roitr_geo_embed_table(rows, C, k, L.ptr(d_idx), L.ptr(a_idx), L.ptr(table), float(interval),
                                          int(n_int_d), int(n_int_a), L.ptr(div_term), L.ptr(w_d), L.ptr(b_d), L.ptr(w_a), L.ptr(b_a),
                                          L.ptr(out), 1 if out_bf16 else 0, L.stream_ptr()), "geo_embed_table")
    return out


def geo_embed(d_idx, a_idx, div_term, w_d, b_d, w_a, b_a, split=False, bf16=False):
    """positional_encoding.py:139-154 fused: proj_d(sinusoid(d_idx)) + max_k proj_a(sinusoid(a_idx[:, k])) for `rows` index
    rows.  split=True: the opt-in three-way bf16 split on the bf16 matrix cores (fp32-level accuracy); bf16=True: plain bf16
    operands (weights stored bf16, the sinusoid rounded to bf16, fp32 accumulate) -- the engine's bf16 operand mode."""
    rows, k = int(a_idx.shape[0]), int(a_idx.shape[1])
    C = int(w_d.shape[0])
    d_idx, a_idx, div_term, w_d, b_d, w_a, b_a = map(_c, (d_idx, a_idx, div_term, w_d, b_d, w_a, b_a))
    out = torch.empty((rows, C), dtype=torch.float32, device=d_idx.device)
    lib = _lib()
    if bf16:
        wdh, wah = w_d.to(torch.bfloat16).contiguous(), w_a.to(torch.bfloat16).contiguous()
        L.check(lib.roitr_geo_embed_bf16(rows, C, k, L.ptr(d_idx), L.ptr(a_idx), L.ptr(div_term), L.ptr(wdh), L.ptr(b_d),
                                         L.ptr(wah), L.ptr(b_a), L.ptr(out), L.stream_ptr()), "geo_embed_bf16")
        return out
    if split:
        wd3 = torch.empty((3, C, C), dtype=torch.int16, device=out.device)
        wa3 = torch.empty((3, C, C), dtype=torch.int16, device=out.device)
        L.check(lib.roitr_split3_bf16(C * C, L.ptr(w_d), L.ptr(wd3), L.stream_ptr()), "split3")
        L.check(lib.roitr_split3_bf16(C * C, L.ptr(w_a), L.ptr(wa3), L.stream_ptr()), "split3")
        L.check(lib.roitr_geo_embed_split(rows, C, k, L.ptr(d_idx), L.ptr(a_idx), L.ptr(div_term), L.ptr(wd3), L.ptr(b_d),
                                          L.ptr(wa3), L.ptr(b_a), L.ptr(out), L.stream_ptr()), "geo_embed_split")
    else:
        L.check(lib.roitr_geo_embed(rows, C, k, L.ptr(d_idx), L.ptr(a_idx), L.ptr(div_term), L.ptr(w_d), L.ptr(b_d),
                                    L.ptr(w_a), L.ptr(b_a), L.ptr(out), L.stream_ptr()), "geo_embed")
    return out


def local_attention_fold(x, q, qt, group_idx, ppf, wpe, wvpe, bvpe, node_order=None, packed=False):
    """TransitionDown form of the local PPF attention with the key / value projections folded into the query side
    (csrc/local_attn.hip local_attn_fold_kernel; include/roitr_engine.h RoitrLocalAttnFold).  x (N_in, I) input rows, q (M, H),
    qt (M, 4, I) = Wk'_h^T q_h per head, group_idx (M, 16) int32 rows of x, ppf (M, 16, 4), wpe / wvpe (H, 4), bvpe (H).
    Returns (xbar (M, 4, I) = sum_j a_hj x_j, vpart (M, H) = Wvpe_h pbar_h + bvpe_h): the attention output of the unfolded form is
    vpart + [Wv'_h xbar_h + bv'_h]_h.  packed=True: q and qt are handed over as the two column blocks of ONE (M, H + 4 I) buffer (row
    stride H + 4 I for both: RoitrLocalAttnFold.ldq / ldqt), the way the engine's single q | q~ GEMM leaves them."""
    x, q, qt, ppf, wpe, wvpe, bvpe = _c(x), _c(q), _c(qt), _c(ppf), _c(wpe), _c(wvpe), _c(bvpe)
    both = torch.cat([q, qt.reshape(q.shape[0], -1)], 1).contiguous() if packed else None
    group_idx = _i32c(group_idx)
    M, H, I = int(q.shape[0]), int(q.shape[1]), int(x.shape[1])
    if int(group_idx.shape[1]) != 16:
        raise L.RoitrError("local_attention_fold: 16 neighbours per node")
    xbar = torch.empty((M, 4, I), dtype=torch.float32, device=x.device)
    vpart = torch.empty((M, H), dtype=torch.float32, device=x.device)
    a = _LocalAttnFold()
    a.M, a.in_dim, a.H = M, I, H
    a.x, a.ldx, a.q, a.ldq, a.qt = L.ptr(x), I, L.ptr(q), H, L.ptr(qt)
    if packed:
        a.q, a.ldq, a.ldqt = L.ptr(both), H + 4 * I, H + 4 * I
        a.qt = ctypes.c_void_p(both.data_ptr() + 4 * H)
    a.group_idx, a.ppf, a.wpe, a.wvpe, a.bvpe = L.ptr(group_idx), L.ptr(ppf), L.ptr(wpe), L.ptr(wvpe), L.ptr(bvpe)
    a.scale, a.xbar, a.vpart = 1.0 / float(H // 4) ** 0.5, L.ptr(xbar), L.ptr(vpart)
    no = _c(node_order)
    a.node_order = L.ptr(no)
    L.check(_lib().roitr_local_attention_fold(ctypes.byref(a), L.stream_ptr()), "local_attention_fold")
    return xbar, vpart


def _attn_rows(t, what, dtype):
    """Row stride of a 2-D device operand of `dtype` whose rows are contiguous (a column block of a wider buffer is fine)."""
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype != dtype:
        raise L.RoitrError(f"local_attention: {what} must be a 2-D {dtype} tensor with contiguous rows")
    return int(t.stride(0))


def local_attention(q, k, v, group_idx, ppf, wvpe, bvpe, wpe=None, bpe=None, ldq=None, ldk=None, ldv=None, ldo=None, bf16=False,
                    node_order=None, out=None, heads=4, scale=None):
    """The generic local PPF attention (csrc/local_attn.hip local_attn_kernel / local_attn_quad_kernel; include/roitr_engine.h
    RoitrLocalAttn; attention.py:152-200 with the positional branch folded).  q (M, >= H) rows of the nodes, k / v (N_in, >= H) rows of the
    input cloud, group_idx (M, K) int32 rows of k / v, K in {8, 16}, ppf (M, K, 4), wvpe (H, 4), bvpe (H).  wpe (H, 4) / bpe (H) given: the
    kernel forms the positional score coefficients itself; None: the q rows carry them as 5 x heads extra columns behind the H channels
    ([Wpe_h^T q_h (4), q_h . bpe_h] per head).  ldq / ldk / ldv / ldo: row strides in elements (default: the tensors' own), so q | k | v may
    be column blocks of one buffer.  bf16=True: q / k / v are torch.bfloat16 rows and so is the output (RoitrLocalAttn::bf16 = 3).
    node_order: optional (M, 4) float32 whose last column holds the node index bits.  out: optional preallocated (>= M, >= H) tensor with
    contiguous rows; only its first H columns of the M node rows are written.  Returns out (M, H)."""
    dt = torch.bfloat16 if bf16 else torch.float32
    sq, sk, sv = _attn_rows(q, "q", dt), _attn_rows(k, "k", dt), _attn_rows(v, "v", dt)
    group_idx, ppf, wvpe, bvpe, wpe, bpe, no = _i32c(group_idx), _c(ppf), _c(wvpe), _c(bvpe), _c(wpe), _c(bpe), _c(node_order)
    M, K, H = int(group_idx.shape[0]), int(group_idx.shape[1]), int(wvpe.shape[0])
    if (wpe is None) != (bpe is None):
        raise L.RoitrError("local_attention: wpe and bpe are given together or not at all")
    if int(q.shape[0]) < M or int(q.shape[1]) < (H if wpe is not None else H + 5 * heads) or int(k.shape[1]) < H or int(v.shape[1]) < H:
        raise L.RoitrError("local_attention: q (M, >= H [+ 5 * heads]), k / v (N_in, >= H)")
    if out is None:
        out = torch.empty((M, H), dtype=dt, device=q.device)
    so = _attn_rows(out, "out", dt)
    if int(out.shape[0]) < M or int(out.shape[1]) < H:
        raise L.RoitrError("local_attention: out (>= M, >= H)")
    a = _LocalAttn()
    a.M, a.K, a.H, a.heads = M, K, H, int(heads)
    a.q, a.ldq, a.k, a.ldk, a.v, a.ldv = L.ptr(q), int(sq if ldq is None else ldq), L.ptr(k), int(sk if ldk is None else ldk), L.ptr(v), int(sv if ldv is None else ldv)
    a.group_idx, a.ppf, a.wvpe, a.bvpe = L.ptr(group_idx), L.ptr(ppf), L.ptr(wvpe), L.ptr(bvpe)
    a.scale = 1.0 / float(H // heads) ** 0.5 if scale is None else float(scale)
    a.out, a.ldo, a.node_order = L.ptr(out), int(so if ldo is None else ldo), L.ptr(no)
    a.bf16 = 3 if bf16 is True else int(bf16)
    a.wpe, a.bpe = L.ptr(wpe), L.ptr(bpe)
    L.check(_lib().roitr_local_attention(ctypes.byref(a), L.stream_ptr()), "local_attention")
    return out


def build_pfold(wpe, bpe, heads=4):
    """roitr_build_pfold (csrc/local_attn.hip): Pfold (5 * heads, H) with row 5 h + j = Wpe[:, j] (j < 4) / bpe (j = 4) on the channels of
    head h and zero elsewhere, so that q @ Pfold.T are the extra q columns of RoitrLocalAttn."""
    wpe, bpe = _c(wpe), _c(bpe)
    H = int(wpe.shape[0])
    out = torch.empty((5 * int(heads), H), dtype=torch.float32, device=wpe.device)
    L.check(_lib().roitr_build_pfold(H, int(heads), L.ptr(wpe), L.ptr(bpe), L.ptr(out), L.stream_ptr()), "build_pfold")
    return out


# ------------------------------------------------------------------------------------------------
# Row-wise layers (csrc/nn_ops.hip; "row-wise layers" of include/roitr_engine.h)
# ------------------------------------------------------------------------------------------------
def add_layernorm(x, gamma, beta, res=None, res_idx=None, post=None, relu=False, eps=1e-5):
    """roitr_add_layernorm: [relu](LayerNorm(x + res[res_idx]) * gamma + beta + post) for x (M, C), C <= 1024; res (R, C) with res_idx
    (M,) int32 rows of it, or (M, C) without; post (M, C).  attention.py:319, model/model.py:138-140."""
    x, gm, bt, rs, ri, po = _c(x), _c(gamma), _c(beta), _c(res), _i32c(res_idx), _c(post)
    M, C = int(x.shape[0]), int(x.shape[1])
    out = torch.empty_like(x)
    L.check(_lib().roitr_add_layernorm(M, C, L.ptr(x), L.ptr(rs), L.ptr(ri), L.ptr(gm), L.ptr(bt), L.ptr(po), int(relu), float(eps),
                                        L.ptr(out), L.stream_ptr()), "add_layernorm")
    return out


def l2_normalize(x):
    """roitr_l2_normalize: F.normalize(x, p=2, dim=1) of x (M, C), C <= 1024 (model/RIGA_v2.py:64-65)."""
    x = _c(x)
    out = torch.empty_like(x)
    L.check(_lib().roitr_l2_normalize(int(x.shape[0]), int(x.shape[1]), L.ptr(x), L.ptr(out), L.stream_ptr()), "l2_normalize")
    return out


def segment_mean(x, offset):
    """roitr_segment_mean: the mean row of every cloud of x (T, C); offset (b,) int32 cumulative cloud ends, no cloud empty
    (model/model.py:101-109).  Returns (b, C)."""
    x, off = _c(x), _i32c(offset)
    b, C = int(off.shape[0]), int(x.shape[1])
    out = torch.empty((b, C), dtype=torch.float32, device=x.device)
    L.check(_lib().roitr_segment_mean(b, C, L.ptr(x), L.ptr(off), L.ptr(out), L.stream_ptr()), "segment_mean")
    return out


def interp3_add(feat, idx, dist2, base=None):
    """roitr_interp3_add: base + the three-nearest-neighbour inverse-distance interpolation of the rows of feat (R, C); idx (n, 3) int32
    rows of feat, dist2 (n, 3) SQUARED distances, base (n, C) or None (functions/pointops.py:168-182 + model/model.py:116)."""
    feat, idx, dist2, base = _c(feat), _i32c(idx), _c(dist2), _c(base)
    n, C = int(idx.shape[0]), int(feat.shape[1])
    out = torch.empty((n, C), dtype=torch.float32, device=feat.device)
    L.check(_lib().roitr_interp3_add(n, C, L.ptr(feat), L.ptr(idx), L.ptr(dist2), L.ptr(base), L.ptr(out), L.stream_ptr()), "interp3_add")
    return out


def gather_rows(x, idx, limit=0):
    """roitr_gather_rows: out[r] = x[idx[r]] for x (R, C), idx (rows,) int32; a negative index gives a zero row, and so does an index
    >= limit when limit > 0 (limit <= 0: every non-negative index must be a row of x)."""
    x, idx = _c(x), _i32c(idx)
    rows, C = int(idx.shape[0]), int(x.shape[1])
    out = torch.empty((rows, C), dtype=torch.float32, device=x.device)
    L.check(_lib().roitr_gather_rows(rows, C, L.ptr(x), L.ptr(idx), int(limit), L.ptr(out), L.stream_ptr()), "gather_rows")
    return out


def compose_idx(outer, inner):
    """roitr_compose_idx: outer[inner] for int32 index vectors."""
    outer, inner = _i32c(outer), _i32c(inner)
    out = torch.empty_like(inner)
    L.check(_lib().roitr_compose_idx(int(inner.shape[0]), L.ptr(outer), L.ptr(inner), L.ptr(out), L.stream_ptr()), "compose_idx")
    return out


def transpose(x, out=None):
    """roitr_transpose: x (rows, cols) float32 -> (cols, rows).  x and a preallocated out may be column blocks of wider buffers (contiguous
    rows; their row strides are the ld_in / ld_out of the call): only the (cols, rows) block of out is written."""
    rows, cols = int(x.shape[0]), int(x.shape[1])
    if out is None:
        out = torch.empty((cols, rows), dtype=torch.float32, device=x.device)
    for t, shape in ((x, (rows, cols)), (out, (cols, rows))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or t.stride(1) != 1 or t.stride(0) < shape[1]:
            raise L.RoitrError("transpose: float32 (rows, cols) -> (cols, rows) with contiguous rows")
    L.check(_lib().roitr_transpose(rows, cols, L.ptr(x), int(x.stride(0)), L.ptr(out), int(out.stride(0)), L.stream_ptr()), "transpose")
    return out


def add_vectors(a, b):
    """roitr_add_vectors: a + b over n floats (the bias of a folded layer)."""
    a, b = _c(a), _c(b)
    if a.shape != b.shape:
        raise L.RoitrError("add_vectors: two vectors of one length")
    out = torch.empty_like(a)
    L.check(_lib().roitr_add_vectors(int(a.numel()), L.ptr(a), L.ptr(b), L.ptr(out), L.stream_ptr()), "add_vectors")
    return out


def local_td(x, node_idx, group_idx, ppf, w, node_order=None):
    """The TransitionDown transformer of the 64 -> 128 wide level in one launch (csrc/local_block.hip local_td_kernel;
    include/roitr_engine.h RoitrLocalTd).  x (N_in, 64) input rows, node_idx (M,) int32 row of x of every node, group_idx (M, 16) int32
    rows of x, ppf (M, 16, 4); w: dict of the folded weights wqqt (384, 64), bqqt (384), wv (128, 64), bv (128), wpe / wvpe (128, 4),
    bvpe (128), wcat (128, 192), bcat, norm_w, norm_b, wout (128, 128), bout.  Returns (M, 128)."""
    x, ppf = _c(x), _c(ppf)
    node_idx, group_idx = _i32c(node_idx), _i32c(group_idx)
    w = {k: _c(v) for k, v in w.items()}
    M, I, H = int(node_idx.shape[0]), int(x.shape[1]), int(w["wout"].shape[0])
    if int(group_idx.shape[1]) != 16 or not _lib().roitr_local_td_supported(I, H, 16):
        raise L.RoitrError("local_td: in_dim 64, H 128, 16 neighbours per node")
    out = torch.empty((M, H), dtype=torch.float32, device=x.device)
    a = _LocalTd()
    a.M, a.in_dim, a.H = M, I, H
    a.x, a.node_idx, a.group_idx, a.ppf = L.ptr(x), L.ptr(node_idx), L.ptr(group_idx), L.ptr(ppf)
    no = _c(node_order)
    a.node_order = L.ptr(no)
    for k in ("wqqt", "bqqt", "wv", "bv", "wpe", "wvpe", "bvpe", "wcat", "bcat", "norm_w", "norm_b", "wout", "bout"):
        setattr(a, k, L.ptr(w[k]))
    a.scale, a.eps, a.out = 1.0 / float(H // 4) ** 0.5, 1e-5, L.ptr(out)
    L.check(_lib().roitr_local_td(ctypes.byref(a), L.stream_ptr()), "local_td")
    return out


def local_block(x, kv, group_idx, ppf, w, node_order=None, variant=None, bf16_weights=False):
    """The block form of the local PPF transformer in one launch (csrc/local_block.hip; model/model.py:131-142 around
    ppftransformer.py:227-253).  x (M, H), kv (M, 2H) = k | v rows of every point, group_idx (M, K) int32, ppf (M, K, 4);
    w: dict of the FOLDED weights (include/roitr_engine.h RoitrLocalBlock): wq (H,H) bq, wpe (H,4) bpe, wvpe (H,4) bvpe,
    wcat (H,2H) bcat, norm_w norm_b, wout (H,H) bout, bn2_w bn2_b.  node_order: optional (M, 4) float32 whose last column
    holds the node index bits (the grid's sorted-point array).  variant: tuning hook (1: no attention, 2: attention only).
    A bfloat16 `kv` tensor is gathered as stored (RoitrLocalBlock::kv_bf16, the engine's bf16 operand mode); bf16_weights (with it):
    the three on-chip GEMMs take bf16 matrix operands (RoitrLocalBlock::wq_h / wcat_h / wout_h; the copies are made here)."""
    M, H = int(x.shape[0]), int(x.shape[1])
    K = int(group_idx.shape[1])
    kv_h = kv.dtype == torch.bfloat16
    x, kv, ppf = _c(x), (kv.contiguous() if kv_h else _c(kv)), _c(ppf)
    group_idx = _i32c(group_idx)
    keep = {k: _c(v) for k, v in w.items()}
    out = torch.empty((M, H), dtype=torch.float32, device=x.device)
    a = _LocalBlock()
    a.M, a.K, a.H = M, K, H
    a.x, a.kv, a.group_idx, a.ppf = L.ptr(x), L.ptr(kv), L.ptr(group_idx), L.ptr(ppf)
    no = _c(node_order)
    a.node_order = L.ptr(no)
    for k in ("wq", "bq", "wpe", "bpe", "wvpe", "bvpe", "wcat", "bcat", "norm_w", "norm_b", "wout", "bout", "bn2_w", "bn2_b"):
        setattr(a, k, L.ptr(keep[k]))
    a.scale, a.eps, a.out = 1.0 / float(H // 4) ** 0.5, 1e-5, L.ptr(out)
    a.kv_bf16 = int(kv_h)
    if bf16_weights:
        keep_h = {k: keep[k].to(torch.bfloat16).contiguous() for k in ("wq", "wcat", "wout")}
        a.wq_h, a.wcat_h, a.wout_h = L.ptr(keep_h["wq"]), L.ptr(keep_h["wcat"]), L.ptr(keep_h["wout"])
    if variant is None:
        L.check(_lib().roitr_local_block(ctypes.byref(a), L.stream_ptr()), "local_block")
    else:
        L.check(_lib().roitr_local_block_dbg(ctypes.byref(a), int(variant), L.stream_ptr()), "local_block_dbg")
    return out


def local_first(x, group_idx, ppf, w, node_order=None, out=None):
    """The first local transformer of the network in its rank-1 form (csrc/local_block.hip local_first_kernel;
    include/roitr_engine.h RoitrLocalFirst).  x (M,) the scalar input feature, group_idx (M, K) int32, K in {8, 16}, ppf (M, K, 4);
    w: dict of head_consts (64), G (64, 32), zero_bias (64), norm_w, norm_b, wout (64, 64), bout.  Returns (M, 64); a preallocated
    contiguous float32 `out` (>= M, 64) is written in its first M rows only."""
    x, ppf = _c(x), _c(ppf)
    group_idx = _i32c(group_idx)
    w = {k: _c(v) for k, v in w.items()}
    M, K = int(x.shape[0]), int(group_idx.shape[1])
    if out is None:
        out = torch.empty((M, 64), dtype=torch.float32, device=x.device)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 2 or out.shape[1] != 64 or out.shape[0] < M:
        raise L.RoitrError("local_first: out must be a contiguous float32 (>= M, 64) tensor")
    a = _LocalFirst()
    a.M, a.K = M, K
    a.x, a.group_idx, a.ppf = L.ptr(x), L.ptr(group_idx), L.ptr(ppf)
    no = _c(node_order)
    a.node_order = L.ptr(no)
    for k in ("head_consts", "G", "zero_bias", "norm_w", "norm_b", "wout", "bout"):
        setattr(a, k, L.ptr(w[k]))
    a.scale, a.eps, a.out = 0.25, 1e-5, L.ptr(out)
    L.check(_lib().roitr_local_first(ctypes.byref(a), L.stream_ptr()), "local_first")
    return out


def _weight_view(t):
    if t.dim() != 2 or t.dtype != torch.float32 or t.stride(1) != 1:
        raise L.RoitrError("local weights: a 2-D float32 tensor with contiguous rows")
    return int(t.shape[0]), int(t.shape[1]), int(t.stride(0))


def local_weights_prepare(w):
    """roitr_local_weights_prepare: a fragment-ordered device copy of the (rows, k) weight `w` (a device tensor, or a row / column
    slice of one), kept by the library under w's address until local_weights_release(w).  local_block / local_td / local_first take
    the fragment path when all of their weights are prepared (include/roitr_engine.h); the caller keeps `w` alive and unchanged."""
    rows, k, ldw = _weight_view(w)
    L.check(_lib().roitr_local_weights_prepare(L.ptr(w), rows, k, ldw, L.stream_ptr()), "local_weights_prepare")


def local_weights_release(w):
    """roitr_local_weights_release: frees every copy kept under w's address (none: a no-op)."""
    L.check(_lib().roitr_local_weights_release(L.ptr(w)), "local_weights_release")


def local_weights_count():
    """roitr_local_weights_count: the number of fragment-ordered copies the library holds."""
    return int(_lib().roitr_local_weights_count())


def local_weights_reorder_host(w):
    """roitr_local_weights_reorder_host: the fragment order of a HOST weight (rows, k) (rows may be strided), as a flat host tensor."""
    rows, k, ldw = _weight_view(w)
    dst = torch.empty(rows * k, dtype=torch.float32)
    L.check(_lib().roitr_local_weights_reorder_host(L.host_ptr(w), rows, k, ldw, L.host_ptr(dst)), "local_weights_reorder_host")
    return dst


# ------------------------------------------------------------------------------------------------
# Global geometric transformer (csrc/geo_attn.hip)
# ------------------------------------------------------------------------------------------------
def _rows(t, what):
    """Row stride of a 2-D float32 device operand whose rows are contiguous (a column slice of a wider buffer is fine)."""
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype != torch.float32:
        raise L.RoitrError(f"multi_head_attention: {what} must be a 2-D float32 tensor with contiguous rows")
    return t.stride(0)


def multi_head_attention(q, k, v, offset, cloud_of_row, nk_max, heads=4, partner=None, E=None, eoff=None, qt=None, bp=None,
                         scale=None, q_row0=0, q_rows=None, out=None, ebar=None):
    """roitr_mha (include/roitr_engine.h RoitrMha): geoattention.py:26-66 without E, geoattention.py:87-136 with the RPE branch
    folded with E.  q / k / v (T, C) rows of all clouds, each with its own leading dimension (their row strides: q | k | v may be
    the column blocks of one (T, 3C) buffer); offset (b,) int32 cumulative cloud ends, cloud_of_row (T,) int32, partner (b,) int32
    key cloud of every cloud (None: self attention); nk_max bounds the key count of every cloud.  With E: E the concatenated
    (n_c, n_c, C) blocks (float32 or bfloat16) at element offsets eoff (b,) int64 / C, qt (T, heads, C) = Wp_h^T q_h,
    bp (C,) = proj_p.bias.  Query rows [q_row0, q_row0 + q_rows) are computed into out (T, C) and ebar (T, heads, C) =
    sum_j a'_hj E_ij (preallocated ones are written in those rows only).  Returns (out, ebar); ebar is None without E."""
    a, out, ebar = mha_args(q, k, v, offset, cloud_of_row, nk_max, heads, partner, E, eoff, qt, bp, scale, q_row0, q_rows, out, ebar)
    L.check(_lib().roitr_mha(ctypes.byref(a), L.stream_ptr()), "mha")
    return out, ebar


def mha_args(q, k, v, offset, cloud_of_row, nk_max, heads=4, partner=None, E=None, eoff=None, qt=None, bp=None,
             scale=None, q_row0=0, q_rows=None, out=None, ebar=None):
    """The RoitrMha of a multi_head_attention call (below) with its checks, and the output tensors: (struct, out, ebar).  The struct
    holds addresses only: the caller keeps the tensors alive until the launch is queued."""
    T, C = int(q.shape[0]), int(q.shape[1])
    q_rows = T - q_row0 if q_rows is None else int(q_rows)
    if q_row0 < 0 or q_row0 + q_rows > min(T, int(cloud_of_row.numel())):
        raise L.RoitrError("multi_head_attention: query rows outside q / cloud_of_row")
    ldq, ldk, ldv = _rows(q, "q"), _rows(k, "k"), _rows(v, "v")
    if out is None:
        out = torch.empty((T, C), dtype=torch.float32, device=q.device)
    ldo = _rows(out, "out")
    a = _Mha()
    a.q_row0, a.q_rows, a.C, a.heads = int(q_row0), q_rows, C, int(heads)
    a.q, a.ldq, a.k, a.ldk, a.v, a.ldv = L.ptr(q), ldq, L.ptr(k), ldk, L.ptr(v), ldv
    a.offset, a.cloud_of_row, a.partner = L.ptr(offset), L.ptr(cloud_of_row), L.ptr(partner)
    a.scale = 1.0 / float(C // heads) ** 0.5 if scale is None else float(scale)
    a.nk_max, a.out, a.ldo = int(nk_max), L.ptr(out), ldo
    if E is not None:
        if E.dtype not in (torch.float32, torch.bfloat16) or not E.is_contiguous() or eoff.dtype != torch.int64:
            raise L.RoitrError("multi_head_attention: E float32 / bfloat16 contiguous, eoff int64")
        if qt.shape != (T, heads, C) or not qt.is_contiguous() or bp.numel() != C:
            raise L.RoitrError("multi_head_attention: qt (T, heads, C) contiguous, bp (C,)")
        if ebar is None:
            ebar = torch.empty((T, heads, C), dtype=torch.float32, device=q.device)
        if ebar.shape != (T, heads, C) or not ebar.is_contiguous():
            raise L.RoitrError("multi_head_attention: ebar (T, heads, C) contiguous")
        a.E, a.eoff, a.qt, a.bp, a.ebar = L.ptr(E), L.ptr(eoff), L.ptr(qt), L.ptr(bp), L.ptr(ebar)
        a.e_bf16 = int(E.dtype == torch.bfloat16)
    return a, out, ebar


def geo_indices(points, sizes, sigma_d=0.2, sigma_a=15.0, angle_k=3):
    """roitr_geo_indices: positional_encoding.py:110-137 get_embedding_indices for the clouds of `sizes` (host ints) laid out back
    to back in points (rows, 3).  Returns (d_idx, a_idx): the concatenated (n_c, n_c) and (n_c, n_c, angle_k) blocks, flat,
    as (sum n_c^2,) and (sum n_c^2, angle_k)."""
    dev = points.device
    sizes = [int(n) for n in sizes]
    ends = torch.tensor(sizes, dtype=torch.int64).cumsum(0)
    blocks = torch.tensor([n * n for n in sizes], dtype=torch.int64)
    eoff = (blocks.cumsum(0) - blocks).to(dev)
    offset = ends.to(torch.int32).to(dev)
    cloud_of_row = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes)).to(dev)
    etot = int(blocks.sum())
    pts = _c(points)
    d_idx = torch.empty((etot,), dtype=torch.float32, device=dev)
    a_idx = torch.empty((etot, angle_k), dtype=torch.float32, device=dev)
    L.check(_lib().roitr_geo_indices(int(ends[-1]), L.ptr(pts), L.ptr(offset), L.ptr(cloud_of_row), L.ptr(eoff), float(sigma_d),
                                      float(sigma_a), int(angle_k), max(sizes), L.ptr(d_idx), L.ptr(a_idx), L.stream_ptr()),
            "geo_indices")
    return d_idx, a_idx


# ------------------------------------------------------------------------------------------------
# Ground-truth side outputs (csrc/gt.hip), batched over pairs; clouds laid out [src_0..src_{B-1}, tgt_0..tgt_{B-1}].
# ------------------------------------------------------------------------------------------------
def build_padded_clouds(points, pt_offset, rot, trans):
    """roitr_build_padded_clouds (lib/utils.py:505-506 + RIGA_v2.py:86-87): points (n,3) of the 2*pairs clouds, pt_offset (2*pairs,)
    cumulative, rot (pairs,3,3), trans (pairs,3) -> (padded (n + 2*pairs, 3), offsets (3*pairs,) i32)."""
    dev = points.device
    pairs = pt_offset.shape[0] // 2
    n = points.shape[0]
    pts, off = _c(points), _i32c(pt_offset)
    r, t = _c(rot), _c(trans)
    out = torch.empty((n + 2 * pairs, 3), dtype=torch.float32, device=dev)
    out_off = torch.empty(3 * pairs, dtype=torch.int32, device=dev)
    L.check(_lib().roitr_build_padded_clouds(pairs, n, L.ptr(pts), L.ptr(off), L.ptr(r), L.ptr(t), L.ptr(out), L.ptr(out_off),
                                              L.stream_ptr()), "build_padded_clouds")
    return out, out_off


def node_occlusion_score(cloud_of_node, pt_offset, knn_idx, knn_mask, node_masks, d2_padded, overlap_thres=0.0375):
    """lib/utils.py:511-527 for all nodes of all clouds: knn_idx / knn_mask (n_nodes, limit) cloud-local with the pad index n_c,
    d2_padded the squared kNN(1) distance of every padded point to the partner cloud -> scores (n_nodes,) f32."""
    dev = knn_idx.device
    n_nodes, limit = knn_idx.shape
    con, off = _i32c(cloud_of_node), _i32c(pt_offset)
    ki, km, nm = _i32c(knn_idx), _i32c(knn_mask), _i32c(node_masks)
    d2 = _c(d2_padded)
    out = torch.empty(n_nodes, dtype=torch.float32, device=dev)
    L.check(_lib().roitr_node_occlusion_score(n_nodes, limit, L.ptr(con), L.ptr(off), L.ptr(ki), L.ptr(km), L.ptr(nm), L.ptr(d2),
                                               float(overlap_thres), L.ptr(out), L.stream_ptr()), "node_occlusion_score")
    return out


def node_correspondences(nodes, node_offset, node_masks, points, pt_offset, knn_idx, knn_mask, rot, trans, pos_radius,
                         max_nodes=None, mat_stride=None):
    """lib/utils.py:530-614 get_node_correspondences for `pairs` pairs (ref = tgt, src = src) -> (out_idx (pairs, mat_stride, 2) i32
    [tgt, src] local node indices in torch.nonzero order, out_overlap (pairs, mat_stride) f32, out_count (pairs,) i32); only the
    first out_count[p] rows of pair p are written."""
    dev = nodes.device
    pairs = node_offset.shape[0] // 2
    n_nodes, limit = knn_idx.shape
    noff, poff = _i32c(node_offset), _i32c(pt_offset)
    if max_nodes is None:
        ends = [0] + noff.tolist()
        max_nodes = max(b - a for a, b in zip(ends[:-1], ends[1:]))
    max_nodes = int(max_nodes)
    mat_stride = max_nodes * max_nodes if mat_stride is None else int(mat_stride)
    nd, pts = _c(nodes), _c(points)
    nm, ki, km = _i32c(node_masks), _i32c(knn_idx), _i32c(knn_mask)
    r, t = _c(rot), _c(trans)
    overlap = torch.empty((pairs, mat_stride), dtype=torch.float32, device=dev)
    out_idx = torch.zeros((pairs, mat_stride, 2), dtype=torch.int32, device=dev)
    out_ov = torch.zeros((pairs, mat_stride), dtype=torch.float32, device=dev)
    out_cnt = torch.zeros(pairs, dtype=torch.int32, device=dev)
    nodes_t = torch.empty((n_nodes, 3), dtype=torch.float32, device=dev)
    radius = torch.empty(n_nodes, dtype=torch.float32, device=dev)
    a = _NodeCorr(pairs=pairs, limit=limit, max_nodes=max_nodes, pos_radius=float(pos_radius), nodes=L.ptr(nd), node_offset=L.ptr(noff),
                  node_masks=L.ptr(nm), points=L.ptr(pts), pt_offset=L.ptr(poff), knn_idx=L.ptr(ki), knn_mask=L.ptr(km), rot=L.ptr(r),
                  trans=L.ptr(t), overlap=L.ptr(overlap), mat_stride=mat_stride, out_idx=L.ptr(out_idx), out_overlap=L.ptr(out_ov),
                  out_count=L.ptr(out_cnt), n_nodes=n_nodes, nodes_t=L.ptr(nodes_t), radius=L.ptr(radius))
    L.check(_lib().roitr_node_correspondences(ctypes.byref(a), L.stream_ptr()), "node_correspondences")
    return out_idx, out_ov, out_cnt
