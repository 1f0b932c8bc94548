"""Float64 restatements (numpy only) of the local PPF attention and of the first local transformer, for the tests of
csrc/local_attn.hip and csrc/local_block.hip local_first_kernel.  Nothing here loads the HIP library.

attention_unfolded64 is attention.py:152-200 the way oracle/roitr_ref.py local_ppf_transformer states it: the positional terms p and vp
are formed per neighbour, nothing is folded.  The folded pieces the kernels consume (the 5 extra q columns per head, the rank-1
constants of RoitrLocalFirst) are derived here in float64 from the same weights, and tests/test_local_attn_cpu.py checks on the CPU
that they evaluate to the unfolded function."""
import numpy as np

F64 = np.float64


def softmax64(s, axis):
    e = np.exp(s - s.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def layer_norm64(t, w, b, eps=1e-5):
    mu = t.mean(-1, keepdims=True)
    return (t - mu) / np.sqrt(((t - mu) ** 2).mean(-1, keepdims=True) + eps) * w + b


def attention_unfolded64(q, k, v, group_idx, ppf, wpe, bpe, wvpe, bvpe, heads=4):
    """q (M, H) rows of the nodes, k / v (N_in, H) rows of the input cloud, group_idx (M, K), ppf (M, K, 4), wpe / wvpe (H, 4), bpe / bvpe (H)
    -> (M, H): softmax_K((q_h . k_h[g] + q_h . p_h) / sqrt(c)) @ (v[g] + vp) per head, p = ppf wpe^T + bpe, vp = ppf wvpe^T + bvpe."""
    q, k, v, ppf, wpe, bpe, wvpe, bvpe = (np.asarray(t, F64) for t in (q, k, v, ppf, wpe, bpe, wvpe, bvpe))
    M, K = group_idx.shape
    H = q.shape[1]
    c = H // heads
    p = (ppf @ wpe.T + bpe).reshape(M, K, heads, c)
    vp = (ppf @ wvpe.T + bvpe).reshape(M, K, heads, c)
    kg = k[group_idx].reshape(M, K, heads, c)
    vg = v[group_idx].reshape(M, K, heads, c)
    qh = q.reshape(M, 1, heads, c)
    s = ((qh * kg).sum(-1) + (qh * p).sum(-1)) / np.sqrt(c)          # (M, K, heads)
    a = softmax64(s, 1)
    return (a[..., None] * (vg + vp)).sum(1).reshape(M, H)


def qp_columns64(q, wpe, bpe, heads=4):
    """The 5 x heads extra q columns of RoitrLocalAttn: per head [Wpe_h^T q_h (4), q_h . bpe_h (1)] -> (M, 5 * heads)."""
    q, wpe, bpe = np.asarray(q, F64), np.asarray(wpe, F64), np.asarray(bpe, F64)
    M, H = q.shape
    c = H // heads
    qh = q.reshape(M, heads, c)
    cols = np.empty((M, heads, 5), F64)
    cols[:, :, :4] = np.einsum("mhc,hct->mht", qh, wpe.reshape(heads, c, 4))
    cols[:, :, 4] = np.einsum("mhc,hc->mh", qh, bpe.reshape(heads, c))
    return cols.reshape(M, 5 * heads)


def attention_folded64(q, qp, k, v, group_idx, ppf, wvpe, bvpe, heads=4):
    """The folded form csrc/local_attn.hip evaluates, in float64: scores from the extra columns qp (M, 5 * heads), the positional value
    term from pbar_h = sum_k a_hk ppf_k."""
    q, qp, k, v, ppf, wvpe, bvpe = (np.asarray(t, F64) for t in (q, qp, k, v, ppf, wvpe, bvpe))
    M, K = group_idx.shape
    H = q.shape[1]
    c = H // heads
    qp = qp.reshape(M, heads, 5)
    s = np.einsum("mhc,mkhc->mhk", q.reshape(M, heads, c), k[group_idx].reshape(M, K, heads, c))
    s = (s + np.einsum("mht,mkt->mhk", qp[:, :, :4], ppf) + qp[:, :, 4:5]) / np.sqrt(c)
    a = softmax64(s, 2)                                               # (M, heads, K)
    out = np.einsum("mhk,mkhc->mhc", a, v[group_idx].reshape(M, K, heads, c))
    pbar = np.einsum("mhk,mkt->mht", a, ppf)
    out = out + np.einsum("hct,mht->mhc", wvpe.reshape(heads, c, 4), pbar)
    return out.reshape(M, H) + bvpe


# ---------------------------------------------------------------- the first local transformer (in_planes = 1, H = 64)
FIRST_KEYS = ("w_in", "b_in", "wq", "bq", "wk", "bk", "wv", "bv", "wpe", "bpe", "wvpe", "bvpe", "w_lin", "b_lin", "norm_w", "norm_b",
              "w_out", "b_out")


def first_layer_weights(rng, H=64):
    """A weight set of the first layer: w_in, b_in (H,); Wq / Wk / Wv / W_lin / W_out N(0, 1) / sqrt(H); biases and the folded positional
    branch N(0, 1); norm 1 + 0.1 N, 0.1 N.  float64 values that are exact in fp32."""
    n = lambda *s: rng.standard_normal(s).astype(np.float32).astype(F64)
    w = dict(w_in=n(H), b_in=n(H))
    for name in ("q", "k", "v", "_lin", "_out"):
        w["w" + name] = (rng.standard_normal((H, H)) / np.sqrt(H)).astype(np.float32).astype(F64)
        w["b" + name] = n(H)
    w.update(wpe=n(H, 4), bpe=n(H), wvpe=n(H, 4), bvpe=n(H))
    w["norm_w"] = (1 + 0.1 * rng.standard_normal(H)).astype(np.float32).astype(F64)
    w["norm_b"] = (0.1 * rng.standard_normal(H)).astype(np.float32).astype(F64)
    return w


def first_layer_unfolded64(w, x, group_idx, ppf, heads=4):
    """The layer the long way (ppftransformer.py:227-253 with a scalar input feature): f = x w_in + b_in, q / k / v / p / vp, attention,
    linear(att) + f, LayerNorm, out_proj.  x (M,), group_idx (M, K) rows of x -> (M, H)."""
    w = {k_: np.asarray(v_, F64) for k_, v_ in w.items()}
    x = np.asarray(x, F64)
    f = x[:, None] * w["w_in"][None, :] + w["b_in"]
    q, k, v = f @ w["wq"].T + w["bq"], f @ w["wk"].T + w["bk"], f @ w["wv"].T + w["bv"]
    att = attention_unfolded64(q, k, v, group_idx, ppf, w["wpe"], w["bpe"], w["wvpe"], w["bvpe"], heads)
    y = layer_norm64(att @ w["w_lin"].T + w["b_lin"] + f, w["norm_w"], w["norm_b"])
    return y @ w["w_out"].T + w["b_out"]


def first_layer_constants64(w, heads=4):
    """(head_consts (heads, 16), G (H, 32)) of RoitrLocalFirst (include/roitr_engine.h) in float64.  With q = x qa + qb, k = x ka + kb,
    v = x va + vb (qa = Wq w_in, qb = Wq b_in + bq, ...): per head c1 c2 c3 c4 = qa.ka qa.kb qb.ka qb.kb | P1 = Wpe_h^T qa_h | P0 = Wpe_h^T qb_h |
    d1 d0 = qa_h . bpe_h, qb_h . bpe_h | 0 0.  G: columns 0-3 S (W_lin restricted to head h times va_h), 4-19 pbar (W_lin_h Wvpe_h), 20 w_in,
    21 the constant b_lin + b_in + W_lin (vb + bvpe), the rest zero."""
    w = {k_: np.asarray(v_, F64) for k_, v_ in w.items()}
    H = w["w_in"].shape[0]
    c = H // heads
    qa, qb = w["wq"] @ w["w_in"], w["wq"] @ w["b_in"] + w["bq"]
    ka, kb = w["wk"] @ w["w_in"], w["wk"] @ w["b_in"] + w["bk"]
    va, vb = w["wv"] @ w["w_in"], w["wv"] @ w["b_in"] + w["bv"]
    hc = np.zeros((heads, 16), F64)
    G = np.zeros((H, 32), F64)
    for h in range(heads):
        s = slice(h * c, (h + 1) * c)
        hc[h, 0:4] = qa[s] @ ka[s], qa[s] @ kb[s], qb[s] @ ka[s], qb[s] @ kb[s]
        hc[h, 4:8] = w["wpe"][s].T @ qa[s]
        hc[h, 8:12] = w["wpe"][s].T @ qb[s]
        hc[h, 12:14] = qa[s] @ w["bpe"][s], qb[s] @ w["bpe"][s]
        G[:, h] = w["w_lin"][:, s] @ va[s]
        G[:, 4 + 4 * h:8 + 4 * h] = w["w_lin"][:, s] @ w["wvpe"][s]
    G[:, 20] = w["w_in"]
    G[:, 21] = w["b_lin"] + w["b_in"] + w["w_lin"] @ (vb + w["bvpe"])
    return hc, G


def first_layer_rank1_64(hc, G, w, x, group_idx, ppf, heads=4):
    """The rank-1 evaluation csrc/local_block.hip local_first_kernel performs, in float64, from head_consts and G."""
    hc, G, x, ppf = np.asarray(hc, F64), np.asarray(G, F64), np.asarray(x, F64), np.asarray(ppf, F64)
    M, K = group_idx.shape
    H = G.shape[0]
    xi, xj = x[:, None, None], x[group_idx][:, None, :]             # (M, 1, 1), (M, 1, K)
    c1, c2, c3, c4 = (hc[None, :, i, None] for i in range(4))       # (1, heads, 1)
    coef = xi * hc[None, :, 4:8] + hc[None, :, 8:12]                # (M, heads, 4): x_i P1 + P0
    s = xi * xj * c1 + xi * c2 + xj * c3 + c4 + np.einsum("mht,mkt->mhk", coef, ppf) + xi * hc[None, :, 12, None] + hc[None, :, 13, None]
    a = softmax64(s / np.sqrt(H // heads), 2)                         # (M, heads, K)
    g = np.zeros((M, 32), F64)
    g[:, :heads] = (a * xj).sum(2)
    g[:, 4:4 + 4 * heads] = np.einsum("mhk,mkt->mht", a, ppf).reshape(M, 4 * heads)
    g[:, 20], g[:, 21] = x, 1.0
    y = layer_norm64(g @ G.T, np.asarray(w["norm_w"], F64), np.asarray(w["norm_b"], F64))
    return y @ np.asarray(w["w_out"], F64).T + np.asarray(w["b_out"], F64)
