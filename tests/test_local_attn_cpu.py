"""CPU: the float64 restatements of tests/local_attn_util.py against each other and against the reference-pinned oracle, before any
kernel is held to them (tests/test_local_attn_gpu.py, tests/test_local_first_gpu.py).

* the folded attention (scores from the 5 extra q columns per head, value term from pbar) is the unfolded function: 1e-12 of mean |ref|;
* the rank-1 form of the first layer, evaluated from first_layer_constants64 in the layout of RoitrLocalFirst, is the unfolded layer:
  1e-12 of mean |ref| (float64 rounding of sums of 64 terms is some 1e-15);
* attention_unfolded64 + linear / norm / out_proj is oracle/roitr_ref.py local_ppf_transformer (fp32, pinned to the reference by
  tests/test_oracle_cpu.py) within the project's fp32 feature bound of 1e-4."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import local_attn_util as U  # noqa: E402


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).mean())


@pytest.mark.parametrize("H,K,M", [(64, 8, 37), (64, 16, 37), (128, 16, 21), (256, 16, 9), (512, 16, 5)])
def test_folded_attention_from_the_extra_columns_is_the_unfolded_attention(H, K, M):
    rng = np.random.default_rng(H + K)
    N_in = 90
    q, k, v = rng.standard_normal((M, H)), rng.standard_normal((N_in, H)), rng.standard_normal((N_in, H))
    wpe, bpe, wvpe, bvpe = rng.standard_normal((H, 4)), rng.standard_normal(H), rng.standard_normal((H, 4)), rng.standard_normal(H)
    grp = rng.integers(0, N_in, (M, K))
    grp[3] = grp[3, 0]                                                # a node whose neighbours are all one row
    ppf = rng.random((M, K, 4)) * 3.0
    ref = U.attention_unfolded64(q, k, v, grp, ppf, wpe, bpe, wvpe, bvpe)
    qp = U.qp_columns64(q, wpe, bpe)
    assert qp.shape == (M, 20)
    err = _rel(U.attention_folded64(q, qp, k, v, grp, ppf, wvpe, bvpe), ref)
    print(f"folded vs unfolded attention H={H} K={K}: {err:.2e}")
    assert err < 1e-12, err
    # softmax rows sum to one: a constant added to every score of a head (the q_h . bpe_h column) cannot change the result
    qp2 = qp.copy()
    qp2[:, 4::5] += 3.0
    assert _rel(U.attention_folded64(q, qp2, k, v, grp, ppf, wvpe, bvpe), ref) < 1e-12


@pytest.mark.parametrize("K,M", [(8, 70), (16, 70)])
def test_rank_one_first_layer_constants_give_the_unfolded_layer(K, M):
    rng = np.random.default_rng(K)
    w = U.first_layer_weights(rng)
    x = rng.standard_normal(M)
    grp = rng.integers(0, M, (M, K))
    ppf = rng.random((M, K, 4)) * 3.0
    hc, G = U.first_layer_constants64(w)
    assert hc.shape == (4, 16) and G.shape == (64, 32)
    assert not hc[:, 14:].any() and not G[:, 22:].any() and G[:, :22].all()
    ref = U.first_layer_unfolded64(w, x, grp, ppf)
    err = _rel(U.first_layer_rank1_64(hc, G, w, x, grp, ppf), ref)
    print(f"rank-1 first layer vs unfolded K={K}: {err:.2e}")
    assert err < 1e-12, err


@pytest.mark.parametrize("H,I,K,M,N_in", [(64, 1, 8, 50, 50), (64, 64, 16, 50, 50), (128, 64, 16, 23, 92)])
def test_unfolded_attention_is_the_oracles_local_transformer(H, I, K, M, N_in):
    from oracle import roitr_ref as R  # checker only
    rng = np.random.default_rng(H + I + K)
    f32 = np.float32
    pre = "layer"
    at = pre + ".transformer.attention"
    sd = {}

    def lin(name, n_out, n_in):
        sd[name + ".weight"] = (rng.standard_normal((n_out, n_in)) / np.sqrt(n_in)).astype(f32)
        sd[name + ".bias"] = (0.5 * rng.standard_normal(n_out)).astype(f32)
    lin(pre + ".embedding.proj", H, 4)
    lin(pre + ".in_proj", H, I)
    for name in ("proj_q", "proj_k", "proj_v", "proj_p", "proj_vp"):
        lin(at + "." + name, H, H)
    lin(pre + ".transformer.linear", H, H)
    lin(pre + ".out_proj", H, H)
    sd[pre + ".transformer.norm.weight"] = (1 + 0.1 * rng.standard_normal(H)).astype(f32)
    sd[pre + ".transformer.norm.bias"] = (0.1 * rng.standard_normal(H)).astype(f32)
    feats = rng.standard_normal((N_in, I)).astype(f32)
    node_idx = np.arange(M) if M == N_in else rng.integers(0, N_in, M)
    grp = rng.integers(0, N_in, (M, K))
    ppf = (rng.random((M, K, 4)) * 3.0).astype(f32)
    want = R.local_ppf_transformer(R.Weights(sd), pre, feats, node_idx, grp, ppf)

    D = {k_: v_.astype(np.float64) for k_, v_ in sd.items()}
    W, B = (lambda n: D[n + ".weight"]), (lambda n: D[n + ".bias"])
    f = feats.astype(np.float64) @ W(pre + ".in_proj").T + B(pre + ".in_proj")
    q, k, v = (f @ W(at + n).T + B(at + n) for n in (".proj_q", ".proj_k", ".proj_v"))
    we, be = W(pre + ".embedding.proj"), B(pre + ".embedding.proj")            # no nonlinearity between the embedding and proj_p / proj_vp
    wpe, bpe = W(at + ".proj_p") @ we, W(at + ".proj_p") @ be + B(at + ".proj_p")
    wvpe, bvpe = W(at + ".proj_vp") @ we, W(at + ".proj_vp") @ be + B(at + ".proj_vp")
    att = U.attention_unfolded64(q[node_idx], k, v, grp, ppf, wpe, bpe, wvpe, bvpe)
    hid = att @ W(pre + ".transformer.linear").T + B(pre + ".transformer.linear")
    y = U.layer_norm64(hid + f[node_idx], D[pre + ".transformer.norm.weight"], D[pre + ".transformer.norm.bias"])
    got = y @ W(pre + ".out_proj").T + B(pre + ".out_proj")
    abs_err = float(np.abs(got - want).max())
    rel_err = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
    print(f"float64 restatement vs fp32 oracle H={H} in={I} K={K}: abs {abs_err:.2e} rel {rel_err:.2e}, max |oracle| {np.abs(want).max():.2f}")
    assert want.shape == (M, H) and np.abs(want).max() > 0.5
    assert abs_err < 1e-4 and rel_err < 1e-4, (abs_err, rel_err)
