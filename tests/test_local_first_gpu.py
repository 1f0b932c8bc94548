"""GPU: roitr_local_first (csrc/local_block.hip local_first_kernel, the rank-1 form of the first local transformer) against the UNFOLDED
layer in float64 (tests/local_attn_util.py first_layer_unfolded64: f = x w_in + b_in, q / k / v / p / vp, attention, linear(att) + f,
LayerNorm, out_proj).  The constants come from first_layer_constants64 (held to the unfolded layer at 1e-12 by tests/test_local_attn_cpu.py),
rounded to fp32 as the engine stores them.  The kernel's tile is 64 nodes: M in {1, 63, 64, 65, 200}, K in {8, 16}.

Bound: max |got - ref| / mean |ref| < 5e-5, the bound local_td is held to against its unfolded float64 layer.  A permuted visiting order
gives the same bits; rows past M keep their sentinel.

Measured on an MI355X: 4.7e-7 ... 1.6e-6 over the ten cases (largest: K = 8, M = 64), some 30 x below the bound -- the __expf of the kernel's
softmax (its siblings use expf) costs nothing that this metric sees."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import local_attn_util as U  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12288.0


def _guarded(x, grp, ppf, w, node_order=None):
    """The call into an output of M + 3 rows prefilled with a sentinel."""
    from roitr_amd import ops
    out = torch.full((int(x.shape[0]) + 3, 64), SENTINEL, dtype=torch.float32, device="cuda")
    return ops.local_first(x, grp, ppf, w, node_order=node_order, out=out)


@pytest.mark.parametrize("K", [8, 16])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 200])
def test_local_first_against_the_unfolded_layer(M, K):
    from roitr_amd import ops
    rng = np.random.default_rng(100 * K + M)
    w = U.first_layer_weights(rng)
    x = rng.standard_normal(M).astype(np.float32)
    grp = rng.integers(0, M, (M, K)).astype(np.int32)
    ppf = (rng.random((M, K, 4)) * 3.0).astype(np.float32)
    hc, G = U.first_layer_constants64(w)
    ref = U.first_layer_unfolded64(w, x, grp, ppf)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    wd = dict(head_consts=dev(hc.astype(np.float32).reshape(64)), G=dev(G.astype(np.float32)), zero_bias=torch.zeros(64, device="cuda"),
              norm_w=dev(w["norm_w"].astype(np.float32)), norm_b=dev(w["norm_b"].astype(np.float32)), wout=dev(w["w_out"].astype(np.float32)),
              bout=dev(w["b_out"].astype(np.float32)))
    xd, gd, pd = dev(x), dev(grp), dev(ppf)
    got = ops.local_first(xd, gd, pd, wd)
    err = float(np.abs(got.double().cpu().numpy() - ref).max() / np.abs(ref).mean())
    print(f"local_first K={K} M={M}: max|d|/mean|ref| = {err:.3e} (bound 5e-05)")
    assert bool(torch.isfinite(got).all()) and err < 5e-5, err
    # the rows past M keep their sentinel; the rows before are the bits of the operator call
    guarded = _guarded(xd, gd, pd, wd)
    assert torch.equal(guarded[:M].view(torch.int32), got.view(torch.int32))
    assert torch.equal(guarded[M:].view(torch.int32), torch.full((3, 64), SENTINEL, device="cuda").view(torch.int32)), "a dead slot stored"
    # a permuted visiting order (float4 with the node index as bits in .w): same bits
    perm = rng.permutation(M).astype(np.int32)
    order = np.zeros((M, 4), np.float32)
    order[:, 3] = perm.view(np.float32)
    ordered = _guarded(xd, gd, pd, wd, node_order=dev(order))
    assert torch.equal(ordered.view(torch.int32), guarded.view(torch.int32)), "the visiting order changed a result"
