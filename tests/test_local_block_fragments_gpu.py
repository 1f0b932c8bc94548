"""GPU: the fragment path of the fused local-transformer kernels (csrc/local_block.hip) against their row-major path.

A launch whose weights all have a fragment-ordered copy (roitr_local_weights_prepare) reads the copies; the arithmetic is the same
operation for operation, so the outputs are the same bits.  Every case runs one operator call with nothing prepared, with the weights
prepared, and with them released again.  Equal bits alone would also hold if the prepared launch quietly stayed on the row-major
path, so each case shows which path ran: with the ORIGINAL weights zeroed in place, a launch on the fragment path still returns
the old result (it reads the copies), a launch on the row-major path does not."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _rand(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return g, (lambda *s: torch.randn(s, device="cuda", generator=g) / (s[-1] ** 0.5))


def _block_case(H, K, M, seed):
    from roitr_amd import ops
    g, r = _rand(seed)
    x = torch.randn((M, H), device="cuda", generator=g)
    kv = torch.randn((M, 2 * H), device="cuda", generator=g)
    grp = torch.randint(0, M, (M, K), device="cuda", generator=g).to(torch.int32)
    ppf = torch.rand((M, K, 4), device="cuda", generator=g)
    w = dict(wq=r(H, H), bq=r(H), wpe=r(H, 4), bpe=r(H), wvpe=r(H, 4), bvpe=r(H), wcat=r(H, 2 * H), bcat=r(H), norm_w=1 + 0.1 * r(H),
             norm_b=0.1 * r(H), wout=r(H, H), bout=r(H), bn2_w=1 + 0.1 * r(H), bn2_b=0.1 * r(H))
    return (lambda: ops.local_block(x, kv, grp, ppf, w)), w, ("wq", "wcat", "wout")


def _td_case(M, N_in, seed):
    from roitr_amd import ops
    I, H = 64, 128
    g, r = _rand(seed)
    x = torch.randn((N_in, I), device="cuda", generator=g)
    node_idx = torch.randint(0, N_in, (M,), device="cuda", generator=g).to(torch.int32)
    grp = torch.randint(0, N_in, (M, 16), device="cuda", generator=g).to(torch.int32)
    ppf = torch.rand((M, 16, 4), device="cuda", generator=g) * 3.0
    w = dict(wqqt=r(H + 4 * I, I), bqqt=r(H + 4 * I), wv=r(H, I), bv=r(H), wpe=r(H, 4), wvpe=r(H, 4), bvpe=r(H), wcat=r(H, H + I), bcat=r(H),
             norm_w=1 + 0.1 * r(H), norm_b=0.1 * r(H), wout=r(H, H), bout=r(H))
    return (lambda: ops.local_td(x, node_idx, grp, ppf, w)), w, ("wqqt", "wv", "wcat", "wout")


def _first_case(K, M, seed):
    from roitr_amd import ops
    g, r = _rand(seed)
    x = torch.randn((M,), device="cuda", generator=g)
    grp = torch.randint(0, M, (M, K), device="cuda", generator=g).to(torch.int32)
    ppf = torch.rand((M, K, 4), device="cuda", generator=g) * 3.0
    G = r(64, 32)
    G[:, 22:] = 0.0                                              # the columns behind [S | pbar | x | 1] are padding
    w = dict(head_consts=r(64), G=G, zero_bias=torch.zeros(64, device="cuda"), norm_w=1 + 0.1 * r(64), norm_b=0.1 * r(64), wout=r(64, 64),
             bout=r(64))
    return (lambda: ops.local_first(x, grp, ppf, w)), w, ("wout",)


CASES = {
    "block H=64 K=8 M=70": lambda: _block_case(64, 8, 70, 1),                   # one full 64-row tile and a ragged one
    "block H=128 K=16 M=40": lambda: _block_case(128, 16, 40, 2),               # 32-row tiles, the second ragged
    "block H=128 K=16 M=65544": lambda: _block_case(128, 16, 65536 + 8, 3),     # the 64-row-tile instantiation (>= 1024 such tiles)
    "td I=64 H=128 K=16 M=40": lambda: _td_case(40, 160, 4),
    "first K=8 M=70": lambda: _first_case(8, 70, 5),
}


def _zeroed(w, names):
    """Context: the named weights zeroed in place (same storage, same addresses), restored on exit."""
    class Z:
        def __enter__(self):
            self.saved = {k: w[k].clone() for k in names}
            for k in names:
                w[k].zero_()

        def __exit__(self, *exc):
            for k in names:
                w[k].copy_(self.saved[k])
    return Z()


@pytest.mark.parametrize("case", list(CASES))
def test_fragment_path_gives_the_bits_of_the_row_major_path(case):
    from roitr_amd import ops
    run, w, names = CASES[case]()
    count0 = ops.local_weights_count()
    plain = run()
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0.1
    try:
        for k in names:
            ops.local_weights_prepare(w[k])
        assert ops.local_weights_count() == count0 + len(names)
        prepared = run()
        assert torch.equal(prepared, plain)
        with _zeroed(w, names):
            assert torch.equal(run(), plain), "the prepared launch did not read the fragment-ordered copies"
    finally:
        for k in names:
            ops.local_weights_release(w[k])
    assert ops.local_weights_count() == count0
    released = run()
    assert torch.equal(released, plain)


def test_after_release_a_launch_reads_the_row_major_weights_again():
    from roitr_amd import ops
    run, w, names = _block_case(64, 8, 70, 6)
    plain = run()
    for k in names:
        ops.local_weights_prepare(w[k])
    try:
        assert torch.equal(run(), plain)
    finally:
        for k in names:
            ops.local_weights_release(w[k])
    assert torch.equal(run(), plain)
    with _zeroed(w, names):
        assert not torch.equal(run(), plain), "a launch after release still read a copy"
    assert torch.equal(run(), plain)


def test_one_missing_weight_keeps_the_launch_on_the_row_major_path():
    from roitr_amd import ops
    run, w, names = _block_case(128, 16, 40, 7)
    plain = run()
    try:
        for k in names[:-1]:
            ops.local_weights_prepare(w[k])
        assert torch.equal(run(), plain)
        with _zeroed(w, names):
            assert not torch.equal(run(), plain)
    finally:
        for k in names:
            ops.local_weights_release(w[k])                      # releasing what was never prepared is a no-op


def test_preparing_the_same_weight_twice_keeps_one_copy_and_refreshes_it():
    from roitr_amd import ops
    run, w, names = _block_case(64, 8, 70, 8)
    count0 = ops.local_weights_count()
    try:
        for _ in range(2):
            for k in names:
                ops.local_weights_prepare(w[k])
        assert ops.local_weights_count() == count0 + len(names)
        first = run()
        # a weight changed in place: preparing it again rewrites the copy it has
        w["wout"].mul_(0.5)
        ops.local_weights_prepare(w["wout"])
        assert ops.local_weights_count() == count0 + len(names)
        changed = run()
        assert not torch.equal(changed, first)
    finally:
        for k in names:
            ops.local_weights_release(w[k])
    assert ops.local_weights_count() == count0
    assert torch.equal(run(), changed)                           # the row-major path over the changed weight


def test_prepare_rejects_views_that_are_not_whole_blocks():
    from roitr_amd import _lib, ops
    count0 = ops.local_weights_count()
    for shape in ((48, 64), (64, 40)):
        with pytest.raises(_lib.RoitrError):
            ops.local_weights_prepare(torch.zeros(shape, device="cuda"))
    assert ops.local_weights_count() == count0
