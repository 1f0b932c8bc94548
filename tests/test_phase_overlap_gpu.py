"""The global transformer and the coarse front of the matching phase run on a stream of the engine's own beside the decoder
(roitr_engine_set_phase_overlap; by default for calls of a few thousand superpoints and more, below that on the main stream; the tests
ask for it at every size with mode 2, so that the small shapes take the three-stream path too), in a scratch region of their own.  No kernel, operand or launch parameter differs
from the single-stream order, so every output and every tapped stage must be the same bytes with the overlap on and off, from run to
run, across calls of different sizes on one engine, through the graph path and with two calls in flight."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TAPS = ("geo.out", "geo.layer5", "dec4.1", "dec1.1")


_MODELS = {}


def _model(benchmark, dtype="f32"):
    """One engine per (benchmark, operand dtype) for the whole module: building one costs more than any of the calls below."""
    from tests.gpu_util import build_model
    if (benchmark, dtype) not in _MODELS:
        _MODELS[(benchmark, dtype)] = build_model(benchmark, operand_dtype=dtype, weights="selective")
    return _MODELS[(benchmark, dtype)]


def _pairs(sizes, config, first_index=0):
    from roitr_amd.synthetic import make_pair
    from tests.gpu_util import pair_to_device
    out = []
    for i, s in enumerate(sizes):
        n_src, n_tgt = s if isinstance(s, tuple) else (s, s)
        out.append(pair_to_device(make_pair(n_src, n_tgt, config=config, pair_index=first_index + i, normals="field")))
    torch.cuda.synchronize()
    return out


def _assert_same(got, ref, what):
    """Every array of every pair's output dict, by bytes."""
    assert len(got) == len(ref), what
    for j, (a, b) in enumerate(zip(got, ref)):
        assert set(a.keys()) == set(b.keys()), (what, j)
        for k in a.keys():
            x, y = a[k], b[k]
            if x is None or y is None:
                assert x is None and y is None, (what, j, k)
                continue
            assert x.shape == y.shape, (what, j, k, tuple(x.shape), tuple(y.shape))
            assert torch.equal(x, y), (what, j, k)


def _run(model, pairs, overlap, taps=True):
    """One forward_batch with the overlap on / off; returns (outputs, {tap: copy})."""
    f = model.factor
    n1 = sum(int(p["src_pcd"].shape[0]) + int(p["tgt_pcd"].shape[0]) for p in pairs)
    n4 = sum(int(p["src_pcd"].shape[0]) // 64 + int(p["tgt_pcd"].shape[0]) // 64 for p in pairs)
    bufs = {}
    if taps:
        shapes = {"geo.out": (n4, 256 * f), "geo.layer5": (n4, 256 * f), "dec4.1": (n4, 256 * f), "dec1.1": (n1, 64 * f)}
        for name in TAPS:
            bufs[name] = torch.full(shapes[name], float("nan"), device="cuda")
            model.set_tap(name, bufs[name])
    model.set_phase_overlap(2 if overlap else 0)
    try:
        with torch.no_grad():
            res = model.forward_batch(pairs)
        torch.cuda.synchronize()
    finally:
        model.set_phase_overlap(1)
        for name in bufs:
            model.set_tap(name, None)
    for name, t in bufs.items():
        assert not torch.isnan(t).any(), name     # the tap was written
    return res, bufs


def _assert_taps_same(a, b, what):
    for name in TAPS:
        assert torch.equal(a[name], b[name]), (what, name)


CASES = {
    # (a) ragged clouds, the coarser levels below the grid threshold
    "3dmatch_ragged": ("3DMatch", "f32", [(700, 1100), (1500, 900), (1300, 760)], 2),
    # (b) long enough for the two chains to run side by side for several milliseconds
    "3dmatch_16x5000": ("3DMatch", "f32", [5000] * 16, 2),
    # (c) factor 2, adaptive coarse matching, compacted patch list
    "4dmatch_f32": ("4DMatch", "f32", [2000, 2000], 4),
    "4dmatch_bf16": ("4DMatch", "bf16", [2000, 2000], 4),
}
REPEATS = {"3dmatch_ragged": 1, "3dmatch_16x5000": 3, "4dmatch_f32": 2, "4dmatch_bf16": 2}


@pytest.mark.parametrize("case", sorted(CASES))
def test_overlap_on_equals_overlap_off_and_itself(case):
    """Same bytes, on against off; and the overlapped call repeated: identical from run to run (a race between the branch and the
    decoder -- shared scratch, a missing join -- shows as a difference in some run)."""
    benchmark, dtype, sizes, config = CASES[case]
    model = _model(benchmark, dtype)
    pairs = _pairs(sizes, config)
    off, taps_off = _run(model, pairs, overlap=False)
    assert sum(int(r["corr_scores"].shape[0]) for r in off) > 0      # the matching tail had real patches to work on
    for rep in range(REPEATS[case]):
        on, taps_on = _run(model, pairs, overlap=True)
        _assert_same(on, off, f"{case}: overlap on (run {rep}) vs off")
        _assert_taps_same(taps_on, taps_off, f"{case}: run {rep}")


def test_scratch_reuse_large_small_large():
    """A large call, a small one and the large one again on ONE FRESH engine: the first call sizes the branch region and the main arena,
    the small call reuses them, the second large call fits them exactly.  Against the same calls on engines of their own."""
    from tests.gpu_util import build_model
    large = _pairs([4000, 5000, 3000, 5000], 2, first_index=20)
    small = _pairs([(700, 1100)], 2, first_index=30)
    model = build_model("3DMatch", weights="selective")
    model.set_phase_overlap(2)
    with torch.no_grad():
        got = [model.forward_batch(large), model.forward_batch(small), model.forward_batch(large)]
        torch.cuda.synchronize()
        ref_large = build_model("3DMatch", weights="selective").forward_batch(large)
        ref_small = build_model("3DMatch", weights="selective").forward_batch(small)
        torch.cuda.synchronize()
    _assert_same(got[0], ref_large, "large, first")
    _assert_same(got[1], ref_small, "small after large")
    _assert_same(got[2], ref_large, "large after small")


def test_graph_path_captures_the_fork_and_returns_the_same_bytes():
    from tests.gpu_util import build_model
    model = build_model("3DMatch", weights="selective")   # (an engine that ever had a tap set stays on the plain path)
    model.set_phase_overlap(2)
    pairs = _pairs([1500, 1024], 2, first_index=40)
    with torch.no_grad():
        ref = model.forward_batch(pairs)
        torch.cuda.synchronize()
        before = model.graph_count()
        for call in range(8):                      # three io buffer sets per shape: each is warmed up, then captured, then replayed
            got = model.forward_batch(pairs, graph=True)
            _assert_same(got, ref, f"graph call {call}")
    assert model.graph_count() > before            # the three-stream forward was captured, not left on the plain path


def test_two_calls_in_flight_with_resident_inputs():
    """What the benchmark loop does: the next call is queued (inputs handed over by event) while this one runs, so its geometry
    chain, and then its branch, follow this call's on the engine's streams."""
    model = _model("3DMatch")
    first = _pairs([5000, 4000, 3000, 5000, 2048, 4500], 2, first_index=50)
    second = _pairs([1024, 1500], 2, first_index=60)
    with torch.no_grad():
        ref_first, ref_second = model.forward_batch(first), model.forward_batch(second)
        torch.cuda.synchronize()
        model.set_phase_overlap(2)
        try:
            for order in ((first, second), (second, first), (first, first)):
                hs = [model.launch_batch(b, inputs_resident=True) for b in order]
                got = [model.finish_batch(h) for h in hs]
                for g, b in zip(got, order):
                    _assert_same(g, ref_first if b is first else ref_second, "two calls in flight")
        finally:
            model.set_phase_overlap(1)


def test_default_mode_picks_the_stream_by_size_and_changes_no_byte():
    """Mode 1 (the default) at the threshold: 256 pairs of 1 024 points are exactly 8 192 superpoints and go to the branch stream, 255 pairs
    stay on the main stream; both equal mode 0.  The main arena's bound holds with room (its fill is a diagnostic of the engine)."""
    base = _pairs([1024] * 8, 2, first_index=70)
    model = _model("3DMatch")
    for n_pairs, on_branch in ((256, True), (255, False)):
        pairs = [base[i % 8] for i in range(n_pairs)]
        with torch.no_grad():
            model.set_phase_overlap(0)
            off = model.forward_batch(pairs)
            torch.cuda.synchronize()
            assert not model.scratch_info()["on_branch_stream"]
            model.set_phase_overlap(1)
            got = model.forward_batch(pairs)
            torch.cuda.synchronize()
        info = model.scratch_info()
        assert info["on_branch_stream"] == on_branch, (n_pairs, info)
        assert 0 < info["main_peak"] <= info["main_cap"] and 0 < info["branch_fill"] <= info["branch_cap"], info
        _assert_same(got, off, f"default mode, {n_pairs} pairs")
