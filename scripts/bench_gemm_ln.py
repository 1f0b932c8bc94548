"""Per-shape table of the 256-wide Linear + LayerNorm layers: the two-launch form (roitr_gemm, then roitr_add_layernorm /
roitr_add_layernorm_interp) against the fused forms of roitr_gemm -- the 64 x 256 instantiation of the general kernel and the
32 x 256 kernel of csrc/gemm_ln256.hip -- at the row counts of the 512-pair forward, in the epilogue variants the engine uses.

Device events around each form, the forms alternated call by call in one process, median over --reps calls after --warmup; the
argument structures are built once, so a timed call is one (two) C calls.  Every form's result is compared with the two-launch bytes.

    python scripts/bench_gemm_ln.py [--reps 25] [--rows 19968,9984] [--out profiles/ln256_shapes.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roitr_amd import _lib as L  # noqa: E402
from roitr_amd import ops  # noqa: E402

N = 256
ROWS = (319488, 79872, 39936)      # levels 3 and 4 and the dec3 rows of 512 pairs of 5 000 points
KS = (256, 512, 384)               # 384: [A (256) | A_cat (128)]
VARIANTS = ("res", "res_idx", "post_relu", "a2", "interp")


def make(M, K, variant):
    g = torch.Generator().manual_seed(M % 1000 + K)
    kx = 256 if K == 384 else K
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).cuda()
    t = {"x": r(M, kx), "xc": r(M, K - kx) if K == 384 else None, "w": r(N, K) / K ** 0.5, "b": r(N), "gam": r(N), "bet": r(N),
         "tmp": torch.empty(M, N, device="cuda"), "out2": torch.empty(M, N, device="cuda"), "out": torch.empty(M, N, device="cuda")}
    if variant in ("res", "res_idx"):
        t["res"] = r(M, N)
    if variant == "res_idx":
        t["idx"] = torch.randint(0, M, (M,), generator=g).to(torch.int32).cuda()
    if variant == "post_relu":
        t["post"] = r(M, N)
    if variant == "a2":
        t["a2"] = r(M, kx)
    if variant == "interp":
        R = max(M // 4, 1)
        t["feat"] = r(R, N)
        t["ip_idx"] = torch.randint(0, R, (M, 3), generator=g).to(torch.int32).cuda()
        t["ip_d2"] = (torch.rand(M, 3, generator=g) + 0.01).cuda()
    return t


def gemm_struct(t, M, K, out, ln):
    p = lambda k: L.ptr(t.get(k))
    kx = t["x"].shape[1]
    g = ops._Gemm(M, N, K, p("x"), p("a2"), kx, L.ptr(None), 0, p("w"), K, L.ptr(None), 0, p("b"), 1.0, 0, L.ptr(out), N, 1, 0, 0, 0, 0, 0, 0,
                  L.ptr(None), 0, 0)
    if t["xc"] is not None:
        g.A_cat, g.lda_cat, g.k_cat = p("xc"), t["xc"].shape[1], kx
    if ln:
        g.ln_gamma, g.ln_beta, g.ln_res, g.ln_res_idx, g.ln_post = p("gam"), p("bet"), p("res"), p("idx"), p("post")
        g.ln_relu, g.ln_eps = int("post" in t or "feat" in t), 1e-5
        g.ip_feat, g.ip_idx, g.ip_dist2 = p("feat"), p("ip_idx"), p("ip_d2")
    return g


def forms(t, M, K):
    lib, st = L.lib(), L.stream_ptr()
    p = lambda k: L.ptr(t.get(k))
    relu = int("post" in t or "feat" in t)
    g_plain, g_ln = gemm_struct(t, M, K, t["tmp"], False), gemm_struct(t, M, K, t["out"], True)
    eps = ctypes.c_float(1e-5)

    def two():
        L.check(lib.roitr_gemm(ctypes.byref(g_plain), st), "gemm")
        if "feat" in t:
            L.check(lib.roitr_add_layernorm_interp(M, N, p("tmp"), p("res"), p("idx"), p("gam"), p("bet"), relu, eps, p("feat"), p("ip_idx"),
                                                   p("ip_d2"), p("out2"), st), "add_layernorm_interp")
        else:
            L.check(lib.roitr_add_layernorm(M, N, p("tmp"), p("res"), p("idx"), p("gam"), p("bet"), p("post"), relu, eps, p("out2"), st), "add_layernorm")

    def fused(rows):
        def run():
            lib.roitr_gemm_set_ln256_tile(rows)
            L.check(lib.roitr_gemm(ctypes.byref(g_ln), st), "gemm+layernorm")
        return run

    def gemm_only():
        L.check(lib.roitr_gemm(ctypes.byref(g_plain), st), "gemm")
    return {"two": two, "gemm": gemm_only, "f64": fused(64), "f32": fused(32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default=None, help="comma-separated row counts instead of those of the 512-pair forward (break-even search)")
    a = ap.parse_args()
    assert a.reps >= 20
    rows = tuple(int(r) for r in a.rows.split(",")) if a.rows else ROWS
    lines = ["256-wide Linear + LayerNorm, fp32, %s: microseconds per call, median of %d (events, forms alternated)." % (
                 torch.cuda.get_device_name(0), a.reps),
             "two = roitr_gemm + roitr_add_layernorm[_interp]; gemm = its first launch alone; 64x256 / 32x256 = the fused launch on that tile.",
             "", "%8s %4s %-9s %8s %8s %8s %8s   %s" % ("M", "K", "epilogue", "two", "gemm", "64x256", "32x256", "32x256 / two")]
    for M in rows:
        for K in KS:
            for variant in VARIANTS:
                t = make(M, K, variant)
                f = forms(t, M, K)
                f["two"]()
                for name in ("f64", "f32"):
                    f[name]()
                    torch.cuda.synchronize()
                    assert torch.equal(t["out"], t["out2"]), (M, K, variant, name)
                times = {k: [] for k in f}
                for it in range(a.warmup + a.reps):
                    for name, fn in f.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        if it >= a.warmup:
                            times[name].append(e0.elapsed_time(e1) * 1e3)
                med = {k: statistics.median(v) for k, v in times.items()}
                lines.append("%8d %4d %-9s %8.1f %8.1f %8.1f %8.1f   %.3f" % (M, K, variant, med["two"], med["gemm"], med["f64"], med["f32"],
                                                                              med["f32"] / med["two"]))
                print(lines[-1], flush=True)
                del t, f
    L.lib().roitr_gemm_set_ln256_tile(32)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
