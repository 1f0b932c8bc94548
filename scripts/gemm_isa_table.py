"""Generated-code table of a set of kernel sources, for A/B reading of a refactor: compiles the named files of csrc/ (default: the GEMM
family, gemm.hip, gemm_bf16.hip and gemm_x3.hip) of two source trees to gfx950 assembly (device side only, the flags of
roitr_amd/build.py) and prints, per kernel instantiation, registers, LDS, scratch, instruction counts by class and whether the K loop
(the backward-branch loop with the most MFMAs; empty for a kernel without MFMAs) is the same instruction sequence up to register
renaming.  No GPU needed.

    python scripts/gemm_isa_table.py PARENT_TREE BRANCH_TREE [FILE.hip ...] > profiles/<name>_isa.txt
"""
import os
import re
import subprocess
import sys
import tempfile

FILES = ("gemm.hip", "gemm_bf16.hip", "gemm_x3.hip")
CLASSES = (("mfma", r"v_mfma"), ("gload", r"global_load"), ("gstore", r"global_store"), ("ds_rd", r"ds_(read|load)"),
           ("ds_wr", r"ds_(write|store)"), ("barrier", r"s_barrier"), ("waitcnt", r"s_waitcnt"))
META = (("vgpr", r"; NumVgprs: (\d+)"), ("agpr", r"; NumAgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"),
        ("scratch", r"; ScratchSize: (\d+)"))


def assembly(tree, name, tmp):
    csrc = os.path.join(tree, "roitr_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-fno-slp-vectorize", "-Wall", "-Wno-unused-function",
             "-I", csrc, "-I", os.path.join(tree, "include")]
    out = os.path.join(tmp, name + ".s")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["-x", "hip", "--cuda-device-only", "-S",
                          os.path.join(csrc, name), "-o", out])
    return open(out).read()


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    short = [re.sub(r"\(anonymous namespace\)::|\([^()]*(\([^()]*\)[^()]*)*\)$|^void ", "", s) for s in r.stdout.split("\n")]   # no argument list
    return dict(zip(names, short))


def kernels(text):
    """name -> dict of figures and the normalised K loop"""
    out = {}
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"^(\w+):\s*; @\1\n", text, re.M)]
    for n, (pos, name) in enumerate(starts):
        chunk = text[pos:starts[n + 1][0] if n + 1 < len(starts) else len(text)]
        if ".amdhsa_kernel " + name not in chunk:
            continue   # a device function, not a kernel
        body, tail = chunk.split(".Lfunc_end", 1)
        body = body.split("\n", 1)[1]
        lines = [re.sub(r"\s*;.*", "", l).strip() for l in body.split("\n")]
        insts = [l for l in lines if l and not l.startswith((".", ";")) and not l.endswith(":")]
        k = {"insts": len(insts)}
        for key, pat in CLASSES:
            k[key] = sum(1 for l in insts if re.match(pat, l))
        for key, pat in META:
            mm = re.search(pat, tail)
            k[key] = int(mm.group(1)) if mm else -1
        # loops: a branch to a label that was defined earlier
        seen, best = {}, []
        code = [l for l in lines if l and not l.startswith(";") and not (l.startswith(".") and not l.endswith(":"))]
        for i, l in enumerate(code):
            if l.endswith(":"):
                seen[l[:-1]] = i
            mm = re.match(r"s_cbranch_\w+ (\S+)", l) or re.match(r"s_branch (\S+)", l)
            if mm and mm.group(1) in seen:
                loop = [x for x in code[seen[mm.group(1)]:i + 1] if not x.endswith(":")]
                if sum("v_mfma" in x for x in loop) > sum("v_mfma" in x for x in best):
                    best = loop
        norm = lambda s: re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", lambda r: r.group(1) + ("#" if r.group(2)[0] != "[" else "[%d]" % (
            1 + int(r.group(2)[1:-1].split(":")[1]) - int(r.group(2)[1:-1].split(":")[0]))), re.sub(r"\s*;.*", "", s))
        k["loop"] = [re.sub(r"\.LBB\d+_\d+", ".L", norm(x)) for x in best]
        out[name] = k
    return out


def main():
    parent, branch, files = sys.argv[1], sys.argv[2], tuple(sys.argv[3:]) or FILES
    cols = ["vgpr", "agpr", "sgpr", "lds", "scratch"] + [c for c, _ in CLASSES] + ["insts"]
    must = cols
    print("%s: gfx950 device code of the parent and of this tree (hipcc -S --cuda-device-only, the flags of roitr_amd/build.py)." % ", ".join(files))
    print("Per kernel: parent -> branch where a figure differs.  kloop: the backward-branch loop with the most MFMAs, compared as an")
    print("instruction sequence with register numbers erased.  `required` = registers, LDS, scratch and every instruction count.\n")
    verdict = True
    with tempfile.TemporaryDirectory() as tmp:
        for f in files:
            os.makedirs(os.path.join(tmp, "p"), exist_ok=True)
            os.makedirs(os.path.join(tmp, "b"), exist_ok=True)
            kp, kb = kernels(assembly(parent, f, os.path.join(tmp, "p"))), kernels(assembly(branch, f, os.path.join(tmp, "b")))
            names = demangle(sorted(set(kp) | set(kb)))
            kp = {names[n]: v for n, v in kp.items()}
            kb = {names[n]: v for n, v in kb.items()}
            names = {n: n for n in list(kp) + list(kb)}
            print("== %s: %d kernels in the parent, %d in this tree" % (f, len(kp), len(kb)))
            figures = lambda k: "  ".join("%s %s" % (c, k[c]) for c in cols)   # of a kernel without a namesake: a renamed or merged one is read against these
            for n in sorted(set(kp) - set(kb)):
                print("  only in the parent: %s\n      %s" % (names[n], figures(kp[n])))
            for n in sorted(set(kb) - set(kp)):
                print("  only in this tree:  %s\n      %s" % (names[n], figures(kb[n])))
                verdict = False
            for n in sorted(set(kp) & set(kb), key=lambda x: names[x]):
                a, b = kp[n], kb[n]
                same_loop = a["loop"] == b["loop"]
                req = all(a[c] == b[c] for c in must)
                verdict = verdict and req and same_loop
                cells = ["%s %s" % (c, a[c]) if a[c] == b[c] else "%s %s -> %s" % (c, a[c], b[c]) for c in cols]
                print("  %s\n      %s\n      required %s; kloop (%d instructions, %d MFMAs) %s" % (
                    names[n], "  ".join(cells), "identical" if req else "DIFFERENT", len(a["loop"]), sum("v_mfma" in x for x in a["loop"]),
                    "identical" if same_loop else "DIFFERENT (%d instructions in this tree)" % len(b["loop"])))
            print()
    print("verdict: every kernel present on both sides keeps its required figures and its K loop: %s" % verdict)


if __name__ == "__main__":
    main()
