"""CPU: no inline-asm DPP instruction reads a VGPR that a VALU instruction wrote fewer than 2 wait states before.

On CDNA a DPP instruction that reads a VGPR written by the VALU op right before it needs 2 wait states in between (the ISA
guide's "VALU writes VGPR -> VALU DPP reads that VGPR").  The compiler's hazard recognizer inserts them for the DPP operations it
emits itself, but the assembler does not look inside an asm string, and the compiler does not look at what an asm string
contains: a kernel that writes DPP instructions by hand has to keep that distance itself, whatever registers and order the
compiler picks for the code around it.  This test compiles every source under csrc/ that holds inline-asm DPP with the build's
flags to gfx950 assembly and walks each function in text order (every instruction is one wait state, `s_nop n` is n + 1).
DPP instructions the compiler emitted are checked too: they must pass by construction.  Branches are not followed, so a write in
a predecessor block that is not the textual one is not seen.
"""
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from roitr_amd import build as B  # noqa: E402

NEED = 2   # wait states between a VALU VGPR write and a DPP read of it
_DPP_WORDS = re.compile(r"_dpp\b|row_shr|row_shl|row_ror|row_rol|row_bcast|row_mirror|row_half_mirror|quad_perm|wave_sh|wave_ro")
_STRING = re.compile(r'"(?:[^"\\\n]|\\.)*"')
_VREG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def dpp_asm_sources():
    """csrc files with an asm statement and a string literal that names a DPP control or a *_dpp instruction."""
    out = []
    for f in sorted(glob.glob(os.path.join(B.CSRC, "*.hip"))):
        text = open(f).read()
        if re.search(r"\basm\b", text) and any(_DPP_WORDS.search(s) for s in _STRING.findall(text)):
            out.append(f)
    return out


def _vregs(operand_text):
    regs = set()
    for m in _VREG.finditer(operand_text):
        if m.group(1) is not None:
            regs.add(int(m.group(1)))
        else:
            regs.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return regs


def _split(line):
    """(mnemonic, [operands]) of an instruction line, or None for labels, directives and comments."""
    s = line.split(";", 1)[0].strip()
    if not s or s.startswith(".") or s.endswith(":"):
        return None
    parts = s.split(None, 1)
    ops = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []
    return parts[0], ops


def dpp_hazards(asm_text):
    """[(function, line number, DPP instruction, writer, wait states)] for every DPP read of a VGPR that a v_* instruction wrote
    fewer than NEED wait states before, walking each function in text order."""
    found = []
    func = None
    recent = []   # (wait states since, written VGPRs, text, line) of the last few instructions, newest last
    for no, line in enumerate(asm_text.splitlines(), 1):
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", line)
        if m and not m.group(1).startswith(".L"):
            func, recent = m.group(1), []
            continue
        ins = _split(line)
        if ins is None:
            continue
        mn, ops = ins
        if func is None:
            continue
        is_dpp = mn.endswith("_dpp") or any(_DPP_WORDS.search(o) for o in ops[1:])
        if is_dpp:
            reads = set()
            for o in ops:   # every operand: the destination of a DPP op is read too (fmac accumulator, old value of masked lanes)
                if _DPP_WORDS.search(o) or o.startswith(("row_mask", "bank_mask", "bound_ctrl")):
                    continue
                reads |= _vregs(o)
            for ws, wr, txt, wno in recent:
                if ws < NEED and wr & reads:
                    found.append((func, no, line.strip(), f"{wno}: {txt}", ws))
        cost = int(ops[0], 0) + 1 if mn == "s_nop" else 1
        recent = [(ws + cost, wr, txt, wno) for ws, wr, txt, wno in recent if ws + cost < NEED]
        if mn.startswith("v_") and ops:
            wr = _vregs(ops[0])
            if wr:
                recent.append((0, wr, line.strip(), no))
    return found


def test_checker_sees_the_hazard():
    """The walker itself: a write right before the DPP read is flagged, s_nop 1 or two other instructions in between clear it,
    s_nop 0 does not, and register ranges count."""
    bad = "k:\n\tv_mov_b32_e32 v150, 0\n\tv_fmac_f32_dpp v150, v145, v10 row_ror:1 row_mask:0xf bank_mask:0xf\n"
    assert len(dpp_hazards(bad)) == 1
    assert dpp_hazards(bad.replace("\tv_fmac", "\ts_nop 1\n\tv_fmac")) == []
    assert len(dpp_hazards(bad.replace("\tv_fmac", "\ts_nop 0\n\tv_fmac"))) == 1
    assert len(dpp_hazards(bad.replace("\tv_fmac", "\ts_mov_b32 s0, 0\n\tv_fmac"))) == 1
    assert dpp_hazards(bad.replace("\tv_fmac", "\ts_mov_b32 s0, 0\n\ts_mov_b32 s1, 0\n\tv_fmac")) == []
    src = "k:\n\tv_lshlrev_b64 v[10:11], 2, v[4:5]\n\tv_max_f32_dpp v0, v11, v0 row_shr:1 row_mask:0xf bank_mask:0xf\n"
    assert len(dpp_hazards(src)) == 1
    assert dpp_hazards(src.replace("v[10:11]", "v[12:13]")) == []


def test_inline_asm_dpp_has_its_wait_states(tmp_path):
    hipcc = B.HIPCC if os.path.exists(B.HIPCC) else shutil.which("hipcc")
    if not hipcc or not os.path.exists(hipcc):
        pytest.skip("hipcc not found: the check needs the gfx950 device assembly")
    srcs = dpp_asm_sources()
    assert any(os.path.basename(s) == "matching.hip" for s in srcs), srcs   # the OT kernel's v_fmac_f32_dpp
    problems, n_dpp = [], 0
    for src in srcs:
        out = tmp_path / (os.path.basename(src) + ".s")
        r = subprocess.run([hipcc] + B.FLAGS + ["-x", "hip", "--cuda-device-only", "-S", src, "-o", str(out)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        text = out.read_text()
        n_dpp += sum(1 for ln in text.splitlines() if (_split(ln) or ("",))[0].endswith("_dpp"))
        problems += [(os.path.basename(src),) + h for h in dpp_hazards(text)]
    assert n_dpp > 0
    assert not problems, "\n".join(f"{s} {fn} line {no}: {ins}  <- {wr} ({ws} wait states)" for s, fn, no, ins, wr, ws in problems[:20])
