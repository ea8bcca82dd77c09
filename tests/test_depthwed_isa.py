"""CPU: the device's floating-point code is compiled as written.  gd_depthwed_cell (goleft_amd/csrc/gd_round4g.hpp)
decides the 4-digit rounding of a depthwed cell from exact remainders, and the proof needs every operation rounded
on its own: HIP clang contracts a multiply and a dependent add into one FMA across statements by default, which
turned `r = hi - d0` (hi = q * P rounded) into fma(q, P, -d0) and moved cells on x.5 ties by one.  The header turns
contraction off inside its two functions; this test compiles the depthwed kernel and the multidepth kernels for
gfx950 with the library's flags and checks what came out, so a change to the pragma, the flags or the compiler that
brings contraction back is seen on the CPU box.  (The multidepth sums divide and then add: nothing to contract.)"""
import os
import re
import shutil
import subprocess

import pytest

from tests import helpers as H

HIPCC = next((p for p in ("/opt/rocm/bin/hipcc", shutil.which("hipcc") or "") if p and os.path.exists(p)), None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc")

CSRC = os.path.join(H.ROOT, "goleft_amd", "csrc")
WED = "_ZN2gd18gd_depthwed_kernelENS_6WedJobE"
MD_SUMS = "_ZN2gd17gd_md_sums_kernelENS_9MdSumsJobE"


def _hipflags():
    """HIPFLAGS of goleft_amd/csrc/Makefile (what libgoleft_depth.so is compiled with)."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= *(\S+)", mk, re.M).group(1)
    flags = re.search(r"^HIPFLAGS \?= *(.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()
    assert "--offload-arch=gfx950" in flags, flags
    return flags


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    d = tmp_path_factory.mktemp("wed_isa")
    src = d / "k.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include <cstdint>\n#include "%s"\n#include "%s"\n' %
                   (os.path.join(CSRC, "gd_depthwed.hpp"), os.path.join(CSRC, "gd_multidepth.hpp")))
    out = {}
    for kind, extra in (("asm", []), ("ir", ["-emit-llvm"])):
        dst = d / ("k." + kind)
        subprocess.check_call([HIPCC] + _hipflags() + ["--cuda-device-only", "-S"] + extra + ["-o", str(dst), str(src)],
                              stderr=subprocess.DEVNULL)
        out[kind] = dst.read_text()
    return out


def _asm_body(text, sym):
    at = text.index("\n%s:" % sym)
    return text[at:text.index("s_endpgm", at)].splitlines()


def _vregs(op):
    """VGPR numbers an operand names (v7, v[6:7], -v[6:7], |v[6:7]|), as a set."""
    m = re.fullmatch(r"[-|]*v(?:(\d+)|\[(\d+):(\d+)\])\|?", op.strip())
    if not m:
        return set()
    if m.group(1):
        return {int(m.group(1))}
    return set(range(int(m.group(2)), int(m.group(3)) + 1))


def _insts(body):
    """[(line, mnemonic, [operands])] of the instructions of an assembly body."""
    out = []
    for i, l in enumerate(body):
        l = l.split(";")[0].strip()
        if not l or l.startswith(".") or l.endswith(":"):
            continue
        mn, _, rest = l.partition(" ")
        out.append((i, mn, [o.strip() for o in rest.split(",")] if rest else []))
    return out


def _uses_until_redefined(insts, k):
    """The instructions after insts[k] that run before its destination registers are written again."""
    dst = _vregs(insts[k][2][0])
    for inst in insts[k + 1:]:
        yield inst
        _, mn, ops = inst
        if ops and mn.startswith(("v_", "global_load", "ds_read", "flat_load", "buffer_load")) and _vregs(ops[0]) & dst:
            return


def test_depthwed_remainder_is_not_contracted(compiled):
    insts = _insts(_asm_body(compiled["asm"], WED))
    rndne = [k for k, (_, mn, _) in enumerate(insts) if mn.startswith("v_rndne_f64")]
    assert rndne, "no v_rndne_f64 in gd_depthwed_kernel"
    fused, halves = [], 0
    for k in rndne:
        d = insts[k][2][0]
        for j, (_, mn, ops) in enumerate(_uses_until_redefined(insts, k)):
            if mn.startswith("v_fma_f64") and len(ops) == 4 and ops[3] == "-" + d:
                fused.append((insts[k][0], mn, ops))
            if mn.startswith("v_add_f64") and len(ops) == 3 and ops[2] == "-" + d:
                # r = hi - d0, then r == 0.5 / r == -0.5
                sub = k + 1 + j
                halves += any(m.startswith("v_cmp") and {"0.5", "-0.5"} & set(o) and o[-1] == insts[sub][2][0]
                              for _, m, o in _uses_until_redefined(insts, sub))
    assert not fused, "a rint() result is the negated addend of an FMA (contracted remainder): %s" % fused
    assert halves >= 1, "the remainder that is compared with 0.5 is not a v_add_f64 of the rint() result"


def test_depthwed_ir_carries_no_contract_flag(compiled):
    ir = compiled["ir"]
    at = ir.index("@%s(" % WED)
    body = ir[ir.rindex("define", 0, at):ir.index("\n}\n", at)]
    ops = re.findall(r"= (fmul|fsub|fadd|fdiv)( [a-z ]*)?double", body)
    # the division sum / len, the scalings by 10^j, hi = q * P, r = hi - d0, the +-1 corrections
    assert len(ops) >= 8, ops
    flagged = [l.strip() for l in body.splitlines() if re.search(r"= (fmul|fsub|fadd|fdiv) [a-z ]*contract", l)]
    assert not flagged, flagged


def test_md_sums_adds_the_rounded_quotient(compiled):
    """multidepth.go: dps[i] += float64(d) / 1000. -- the correctly rounded division (v_div_* ending in
    v_div_fixup_f64), then a separate v_add_f64 into the accumulator."""
    insts = _insts(_asm_body(compiled["asm"], MD_SUMS))
    fix = [k for k, (_, mn, _) in enumerate(insts) if mn.startswith("v_div_fixup_f64")]
    assert fix, "no v_div_fixup_f64 in gd_md_sums_kernel"
    for k in fix:
        q = _vregs(insts[k][2][0])
        users = [(mn, ops) for _, mn, ops in _uses_until_redefined(insts, k) if any(_vregs(o) & q for o in ops[1:])]
        assert users and all(mn.startswith("v_add_f64") for mn, _ in users), users
