#!/usr/bin/env python3
"""Which gfx950 kernels does a change recompile differently?  For a refactor that claims "same code":

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -I include -o before.s goleft_amd/csrc/gd_api.hip   # at the parent
    ... the same at the branch, -o after.s ...
    tools/compare_kernel_asm.py before.s after.s [--strip TEXT ...] [--rename OLD=NEW ...]

Kernels are matched by demangled name (--strip removes what a rename took out of the names, e.g. "4096, 256, "; --rename
replaces OLD by NEW in the names of the first file, in the order given, so that a kernel pairs up with what it became), bodies are
compared instruction by instruction: comments, directives and basic-block label numbers do not count.  A kernel whose only
differences are trailing immediates (the offset of a kernel argument or a struct's stride, after a field went) is marked."""
import re
import subprocess
import sys


def kernels(path, strip, rename):
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for name, d in zip(names, dem):
        body = text[text.index("\n%s:" % name):text.index(".amdhsa_kernel %s" % name)]
        ins = []
        for line in body.split("\n")[2:]:
            line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
            if line and not (line.startswith(".") and not line.startswith(".LBB_")):
                ins.append(line)
        for s in ["void "] + strip:                  # (a kernel that stops being a template loses its return type)
            d = d.replace(s, "")
        for old, new in rename:
            d = d.replace(old, new)
        out[d] = ins
    return out


def main():
    strip = [a for i, a in enumerate(sys.argv) if i and sys.argv[i - 1] == "--strip"]
    rename = [a.split("=", 1) for i, a in enumerate(sys.argv) if i and sys.argv[i - 1] == "--rename"]
    a, b = kernels(sys.argv[1], strip, rename), kernels(sys.argv[2], strip, [])
    same = [k for k in a if k in b and a[k] == b[k]]
    print("%d kernels before, %d after, %d identical" % (len(a), len(b), len(same)))
    imm = lambda ins: [re.sub(r"(, |offset:)(0x[0-9a-f]+|-?\d+)$", r"\1#", i) for i in ins]   # a trailing immediate operand
    for k in sorted(set(a) | set(b)):
        if k in same:
            continue
        n = lambda d: "%d instructions" % sum(not i.endswith(":") for i in d[k]) if k in d else "absent"
        note = ""
        if k in a and k in b and imm(a[k]) == imm(b[k]):
            note = " (the same but for %d immediate operands)" % sum(x != y for x, y in zip(a[k], b[k]))
        print("  differs: %s: %s -> %s%s" % (k, n(a), n(b), note))


if __name__ == "__main__":
    main()
