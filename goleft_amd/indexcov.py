"""`goleft indexcov` entry point mirroring goleft's indexcov/indexcov.go Main()
(flag parsing, the index reading, the text and the exit codes live in the C++ host twin)."""
from __future__ import annotations

import ctypes as C
import sys

from . import _hostlib


def Main(argv) -> int:
    """argv: the arguments after the program name, e.g. ["-d", "out", "a.bam", "b.bam"]; the inputs are .bam, .bai
    or .crai files in any mix (a .bai or .crai first needs "-f", "ref.fai"; for a .cram pass its .crai).
    Writes out/out-indexcov.bed.gz, .roc and .ped; returns the exit code."""
    lib = _hostlib.load()
    args = [b"indexcov"] + [str(a).encode() for a in argv]
    arr = (C.c_char_p * len(args))(*args)
    return int(lib.gdh_indexcov_run(len(args), arr))


if __name__ == "__main__":
    sys.exit(Main(sys.argv[1:]))
