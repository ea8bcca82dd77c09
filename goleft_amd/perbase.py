"""`perbase` entry point: the per-base depth of a BAM as a bedGraph -- runs of equal depth, or with --quantize of equal
depth bin --, run-length encoded on the device (the BAM read, the text and the exit codes live in the C++ host twin;
DepthEngine.perbase_runs is the call underneath)."""
from __future__ import annotations

import ctypes as C
import sys

from . import _hostlib


def Main(argv, out_path=None) -> int:
    """argv: the arguments after the program name, e.g. ["-Q", "0", "-c", "chr20", "--quantize", "1,4,100", "x.bam"].
    The lines go to out_path (stdout, or -o, when None); returns the exit code."""
    lib = _hostlib.load()
    args = [b"perbase"] + [str(a).encode() for a in argv]
    arr = (C.c_char_p * len(args))(*args)
    return int(lib.gdh_perbase_run(len(args), arr, out_path.encode() if out_path else None))


if __name__ == "__main__":
    sys.exit(Main(sys.argv[1:]))
