"""`emdepth` entry point: copy numbers per site of a depthwed matrix, goleft's emdepth.EMDepth run on the device
(the matrix reading, the blocks of rows, the output rows and the exit codes live in the C++ host twin)."""
from __future__ import annotations

import ctypes as C
import sys

from . import _hostlib


def Main(argv, out_path=None) -> int:
    """argv: the arguments after the program name, e.g. ["--scales", "scales.txt", "matrix.bed.gz"]: a depthwed
    matrix (`#chrom start end samples...` and its rows), plain or gzipped, already normalised.
    The rows go to out_path (stdout when None); returns the exit code."""
    lib = _hostlib.load()
    args = [b"emdepth"] + [str(a).encode() for a in argv]
    arr = (C.c_char_p * len(args))(*args)
    return int(lib.gdh_emdepth_run(len(args), arr, out_path.encode() if out_path else None))


if __name__ == "__main__":
    sys.exit(Main(sys.argv[1:]))
