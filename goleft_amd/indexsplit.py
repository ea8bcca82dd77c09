"""`goleft indexsplit` entry point mirroring goleft's indexsplit/indexsplit.go Main()
(flag parsing, the index reading, the walk over the tiles and the exit codes live in the C++ host twin)."""
from __future__ import annotations

import ctypes as C
import sys

from . import _hostlib


def Main(argv, out_path=None) -> int:
    """argv: the arguments after the program name, e.g. ["-n", "1000", "a.bam", "b.bam"]; the inputs are .bam, .bai
    or .crai files in any mix (a .bai or .crai first needs "--fai", "ref.fai"; for a .cram pass its .crai).
    The rows go to out_path (stdout when None); returns the exit code."""
    lib = _hostlib.load()
    args = [b"indexsplit"] + [str(a).encode() for a in argv]
    arr = (C.c_char_p * len(args))(*args)
    return int(lib.gdh_indexsplit_run(len(args), arr, out_path.encode() if out_path else None))


if __name__ == "__main__":
    sys.exit(Main(sys.argv[1:]))
