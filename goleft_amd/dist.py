"""`dist` entry point: the depth distribution (PREFIX.dist.txt), the summary (PREFIX.summary.txt) and, over the lines of a
BED file, the region distribution and the threshold counts of a BAM, counted on the device (the BAM read, the text and the
exit codes live in the C++ host twin; DepthEngine.depth_hist and DepthEngine.region_bins are the calls underneath)."""
from __future__ import annotations

import ctypes as C
import sys

from . import _hostlib


def Main(argv) -> int:
    """argv: the arguments after the program name, e.g. ["-Q", "0", "-b", "exons.bed", "--thresholds", "10,20,30",
    "--prefix", "out/sample", "x.bam"].  Returns the exit code."""
    lib = _hostlib.load()
    args = [b"dist"] + [str(a).encode() for a in argv]
    arr = (C.c_char_p * len(args))(*args)
    return int(lib.gdh_dist_run(len(args), arr))


if __name__ == "__main__":
    sys.exit(Main(sys.argv[1:]))
