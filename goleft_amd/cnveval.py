"""`cnveval` entry points mirroring the reference's cnveval command and its Evaluate: precision and recall of a call set
against a truth set, counted on the device (the file reading, the report and the exit codes live in the C++ host twin)."""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _hostlib
from .engine import DepthEngine

FP, FN, TP, TN = 0, 1, 2, 3                      # the last axis of evaluate()'s array, the reference's Stat field order
SIZE_CLASSES = ("0-20000", "20000-100000", ">=100000")


def Main(argv, out_path=None) -> int:
    """argv: the arguments after the program name, e.g. ["-m", "0.5", "-s", "truth.bed", "test.bed.gz"].
    The four size-class lines go to out_path (stdout when None); returns the exit code."""
    lib = _hostlib.load()
    args = [b"cnveval"] + [str(a).encode() for a in argv]
    arr = (C.c_char_p * len(args))(*args)
    return int(lib.gdh_cnveval_run(len(args), arr, out_path.encode() if out_path else None))


def evaluate(cnvs, truths, min_overlap=0.4, device=0):
    """cnveval.Evaluate through gd_cnveval.  cnvs: (chrom, start, end, cn, sample) tuples; truths: (chrom, start, end,
    cn, samples) tuples, samples a sequence of names.  Returns (names, stats): the sorted union of the samples of both
    sets, and an int64 array [len(names)][3][4] -- size class by FP, FN, TP, TN -- what CohortStats holds per sample.
    Chromosomes order as byte strings; calls of one sample with equal (chrom, start) keep their order in cnvs."""
    cnvs = list(cnvs)
    truths = [(t[0], t[1], t[2], t[3], list(t[4])) for t in truths]
    names = sorted({c[4] for c in cnvs}.union(*[t[4] for t in truths]))
    sid = {s: i for i, s in enumerate(names)}
    as_bytes = lambda s: s if isinstance(s, bytes) else str(s).encode()
    rank = {c: i for i, c in enumerate(sorted({x[0] for x in cnvs} | {t[0] for t in truths}, key=as_bytes))}
    rows = sorted(cnvs, key=lambda c: (sid[c[4]], rank[c[0]], c[1]))          # stable
    i32 = lambda xs: np.ascontiguousarray(np.array(xs, np.int64).reshape(-1).astype(np.int32))
    for what, xs in (("call", rows), ("truth", truths)):
        for x in xs:
            if not all(-2 ** 31 <= int(v) < 2 ** 31 for v in x[1:4]):
                raise ValueError("cnveval: %s %r: start, end and copy number are 32-bit integers" % (what, x))
    cnv_off = np.zeros(len(names) + 1, np.int64)
    for c in rows:
        cnv_off[sid[c[4]] + 1] += 1
    cnv_off = np.cumsum(cnv_off).astype(np.int64)
    t_off = np.cumsum([0] + [len(t[4]) for t in truths]).astype(np.int64)
    arrays = [cnv_off, i32([rank[c[0]] for c in rows]), i32([c[1] for c in rows]), i32([c[2] for c in rows]), i32([c[3] for c in rows]),
              i32([rank[t[0]] for t in truths]), i32([t[1] for t in truths]), i32([t[2] for t in truths]), i32([t[3] for t in truths]),
              t_off, i32([sid[s] for t in truths for s in t[4]])]
    stats = np.zeros((len(names), 3, 4), np.int64)
    ptr = lambda a: a.ctypes.data if a.size else None
    eng = DepthEngine(device)
    try:
        eng._chk(eng._lib.gd_cnveval(eng._ctx, len(names), arrays[0].ctypes.data, *[ptr(a) for a in arrays[1:5]], len(truths),
                                     *[ptr(a) for a in arrays[5:9]], arrays[9].ctypes.data, ptr(arrays[10]), float(min_overlap),
                                     stats.ctypes.data))
    finally:
        eng.close()
    return names, stats


if __name__ == "__main__":
    sys.exit(Main(sys.argv[1:]))
