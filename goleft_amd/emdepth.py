"""`emdepth`, `scales` and `debias` entry points: copy numbers per site of a depthwed matrix, goleft's emdepth.EMDepth run
on the device, the per-sample factors that normalise such a matrix first, dcnv's ChunkDebiaser or GeneralDebiaser,
which free it of GC bias before that, and its SVD debiaser for the bias without a covariate (the matrix reading, the blocks of rows, the output
rows and the exit codes live in the C++ host twin)."""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _hostlib


def _argv(name, argv):
    args = [name] + [str(a).encode() for a in argv]
    return len(args), (C.c_char_p * len(args))(*args)


def Main(argv, out_path=None) -> int:
    """argv: the arguments after the program name, e.g. ["--scales", "scales.txt", "matrix.bed.gz"] or
    ["--normalize", "--level", "30", "--cnvs", "cnvs.tsv", "matrix.bed"] or ["--gc-values", "gc.txt", "matrix.bed"]: a
    depthwed matrix (`#chrom start end samples...` and its rows), plain or gzipped, already normalised unless --normalize
    or a GC flag (--gc-values FILE | --gc-fasta REF.fa, [--gc-window W | --gc-moving ROWS]: debias as Debias does, then normalise) is given;
    ["--svd", "2"] runs `debias --svd 2 --zscore` after that and before the normalisation, ["--svd", "2", "--log2"] runs
    `debias --svd 2 --log2` there.
    The rows go to out_path (stdout when None); returns the exit code."""
    lib = _hostlib.load()
    n, arr = _argv(b"emdepth", argv)
    return int(lib.gdh_emdepth_run(n, arr, out_path.encode() if out_path else None))


def Scales(argv, out_path=None) -> int:
    """`goleft-depth scales`: argv e.g. ["--level", "1", "matrix.bed.gz"].  One factor per sample and line goes to
    out_path (stdout when None), the file `emdepth --scales` takes; returns the exit code."""
    lib = _hostlib.load()
    n, arr = _argv(b"scales", argv)
    return int(lib.gdh_scales_run(n, arr, out_path.encode() if out_path else None))


def Debias(argv, out_path=None) -> int:
    """`goleft-depth debias`: argv e.g. ["--gc-values", "gc.txt", "--window", "0.02", "matrix.bed.gz"] or ["--fasta",
    "ref.fa", "matrix.bed"].  The matrix with every cell divided by its sample's median over the rows of similar covariate
    (dcnv's ChunkDebiaser; with ["--moving", "9"] in place of --window by the moving median of dcnv's GeneralDebiaser) goes
    to out_path (stdout when None); returns the exit code.  ["--svd", "2", "--zscore", "matrix.bed"] takes no covariate:
    dcnv's SVD debiaser zeroes the leading singular values whose share of the spectrum exceeds 2 per cent, at most 15, between
    the z-score scaler's two halves; the removed shares go to stderr.  ["--svd", "2", "--log2", "matrix.bed"] puts dcnv's
    Log2 scaler in the z-score's place: log2(1 + depth) centred per sample, and back by max(0, 2^x - 1)."""
    lib = _hostlib.load()
    n, arr = _argv(b"debias", argv)
    return int(lib.gdh_debias_run(n, arr, out_path.encode() if out_path else None))


def scales(med, level=None):
    """The factors that carry every sample to one level, from DepthEngine.sample_medians' medians (all > 0):
    float32(T / med[s]) with the division in float64 and T = sorted(med)[N // 2], or `level` (1: the 1 / med[s] dcnv's
    NormalizeBySampleMedian divides by).  What `goleft-depth scales` writes and emdepth_cells takes as its scale."""
    m = [float(v) for v in np.asarray(med).ravel()]
    if not m or not all(v > 0 and np.isfinite(v) for v in m):
        raise ValueError("scales: every sample needs a finite median above 0")
    T = sorted(m)[len(m) // 2] if level is None else float(level)
    if not (T > 0 and np.isfinite(T)):
        raise ValueError("scales: the level must be a finite number > 0")
    with np.errstate(over="ignore"):
        out = np.array([np.float32(T / v) for v in m], np.float32)
    if not np.isfinite(out).all():
        raise ValueError("scales: a factor is not finite as a float32")
    return out


def _factors(med, nonzero, T):
    """scales() with the two refusals of the command line's sample_scales, each naming the sample; T None: the level"""
    for s, k in enumerate(np.asarray(nonzero).tolist()):
        if k == 0:
            raise ValueError("cohort_cnvs: sample %d has no depth above 0: it has no factor" % s)
    if T is None:
        return float(sorted(np.asarray(med).tolist())[len(med) // 2])
    with np.errstate(over="ignore", divide="ignore"):
        out = np.array([np.float32(float(T) / float(v)) for v in np.asarray(med).ravel()], np.float32)
    for s, f in enumerate(out.tolist()):
        if not np.isfinite(f):
            raise ValueError("cohort_cnvs: sample %d: the factor %g / %g is not finite as a float32" % (s, T, float(med[s])))
    return out


def cohort_cnvs(eng, dptr, rows, n_samples, starts, ends, vals=None, window=None, level=None, block_rows=None,
                site_cn=False, moving=None, svd=None, svd_scaler="zscore"):
    """From DepthEngine.depthwed_device's int64 cells (dptr, rows) to CNV calls without the matrix leaving HBM: the
    resident twin of `goleft-depth emdepth --normalize --cnvs` (vals None) and of `emdepth --gc-values --cnvs` (vals: the
    covariate of every row, window: --gc-window, 0.01 when None; or moving: --gc-moving, the odd window of dcnv's
    GeneralDebiaser in place of the ChunkDebiaser -- giving both is a ValueError).  svd: --svd, the share in per cent above
    which dcnv's SVD debiaser zeroes a leading singular value, z-scored (svd_scaler "zscore") or between the halves of
    dcnv's Log2 scaler (svd_scaler "log2": --log2; anything else is a ValueError), after the GC debias when vals is given and
    before the normalisation; with svd and without vals the level None is the middle sample median of the debiased matrix,
    as `debias --svd PCT --zscore | emdepth --normalize` has it.  level: --level; None is the middle sample median of the matrix as
    read.  Returns (factors float32 [samples], level, what DepthEngine.emdepth_cnvs* returns); the per-site copy numbers
    are read back only when site_cn is set, everything else that comes back is O(samples + calls).

    With vals the order is the command line's (DESIGN.md sections 3.13, 3.14): the level from the cells, ChunkDebiaser
    into a device float32 matrix of this call's own, the sample medians of the quotients, the factors
    float32(level / med[s]), the quotients scaled in place, emdepth.Cache over them.  ValueError names a sample that has
    no depth above 0 or whose factor is not finite as a float32; the engine's refusals come as GdError."""
    if level is not None and not (float(level) > 0 and np.isfinite(float(level))):
        raise ValueError("cohort_cnvs: the level must be a finite number > 0")
    if moving is not None and window is not None:
        raise ValueError("cohort_cnvs: window (the ChunkDebiaser) and moving (the GeneralDebiaser) exclude each other")
    if svd_scaler not in ("zscore", "log2"):
        raise ValueError("cohort_cnvs: svd_scaler is 'zscore' or 'log2'")
    if moving is not None and vals is None:
        raise ValueError("cohort_cnvs: moving needs the covariate of every row")
    T = None if level is None else float(level)
    if (T is None or vals is None) and not (svd is not None and vals is None):
        med, nz = eng.sample_medians_cells(dptr, rows, n_samples)
        # (float)median: the rounding is monotone, so this is the median of the float32 matrix the command line reads
        med = med.astype(np.float32)
        if T is None:
            T = _factors(med, nz, None)
    if vals is None and svd is None:
        f = _factors(med, nz, T)
        return f, T, eng.emdepth_cnvs_cells(dptr, rows, n_samples, starts, ends, scale=f, block_rows=block_rows, site_cn=site_cn)
    out = eng.device_alloc(max(rows * n_samples * 4, 1))
    try:
        if vals is None:
            eng.svd_debias_cells(dptr, rows, n_samples, svd, True, out, scaler=svd_scaler)
        else:
            if moving is not None:
                eng.moving_debias_cells(dptr, rows, n_samples, vals, moving, out)
            else:
                eng.chunk_debias_cells(dptr, rows, n_samples, vals, 0.01 if window is None else window, out)
            if svd is not None:
                eng.svd_debias_device(out, rows, n_samples, svd, True, out, scaler=svd_scaler)
        med, nz = eng.sample_medians_device(out, rows, n_samples)
        if vals is None and level is None:
            T = _factors(med, nz, None)
        f = _factors(med, nz, T)
        eng.scale_device(out, rows, n_samples, f)
        return f, T, eng.emdepth_cnvs_device(out, rows, n_samples, starts, ends, block_rows=block_rows, site_cn=site_cn)
    finally:
        eng.device_free(out)


if __name__ == "__main__":
    sys.exit(Main(sys.argv[1:]))
