#!/usr/bin/env python3
"""Time gd_chunk_debias on a cohort-sized matrix ("Measured").

    python tools/chunk_debias_time.py [--rows 250000] [--samples 200] [--out FILE]

The matrix is that of tools/sample_medians_time.py (integer cells at a 20 - 40x level per row, 2 % of them carrying a
factor of {0, 1/2, 1, 1 1/2, 2, 4}); the covariate is drawn like GC content: a bell around 0.41, sd 0.05, clipped to
[0, 1].  Three windows: 0.01 (the command line's default), one small enough for about 10^4 chunks, and one that leaves a
single chunk.  Seven calls each, the first two left out, the median of the other five.  The seconds are the library's own
(gd_chunk_debias_timing): host sort + chunking, upload, kernels, read-back; with GOLEFT_CHUNKDEBIAS_SPLIT=1 in the
environment the median kernel is also timed apart from the divide kernel.  The rate is the bytes the kernels must move
(the matrix read four times for the medians and once for the division, the quotients written once) over the kernel
seconds.  The same job is timed on the host in the same run, for scale -- numpy's partition (an introselect, what
nth_element is) per chunk, over all columns at once, and a float64 division -- and the device's quotients are compared
with it bit for bit."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from goleft_amd import _lib                                             # noqa: E402
from tools.sample_medians_time import matrix                            # noqa: E402


def gc_vals(rows, seed=311):
    return np.clip(np.random.default_rng(seed).normal(0.41, 0.05, rows), 0.0, 1.0)


def host_debias(m, vals, window):
    """(out float32, chunks, seconds of the chunking, seconds of the selection and division)"""
    t0 = time.perf_counter()
    order = np.argsort(vals, kind="stable")
    s = vals[order]
    slices, v0 = [0], s[0]
    while True:                                  # the first i with s[i] - v0 > window: a bisection, then the exact test
        i = int(np.searchsorted(s, v0 + window, side="right"))
        while i < len(s) and not s[i] - v0 > window:
            i += 1
        while i > slices[-1] and s[i - 1] - v0 > window:
            i -= 1
        if i >= len(s):
            break
        v0 = s[i]
        slices.append(i)
    slices.append(len(s))
    t1 = time.perf_counter()
    out = np.empty(m.shape, np.float32)
    cols = np.arange(m.shape[1])
    for c in range(len(slices) - 1):
        rows = order[slices[c]:slices[c + 1]]
        sub = m[rows]
        n = len(rows)
        idx = (n - (sub == 0).sum(0)) // 2
        med = np.partition(sub, np.unique(idx), axis=0)[idx, cols]
        q = sub.astype(np.float64)
        np.divide(q, med.astype(np.float64)[None, :], out=q, where=(med > 0)[None, :])
        out[rows] = q
    return out, len(slices) - 1, t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=250000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--small-window", type=float, default=3e-5)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows, n = a.rows, a.samples
    depths = matrix(rows, n).astype(np.float32)
    vals = gc_vals(rows)
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.gd_create(0, C.byref(h)) == 0

    def ok(rc):
        assert rc == 0, lib.gd_last_error(h).decode()

    out = np.empty((rows, n), np.float32)
    res = dict(rows=rows, samples=n, matrix_bytes=int(depths.nbytes))
    for name, window in (("window_0.01", 0.01), ("small_window", a.small_window), ("one_chunk", 2.0)):
        wall, split = [], []
        for _ in range(7):
            t0 = time.perf_counter()
            ok(lib.gd_chunk_debias(h, depths.ctypes.data, rows, n, vals.ctypes.data, window, out.ctypes.data, None, None, None,
                                   None, 0))
            wall.append(time.perf_counter() - t0)
            t = (C.c_double * 7)()
            ok(lib.gd_chunk_debias_timing(h, t, 7))
            split.append(list(t))
        med = lambda k: float(np.median([s[k] for s in split[2:]]))
        r = dict(window=window, chunks=int(split[-1][4]), largest_chunk=int(split[-1][5]), wall_s=float(np.median(wall[2:])),
                 sort_s=med(0), upload_s=med(1), kernels_s=med(2), readback_s=med(3), median_kernel_s=med(6),
                 kernels_all=[round(s[2], 6) for s in split])
        r["GBps"] = 6 * depths.nbytes / r["kernels_s"] / 1e9
        want, chunks, host_chunk_s, host_select_s = host_debias(depths, vals, window)
        r["host_chunking_s"], r["host_select_divide_s"] = host_chunk_s, host_select_s
        r["agrees_with_host"] = bool(chunks == r["chunks"] and np.array_equal(out.view(np.uint32), want.view(np.uint32)))
        res[name] = r
    lib.gd_destroy(h)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
