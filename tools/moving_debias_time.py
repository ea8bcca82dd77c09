#!/usr/bin/env python3
"""Time gd_moving_debias on a cohort-sized matrix ("Measured").

    python tools/moving_debias_time.py [--rows 250000] [--samples 200] [--windows 9,255] [--host-rows 10000] [--out FILE]

The matrix and the covariate are those of tools/chunk_debias_time.py (integer cells at a 20 - 40x level per row; GC content
drawn as a bell around 0.41, sd 0.05), so the figures stand beside gd_chunk_debias's.  Seven calls a window, the first two
left out, the median of the other five.  The seconds are the library's own (gd_moving_debias_timing): host sort, upload,
kernel, read-back.  The rate is the bytes the kernel must move (the matrix read once to push and once to divide, the
quotients written once) over the kernel seconds; the second read mostly hits the cache, so it flatters nobody.

The restatement (tests/movdebias_ref.py: numpy, one sort of a window over all columns per row) is timed in the same run on
the first --host-rows rows in covariate order -- at W = 255 the whole matrix would take minutes -- and the device's
quotients of those rows (a call of their own) are compared with it bit for bit; restatement_s_per_row x rows is what the
whole matrix would cost it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from goleft_amd import _lib                                             # noqa: E402
from tests import movdebias_ref as MR                                   # noqa: E402
from tools.chunk_debias_time import gc_vals                             # noqa: E402
from tools.sample_medians_time import matrix                            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=250000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--windows", default="9,255")
    ap.add_argument("--host-rows", type=int, default=10000)
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
    sub = np.sort(np.argsort(vals, kind="stable")[:min(a.host_rows, rows)])
    sub_depths, sub_vals = np.ascontiguousarray(depths[sub]), np.ascontiguousarray(vals[sub])
    sub_out = np.empty(sub_depths.shape, np.float32)
    for W in [int(w) for w in a.windows.split(",")]:
        wall, split = [], []
        for _ in range(7):
            t0 = time.perf_counter()
            ok(lib.gd_moving_debias(h, depths.ctypes.data, rows, n, vals.ctypes.data, W, out.ctypes.data, None))
            wall.append(time.perf_counter() - t0)
            t = (C.c_double * 4)()
            ok(lib.gd_moving_debias_timing(h, t, 4))
            split.append(list(t))
        med = lambda k: float(np.median([s[k] for s in split[2:]]))
        r = dict(window=W, wall_s=float(np.median(wall[2:])), sort_s=med(0), upload_s=med(1), kernels_s=med(2),
                 readback_s=med(3), kernels_all=[round(s[2], 6) for s in split])
        r["GBps"] = 3 * depths.nbytes / r["kernels_s"] / 1e9
        ok(lib.gd_moving_debias(h, sub_depths.ctypes.data, len(sub), n, sub_vals.ctypes.data, W, sub_out.ctypes.data, None))
        t0 = time.perf_counter()
        want, _ = MR.debias(sub_depths, sub_vals, W)
        r["restatement_rows"] = int(len(sub))
        r["restatement_s"] = time.perf_counter() - t0
        r["restatement_s_per_row"] = r["restatement_s"] / len(sub)
        r["restatement_whole_matrix_s"] = r["restatement_s_per_row"] * rows
        r["agrees_with_restatement"] = bool(np.array_equal(sub_out.view(np.uint32), want.view(np.uint32)))
        res["window_%d" % W] = r
    lib.gd_destroy(h)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
