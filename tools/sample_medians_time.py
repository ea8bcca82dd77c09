#!/usr/bin/env python3
"""Time gd_sample_medians (host float32) and gd_sample_medians_cells (int64 cells resident on the device) on the matrix
of DESIGN.md section 3.10's measurement (section 3.12, "Measured").

    python tools/sample_medians_time.py [--rows 250000] [--samples 200] [--out FILE]

The matrix is integer cells at a 20 - 40x level per row, 2 % of the cells carrying a factor of {0, 1/2, 1, 1 1/2, 2, 4}.
Seven calls of each form, the first two left out, the median of the other five.  The kernel seconds are the library's
own (gd_sample_medians_timing: from the first launch to the end of the last pass, the counters' clearing included); with
the passes it ran and the bytes a pass reads they give the rate the matrix streamed at.  Both results are checked against
a sort on the host."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from goleft_amd import _lib                                             # noqa: E402


def matrix(rows, n, seed=310):
    rng = np.random.default_rng(seed)
    level = rng.uniform(20.0, 40.0, size=(rows, 1))
    cells = rng.poisson(level, size=(rows, n)).astype(np.float64)
    factor = np.where(rng.random((rows, n)) < 0.02, rng.choice([0, 0.5, 1, 1.5, 2, 4], size=(rows, n)), 1.0)
    return np.floor(cells * factor).astype(np.int64)


def host_medians(m):
    s = np.sort(m, axis=0)
    k = (s == 0).sum(0)
    idx = k + (0.65 * (m.shape[0] - k).astype(np.float64)).astype(np.int64)
    return s[np.minimum(idx, m.shape[0] - 1), np.arange(m.shape[1])]


def seven(f, lib, h, ok):
    wall, split = [], []
    for _ in range(7):
        t0 = time.perf_counter()
        f()
        wall.append(time.perf_counter() - t0)
        t = (C.c_double * 4)()
        ok(lib.gd_sample_medians_timing(h, t, 4))
        split.append(list(t))
    med = lambda k: float(np.median([s[k] for s in split[2:]]))
    return dict(wall_s=float(np.median(wall[2:])), upload_s=med(0), kernels_s=med(1), readback_s=med(2), passes=int(split[-1][3]),
                kernels_all=[round(s[1], 6) for s in split])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=250000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows, n = a.rows, a.samples
    cells = matrix(rows, n)
    depths = cells.astype(np.float32)
    want = host_medians(cells)
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.gd_create(0, C.byref(h)) == 0

    def ok(rc):
        assert rc == 0, lib.gd_last_error(h).decode()

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    p = C.c_void_p()
    ok(lib.gd_device_alloc(h, cells.nbytes, C.byref(p)))
    assert hip.hipMemcpy(p, cells.ctypes.data, cells.nbytes, 1) == 0
    res = dict(rows=rows, samples=n)
    fmed, imed, nz = np.empty(n, np.float32), np.empty(n, np.int64), np.empty(n, np.uint64)

    r = seven(lambda: ok(lib.gd_sample_medians(h, depths.ctypes.data, rows, n, fmed.ctypes.data, nz.ctypes.data)), lib, h, ok)
    r["bytes_per_pass"] = int(depths.nbytes)
    r["GBps"] = r["passes"] * depths.nbytes / r["kernels_s"] / 1e9
    r["agrees_with_host_sort"] = bool(np.array_equal(fmed, want.astype(np.float32)))
    res["float32"] = r

    r = seven(lambda: ok(lib.gd_sample_medians_cells(h, p, rows, n, imed.ctypes.data, nz.ctypes.data)), lib, h, ok)
    r["bytes_per_pass"] = int(cells.nbytes)
    r["GBps"] = r["passes"] * cells.nbytes / r["kernels_s"] / 1e9
    r["agrees_with_host_sort"] = bool(np.array_equal(imed, want))
    res["int64_cells"] = r

    ok(lib.gd_device_free(h, p))
    lib.gd_destroy(h)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
