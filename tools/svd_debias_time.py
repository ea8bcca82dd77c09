#!/usr/bin/env python3
"""Time gd_svd_debias on a cohort-sized matrix (DESIGN.md sections 3.16 and 3.17, "Measured").

    python tools/svd_debias_time.py [--rows 250000] [--samples 200] [--planted 3] [--log2] [--skip-host] [--out FILE]

The matrix is tests/svddebias_shapes.planted_matrix's: Poisson depths at 30x whose rate carries --planted rank-one
components; the share that cuts the scaled spectrum after them comes from numpy's singular values.  The scaler is the z-score,
or with --log2 dcnv's Log2 scaler (gd_svd_debias_scaled, tests/svdlog2_ref.py).  Seven calls, the first two left out, the
median of the other five.  The seconds are the library's own (gd_svd_debias_timing): upload, row statistics (log2: the
samples' centres) + Gram matrix (with its read-back), eigenpairs on the host, projection, read-back.
gram_share_of_fp64_peak is 2 rows samples^2 flops over the second phase and 78.6 TFLOP/s; project_GBps is the bytes the
projection must move (the matrix read once, the result written once; the statistics pass before it read it once more) over
the fourth phase.

The yardstick is the same job through the oracle on the host -- numpy.linalg.svd of the scaled matrix, the projection, the
unscale -- timed in the same run, and the device's result is held to the contract of tests/test_gpu_svddebias.py (--log2:
tests/test_gpu_svdlog2.py) against it.  --skip-host leaves the yardstick out where it would take minutes: the share then
comes from the eigenvalues of the scaled matrix's Gram matrix, and agrees_with_oracle is null."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from goleft_amd import _lib                                             # noqa: E402
from tests import svddebias_ref as SR                                   # noqa: E402
from tests import svdlog2_ref as LR                                     # noqa: E402
from tests.svddebias_shapes import planted_matrix                       # noqa: E402

FP64_PEAK = 78.6e12
LOG2_DELTA = 2.0 ** -41                                                  # tests/test_gpu_svdlog2.py DELTA


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=250000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--planted", type=int, default=3)
    ap.add_argument("--log2", action="store_true")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    rows, n, k = a.rows, a.samples, a.planted
    depths = planted_matrix(rows, n, k, 30, 1)
    t0 = time.perf_counter()
    Z = (LR.scale if a.log2 else SR.scale)(depths.astype(np.float64))[0]
    if a.skip_host:
        s = np.sqrt(np.maximum(np.linalg.eigvalsh(Z.T @ Z)[::-1], 0.0))
    else:
        s = np.linalg.svd(Z, compute_uv=False)
    del Z
    svd_values_s = time.perf_counter() - t0
    share = 100.0 * s / s.sum()
    pct = float((share[k - 1] + share[k]) / 2) if k else float((share[0] + 100) / 2)
    want, host_s = None, None
    if not a.skip_host:
        t0 = time.perf_counter()
        want = LR.svd_log2(depths, pct) if a.log2 else SR.svd_debias(depths, pct, True)
        host_s = time.perf_counter() - t0

    lib = _lib.load()
    h = C.c_void_p()
    assert lib.gd_create(0, C.byref(h)) == 0

    def ok(rc):
        assert rc == 0, lib.gd_last_error(h).decode()

    out = np.empty((rows, n), np.float32)
    sv, removed = np.empty(min(rows, n), np.float64), C.c_int()
    wall, split = [], []
    for _ in range(7):
        t0 = time.perf_counter()
        ok(lib.gd_svd_debias_scaled(h, depths.ctypes.data, rows, n, pct, 2 if a.log2 else 1, out.ctypes.data, sv.ctypes.data,
                                    C.byref(removed), None))
        wall.append(time.perf_counter() - t0)
        t = (C.c_double * 5)()
        ok(lib.gd_svd_debias_timing(h, t, 5))
        split.append(list(t))
    lib.gd_destroy(h)
    med = lambda i: float(np.median([x[i] for x in split[2:]]))
    res = dict(rows=rows, samples=n, scaler="log2" if a.log2 else "zscore", matrix_bytes=int(depths.nbytes), pct=pct,
               removed=removed.value, wall_s=float(np.median(wall[2:])), upload_s=med(0), stats_gram_s=med(1), eigen_s=med(2),
               project_s=med(3), readback_s=med(4), stats_gram_all=[round(x[1], 6) for x in split],
               project_all=[round(x[3], 6) for x in split], host_numpy_s=host_s, host_singular_values_only_s=svd_values_s)
    res["gram_share_of_fp64_peak"] = 2.0 * rows * n * n / res["stats_gram_s"] / FP64_PEAK
    res["project_GBps"] = 2 * depths.nbytes / res["project_s"] / 1e9
    res["agrees_with_oracle"] = None
    if want is not None:
        ref = want[3]
        err = np.abs(out.astype(np.float64) - ref)
        if a.log2:
            slack = (1.0 + ref) * np.log(2.0) * LOG2_DELTA
        else:
            slack = 2.0 ** -36 * depths.astype(np.float64).max(axis=1, keepdims=True)
        res["agrees_with_oracle"] = bool(removed.value == want[2] and (err <= 2.0 ** -24 * np.abs(ref) + slack).all())
        res["spectrum_off_by_s0"] = float(np.abs(sv - want[1]).max() / want[1][0])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
