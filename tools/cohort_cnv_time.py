#!/usr/bin/env python3
"""Time the chain debias -> medians -> scale -> emdepth -> CNV calls on a cohort-sized matrix, resident against through
the host ("Measured").

    python tools/cohort_cnv_time.py [--rows 250000] [--samples 200] [--block-rows 65536] [--out FILE]

The matrix and the covariate are those of tools/chunk_debias_time.py (section 3.12's integer cells, vals drawn like GC
content, window 0.01); the rows are back-to-back 1000-base sites.  The int64 cells are put into HBM once, outside the
timing, as gd_depthwed_device leaves them.  Two routes, seven runs each, the first two left out, the median of the other
five:

  resident   goleft_amd.emdepth.cohort_cnvs' steps on the device pointer: gd_sample_medians_cells (the level),
             gd_chunk_debias_cells into a device matrix, gd_sample_medians_device, gd_device_scale, gd_emcnv_add_device
  host       the same chain through the host-matrix entry points, from the float32 matrix in host memory:
             gd_sample_medians, gd_chunk_debias, gd_sample_medians, the factors applied by numpy, gd_emcnv_add

Every step's wall clock is taken around the call and the library's own split (the *_timing calls) beside it.  The two routes'
factors, level and calls are compared byte for byte in the same run, and the composed cohort_cnvs is run once more and
compared too."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from goleft_amd import emdepth                                          # noqa: E402
from goleft_amd.engine import DepthEngine                               # noqa: E402
from tools.chunk_debias_time import gc_vals                             # noqa: E402
from tools.sample_medians_time import matrix                            # noqa: E402

WINDOW = 0.01
KEYS = ("sample", "psize", "emit_row", "member_off", "member_row", "depth", "cn", "log2fc")


class Steps:
    """wall seconds per named step of one run, and the library's split of it"""

    def __init__(self):
        self.wall, self.lib = {}, {}

    def run(self, name, f, timing=None):
        t0 = time.perf_counter()
        out = f()
        self.wall[name] = time.perf_counter() - t0
        if timing is not None:
            self.lib[name] = [float(v) for v in timing()]
        return out


def resident(eng, p, rows, n, st, en, vals, block):
    s = Steps()
    med, nz = s.run("level_medians", lambda: eng.sample_medians_cells(p, rows, n), eng.sample_medians_timing)
    T = float(sorted(med.astype(np.float32).tolist())[n // 2])
    out = s.run("alloc", lambda: eng.device_alloc(rows * n * 4))
    try:
        s.run("debias", lambda: eng.chunk_debias_cells(p, rows, n, vals, WINDOW, out), eng.chunk_debias_timing)
        med, nz = s.run("medians", lambda: eng.sample_medians_device(out, rows, n), eng.sample_medians_timing)
        f = emdepth.scales(med, T)
        s.run("scale", lambda: eng.scale_device(out, rows, n, f))
        calls = s.run("cnvs", lambda: eng.emdepth_cnvs_device(out, rows, n, st, en, block_rows=block))
    finally:
        s.run("free", lambda: eng.device_free(out))
    s.lib["cnvs"] = list(calls.pop("timing"))
    return s, f, T, calls


def through_host(eng, m, st, en, vals, block):
    s = Steps()
    med, nz = s.run("level_medians", lambda: eng.sample_medians(m), eng.sample_medians_timing)
    T = float(sorted(med.tolist())[m.shape[1] // 2])
    deb = s.run("debias", lambda: eng.chunk_debias(m, vals, WINDOW)[0], eng.chunk_debias_timing)
    med, nz = s.run("medians", lambda: eng.sample_medians(deb), eng.sample_medians_timing)
    f = emdepth.scales(med, T)
    scaled = s.run("scale", lambda: deb * f[None, :])
    calls = s.run("cnvs", lambda: eng.emdepth_cnvs(scaled, st, en, block_rows=block))
    calls.pop("site_cn")                         # (rows x samples bytes the resident route does not ask for)
    s.lib["cnvs"] = list(calls.pop("timing"))
    return s, f, T, calls


def summary(runs):
    """medians over the runs kept"""
    names = list(runs[0].wall)
    out = dict(wall_s=float(np.median([sum(r.wall.values()) for r in runs])),
               steps_s={k: float(np.median([r.wall[k] for r in runs])) for k in names},
               library_split={k: [float(np.median([r.lib[k][i] for r in runs])) for i in range(len(runs[0].lib[k]))]
                              for k in runs[0].lib},
               wall_all=[round(sum(r.wall.values()), 6) for r in runs])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=250000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--block-rows", type=int, default=65536)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows, n = a.rows, a.samples
    cells = matrix(rows, n)
    m = cells.astype(np.float32)
    vals = gc_vals(rows)
    st = (np.arange(rows, dtype=np.int64) * 1000 & 0xFFFFFFFF).astype(np.uint32)
    en = ((np.arange(rows, dtype=np.int64) + 1) * 1000 & 0xFFFFFFFF).astype(np.uint32)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    res = dict(rows=rows, samples=n, window=WINDOW, block_rows=a.block_rows, cells_bytes=int(cells.nbytes),
               float_matrix_bytes=int(m.nbytes))
    with DepthEngine(0) as eng:
        p = eng.device_alloc(cells.nbytes)
        assert hip.hipMemcpy(p, cells.ctypes.data, cells.nbytes, 1) == 0
        try:
            dev = [resident(eng, p, rows, n, st, en, vals, a.block_rows) for _ in range(7)]
            host = [through_host(eng, m, st, en, vals, a.block_rows) for _ in range(7)]
            t0 = time.perf_counter()
            cf, cT, ccalls = emdepth.cohort_cnvs(eng, p, rows, n, st, en, vals=vals, window=WINDOW, block_rows=a.block_rows)
            res["cohort_cnvs_wall_s"] = time.perf_counter() - t0
        finally:
            eng.device_free(p)
    (_, f, T, calls), (_, hf, hT, hcalls) = dev[-1], host[-1]
    res["resident"] = summary([d[0] for d in dev[2:]])
    res["host"] = summary([h[0] for h in host[2:]])
    res["host_over_resident"] = res["host"]["wall_s"] / res["resident"]["wall_s"]
    res["level"], res["cnvs"], res["members"] = T, int(len(calls["sample"])), int(len(calls["member_row"]))
    res["routes_identical"] = bool(T == hT == cT and f.tobytes() == hf.tobytes() == cf.tobytes()
                                   and all(calls[k].tobytes() == hcalls[k].tobytes() == ccalls[k].tobytes() for k in KEYS))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if res["routes_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
