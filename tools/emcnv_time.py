#!/usr/bin/env python3
"""Time gd_emcnv_* against what a caller did before it: gd_emdepth_cells with all four outputs read back, then a walk
of those arrays on the host ("Measured").

    python tools/emcnv_time.py [--rows 250000] [--samples 200] [--run 1|20|5000] [--out FILE]

The matrix is section 3.10's: integer cells at a 20 - 40x level per row, 2 % of the cells carrying a factor of
{0, 1/2, 1, 1 1/2, 2, 4}.  --run 1 draws the factor per cell, as 3.10 did (a member needs the same state in two rows
running, so there are few); --run 20 gives every factor to 20 rows of its sample running, which is what a CNV looks
like, and --run 5000 makes calls of thousands of sites.  Rows are 1000 wide, back to back.  Seven calls of each, the
first two left out, the median of the other five; every gd_emcnv_begin allocates its state anew.
The host walk is timed in two steps, both vectorised in numpy: the float64 log2, the states and the member mask; then
the joining of each column's members into runs with F from a binary search (which tiled rows allow).  That join leaves
out sample 0's rule, PSize and the members' values: the walk a caller needs costs at least the two together."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from goleft_amd import _lib                                             # noqa: E402


def matrix(rows, n, run, seed=310):
    rng = np.random.default_rng(seed)
    level = rng.uniform(20.0, 40.0, size=(rows, 1))
    cells = rng.poisson(level, size=(rows, n)).astype(np.float64)
    starts = rng.random((rows, n)) < 0.02 / run
    factor = np.where(starts, rng.choice([0, 0.5, 1, 1.5, 2, 4], size=(rows, n)), np.nan)
    if run > 1:                                  # a start holds for `run` rows of its column
        idx = np.where(starts, np.arange(rows)[:, None], -1)
        np.maximum.accumulate(idx, axis=0, out=idx)
        live = (idx >= 0) & (np.arange(rows)[:, None] - idx < run)
        factor = np.where(live, np.take_along_axis(factor, np.maximum(idx, 0), axis=0), np.nan)
    return np.floor(np.where(np.isnan(factor), cells, cells * factor)).astype(np.int64)


def median5(f):
    t = []
    for _ in range(7):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return float(np.median(t[2:])), [round(v, 6) for v in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=250000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--run", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows, n = a.rows, a.samples
    cells = matrix(rows, n, a.run)
    starts = (np.arange(rows, dtype=np.int64) * 1000).astype(np.uint32)
    ends = starts + np.uint32(1000)
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
    res = dict(rows=rows, samples=n, run=a.run)

    lam, it = np.empty((rows, 9)), np.empty(rows, np.uint8)
    cn, fc = np.empty((rows, n), np.uint8), np.empty((rows, n), np.float32)
    split = []

    def before():
        ok(lib.gd_emdepth_cells(h, p, rows, n, None, lam.ctypes.data, it.ctypes.data, cn.ctypes.data, fc.ctypes.data))
        t = (C.c_double * 3)()
        ok(lib.gd_emdepth_timing(h, t, 3))
        split.append(list(t))

    res["emdepth_cells_s"], res["emdepth_cells_all"] = median5(before)
    res["emdepth_cells_split_upload_kernel_readback"] = [float(np.median([s[k] for s in split[2:]])) for k in range(3)]
    res["emdepth_cells_bytes_back"] = int(lam.nbytes + it.nbytes + cn.nbytes + fc.nbytes)

    def walk():
        d = cells.astype(np.float32).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.log2(d / lam[:, 2:3])
        st = np.where(f >= 0.40, 1, np.where(f <= -0.80, 2, 0)).astype(np.uint8)
        up = np.vstack([st[:1], st[:-1]])
        return (st != 0) & (st == up)

    t0 = time.perf_counter()
    member = walk()
    res["host_member_mask_numpy_s"] = time.perf_counter() - t0
    res["member_share"] = float(member.mean())

    def join():
        cols, at = np.nonzero(member.T)                                  # by column, then by row
        first_gap = np.searchsorted(starts, ends.astype(np.int64) + 30000, side="left")
        new = np.ones(len(at), bool)
        new[1:] = ~((cols[1:] == cols[:-1]) & (first_gap[at[:-1]] > at[1:]))
        return int(new.sum())

    t0 = time.perf_counter()
    res["host_join_runs"] = join()
    res["host_join_numpy_s"] = time.perf_counter() - t0

    out, split = {}, []

    def after():
        ok(lib.gd_emcnv_begin(h, n))
        ok(lib.gd_emcnv_add_cells(h, p, rows, None, starts.ctypes.data, ends.ctypes.data, None))
        nc, nm = C.c_uint64(), C.c_uint64()
        ok(lib.gd_emcnv_finish(h, C.byref(nc), C.byref(nm)))
        nc, nm = nc.value, nm.value
        if out.get("cnvs") != nc or out.get("members") != nm:            # the caller's buffers: made once, like `cn` and `fc` above
            out["bufs"] = [np.empty(nc, np.uint32), np.empty(nc, np.uint32), np.empty(nc, np.uint32), np.empty(nc + 1, np.uint64),
                           np.empty(nm, np.uint32), np.empty(nm, np.float32), np.empty(nm, np.uint8), np.empty(nm, np.float32)]
        bufs = out["bufs"]
        ok(lib.gd_emcnv_read(h, *[b.ctypes.data for b in bufs]))
        t = (C.c_double * 4)()
        ok(lib.gd_emcnv_timing(h, t, 4))
        split.append(list(t))
        out.update(cnvs=nc, members=nm, bytes=int(sum(b.nbytes for b in bufs)), rows=bufs[4], sample=bufs[0], off=bufs[3])

    res["emcnv_s"], res["emcnv_all"] = median5(after)
    res["emcnv_split_upload_em_cnv_readback"] = [float(np.median([s[k] for s in split[2:]])) for k in range(4)]
    res.update(cnvs=out["cnvs"], members_in_cnvs=out["members"], emcnv_bytes_back=out["bytes"])
    # every member the device reports is a member of the host mask
    col = np.repeat(out["sample"], np.diff(out["off"]).astype(np.int64))
    res["members_agree_with_host_mask"] = bool(member[out["rows"], col].all())
    ok(lib.gd_emcnv_end(h))
    ok(lib.gd_device_free(h, p))
    lib.gd_destroy(h)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
