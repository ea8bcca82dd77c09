#!/usr/bin/env python3
"""Time gd_perbase_runs at the size of a human chromosome 1 ("Measured").

    python tools/perbase_time.py [--length 248956422] [--coverage 30] [--cuts 1,4,100] [--limit 300] [--out FILE]

One contig of --length positions with goleft_amd.synth's short reads at --coverage, generated on the device and computed
once with the per-base vector kept.  gd_perbase_runs over the whole contig runs once cold and five times warm, without cuts
and with --cuts, all under one time limit (SIGALRM ends the process); gd_perbase_runs_timing's split of every run (count,
scan, emit, read-back), the number of runs, the bytes each kernel reads and writes and its GB/s are printed as one JSON
line.  The yardstick, in the same process and timed the same way (host clock around an enqueue and a synchronisation): a
device-to-device copy of the same per-base vector -- the rate a streaming kernel can reach on this box.  The runs of all
calls must agree; nothing is checked against the restatement at this size (the tests do that)."""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from goleft_amd import synth                                            # noqa: E402
from goleft_amd.engine import DepthEngine                               # noqa: E402

CHUNK = 4096                                                            # gd_perbase_runs.hpp PB_CHUNK


class _DevVec:
    """A device int32 array as torch takes it (zero copy)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=248956422)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--cuts", default="1,4,100")
    ap.add_argument("--limit", type=int, default=300, help="seconds for everything")
    ap.add_argument("--out")
    a = ap.parse_args()
    signal.alarm(a.limit)
    import torch
    dev = torch.device("cuda", 0)
    L = a.length
    n = synth.n_reads_for(L, a.coverage)
    eng = DepthEngine(0)
    eng.set_params()
    eng.set_contigs([L])
    t0 = time.perf_counter()
    eng.adopt_device(0, *synth.short_reads_torch(L, n, 20, dev))
    eng.compute()
    res = dict(length=L, reads=n, coverage=a.coverage, make_and_compute_s=round(time.perf_counter() - t0, 3))
    ptr, _ = eng.device_perbase(0)
    src = torch.as_tensor(_DevVec(int(ptr), L), device=dev)
    dst = torch.empty(L, dtype=torch.int32, device=dev)
    copies = []
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        copies.append(time.perf_counter() - t0)
    assert bool((dst == src).all())
    del dst
    copy_s = float(np.median(copies[1:]))
    res["copy"] = dict(cold_s=round(copies[0], 6), warm_median_s=round(copy_s, 6), bytes=8 * L, gbps=round(8 * L / copy_s / 1e9, 1),
                       read_gbps=round(4 * L / copy_s / 1e9, 1))
    n_chunks = (L + CHUNK - 1) // CHUNK
    for key, cuts in (("depth", None), ("quantized", [int(x) for x in a.cuts.split(",")])):
        runs, first = [], None
        for _ in range(6):
            t0 = time.perf_counter()
            s, v = eng.perbase_runs(0, 0, L, cuts)
            wall = time.perf_counter() - t0
            runs.append(dict(wall_s=round(wall, 6), **{k: round(x, 6) for k, x in eng.perbase_runs_timing().items()}))
            if first is None:
                first = (s, v)
            else:
                assert s.tobytes() == first[0].tobytes() and v.tobytes() == first[1].tobytes(), "the runs of two calls differ"
        k = int(first[0].shape[0])
        med = {f: float(np.median([r[f] for r in runs[1:]])) for f in runs[0]}
        by = dict(count=4 * L + 4 * n_chunks, scan=8 * n_chunks, emit=4 * L + 4 * n_chunks + 8 * k, readback=8 * k)
        res[key] = dict(cuts=cuts, runs=k, positions_per_run=round(L / max(k, 1), 2), cold=runs[0], warm_median=med, bytes=by,
                        gbps={f: round(by[f] / med[f + "_s"] / 1e9, 1) for f in by if med[f + "_s"] > 0},
                        count_vs_copy=round((by["count"] / med["count_s"]) / (8 * L / copy_s), 3),
                        emit_vs_copy=round((by["emit"] / med["emit_s"]) / (8 * L / copy_s), 3))
        del first, s, v
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
