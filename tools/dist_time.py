#!/usr/bin/env python3
"""Time gd_depth_hist and gd_region_bins at the size of a human chromosome 1 ("Measured").

    python tools/dist_time.py [--length 248956422] [--coverage 30] [--cuts 1,10,20,30] [--regions 200000] [--region-length 150]
                              [--limit 300] [--out FILE]

One contig of --length positions with goleft_amd.synth's short reads at --coverage, generated on the device and computed
once with the per-base vector kept; then a contig of the same size without a read (every position at depth 0: the worst
case for contention on one LDS counter).  Every call runs once cold and five times warm under one time limit (SIGALRM ends
the process), and the median of the warm calls' split (gd_dist_timing: upload, kernel, read-back) is reported with the
bytes the kernel reads and its GB/s, as one JSON line:
  hist         gd_depth_hist over the whole contig, 65536 bins; on the empty contig too, with the ratio of the kernel times
  region_bins  gd_region_bins with --cuts for --regions regions of --region-length positions at random places, and for one
               region that is the whole contig
The yardstick, in the same process and timed the same way (host clock around an enqueue and a synchronisation): a
device-to-device copy of the same per-base vector, which moves 8 bytes a position where the histogram reads 4.  The numbers
of all calls must agree; nothing is checked against the restatement at this size (the tests do that)."""
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

CHUNK = 4096                                                            # gd_depth_hist.hpp DH_CHUNK


class _DevVec:
    """A device int32 array as torch takes it (zero copy)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 2}


def timed(eng, call):
    """(cold split, median warm split, the result): six calls, all results equal."""
    runs, first = [], None
    for _ in range(6):
        t0 = time.perf_counter()
        got = call()
        wall = time.perf_counter() - t0
        runs.append(dict(wall_s=round(wall, 6), **{k: round(x, 6) for k, x in eng.dist_timing().items()}))
        blob = b"".join(np.asarray(x).tobytes() for x in (got if isinstance(got, tuple) else (got,)))
        if first is None:
            first, result = blob, got
        else:
            assert blob == first, "the numbers of two calls differ"
    return runs[0], {f: float(np.median([r[f] for r in runs[1:]])) for f in runs[0]}, result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=248956422)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--cuts", default="1,10,20,30")
    ap.add_argument("--regions", type=int, default=200000)
    ap.add_argument("--region-length", type=int, default=150)
    ap.add_argument("--limit", type=int, default=300, help="seconds for everything")
    ap.add_argument("--out")
    a = ap.parse_args()
    signal.alarm(a.limit)
    import torch
    dev = torch.device("cuda", 0)
    L = a.length
    cuts = [int(x) for x in a.cuts.split(",")]
    n = synth.n_reads_for(L, a.coverage)
    res = dict(length=L, reads=n, coverage=a.coverage)

    eng = DepthEngine(0)
    eng.set_params()
    eng.set_contigs([L])
    t0 = time.perf_counter()
    eng.adopt_device(0, *synth.short_reads_torch(L, n, 20, dev))
    eng.compute()
    res["make_and_compute_s"] = round(time.perf_counter() - t0, 3)
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
    del dst, src
    copy_s = float(np.median(copies[1:]))
    res["copy"] = dict(cold_s=round(copies[0], 6), warm_median_s=round(copy_s, 6), bytes=8 * L, gbps=round(8 * L / copy_s / 1e9, 1),
                       read_gbps=round(4 * L / copy_s / 1e9, 1))

    n_chunks = (L + CHUNK - 1) // CHUNK
    cold, med, (bins, total, lo, hi) = timed(eng, lambda: eng.depth_hist(0, 0, L, 65536))
    assert int(bins.sum()) == L
    res["hist"] = dict(cold=cold, warm_median=med, bytes=4 * L + 4 * n_chunks, gbps=round((4 * L + 4 * n_chunks) / med["kernel_s"] / 1e9, 1),
                       kernel_vs_copy_time=round(med["kernel_s"] / copy_s, 3), mean_depth=round(total / L, 2), min=lo, max=hi,
                       nonzero_bins=int(np.count_nonzero(bins)))
    hist_kernel_s = med["kernel_s"]

    rng = np.random.default_rng(11)
    starts = np.sort(rng.integers(0, L - a.region_length, size=a.regions)).astype(np.int64)
    tids = np.zeros(a.regions, np.int32)
    cold, med, rows = timed(eng, lambda: eng.region_bins(tids, starts, starts + a.region_length, cuts))
    assert (rows.sum(axis=1) == a.region_length).all()
    # a region of 150 positions at a random alignment lies in one chunk, or in two: the table's entries, 4096 lanes each
    res["region_bins_many"] = dict(regions=a.regions, region_length=a.region_length, cuts=cuts, cold=cold, warm_median=med,
                                   positions=a.regions * a.region_length,
                                   ns_per_region=round(med["kernel_s"] / a.regions * 1e9, 2))
    cold, med, row = timed(eng, lambda: eng.region_bins(0, 0, L, cuts))
    assert int(row.sum()) == L
    res["region_bins_whole"] = dict(cuts=cuts, cold=cold, warm_median=med, bytes=4 * L + 4 * n_chunks,
                                    gbps=round((4 * L + 4 * n_chunks) / med["kernel_s"] / 1e9, 1),
                                    kernel_vs_copy_time=round(med["kernel_s"] / copy_s, 3))
    eng.close()

    eng = DepthEngine(0)                                                # the same size without a read
    eng.set_params()
    eng.set_contigs([L])
    eng.compute()
    cold, med, (bins, total, lo, hi) = timed(eng, lambda: eng.depth_hist(0, 0, L, 65536))
    assert int(bins[0]) == L and (total, lo, hi) == (0, 0, 0)
    res["hist_no_reads"] = dict(cold=cold, warm_median=med, gbps=round((4 * L + 4 * n_chunks) / med["kernel_s"] / 1e9, 1),
                                kernel_vs_30x=round(med["kernel_s"] / hist_kernel_s, 3))
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
