#!/usr/bin/env python3
"""Device BGZF inflate (gd_inflate_bgzf) against zlib on a synthetic BAM: correctness + kernel time."""
import os
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from goleft_amd.engine import DepthEngine, K_INFLATE

length = sys.argv[1] if len(sys.argv) > 1 else "10000000"      # one contig length, or several separated by commas
# GD_OPT_INFLATE_KERNEL values to time: 0 = a lane per member (the default), 1 = a workgroup per member (round 6)
probes = [int(x) for x in os.environ.get("INFLATE_BENCH_KERNELS", "0,1").split(",")]
path = "/tmp/gd_inflate_test.bam"
subprocess.check_call([os.path.join(ROOT, "goleft_amd", "synth-bam"), path, "chr20", length, "30", "20"],
                      stdout=subprocess.DEVNULL)
data = open(path, "rb").read()


def zlib_bgzf(raw):
    """The members of a BGZF byte string inflated with Python's zlib (the yardstick)."""
    out, off = [], 0
    while off < len(raw):
        xlen, = struct.unpack_from("<H", raw, off + 10)
        bsize, = struct.unpack_from("<H", raw, off + 16)          # synth-bam writes BC as the only subfield
        out.append(zlib.decompress(raw[off + 12 + xlen:off + bsize + 1 - 8], -15))
        off += bsize + 1
    return b"".join(out)


t0 = time.perf_counter()
want = None if os.environ.get("INFLATE_BENCH_NO_ZLIB") else zlib_bgzf(data)      # (counter passes: the yardstick ran in the trace pass)
t_cpu = time.perf_counter() - t0
with DepthEngine(0) as eng:
    eng.set_profiling(True)
    eng.inflate_bgzf(data[:1 << 20] if False else data)          # warm-up (allocations, code load)
    for probe in probes:
        eng.set_option(20, probe)                                # GD_OPT_INFLATE_KERNEL
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            got, status = eng.inflate_bgzf(data)
            t_all = time.perf_counter() - t0
            ms = eng.kernel_ms(K_INFLATE)
            best = ms if best is None else min(best, ms)
        ms = best
        print("kernel %d: members %d, %.1f MB -> %.1f MB; status ok %s; equal %s" % (probe, len(status), len(data) / 1e6, len(got) / 1e6,
                                                                                   bool((status == 0).all()), None if want is None else got == want))
        print("   kernel %.2f ms = %.2f GB/s of output (%.2f GB/s of BGZF); python zlib 1 thread %.2f s; call incl. H2D/D2H %.3f s"
              % (ms, len(got) / ms / 1e6, len(data) / ms / 1e6, t_cpu, t_all), flush=True)
os.unlink(path)
