"""Times `goleft-depth indexcov` on synthetic human-shaped cohorts of .bai files.

    python tools/indexcov_time.py [--samples 30,500,2500] [--tiles 190000] [--dir DIR] [--extra-normalize]

Writes N .bai files over 24 references (22 autosomes, X, Y; --tiles 16 384-base tiles in all, shared structure, half the
samples at half depth on X) unless they exist, runs the CLI once per N with the page cache warm (the files were just
written) and GOLEFT_INDEXCOV_TIMING=1, and prints one JSON line per run: process wall seconds and the split the CLI
reports (index reading, upload, device kernels, read-back, -n, eigen-solver, text, BGZF).  Measurement only; the
per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- goleft-depth indexcov ...` run."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
# GRCh37 chromosome lengths in megabases, 1 .. 22, X, Y: the shares of the tiles
MB = [249, 243, 198, 191, 181, 171, 159, 146, 141, 136, 135, 134, 115, 107, 103, 90, 81, 78, 59, 63, 48, 51, 155, 59]
NAMES = [str(i) for i in range(1, 23)] + ["X", "Y"]


def make(d, n, tiles):
    from tests import indexcov_ref as R
    rng = np.random.default_rng(7)
    per = [max(3, int(tiles * m / sum(MB))) for m in MB]
    shape = [rng.integers(20000, 90000, t).astype(np.float64) for t in per]
    for sh in shape[:22]:
        sh[len(sh) // 3:len(sh) // 3 + len(sh) // 40] = 0                    # a centromere
    fai = os.path.join(d, "ref.fai")
    with open(fai, "w") as f:
        off = 10
        for c, t in zip(NAMES, per):
            f.write("%s\t%d\t%d\t60\t61\n" % (c, t * 16384, off))
            off += t * 16384 + 100
    paths = []
    for s in range(n):
        p = os.path.join(d, "s%05d.bai" % s)
        paths.append(p)
        if os.path.exists(p):
            continue
        scale = rng.uniform(0.5, 2.0)
        refs, at = [], 1 << 20
        for r, t in enumerate(per):
            v = shape[r] * scale * rng.uniform(0.9, 1.1, t)
            if r >= 22 and s % 2:
                v = v * (0.5 if r == 22 else 0.01)
            iv = np.concatenate([[at], at + np.cumsum(v.astype(np.int64))]).astype(np.uint64)
            at = int(iv[-1]) + 4096
            refs.append((iv, (int(v.sum()) // 300, s)))
        R.write_bai(p, refs)
    return paths, fai


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="30,500,2500")
    ap.add_argument("--tiles", type=int, default=190000)
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "indexcov_time"))
    ap.add_argument("--extra-normalize", action="store_true")
    ap.add_argument("--timeout", type=int, default=3000)
    a = ap.parse_args()
    for n in [int(x) for x in a.samples.split(",")]:
        d = os.path.join(a.dir, "n%d" % n)
        os.makedirs(d, exist_ok=True)
        t0 = time.perf_counter()
        paths, fai = make(d, n, a.tiles)
        gen = time.perf_counter() - t0
        env = dict(os.environ, GOLEFT_INDEXCOV_TIMING="1")
        t0 = time.perf_counter()
        r = subprocess.run([EXE, "indexcov", "-d", os.path.join(d, "out"), "-f", fai] + (["-n"] if a.extra_normalize else []) + paths,
                           capture_output=True, text=True, env=env, timeout=a.timeout)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            sys.exit("indexcov failed: %s" % r.stderr[-2000:])
        split = [json.loads(ln) for ln in r.stderr.splitlines() if ln.startswith('{"samples"')]
        bed = os.path.join(d, "out", "out-indexcov.bed.gz")
        print(json.dumps(dict(samples=n, generate_s=round(gen, 1), process_wall_s=round(wall, 3), bed_gz_bytes=os.path.getsize(bed),
                              split=split[0] if split else None)), flush=True)


if __name__ == "__main__":
    main()
