"""Times `goleft-depth indexcov` on a cohort of copies of the reference's long-read .crai fixture.

    python tools/crai_time.py [--samples 200] [--dir DIR]

Copies tests/golden/ref/viral.crai N times (s00000.crai ...), runs the CLI once with GOLEFT_INDEXCOV_TIMING=1 and the page
cache warm, and prints one JSON line: process wall seconds, the split the CLI reports (crai_read_s: inflate + parse, summed
over the files -- eight reader threads share it; crai_tile_s: upload, the two device passes and read-back of
gd_crai_sizes; index_read_s: the wall clock of the reading phase), and for comparison the seconds the Python restatement
of makeSizes (tests/crai_ref.py) takes for the same slices on one host thread.  Measurement only."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
GOLD = os.path.join(ROOT, "tests", "golden", "ref")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "crai_time"))
    ap.add_argument("--timeout", type=int, default=600)
    a = ap.parse_args()
    from tests import crai_ref as R
    os.makedirs(a.dir, exist_ok=True)
    paths = []
    for s in range(a.samples):
        paths.append(os.path.join(a.dir, "s%05d.crai" % s))
        if not os.path.exists(paths[-1]):
            shutil.copyfile(os.path.join(GOLD, "viral.crai"), paths[-1])
    env = dict(os.environ, GOLEFT_INDEXCOV_TIMING="1")
    t0 = time.perf_counter()
    r = subprocess.run([EXE, "indexcov", "-d", os.path.join(a.dir, "out"), "-f", os.path.join(GOLD, "viral.fa.fai")] + paths,
                       capture_output=True, text=True, env=env, timeout=a.timeout)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit("indexcov failed: %s" % r.stderr[-2000:])
    split = [json.loads(ln) for ln in r.stderr.splitlines() if ln.startswith('{"samples"')]
    refs = R.read_index(paths[0])
    t0 = time.perf_counter()
    tiles = sum(len(R.make_sizes(sl)[0]) for sl in refs)
    one = time.perf_counter() - t0
    print(json.dumps(dict(samples=a.samples, process_wall_s=round(wall, 3), split=split[0] if split else None,
                          tiles_per_sample=tiles, restatement_tile_s=round(one * a.samples, 3))), flush=True)


if __name__ == "__main__":
    main()
