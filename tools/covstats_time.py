"""Times `goleft-depth covstats` on synth-bam files (SYNTH_BAM_AUX=1: mate fields, TLEN, duplicate flags, tags).

    python tools/covstats_time.py [--lengths L1,L2,...] [--cov 30] [--files 3] [--dir DIR]

Writes --files synthetic BAMs of the given contig lengths at --cov (BGZF level 6) unless they exist, then runs
covstats on one file and on all of them in one invocation, with GOLEFT_COVSTATS_TIMING=1, and prints one JSON line
per run: wall seconds per BAM and the split the CLI reports (member listing, begin + feed, decode = waiting for the
read and inflate + walk + scan + histograms, histogram read-back, host finish).  Measurement only."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
SYNTH = os.path.join(ROOT, "goleft_amd", "synth-bam")


def make(path, lengths, cov, seed):
    if os.path.exists(path) and os.path.exists(path + ".bai"):
        return
    env = dict(os.environ, SYNTH_BAM_AUX="1", SYNTH_BAM_LEVEL="6")
    subprocess.run([SYNTH, path, "chrS", lengths, str(cov), str(seed), "16"], check=True, env=env, capture_output=True)
    from tests import covstats_ref as R
    R.add_pseudo_bins(path)


def run(bams):
    env = dict(os.environ, GOLEFT_COVSTATS_TIMING="1")
    t0 = time.perf_counter()
    r = subprocess.run([EXE, "covstats"] + bams, capture_output=True, text=True, env=env, timeout=900)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit("covstats failed: %s" % r.stderr)
    per = [json.loads(ln) for ln in r.stderr.splitlines() if ln.startswith('{"bam"')]
    split = [json.loads(ln) for ln in r.stderr.splitlines() if ln.startswith('{"total_s"')]
    return dict(n_bams=len(bams), process_wall_s=round(wall, 4), per_bam_s=[p["wall_s"] for p in per],
                split=split[0] if split else None, rows=r.stdout.splitlines()[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="60000000,40000000")
    ap.add_argument("--cov", type=float, default=30)
    ap.add_argument("--files", type=int, default=3)
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "covstats_time"),
                    help="where the synthetic BAMs are written (and reused when present)")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    t0 = time.perf_counter()
    bams = [os.path.join(a.dir, "s%d.bam" % k) for k in range(a.files)]
    for k, b in enumerate(bams):
        make(b, a.lengths, a.cov, 100 + k)
    print(json.dumps(dict(generate_s=round(time.perf_counter() - t0, 1), bytes=[os.path.getsize(b) for b in bams])), flush=True)
    print(json.dumps(dict(run="one", **run(bams[:1]))), flush=True)
    print(json.dumps(dict(run="one_again", **run(bams[:1]))), flush=True)
    print(json.dumps(dict(run="all", **run(bams))), flush=True)


if __name__ == "__main__":
    main()
