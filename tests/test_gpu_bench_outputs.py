"""-m gpu: a plain `bench.py` run (no --full) on config 2 (chr20) times exactly --steps steps, prints the line's contract
fields and nothing it needs extra runs for, and --dump-outputs writes what the last timed step computed: window sums,
minima, class runs and the per-base depth at the seeded positions, all equal to what the CPU oracle makes of the same
seeded records."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_what_the_oracle_computes(tmp_path):
    import bench
    from goleft_amd import synth
    from oracle import pyoracle as po

    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(H.ROOT, "bench.py"), "--gpus", "1", "--workload", "chr20",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "ref-bases/s" and d["dtype"] == "int32"
    assert d["higher_is_better"] is True and d["metric"] == "ref bases/sec per-base depth, 30x WGS synthetic"
    assert abs(d["value"] - d["config"]["total_ref_bases"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9
    for k in ("roofline", "kernels_ms", "first_compute", "cpu_baseline", "host_stream_scope", "bam_file_scope"):
        assert k not in d, k                                      # side measurements run with --full only

    L, W = synth.CHR20_LEN, 1000
    r = po.Reads(*synth.short_reads_numpy(L, synth.n_reads_for(L, 30.0), 20))
    want = po.tiled_contig_check(r, 1, L, W, 4, 0, po.step_for(W), 4)
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {"window_sums", "window_mins", "callable_runs", "perbase_sample"}
    assert got["window_sums"].dtype == np.float64 and np.array_equal(got["window_sums"], want["sums"])
    assert got["window_mins"].dtype == np.float32 and np.array_equal(got["window_mins"], want["mins"])
    runs = got["callable_runs"]
    assert np.array_equal(runs[:, 0], want["run_starts"]) and np.array_equal(runs[:, 2], want["run_cls"])
    assert runs[-1, 1] == L and np.array_equal(runs[1:, 0], runs[:-1, 1])
    pick = bench.sample_rows(L, bench.DUMP_SPEC["perbase_sample"][1], 4)
    depth = po.perbase_c(r, 1, 0, L)
    assert np.array_equal(got["perbase_sample"], depth[pick])
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_LIMIT_BYTES


@pytest.mark.parametrize("full", [False, True])
def test_the_clock_holds_exactly_the_timed_steps(full, monkeypatch, capsys):
    """A real run (engine, run_case, the line), in this process: the interval whose length gives `ms_per_step` holds
    exactly --steps computes -- not the warm-up, not the cold step or the profiled steps of --full.  A plain run computes
    nothing beyond warm-up + steps; --full adds the cold step and one profiled pass of --steps after the clock stops."""
    import time
    import bench
    from goleft_amd.engine import DepthEngine

    events = []
    real_compute, real_clock = DepthEngine.compute, time.perf_counter

    def compute(self):
        events.append(("c", None))
        return real_compute(self)

    def clock():
        t = real_clock()
        events.append(("t", t))
        return t

    N, W = 4, 2
    argv = ["bench.py", "--gpus", "1", "--workload", "chr20", "--steps", str(N), "--warmup", str(W)]
    if full:
        argv += ["--full", "--no-cpu-baseline", "--no-host-stream", "--emulate-shards="]
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", argv)
    monkeypatch.setattr(DepthEngine, "compute", compute)
    monkeypatch.setattr(time, "perf_counter", clock)
    bench.main()
    monkeypatch.undo()
    d = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == N and d["warmup"] == W
    n_compute = sum(1 for e in events if e[0] == "c")
    assert n_compute == (1 + W + 2 * N if full else W + N), events
    clocked = [(i, t) for i, (k, t) in enumerate(events) if k == "t"]
    spans = [(i, j) for a, (i, ti) in enumerate(clocked) for (j, tj) in clocked[a + 1:]
             if (tj - ti) / N * 1e3 == d["ms_per_step"]]
    assert len(spans) == 1, spans                      # the one interval bench.py divided by --steps
    i, j = spans[0]
    assert sum(1 for k, _ in events[i:j] if k == "c") == N
    assert sum(1 for k, _ in events[:i] if k == "c") == (1 + W if full else W)
