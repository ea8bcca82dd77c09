"""CPU: the bench line the driver parses.  The latest committed bench line (profiles/r*_bench_wgs_n1.json,
written by `bench.py --full` on an MI355X) must carry every field of the contract, with BASELINE.json's metric."""
import glob
import json
import os

from tests import helpers as H


def _latest(pattern):
    files = sorted(glob.glob(os.path.join(H.ROOT, "profiles", pattern)))
    assert files, pattern
    return json.load(open(files[-1]))


def test_wgs_bench_line_has_the_contract_fields():
    d = _latest("r*_bench_wgs_n1.json")
    base = json.load(open(os.path.join(H.ROOT, "BASELINE.json")))
    assert d["metric"].split(",")[0] in base["metric"].replace("×", "x")
    for k, t in (("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                 ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str)):
        assert isinstance(d[k], t), k
    assert d["vs_baseline"] is None and base["published"] == {}          # no published number for this metric
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["scaling"] in ("weak", "strong")
    assert d["data"] == "synthetic" and d["dtype"] == "int32"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic"] is None or r["traffic"] > 0
    # achieved = algorithmic bytes per launch / average launch duration of the dominant kernel
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["avg_kernel_ms"] * 1e-3) / 1e9) / r["achieved"] < 1e-6
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == d["unit"] and c["sample"]
    # whole-job throughput: the units of one step over its duration
    assert abs(d["value"] - d["config"]["total_ref_bases"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    assert d["value"] >= 1e9                                            # BASELINE.json's target at one GPU
    # round 3: the step starts from the records as they crossed the ABI; what round 2 called `value` is a side field
    assert "as they arrived" in d["config"]["step"] and d["roofline"]["kernel"].endswith("<raw>")
    # round 4: the roofline is on SURVEY.md 8(d)'s byte count; the cold step and the BAM-file scope are in the line
    assert abs(d["roofline"]["frac_survey_8d"] - d["roofline"]["frac"]) < 1e-12
    assert d["roofline"]["frac_bytes_really_read"] > d["roofline"]["frac"]
    f = d["first_compute"]
    # (1.04 on a box whose result arrays were allocated in half a millisecond, 1.13-1.16 on boxes where that allocation waited
    # three seconds for the driver to clear what the process before had released -- prepare_alloc_ms, reported beside it --
    # and the clearing went on under the compute: profiles/r12i_, r12s_bench_wgs_n1.json)
    assert f["reruns"] == 0 and f["ratio_to_warm"] <= 1.25 and f["lookback"] == 192
    assert d["ranks_seen"] == 1 and d["distinct_devices"] == 1
    b = d["bam_file_scope"]
    # (BAM file -> BED at genome size: 1.02 - 1.06e9 ref-bases/s on three boxes of the round, 6.8e8 on one whose page-cache
    # reads and device allocations ran at half speed -- profiles/README.md; the line must carry the measurement, the claim
    # is DESIGN.md's)
    assert b["file"] == "genome" and b["value"] >= 5e8 and b["outputs_identical"] is True
    e = d["emulated_sharding"]["by_n_gpus"]
    assert set(e) == {"2", "4", "8"} and all(len(e[n]["per_shard_ms"]) == int(n) for n in e)
    assert e["8"]["projected_speedup"] >= 6.0                           # north_star: >= 6x aggregate at 8 GPUs
    for k in ("host_stream_scope", "host_stream_scope_wgs"):
        assert set(d[k]["variants"]) == {"push", "in_place"} and d[k]["value"] > 3e9
    # round 5: BASELINE.json's configs 2, 4 and 5 ride in the same line, each with its cold step and its own roofline
    ow = d["other_workloads"]
    assert set(ow) == {"chr20", "ont", "cohort"}
    for name, cfg, kernel in (("chr20", 2, "gd_tile_fast_kernel<raw>"), ("cohort", 4, "gd_sums_stream_kernel<raw>"),
                              ("ont", 5, "gd_dels_raw_kernel + gd_ltile2_kernel (the inclusive step)")):
        w = ow[name]
        assert "error" not in w, (name, w.get("error"))
        assert w["baseline_config"] == cfg and w["unit"] == "ref-bases/s" and w["roofline"]["kernel"] == kernel
        r = w["roofline"]
        assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["avg_kernel_ms"] * 1e-3) / 1e9) / r["achieved"] < 1e-6
        assert abs(w["value"] - w["total_ref_bases"] / (w["ms_per_step"] * 1e-3)) / w["value"] < 1e-6
        assert w["first_compute"]["ms"] > 0 and w["first_compute"]["reruns"] == 0 and w["value_first_compute"] > 0
        assert w["value"] >= 1e9                                        # every config clears BASELINE.json's 1-GPU target
    assert sum(w["seconds_in_bench"] for w in ow.values()) < 60
    assert ow["ont"]["kernels_ms"]["long_read_structures"] > 0 and ow["ont"]["device_path"] == "chunk"
    # round 6: the long-read roofline is on SURVEY 8(d)'s ORIGINAL op count over the inclusive step, each
    # of the two kernels' own figures a sub-key; every roofline also says what fraction of the ACHIEVABLE rate it is
    ro = ow["ont"]["roofline"]
    assert ro["cigar_ops_counted"] == ow["ont"]["cigar_ops"] and abs(ro["avg_kernel_ms"] - ow["ont"]["ms_per_step"]) < 1e-9
    assert set(ro["kernels"]) == {"gd_dels_raw_kernel", "gd_ltile2_kernel"} and ro["kernels"]["gd_ltile2_kernel"]["cigar_ops_counted"] < ro["cigar_ops_counted"]
    assert abs(d["roofline"]["frac_of_achievable"] - d["roofline"]["achieved"] / 6290.0) < 1e-9
    # ... and the genome as an aligner leaves it is in the driver's line
    g6 = b["genome_libdeflate6_aux_tags"]
    assert g6["oracle_identical"] is True and g6["ref_bases"] == 3095677412 and g6["wall_s"] > 0 and "level 6" in g6["deflate"]
    assert d["cpu_baseline"]["reference_pipeline"] is not None
    # ... the BAM-file scope is checked against the ORACLE (not only decoder against decoder), on records as an aligner leaves
    # them too, and holds the reference's own timed invocation
    assert b["oracle_identical"] is True and b["oracle_bed_sha256"] == b["bed_sha256"]
    assert set(b["variants"]) == {"libdeflate1_short_records", "libdeflate6_aux_tags"}
    for v in b["variants"].values():
        assert v["outputs_identical"] is True and v["oracle_identical"] is True and v["device_wall_s"] < v["host_wall_s"]
    assert "tags" in b["variants"]["libdeflate6_aux_tags"]["records"] and "level 6" in b["variants"]["libdeflate6_aux_tags"]["deflate"]
    pi = b["paper_invocation"]
    assert pi["oracle_identical"] is True and 0 < b["paper_invocation_s"] == pi["wall_s"] < 2.0 and pi["ref_bases"] == 249250621


def test_product_never_uses_the_oracle():
    """The oracle is test infrastructure: nothing under goleft_amd/ (Python, C++, HIP, Makefile) may import,
    include, link or execute anything under oracle/ -- comments that cite it aside."""
    import re
    bad = []
    for dirpath, _, files in os.walk(os.path.join(H.ROOT, "goleft_amd")):
        for f in files:
            if not f.endswith((".py", ".cpp", ".hpp", ".hip", ".inc", ".h")) and f != "Makefile":
                continue
            for n, line in enumerate(open(os.path.join(dirpath, f), errors="replace"), 1):
                code = re.sub(r"(//|#(?!include)).*$", "", line) if not f.endswith(".py") else re.sub(r"#.*$", "", line)
                if re.search(r"\boracle\b", code) and not code.lstrip().startswith(("*", '"""')):
                    if re.search(r"import|include|dlopen|CDLL|-l|\.so|subprocess", code):
                        bad.append("%s:%d: %s" % (os.path.relpath(os.path.join(dirpath, f), H.ROOT), n, line.strip()))
    assert not bad, bad


def test_genome_bed_of_the_bench_line_is_the_oracles():
    """bam_file_scope: the SHA-256 pair of the BED files the CLI wrote for the genome-sized synthetic BAM on the MI355X
    equals what the ORACLE makes of the same records (tests/golden/synth_bam_expected.json: oracle/synthbam.py's twin of the
    generator's record function -> oracle/depth_oracle.c -> the restated callback, computed on the CPU by
    tools/expected_bed_sha.py) -- file -> BED at BASELINE.json's full size is checked against the oracle, not only
    against the product's other decoder."""
    d = _latest("r*_bench_wgs_n1.json")
    b = d["bam_file_scope"]
    exp = json.load(open(os.path.join(H.ROOT, "tests", "golden", "synth_bam_expected.json")))
    assert b["file"] == "genome" and b["bed_sha256"] == exp["genome:cov30:seed20:w1000"]["bed_sha256"]
    assert exp["genome:cov30:seed20:w1000"]["rows"][0] == 3095689          # one depth row per 1 kb window of hg19's 24 contigs


def test_reference_children_hook_runs_with_a_samtools_on_path(tmp_path, monkeypatch):
    """BASELINE.md section 3 / VERDICT r5 item 5: where a samtools exists, bench.py times the reference's own children
    (`samtools depth -Q q -d 2500 -r chr:s-e bam`, depth/depth.go:45) by itself.  Here: a stand-in executable that answers
    `--version` and `depth` the way samtools does (there is none in this image); the repository's own shim is not taken for one."""
    import importlib
    import stat
    bench = importlib.import_module("bench")
    fake = tmp_path / "samtools"
    fake.write_text("#!/bin/sh\nif [ \"$1\" = --version ]; then echo 'samtools 9.9-standin'; exit 0; fi\n"
                    "r=$7; echo \"$r\" >&2; printf 'chrS\\t1\\t3\\nchrS\\t2\\t4\\n'\n")
    fake.chmod(fake.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setenv("PATH", str(tmp_path) + os.pathsep + os.environ.get("PATH", ""))
    monkeypatch.delenv("SAMTOOLS", raising=False)
    st = bench.real_samtools()
    assert st and st[0] == str(fake) and "standin" in st[1]
    out = bench.reference_children(st[0], "x.bam", [("chrS", 25_000_000)], 1000, 1, 2)
    assert out["kind"] == "reference" and out["cores"] == 2 and out["value"] > 0 and out["text_bytes"] == 3 * 18
    assert "3 tiles" in out["sample"]
    monkeypatch.setenv("SAMTOOLS", os.path.join(bench.ROOT, "goleft_amd", "shim", "samtools"))
    assert bench.real_samtools() is None


def test_dumped_outputs_fit_the_limit_and_their_samples_are_fixed():
    """--dump-outputs: the arrays one run can write stay under 64 MB together, and a sampled output keeps the same rows
    in every run (a generator seeded by the output's shape)."""
    import importlib
    import numpy as np
    bench = importlib.import_module("bench")
    size = {k: np.dtype(t).itemsize * n for k, (t, n) in bench.DUMP_SPEC.items()}
    runs = {"window_sums", "window_mins", "callable_runs"}
    for case in (runs | {"perbase_sample"}, runs | {"depthwed"}, {"window_sums", "depthwed"},
                 {"window_sums", "window_mins", "run_bounds"}):
        assert sum(size[k] for k in case) <= bench.DUMP_LIMIT_BYTES <= 64_000_000, case
    assert bench.sample_rows(1000, 1000, 1) is None
    a, b = bench.sample_rows(3_095_677_412, 1_000_000, 4), bench.sample_rows(3_095_677_412, 1_000_000, 4)
    assert np.array_equal(a, b) and len(a) == 1_000_000 and np.all(a[1:] >= a[:-1]) and a[-1] < 3_095_677_412
    name, arr = bench._dump_entry("callable_runs", np.arange(3 * 400_000, dtype=np.int32).reshape(-1, 3), 3, 3)
    assert arr.dtype == np.float64 and arr.shape == (bench.DUMP_SPEC["callable_runs"][1] // 3, 3)
