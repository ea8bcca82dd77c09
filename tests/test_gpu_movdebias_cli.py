"""GPU: `goleft-depth debias --moving W`, `goleft-depth emdepth --gc-moving W` and goleft_amd.emdepth.cohort_cnvs(moving=W)
on the 9-sample, 40-row matrix of tests/test_gpu_debias_cli.py: the debiased text against the restatement of dcnv's
GeneralDebiaser (tests/movdebias_ref.py), the one-call forms byte for byte against the two-step ones.  Every call runs under
its own timeout; nothing is retried."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import debias_ref as DR
from tests import movdebias_ref as MR
from tests import test_gpu_debias_cli as DC

pytestmark = pytest.mark.gpu

W = 9
LEVEL = "60"


def tied_vals():
    return np.round(DC.vals(), 2)                # five values, eight rows each: the order among them is by row


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("movdebias")
    plain, gc, tied = d / "m.bed", d / "gc.txt", d / "tied.txt"
    plain.write_text(DC.matrix_text(DC.cli_cells()))
    gc.write_text("".join("%r\n" % float(v) for v in DC.vals()))
    tied.write_text("".join("%r\n" % float(v) for v in tied_vals()))
    return d, str(plain), str(gc), str(tied)


def want_text(vals, window):
    out, _ = MR.debias(DC.cli_cells().astype(np.float32), vals, window)
    assert np.isfinite(out).all()
    return DR.matrix_text(DC.HEADER, [DC.where(i) for i in range(DC.ROWS)], out)


def test_debias_moving_writes_the_restatements_text(files):
    d, plain, gc, tied = files
    p = DC.run("debias", ["--gc-values", gc, "--moving", "9", plain], {"GOLEFT_EMDEPTH_TIMING": "1"})
    assert p.returncode == 0, p.stderr
    assert p.stdout == want_text(DC.vals(), 9)
    assert '"debias_kernels_s"' in p.stderr
    p = DC.run("debias", ["--moving=9", "--gc-values=" + tied, plain])
    assert p.returncode == 0 and p.stdout == want_text(tied_vals(), 9), p.stderr
    for w in (1, 3, 79):                         # (79: mid = 40 rows, one partial window for the whole matrix)
        p = DC.run("debias", ["--gc-values", gc, "--moving", str(w), plain])
        assert p.returncode == 0 and p.stdout == want_text(DC.vals(), w), (w, p.stderr)
    # the chunk debiaser is what it was
    p = DC.run("debias", ["--gc-values", gc, plain])
    assert p.returncode == 0 and p.stdout == DC.expected()[0], p.stderr
    from goleft_amd import emdepth
    out = str(d / "deb.bed")
    assert emdepth.Debias(["--gc-values", gc, "--moving", "9", plain], out_path=out) == 0
    with open(out) as f:
        assert f.read() == want_text(DC.vals(), 9)


def test_emdepth_gc_moving_is_debias_moving_then_normalize(files):
    d, plain, gc, tied = files
    deb, c1, c2 = d / "deb2.bed", str(d / "c1.tsv"), str(d / "c2.tsv")
    p = DC.run("debias", ["--gc-values", gc, "--moving", "9", plain])
    assert p.returncode == 0, p.stderr
    deb.write_text(p.stdout)
    two = DC.run("emdepth", ["--normalize", "--level", LEVEL, "--cnvs", c2, str(deb)])
    assert two.returncode == 0, two.stderr
    one = DC.run("emdepth", ["--gc-values", gc, "--gc-moving", "9", "--level", LEVEL, "--cnvs", c1, plain])
    assert one.returncode == 0, one.stderr
    assert one.stdout == two.stdout and one.stdout.startswith(DC.HEADER + "\n")
    with open(c1) as a, open(c2) as b:
        calls = a.read()
        assert calls == b.read() and calls.startswith("#sample\t")
    # blocks of rows change nothing
    p = DC.run("emdepth", ["--gc-values", gc, "--gc-moving=9", "--level", LEVEL, plain], {"GOLEFT_EMDEPTH_ROWS": "7"})
    assert p.returncode == 0 and p.stdout == one.stdout, p.stderr


def test_cohort_cnvs_moving_is_the_command_lines(files):
    from goleft_amd import emdepth
    from goleft_amd.engine import DepthEngine
    d, plain, gc, tied = files
    calls = d / "calls.tsv"
    run = DC.run("emdepth", ["--gc-values", gc, "--gc-moving", "9", "--level", LEVEL, "--cnvs", str(calls), plain])
    assert run.returncode == 0, run.stderr
    cells = np.ascontiguousarray(DC.cli_cells(), np.int64)
    st = np.array([(i % 25) * 1000 for i in range(DC.ROWS)], np.uint32)
    en = st + np.uint32(1000)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    with DepthEngine(0) as eng:
        p = eng.device_alloc(cells.nbytes)
        try:
            assert hip.hipMemcpy(p, cells.ctypes.data, cells.nbytes, 1) == 0           # hipMemcpyHostToDevice
            _, _, got = emdepth.cohort_cnvs(eng, p, DC.ROWS, DC.N, st, en, vals=DC.vals(), moving=9, level=float(LEVEL),
                                            site_cn=True)
            assert run.stdout == DC.matrix_text(got["site_cn"])
            mine = list(zip(got["sample"].tolist(), np.diff(got["member_off"]).astype(np.int64).tolist()))
            lines = calls.read_text().split("\n")
            assert lines[0].startswith("#sample\t") and lines[-1] == ""
            assert [(int(f[1]), int(f[3])) for f in (ln.split("\t") for ln in lines[1:-1])] == mine
            # window and moving exclude each other; moving needs the covariate; the default path is what it was
            with pytest.raises(ValueError, match="exclude"):
                emdepth.cohort_cnvs(eng, p, DC.ROWS, DC.N, st, en, vals=DC.vals(), window=0.01, moving=9)
            with pytest.raises(ValueError, match="covariate"):
                emdepth.cohort_cnvs(eng, p, DC.ROWS, DC.N, st, en, moving=9)
            a = emdepth.cohort_cnvs(eng, p, DC.ROWS, DC.N, st, en, vals=DC.vals(), level=60.0, site_cn=True)[2]
            b = emdepth.cohort_cnvs(eng, p, DC.ROWS, DC.N, st, en, vals=DC.vals(), window=0.01, level=60.0, site_cn=True)[2]
            assert np.array_equal(a["site_cn"], b["site_cn"]) and DC.matrix_text(a["site_cn"]) == DC.expected()[1]
        finally:
            eng.device_free(p)


def test_the_exclusive_flags_are_refused(files):
    d, plain, gc, tied = files
    p = DC.run("debias", ["--gc-values", gc, "--window", "0.01", "--moving", "9", plain])
    assert p.returncode == 1 and p.stdout == "" and "--window" in p.stderr and "--moving" in p.stderr
    p = DC.run("emdepth", ["--gc-values", gc, "--gc-moving", "9", "--gc-window", "0.01", plain])
    assert p.returncode == 1 and p.stdout == "" and "--gc-window" in p.stderr and "--gc-moving" in p.stderr
    # usage errors, as the other flags': a window that is not odd and 1 .. 255, a window without a covariate, the other
    # command's spelling
    for w in ("0", "2", "8", "256", "-1", "9.5", "x", ""):
        assert DC.run("debias", ["--gc-values", gc, "--moving=" + w, plain]).returncode == 255, w
        assert DC.run("emdepth", ["--gc-values", gc, "--gc-moving=" + w, plain]).returncode == 255, w
    assert DC.run("emdepth", ["--gc-moving", "9", plain]).returncode == 255
    assert DC.run("debias", ["--gc-values", gc, "--gc-moving", "9", plain]).returncode == 255
    assert DC.run("emdepth", ["--gc-values", gc, "--moving", "9", plain]).returncode == 255
    # fewer rows than the window needs: the engine's refusal, exit 1
    p = DC.run("debias", ["--gc-values", gc, "--moving", "81", plain])
    assert p.returncode == 1 and p.stdout == "" and "gd_moving_debias" in p.stderr
