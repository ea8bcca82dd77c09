"""GPU: `goleft-depth debias --svd PCT --log2`, `goleft-depth emdepth --svd PCT --log2` and
goleft_amd.emdepth.cohort_cnvs(svd=PCT, svd_scaler="log2") on the 9-sample, 40-row matrix of tests/test_gpu_debias_cli.py:
the debiased text against the oracle (tests/svdlog2_ref.py) under the contract of tests/test_gpu_svdlog2.py, the stderr
line of the removed shares, the one-call forms byte for byte against the piped ones, the flag errors.  PCT is taken from the
oracle's own spectrum, half way between two shares, and held to the margins of tests/test_svdlog2_ref.py before any device
call.  Every call runs under its own timeout; nothing is retried."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import svdlog2_ref as LR
from tests import test_gpu_debias_cli as DC
from tests import test_gpu_svddebias_cli as SC
from tests.test_gpu_svdlog2 import DELTA, LN2

pytestmark = pytest.mark.gpu

LEVEL = "60"


@functools.lru_cache(maxsize=None)
def want(n):
    """(pct as the command line takes it, the oracle's (out, s, n, out64, e, m)) for a cut after n components"""
    A = DC.cli_cells().astype(np.float32)
    s, _ = LR.SR.spectrum_svd(LR.scale(A.astype(np.float64))[0])
    share = 100.0 * s / s.sum()
    pct = float("%.6g" % ((share[n - 1] + share[n]) / 2))
    assert share[n - 1] - pct >= 0.05 and pct - share[n] >= 0.05 and (s[n - 1] - s[n]) / s[0] >= 0.01
    res = LR.svd_log2(A, pct)
    assert res[2] == n
    return repr(pct), res


def hold(text, res):
    ref = res[3]
    got = SC.parse(text).astype(np.float32).astype(np.float64)                         # %.9g of a float32: the reader's narrowing takes it back
    assert (np.abs(got - ref) <= 2.0 ** -24 * np.abs(ref) + (1.0 + ref) * LN2 * DELTA).all()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("svdlog2")
    plain, gc = d / "m.bed", d / "gc.txt"
    plain.write_text(DC.matrix_text(DC.cli_cells()))
    gc.write_text("".join("%r\n" % float(v) for v in DC.vals()))
    return d, str(plain), str(gc)


@pytest.mark.parametrize("n", [1, 2])
def test_debias_svd_log2_writes_the_oracles_matrix(files, n):
    d, plain, gc = files
    pct, res = want(n)
    p = DC.run("debias", ["--svd", pct, "--log2", plain], {"GOLEFT_EMDEPTH_TIMING": "1"})
    assert p.returncode == 0, p.stderr
    hold(p.stdout, res)
    got, k = SC.shares(p.stderr)
    s = res[1]
    assert k == n and np.allclose(got, (100.0 * s / s.sum())[:n], rtol=0, atol=0.0051)
    assert '"svd_gram_s"' in p.stderr and '"svd_removed": %d' % n in p.stderr
    assert (SC.parse(p.stdout) >= 0).all()
    # it is not the z-score's answer
    z = DC.run("debias", ["--svd", pct, "--zscore", plain])
    assert z.returncode == 0 and z.stdout != p.stdout


def test_the_python_entry_writes_the_same_file(files):
    from goleft_amd import emdepth
    d, plain, gc = files
    pct, res = want(1)
    out = str(d / "deb.bed")
    assert emdepth.Debias(["--svd=" + pct, "--log2", plain], out_path=out) == 0
    p = DC.run("debias", ["--log2", "--svd", pct, plain])
    with open(out) as f:
        assert p.returncode == 0 and f.read() == p.stdout


@pytest.mark.parametrize("with_gc", [False, True])
def test_emdepth_svd_log2_is_the_pipe(files, with_gc):
    d, plain, gc = files
    pct, _ = want(1)
    tag = "gc" if with_gc else "raw"
    deb, c1, c2 = d / ("deb_%s.bed" % tag), str(d / ("c1_%s.tsv" % tag)), str(d / ("c2_%s.tsv" % tag))
    src = plain
    if with_gc:
        p = DC.run("debias", ["--gc-values", gc, plain])
        assert p.returncode == 0, p.stderr
        src = str(d / "gc_deb.bed")
        with open(src, "w") as f:
            f.write(p.stdout)
    p = DC.run("debias", ["--svd", pct, "--log2", src])
    assert p.returncode == 0, p.stderr
    deb.write_text(p.stdout)
    gc_flags = ["--gc-values", gc] if with_gc else []
    for level in ([], ["--level", LEVEL]):
        if with_gc and not level:
            continue                             # (with a GC flag the default level is the matrix's as read, which the pipe has lost)
        two = DC.run("emdepth", ["--normalize"] + level + [str(deb)])
        one = DC.run("emdepth", gc_flags + ["--svd", pct, "--log2"] + level + [plain])
        assert two.returncode == 0 and one.returncode == 0, (two.stderr, one.stderr)
        assert one.stdout == two.stdout and one.stdout.startswith(DC.HEADER + "\n")
    two = DC.run("emdepth", ["--normalize", "--level", LEVEL, "--cnvs", c2, str(deb)])
    one = DC.run("emdepth", gc_flags + ["--log2", "--svd", pct, "--level", LEVEL, "--cnvs", c1, plain],
                 {"GOLEFT_EMDEPTH_ROWS": "7", "GOLEFT_EMDEPTH_TIMING": "1"})
    assert two.returncode == 0 and one.returncode == 0, (two.stderr, one.stderr)
    assert one.stdout == two.stdout and '"svd_project_s"' in one.stderr
    with open(c1) as a, open(c2) as b:
        calls = a.read()
        assert calls == b.read() and calls.startswith("#sample\t")


@pytest.mark.parametrize("with_gc", [False, True])
def test_cohort_cnvs_log2_is_the_host_matrix_chain(files, with_gc):
    from goleft_amd import emdepth
    from goleft_amd.engine import DepthEngine
    d, plain, gc = files
    pct, res = want(1)
    calls = d / ("calls_%d.tsv" % with_gc)
    level = ["--level", LEVEL] if with_gc else []
    run = DC.run("emdepth", (["--gc-values", gc] if with_gc else []) + ["--svd", pct, "--log2"] + level + ["--cnvs", str(calls), plain])
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
            _, _, got = emdepth.cohort_cnvs(eng, p, DC.ROWS, DC.N, st, en, vals=DC.vals() if with_gc else None,
                                            level=float(LEVEL) if with_gc else None, svd=float(pct), svd_scaler="log2",
                                            site_cn=True)
            assert run.stdout == DC.matrix_text(got["site_cn"])
            mine = list(zip(got["sample"].tolist(), np.diff(got["member_off"]).astype(np.int64).tolist()))
            lines = calls.read_text().split("\n")
            assert lines[0].startswith("#sample\t") and lines[-1] == ""
            assert [(int(f[1]), int(f[3])) for f in (ln.split("\t") for ln in lines[1:-1])] == mine
            # the engine's own entry gives the command line's matrix, by name and by number; None is as zscore says
            text = DC.run("debias", ["--svd", pct, "--log2", plain]).stdout
            for scaler in ("log2", 2):
                out, s, k = eng.svd_debias(cells.astype(np.float32), float(pct), scaler=scaler)
                assert k == 1 and out.tobytes() == np.ascontiguousarray(SC.parse(text), np.float32).tobytes()
            assert all(v > 0 for v in eng.svd_debias_timing())
            a = eng.svd_debias(cells.astype(np.float32), float(pct), True)
            b = eng.svd_debias(cells.astype(np.float32), float(pct), scaler="zscore")
            assert a[0].tobytes() == b[0].tobytes() and a[0].tobytes() != out.tobytes()
            with pytest.raises(ValueError):
                emdepth.cohort_cnvs(eng, p, DC.ROWS, DC.N, st, en, svd=float(pct), svd_scaler="none")
        finally:
            eng.device_free(p)


def test_flag_conflicts(files):
    d, plain, gc = files
    p = DC.run("debias", ["--svd", "2", "--log2", "--zscore", plain])
    assert p.returncode == 255 and p.stdout == "" and "--log2" in p.stderr and "--zscore" in p.stderr
    for cmd in ("debias", "emdepth"):
        p = DC.run(cmd, ["--log2", plain])
        assert p.returncode == 255 and p.stdout == "" and "--log2" in p.stderr and "--svd" in p.stderr, cmd
    p = DC.run("debias", ["--log2", "--gc-values", gc, plain])
    assert p.returncode == 255 and p.stdout == "" and "--log2" in p.stderr
    p = DC.run("debias", ["--svd", "2", "--log2", "--gc-values", gc, plain])
    assert p.returncode == 1 and p.stdout == "" and "--svd" in p.stderr and "pipe" in p.stderr
    p = DC.run("emdepth", ["--svd", "2", "--log2", "--scales", gc, plain])
    assert p.returncode == 255 and p.stdout == "" and "--scales" in p.stderr
    assert DC.run("scales", ["--log2", plain]).returncode == 255
    assert DC.run("debias", ["--svd", "2", "--log2=1", plain]).returncode == 255
