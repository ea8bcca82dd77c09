"""GPU: gd_emcnv_* (goleft_amd/csrc/gd_emcnv.hpp, gd_api_emcnv.inc) through the C ABI against the sequential restatement
of emdepth.Cache (tests/emcnv_ref.py), on the cases of tests/emcnv_shapes.py.

The contract: sample, psize, emit_row, member_off, member_row and the bits of depth are equal;
cn is equal but on the members emdepth_ref.pair_excluded names; log2fc has its infinities identical and finite values
within one float32 ulp.  That is exact because tests/test_emcnv_ref.py holds every case to: no cell within 1e-9 of a
state threshold, no row left out, at most 1 % of member cells excluded.  Cutting the rows into blocks changes no byte."""
import ctypes as C

import numpy as np
import pytest

from goleft_amd import _lib
from tests import emcnv_shapes as S
from tests import emdepth_ref as R
from tests import helpers as H

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE, E_RANGE = -1, -4, -5
KEYS = ("sample", "psize", "emit_row", "member_off", "member_row", "depth", "cn", "log2fc")
DTYPES = (np.uint32, np.uint32, np.uint32, np.uint64, np.uint32, np.float32, np.uint8, np.float32)


class Ctx:
    def __init__(self):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        assert self.lib.gd_create(0, C.byref(self.h)) == 0
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def ok(self, rc):
        assert rc == 0, self.lib.gd_last_error(self.h).decode()

    def err(self):
        return self.lib.gd_last_error(self.h)

    def close(self):
        self.lib.gd_destroy(self.h)

    def add(self, d, st, en, cn=None):
        return self.lib.gd_emcnv_add(self.h, d.ctypes.data if d.size else None, d.shape[0], st.ctypes.data if st.size else None,
                                     en.ctypes.data if en.size else None, cn.ctypes.data if cn is not None else None)

    def finish(self):
        nc, nm = C.c_uint64(), C.c_uint64()
        self.ok(self.lib.gd_emcnv_finish(self.h, C.byref(nc), C.byref(nm)))
        return nc.value, nm.value

    def read(self, nc, nm, want=(True,) * 8):
        sizes = (nc, nc, nc, nc + 1, nm, nm, nm, nm)
        out = [np.full(k, 0xA5, np.uint8).repeat(np.dtype(dt).itemsize).view(dt) if w else None for k, dt, w in zip(sizes, DTYPES, want)]
        self.ok(self.lib.gd_emcnv_read(self.h, *[o.ctypes.data if o is not None else None for o in out]))
        return dict(zip(KEYS, out))

    def run(self, case, block=None, site_cn=True):
        """begin .. read on the host float32 form, `block` rows a call"""
        d, rows = case.depths, case.depths.shape[0]
        self.ok(self.lib.gd_emcnv_begin(self.h, d.shape[1]))
        cn = np.full(d.shape, 255, np.uint8) if site_cn else None
        step = block or max(rows, 1)
        for r0 in range(0, rows, step):
            r1 = min(rows, r0 + step)
            self.ok(self.add(d[r0:r1], case.starts[r0:r1], case.ends[r0:r1], cn[r0:r1] if site_cn else None))
        out = self.read(*self.finish())
        out["site_cn"] = cn
        return out

    def upload(self, cells):
        cells = np.ascontiguousarray(cells, np.int64)
        p = C.c_void_p()
        self.ok(self.lib.gd_device_alloc(self.h, cells.nbytes, C.byref(p)))
        assert self.hip.hipMemcpy(p, cells.ctypes.data, cells.nbytes, 1) == 0           # hipMemcpyHostToDevice
        return p


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def same_bytes(a, b):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in a)


def compare(name, got):
    """Holds one case's device result to the contract; prints the figures first."""
    case, ref = S.cases()[name], S.reference(name)
    left_out, members, excluded = S.plan(name)
    assert left_out == 0 and ref.near == [] and len(excluded) <= S.CAP * len(members), name
    want = S.flatten(ref.cnvs)
    print("%s: %d rows x %d, CNVs %d (reference %d), members %d (reference %d), %d member cells left out of cn" % (
        name, case.depths.shape[0], case.depths.shape[1], len(got["sample"]), len(want["sample"]), len(got["member_row"]),
        len(want["member_row"]), len(excluded)))
    for k in ("sample", "psize", "emit_row", "member_off", "member_row"):
        assert np.array_equal(got[k], want[k]), k
    assert got["depth"].tobytes() == want["depth"].tobytes()
    col = np.repeat(want["sample"], np.diff(want["member_off"]).astype(np.int64))
    keep = np.array([(int(r), int(s)) not in excluded for r, s in zip(want["member_row"], col)], bool)
    assert np.array_equal(got["cn"][keep], want["cn"][keep])
    a, b = got["log2fc"], want["log2fc"]
    assert not np.isnan(a).any() and not np.isnan(b).any()
    assert np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b))
    fin = np.isfinite(b)
    diff = np.abs(a[fin].astype(np.float64) - b[fin].astype(np.float64))
    print("  log2fc: largest difference %.3g (one ulp there is at least %.3g)" % (
        float(diff.max()) if diff.size else 0.0, float(np.spacing(np.abs(b[fin])).min()) if diff.size else 0.0))
    assert np.all(diff <= np.spacing(np.abs(b[fin])).astype(np.float64))
    if got.get("site_cn") is not None and case.depths.size:
        r_cn = np.array([r.cn for r in ref.rows], np.uint8)
        mask = np.ones(r_cn.shape, bool)
        for i, s in S.ES.plan(case, ref.rows)[1]:
            mask[i, s] = False
        assert np.array_equal(got["site_cn"][mask], r_cn[mask])


F32 = sorted(k for k, c in S.cases().items() if c.kind == "f32")


@pytest.mark.parametrize("name", F32)
def test_host_float32(ctx, name):
    compare(name, ctx.run(S.cases()[name]))


@pytest.mark.parametrize("name", ["psize", "sample0", "one_sample", "zero_rows", "random_n65", "random_n257", "start_before_end",
                                  "float_n200"])
def test_block_seams_change_no_byte(ctx, name):
    case = S.cases()[name]
    whole = ctx.run(case)
    compare(name, whole)
    for block in S.BLOCKS:
        assert same_bytes(ctx.run(case, block), whole), block


def test_chunk_seams_in_blocks(ctx):
    """blocks that end one row before, on and one row after the chunk, under a CNV longer than a chunk"""
    case = S.cases()["long_cnv"]
    whole = ctx.run(case)
    for block in (S.CHUNK - 1, S.CHUNK, S.CHUNK + 1):
        assert same_bytes(ctx.run(case, block), whole), block


def test_span_seams_in_blocks(ctx):
    """blocks that end on and one row after the blocks the gap kernel steps over, on rows that never gap"""
    for name in ("near_long", "repeated_wrap"):
        case = S.cases()[name]
        whole = ctx.run(case)
        for block in (S.SPAN2, S.SPAN1 + 1):
            assert same_bytes(ctx.run(case, block), whole), (name, block)


def test_two_runs_give_identical_bytes(ctx):
    for name in ("dense", "many_at_one_row", "float_n200"):
        assert same_bytes(ctx.run(S.cases()[name]), ctx.run(S.cases()[name])), name


def test_null_outputs(ctx):
    case = S.cases()["psize"]
    full = ctx.run(case)
    ctx.ok(ctx.lib.gd_emcnv_begin(ctx.h, case.depths.shape[1]))
    ctx.ok(ctx.add(case.depths, case.starts, case.ends))                 # no cn_out
    nc, nm = ctx.finish()
    assert ctx.lib.gd_emcnv_finish(ctx.h, None, None) == 0               # again, and without the counts
    for i in range(8):
        for want in ([j == i for j in range(8)], [j != i for j in range(8)], [False] * 8):
            got = ctx.read(nc, nm, want)
            for k in KEYS:
                assert got[k] is None or got[k].tobytes() == full[k].tobytes(), (k, want)
    ctx.ok(ctx.lib.gd_emcnv_end(ctx.h))


def test_no_rows_at_all(ctx):
    for adds in (0, 2):
        ctx.ok(ctx.lib.gd_emcnv_begin(ctx.h, 5))
        for _ in range(adds):
            assert ctx.lib.gd_emcnv_add(ctx.h, None, 0, None, None, None) == 0
            assert ctx.lib.gd_emcnv_add_cells(ctx.h, None, 0, None, None, None, None) == 0
        assert ctx.finish() == (0, 0)
        out = ctx.read(0, 0)
        assert out["member_off"].tolist() == [0]
        ctx.ok(ctx.lib.gd_emcnv_end(ctx.h))


def test_calls_out_of_order(ctx):
    case = S.cases()["u_run"]
    ctx.ok(ctx.lib.gd_emcnv_end(ctx.h))                                  # nothing to free is fine
    assert ctx.add(case.depths, case.starts, case.ends) == E_STATE
    assert ctx.lib.gd_emcnv_finish(ctx.h, None, None) == E_STATE
    assert ctx.lib.gd_emcnv_read(ctx.h, *[None] * 8) == E_STATE
    assert b"gd_emcnv_begin" in ctx.err()
    ctx.ok(ctx.lib.gd_emcnv_begin(ctx.h, 5))
    ctx.ok(ctx.add(case.depths, case.starts, case.ends))
    assert ctx.lib.gd_emcnv_read(ctx.h, *[None] * 8) == E_STATE          # read before finish
    assert b"gd_emcnv_finish" in ctx.err()
    # begin after begin drops what was added
    ctx.ok(ctx.lib.gd_emcnv_begin(ctx.h, 5))
    other = S.cases()["d_run"]
    ctx.ok(ctx.add(other.depths, other.starts, other.ends))
    nc, nm = ctx.finish()
    compare("d_run", ctx.read(nc, nm))
    assert ctx.add(case.depths, case.starts, case.ends) == E_STATE       # add after finish
    compare("d_run", ctx.read(nc, nm))
    ctx.ok(ctx.lib.gd_emcnv_end(ctx.h))
    assert ctx.lib.gd_emcnv_read(ctx.h, *[None] * 8) == E_STATE


def test_refused_inputs_leave_the_state_as_it_was(ctx):
    case = S.cases()["psize"]
    d, st, en = case.depths, case.starts, case.ends
    for n in (2, 0, -1, 4097):
        assert ctx.lib.gd_emcnv_begin(ctx.h, n) == E_RANGE, n
    ctx.ok(ctx.lib.gd_emcnv_begin(ctx.h, d.shape[1]))
    ctx.ok(ctx.add(d[:11], st[:11], en[:11]))
    assert ctx.lib.gd_emcnv_begin(ctx.h, 2) == E_RANGE                   # a refused begin drops nothing
    for bad in (np.nan, -1.0, np.inf, -np.inf):
        x = d[11:].copy()
        x[3, 2] = bad
        assert ctx.add(x, st[11:], en[11:]) == E_INVALID, bad
        assert b"row 3, sample 2" in ctx.err()
    assert ctx.lib.gd_emcnv_add(ctx.h, d[11:].ctypes.data, d.shape[0] - 11, None, en[11:].ctypes.data, None) == E_INVALID
    p = ctx.upload(d[11:].astype(np.int64))
    try:
        for bad in (np.nan, -0.5, np.inf):
            scale = np.ones(d.shape[1], np.float32)
            scale[4] = bad
            assert ctx.lib.gd_emcnv_add_cells(ctx.h, p, d.shape[0] - 11, scale.ctypes.data, st[11:].ctypes.data,
                                              en[11:].ctypes.data, None) == E_INVALID, bad
        # the rest goes in as cells: the depths are integers
        ctx.ok(ctx.lib.gd_emcnv_add_cells(ctx.h, p, d.shape[0] - 11, None, st[11:].ctypes.data, en[11:].ctypes.data, None))
    finally:
        ctx.ok(ctx.lib.gd_device_free(ctx.h, p))
    compare("psize", ctx.read(*ctx.finish()))
    t = (C.c_double * 4)()
    ctx.ok(ctx.lib.gd_emcnv_timing(ctx.h, t, 4))
    assert t[0] > 0 and t[1] > 0 and t[2] > 0 and t[3] > 0
    ctx.ok(ctx.lib.gd_emcnv_end(ctx.h))


@pytest.mark.parametrize("n_samples", S.ES.COHORT_SAMPLES)
def test_cells_of_a_real_depthwed(n_samples):
    """BAM records -> window sums -> gd_depthwed_device -> gd_emcnv_add_cells: the matrix never leaves the device."""
    from goleft_amd.engine import DepthEngine
    ES = S.ES
    sums, cells = ES.cohort(n_samples)
    n_ref = len(ES.COHORT_LENGTHS)
    rng = np.random.default_rng(n_samples)
    tids = np.arange(n_samples * n_ref, dtype=np.int32).reshape(n_samples, n_ref)
    with DepthEngine(0) as eng:
        eng.set_params(window_size=ES.COHORT_W, min_mapq=1, min_cov=4)
        eng.set_contigs([ES.COHORT_LENGTHS[j] for s in range(n_samples) for j in range(n_ref)])
        for s in range(n_samples):
            for j in range(n_ref):
                r = H.window_sum_reads(rng, ES.COHORT_LENGTHS[j], ES.COHORT_W, sums[s][j])
                eng.push(int(tids[s, j]), r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
        eng.compute()
        ptr, rows = eng.depthwed_device(tids, ES.COHORT_W)
        assert rows == cells.shape[0]
        for name in ("cohort_n%d", "cohort_pow2_n%d"):
            case = S.cases()[name % n_samples]
            whole = eng.emdepth_cnvs_cells(ptr, rows, n_samples, case.starts, case.ends, case.scale, site_cn=True)
            assert whole.pop("timing")[2] > 0
            compare(name % n_samples, whole)
            cut = eng.emdepth_cnvs_cells(ptr, rows, n_samples, case.starts, case.ends, case.scale, block_rows=7, site_cn=True)
            cut.pop("timing")
            assert same_bytes(cut, whole)
        # the float32 form through the same handle
        case = S.cases()["cohort_pow2_n%d" % n_samples]
        got = eng.emdepth_cnvs(R.cells_to_depths(cells, case.scale), case.starts, case.ends, block_rows=5)
        got.pop("timing")
        compare("cohort_pow2_n%d" % n_samples, got)
