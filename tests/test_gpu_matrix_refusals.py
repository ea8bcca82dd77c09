"""GPU: what the depth-matrix entry points refuse, word for word (gd_api_emdepth.inc, gd_api_emcnv.inc, gd_api_colselect.inc,
gd_api_chunkdebias.inc, gd_api_movdebias.inc, gd_api_devmat.inc) through the C ABI.

Every host, _cells and _device form gets one input per refusal: a cell that is NaN, +inf or negative, a bad scale, a
negative int64 cell, an output that overlaps its input, a covariate that is not finite, a bad window, the sample and row
ranges, a matrix that does not fit an allocation, medians without room for the chunks, and emcnv's calls out of order.  The
status and the whole gd_last_error text are compared byte for byte with the format strings of the `fail` calls as they
stood when this file was written: the layer around the kernels may be rearranged, what a caller reads may not change.  The
call after a refusal must succeed and give the bytes it gave before.

The matrix is 6 rows x 4 samples with the bad cell at row 3, sample 2; the check on the device also runs on 2 rows x 65
samples with the bad cell at row 1, sample 64, so the cell it names lies behind a 64-column tile.  (gd_emcnv_add*'s own "do
not fit an allocation" cannot be reached: at most 4096 samples, and more than 2^32 - 3 rows are refused before it.)"""
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_devmat import Ctx

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE, E_RANGE, E_CAPACITY = -1, -4, -5, -8
ROWS, N, AT = 6, 4, (3, 2)
WIDE_ROWS, WIDE_N, WIDE_AT = 2, 65, (1, 64)
BAD = (("nan", np.nan), ("inf", np.inf), ("negative", -1.0))
VALS = np.array([0.1, 0.5, 0.1, 0.9, 0.5, 0.1])          # three chunks at a window of 0.1
WINDOW, MOVING = 0.1, 3
FIT_ROWS = (2 ** 64 - 1) // 8 // 9 + 1                   # the first row count whose nine float64 centres a row overflow a size_t
DEPTH = "%s: the depth of row %d, sample %d is not a finite number >= 0"
SCALE = "%s: the scale of sample %d is not a finite number >= 0"
NEGATIVE = "%s: a cell of the device matrix is negative"
OVERLAP = "%s: the quotients would overlap the cells they are made of"
VALUE = "%s: the value of row %d is not finite"
FIT = "emdepth: %d rows of %d samples do not fit an allocation"
TWO = "emdepth: 2 samples: the reference's median of an even row reads b[N/2 + 1], which two values do not have"
EM_N = "emdepth: 1 or 3 .. 4096 samples, not %d"
NO_BEGIN = "gd_emcnv_begin has not been called"
FINISHED = "emcnv: gd_emcnv_finish has run: gd_emcnv_begin starts another"
KINDS = ("host", "cells", "device")


class Env:
    """The good inputs and one method per family of entry points: (status, every output as bytes)."""

    def __init__(self, ctx):
        self.c, self.lib, self.h = ctx, ctx.lib, ctx.h
        rng = np.random.default_rng(11)
        self.cells = rng.integers(1, 200, (ROWS, N)).astype(np.int64)
        self.cells[0, 1] = 0
        self.d = self.cells.astype(np.float32)
        self.wide = rng.integers(1, 200, (WIDE_ROWS, WIDE_N)).astype(np.float32)
        self.f = np.array([1.0, 0.5, 2.0, 1.25], np.float32)
        self.base = {}

    def good(self, kind):
        return self.cells if kind == "cells" else self.d

    @contextlib.contextmanager
    def dev(self, *arrays):
        ptrs = [self.c.upload(a) for a in arrays]
        try:
            yield ptrs[0] if len(ptrs) == 1 else ptrs
        finally:
            self.c.free(*ptrs)

    def emdepth(self, kind, m, rows=None, n=None, scale=None, null=False):
        rows, n = m.shape[0] if rows is None else rows, m.shape[1] if n is None else n
        out = self.c.em_outputs(*m.shape)
        ptrs = [o.ctypes.data for o in out]
        if kind == "host":
            rc = self.lib.gd_emdepth(self.h, m.ctypes.data, rows, n, *ptrs)
        else:
            with self.dev(m) as p:
                if kind == "device":
                    rc = self.lib.gd_emdepth_device(self.h, p, rows, n, *ptrs)
                else:
                    rc = self.lib.gd_emdepth_cells(self.h, None if null else p, rows, n,
                                                   None if scale is None else scale.ctypes.data, *ptrs)
        return rc, b"".join(o.tobytes() for o in out)

    def medians(self, kind, m, rows=None, n=None):
        rows, n = m.shape[0] if rows is None else rows, m.shape[1] if n is None else n
        med = np.full(m.shape[1], -1, np.int64) if kind == "cells" else np.full(m.shape[1], np.nan, np.float32)
        nz = np.full(m.shape[1], 2 ** 64 - 1, np.uint64)
        if kind == "host":
            rc = self.lib.gd_sample_medians(self.h, m.ctypes.data, rows, n, med.ctypes.data, nz.ctypes.data)
        else:
            fn = self.lib.gd_sample_medians_cells if kind == "cells" else self.lib.gd_sample_medians_device
            with self.dev(m) as p:
                rc = fn(self.h, p, rows, n, med.ctypes.data, nz.ctypes.data)
        return rc, med.tobytes() + nz.tobytes()

    def debias(self, kind, m, vals=VALS, window=WINDOW, rows=None, n=None, med_rows=None, overlap=False):
        rows, n = m.shape[0] if rows is None else rows, m.shape[1] if n is None else n
        v = np.ascontiguousarray(vals, np.float64)
        cor, nc = np.full(m.shape[0], 0xffffffff, np.uint32), C.c_size_t(2 ** 63)
        med = np.full(m.shape, np.nan, np.float32)
        cap = m.shape[0] if med_rows is None else med_rows
        out = np.full(m.shape, np.nan, np.float32)
        if kind == "host":
            rc = self.lib.gd_chunk_debias(self.h, m.ctypes.data, rows, n, v.ctypes.data, float(window), out.ctypes.data, None,
                                          cor.ctypes.data, C.byref(nc), med.ctypes.data, cap)
        else:
            with self.dev(m, out) as (p, q):
                at = C.c_void_p(p.value + 8) if overlap else q
                rc = self.lib.gd_chunk_debias_cells(self.h, p, rows, n, v.ctypes.data, float(window), at, cor.ctypes.data,
                                                    C.byref(nc), med.ctypes.data, cap)
                out = self.c.read(q, m.shape, np.float32)
        return rc, out.tobytes() + cor.tobytes() + med.tobytes() + b"%d" % nc.value

    def moving(self, kind, m, vals=VALS, window=MOVING, rows=None, n=None, overlap=False):
        rows, n = m.shape[0] if rows is None else rows, m.shape[1] if n is None else n
        v = np.ascontiguousarray(vals, np.float64)
        out = np.full(m.shape, np.nan, np.float32)
        if kind == "host":
            med = np.full(m.shape, np.nan, np.float64)
            rc = self.lib.gd_moving_debias(self.h, m.ctypes.data, rows, n, v.ctypes.data, int(window), out.ctypes.data,
                                           med.ctypes.data)
            return rc, out.tobytes() + med.tobytes()
        with self.dev(m, out) as (p, q):
            at = C.c_void_p(p.value + 8) if overlap else q
            rc = self.lib.gd_moving_debias_cells(self.h, p, rows, n, v.ctypes.data, int(window), at)
            return rc, self.c.read(q, m.shape, np.float32).tobytes()

    def scale(self, m, f, n=None):
        with self.dev(m) as p:
            rc = self.lib.gd_device_scale(self.h, p, m.shape[0], m.shape[1] if n is None else n, f.ctypes.data)
            return rc, self.c.read(p, m.shape, np.float32).tobytes()

    # ---- emcnv: a run is begin, the adds, finish, read, end
    def begin(self, n):
        return self.lib.gd_emcnv_begin(self.h, n)

    def add(self, kind, m, rows=None, scale=None):
        """(status, the block's copy numbers) of one gd_emcnv_add* in the run that is open"""
        rows = m.shape[0] if rows is None else rows
        st = np.arange(m.shape[0], dtype=np.uint32) * 1000
        en = st + np.uint32(1000)
        cn = np.full(m.shape, 255, np.uint8)
        if kind == "host":
            rc = self.lib.gd_emcnv_add(self.h, m.ctypes.data, rows, st.ctypes.data, en.ctypes.data, cn.ctypes.data)
        else:
            with self.dev(m) as p:
                if kind == "device":
                    rc = self.lib.gd_emcnv_add_device(self.h, p, rows, st.ctypes.data, en.ctypes.data, cn.ctypes.data)
                else:
                    rc = self.lib.gd_emcnv_add_cells(self.h, p, rows, None if scale is None else scale.ctypes.data,
                                                     st.ctypes.data, en.ctypes.data, cn.ctypes.data)
        return rc, cn.tobytes()

    def run(self, kind, begun=False):
        """a whole run over the good matrix (in the run that is open when begun): (status, the calls and copy numbers)"""
        if not begun:
            self.c.ok(self.begin(N))
        rc, cn = self.add(kind, self.good(kind), scale=self.f if kind == "cells" else None)
        if rc != 0:
            return rc, b""
        return 0, cn + b"".join(v.tobytes() for v in self.c.calls().values())

    def fine(self, family, kind, begun=False):
        if family == "emdepth":
            return self.emdepth(kind, self.good(kind), scale=self.f if kind == "cells" else None)
        if family == "medians":
            return self.medians(kind, self.good(kind))
        if family == "debias":
            return self.debias(kind, self.good(kind))
        if family == "moving":
            return self.moving(kind, self.good(kind))
        if family == "scale":
            return self.scale(self.d, self.f)
        return self.run(kind, begun)


@pytest.fixture(scope="module")
def env():
    c = Ctx()
    yield Env(c)
    c.close()


def spoilt(m, at, v):
    m = m.copy()
    m[at] = v
    return m


def cases():
    """(family, kind, the refused call: env -> status, the status, the text, whether it leaves an emcnv run open)"""
    out = []

    def case(name, family, kind, call, status, text, begun=False):
        out.append(pytest.param(family, kind, call, status, text.encode(), begun, id="%s_%s-%s" % (family, kind, name)))

    def in_run(n, call):
        """the refused gd_emcnv_add* in a run of n samples that it leaves open"""
        def f(e):
            e.c.ok(e.begin(n))
            return call(e)
        return f

    # ---- a cell that is NaN, +inf or negative: the host forms, and the device forms on both shapes
    for tag, v in BAD:
        for kind in ("host", "device"):
            for shape, pick, at in (("", lambda e: e.d, AT),) + ((("-wide", lambda e: e.wide, WIDE_AT),) if kind == "device" else ()):
                bad = lambda e, pick=pick, at=at, v=v: spoilt(pick(e), at, v)
                case(tag + shape, "emdepth", kind, lambda e, k=kind, b=bad: e.emdepth(k, b(e))[0], E_INVALID, DEPTH % (("emdepth",) + at))
                case(tag + shape, "medians", kind, lambda e, k=kind, b=bad: e.medians(k, b(e))[0], E_INVALID,
                     DEPTH % (("sample medians",) + at))
                case(tag + shape, "emcnv", kind, in_run(WIDE_N if shape else N, lambda e, k=kind, b=bad: e.add(k, b(e))[0]), E_INVALID,
                     DEPTH % (("emcnv",) + at), begun=not shape)
        bad = lambda e, v=v: spoilt(e.d, AT, v)
        case(tag, "debias", "host", lambda e, b=bad: e.debias("host", b(e))[0], E_INVALID, DEPTH % (("chunk debias",) + AT))
        case(tag, "moving", "host", lambda e, b=bad: e.moving("host", b(e))[0], E_INVALID, DEPTH % (("moving debias",) + AT))
        # ---- a bad scale
        g = lambda e, v=v: spoilt(e.f, AT[1], v)
        case("scale-" + tag, "emdepth", "cells", lambda e, g=g: e.emdepth("cells", e.cells, scale=g(e))[0], E_INVALID, SCALE % ("emdepth", AT[1]))
        case("scale-" + tag, "emcnv", "cells", in_run(N, lambda e, g=g: e.add("cells", e.cells, scale=g(e))[0]), E_INVALID,
             SCALE % ("emcnv", AT[1]), begun=True)
        case(tag, "scale", "device", lambda e, g=g: e.scale(e.d, g(e))[0], E_INVALID, SCALE % ("device scale", AT[1]))
        # ---- a covariate that is not finite
        if tag != "negative":
            w = lambda v=v: spoilt(VALS, 4, v)
            for kind in ("host", "cells"):
                case("value-" + tag, "debias", kind, lambda e, k=kind, w=w: e.debias(k, e.good(k), vals=w())[0], E_INVALID, VALUE % ("chunk debias", 4))
                case("value-" + tag, "moving", kind, lambda e, k=kind, w=w: e.moving(k, e.good(k), vals=w())[0], E_INVALID, VALUE % ("moving debias", 4))

    # ---- a negative int64 cell, an output inside the input
    neg = lambda e: spoilt(e.cells, AT, -1)
    case("negative", "medians", "cells", lambda e: e.medians("cells", neg(e))[0], E_INVALID, NEGATIVE % "sample medians")
    case("negative", "debias", "cells", lambda e: e.debias("cells", neg(e))[0], E_INVALID, NEGATIVE % "chunk debias")
    case("negative", "moving", "cells", lambda e: e.moving("cells", neg(e))[0], E_INVALID, NEGATIVE % "moving debias")
    case("overlap", "debias", "cells", lambda e: e.debias("cells", e.cells, overlap=True)[0], E_INVALID, OVERLAP % "chunk debias")
    case("overlap", "moving", "cells", lambda e: e.moving("cells", e.cells, overlap=True)[0], E_INVALID, OVERLAP % "moving debias")

    # ---- windows, ranges, capacity
    for kind in ("host", "cells"):
        for w in (0.0, -0.01, float("nan"), float("inf")):
            case("window%g" % w, "debias", kind, lambda e, k=kind, w=w: e.debias(k, e.good(k), window=w)[0], E_INVALID,
                 "chunk debias: the score window must be a finite number > 0, not %g" % w)
        for w in (0, 2, 257, -1):
            case("window%d" % w, "moving", kind, lambda e, k=kind, w=w: e.moving(k, e.good(k), window=w)[0], E_RANGE,
                 "moving debias: the window must be odd and 1 .. 255, not %d" % w)
        for n in (0, 4097):
            case("n%d" % n, "debias", kind, lambda e, k=kind, n=n: e.debias(k, e.good(k), n=n)[0], E_RANGE,
                 "chunk debias: 1 .. 4096 samples, not %d" % n)
            case("n%d" % n, "moving", kind, lambda e, k=kind, n=n: e.moving(k, e.good(k), n=n)[0], E_RANGE,
                 "moving debias: 1 .. 4096 samples, not %d" % n)
        for rows in (0, 2 ** 31):
            case("rows%d" % rows, "debias", kind, lambda e, k=kind, r=rows: e.debias(k, e.good(k), rows=r)[0], E_RANGE,
                 "chunk debias: 1 .. 2^31 - 1 rows, not %d" % rows)
        for rows, w in ((5, 11), (2 ** 31, 3)):
            case("rows%d" % rows, "moving", kind, lambda e, k=kind, r=rows, w=w: e.moving(k, e.good(k), rows=r, window=w)[0], E_RANGE,
                 "moving debias: %d .. 2^31 - 1 rows for a window of %d, not %d" % ((w - 1) // 2 + 1, w, rows))
        case("capacity", "debias", kind, lambda e, k=kind: e.debias(k, e.good(k), med_rows=2)[0], E_CAPACITY,
             "chunk debias: 3 chunks, the medians have room for 2")
    for kind in KINDS:
        for n in (0, 4097):
            case("n%d" % n, "medians", kind, lambda e, k=kind, n=n: e.medians(k, e.good(k), n=n)[0], E_RANGE,
                 "sample medians: 1 .. 4096 samples, not %d" % n)
        for rows in (0, 2 ** 31):
            case("rows%d" % rows, "medians", kind, lambda e, k=kind, r=rows: e.medians(k, e.good(k), rows=r)[0], E_RANGE,
                 "sample medians: 1 .. 2^31 - 1 rows, not %d" % rows)
        for n in (2, 0, 4097):
            case("n%d" % n, "emdepth", kind, lambda e, k=kind, n=n: e.emdepth(k, e.good(k), n=n)[0], E_RANGE, TWO if n == 2 else EM_N % n)
        for n in (1, 4):                                     # nine centres a row however few the samples
            case("fit-n%d" % n, "emdepth", kind, lambda e, k=kind, n=n: e.emdepth(k, e.good(k), rows=FIT_ROWS, n=n)[0], E_RANGE,
                 FIT % (FIT_ROWS, n))
        # ---- emcnv's own: the rows a run can hold, and the calls out of order
        case("rows", "emcnv", kind, in_run(N, lambda e, k=kind: e.add(k, e.good(k), rows=2 ** 32 - 2)[0]), E_RANGE,
             "emcnv: more than 2^32 - 3 rows", begun=True)
        case("no-begin", "emcnv", kind, lambda e, k=kind: (e.c.ok(e.lib.gd_emcnv_end(e.h)), e.add(k, e.good(k))[0])[1], E_STATE, NO_BEGIN)
        case("finished", "emcnv", kind,
             in_run(N, lambda e, k=kind: (e.c.ok(e.lib.gd_emcnv_finish(e.h, None, None)), e.add(k, e.good(k))[0])[1]), E_STATE, FINISHED)
    for n in (2, 0, 4097):
        case("begin-n%d" % n, "emcnv", "host", lambda e, n=n: e.begin(n), E_RANGE, TWO if n == 2 else EM_N % n)
    for n in (0, 4097):
        case("n%d" % n, "scale", "device", lambda e, n=n: e.scale(e.d, e.f, n=n)[0], E_RANGE, "device scale: 1 .. 4096 samples, not %d" % n)
    # the order of the checks: the sample count before the pointer
    case("null-n2", "emdepth", "cells", lambda e: e.emdepth("cells", e.cells, n=2, null=True)[0], E_RANGE, TWO)
    return out


@pytest.mark.parametrize("family,kind,call,status,text,begun", cases())
def test_a_refusal_in_its_own_words_and_the_call_after_it(env, family, kind, call, status, text, begun):
    key = (family, kind)
    if key not in env.base:                              # once a form, before its first refusal
        rc, env.base[key] = env.fine(family, kind)
        env.c.ok(rc)
    assert call(env) == status
    assert env.c.err() == text
    rc, after = env.fine(family, kind, begun)
    env.c.ok(rc)
    assert after == env.base[key]
