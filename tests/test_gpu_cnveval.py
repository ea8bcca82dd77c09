"""GPU: gd_cnveval (goleft_amd/csrc/gd_cnveval.hpp) through the C ABI against the literal restatement of
cnveval.Evaluate (tests/cnveval_ref.py), on every case of tests/cnveval_shapes.py.

The counts are integers: every cell of every case's [n_samples][3][4] array is compared, and nothing is left out.  Then
the refusals, each with its status and a context that still serves the next call, the equal bytes of two calls and the
three timings."""
import ctypes as C

import numpy as np
import pytest

from goleft_amd import _lib
from tests import cnveval_shapes as S

pytestmark = pytest.mark.gpu

E_INVALID, E_RANGE, E_UNSORTED = -1, -5, -7
ORDER = ("cnv_off", "cnv_chrom", "cnv_start", "cnv_end", "cnv_cn", "t_chrom", "t_start", "t_end", "t_cn", "t_off", "t_samples")


class Ctx:
    def __init__(self):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        assert self.lib.gd_create(0, C.byref(self.h)) == 0

    def close(self):
        self.lib.gd_destroy(self.h)

    def run(self, n_samples, a, po, fill=0):
        """(status, stats); stats starts as `fill` everywhere"""
        stats = np.full((n_samples, 3, 4), fill, np.int64)
        ptr = lambda x: x.ctypes.data if x.size else None
        v = [a[k] for k in ORDER]
        rc = self.lib.gd_cnveval(self.h, n_samples, v[0].ctypes.data, ptr(v[1]), ptr(v[2]), ptr(v[3]), ptr(v[4]), len(a["t_chrom"]),
                                 ptr(v[5]), ptr(v[6]), ptr(v[7]), ptr(v[8]), v[9].ctypes.data, ptr(v[10]), po, stats.ctypes.data)
        return rc, stats

    def error(self):
        return self.lib.gd_last_error(self.h).decode()


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(S.cases()))
def test_every_count_of_every_case(ctx, name):
    case = S.cases()[name]
    names, want = S.reference(name)
    got_names, a = S.device_inputs(case)
    assert got_names == names
    rc, got = ctx.run(len(names), a, case.po, fill=-1)
    assert rc == 0, ctx.error()
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(names[s], int(k), int(f), int(got[s, k, f]), int(want[s, k, f])) for s, k, f in bad[:10]]


def test_two_calls_give_the_same_bytes(ctx):
    for name in ("longest_window", "samples_65", "launch_%d" % ((S.TARGET_BLOCKS // 256) * S.WG + 1)):
        case = S.cases()[name]
        names, a = S.device_inputs(case)
        rc1, one = ctx.run(len(names), a, case.po)
        rc2, two = ctx.run(len(names), a, case.po, fill=7)
        assert rc1 == 0 and rc2 == 0, ctx.error()
        assert one.tobytes() == two.tobytes()


def _worked():
    case = S.cases()["hand_worked"]
    names, a = S.device_inputs(case)
    return case, names, a, S.reference("hand_worked")[1]


def _refused(ctx, names, a, po, status, word):
    rc, stats = ctx.run(len(names), a, po, fill=-5)
    assert rc == status, (rc, ctx.error())
    assert word in ctx.error(), ctx.error()
    assert (stats == -5).all()                                   # a refused call leaves the counts untouched


def test_refusals_and_the_context_goes_on(ctx):
    case, names, a, want = _worked()
    swap = dict(a)
    for k in ("cnv_chrom", "cnv_start", "cnv_end", "cnv_cn"):
        swap[k] = a[k].copy()
        swap[k][[0, 1]] = swap[k][[1, 0]]                        # sample a's first two calls: 1:1200 and 1:1300
    _refused(ctx, names, swap, case.po, E_UNSORTED, "call 1 of sample 0")
    off = dict(a, cnv_off=a["cnv_off"].copy())
    off["cnv_off"][1], off["cnv_off"][2] = a["cnv_off"][2], a["cnv_off"][1]
    _refused(ctx, names, off, case.po, E_INVALID, "offset 2")
    first = dict(a, t_off=a["t_off"] + 1)
    _refused(ctx, names, first, case.po, E_INVALID, "offset 0")
    ids = dict(a, t_samples=a["t_samples"].copy())
    ids["t_samples"][2] = len(names)
    _refused(ctx, names, ids, case.po, E_RANGE, "entry 2")
    ids["t_samples"][2] = -1
    _refused(ctx, names, ids, case.po, E_RANGE, "entry 2")
    neg = dict(a, t_start=a["t_start"].copy())
    neg["t_start"][3] = -1
    _refused(ctx, names, neg, case.po, E_RANGE, "truth 3")
    back = dict(a, cnv_end=a["cnv_end"].copy())
    back["cnv_end"][4] = back["cnv_start"][4] - 1
    _refused(ctx, names, back, case.po, E_RANGE, "call 4")
    for po in (0.0, 1.5, -0.1, float("nan")):
        _refused(ctx, names, a, po, E_RANGE, "overlap")
    rc, got = ctx.run(len(names), a, case.po)
    assert rc == 0 and (got == want).all(), ctx.error()


def test_timing_fills_three_numbers(ctx):
    case, names, a, want = _worked()
    rc, _ = ctx.run(len(names), a, case.po)
    assert rc == 0
    t = np.full(4, -1.0)
    assert ctx.lib.gd_cnveval_timing(ctx.h, t.ctypes.data, 3) == 0
    assert (t[:3] >= 0).all() and t[1] > 0 and t[3] == -1.0
    assert ctx.lib.gd_cnveval_timing(ctx.h, t.ctypes.data, 9) == 0
    assert 0 < t[3] <= t[1]                                      # the first kernel's part of the kernels
