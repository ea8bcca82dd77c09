"""GPU: gd_crai_sizes (gd_crai.hpp, the count pass and the write pass of one walk) through the device ABI, word for word
against the restatement of the reference's makeSizes (tests/crai_ref.py): every tile count, status and tile size.  No
tolerance: everything is integer but one correctly rounded float64 quotient.  One context for the module; a test is one
or a few calls that carry all of its sequences."""
import ctypes as C

import numpy as np
import pytest

from goleft_amd import _lib
from tests import crai_cases as CC
from tests import crai_ref as CR

pytestmark = pytest.mark.gpu

T = CR.T
GD_E_INVALID, GD_E_RANGE, GD_E_CAPACITY = -1, -5, -8


class Ctx:
    def __init__(self):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        assert self.lib.gd_create(0, C.byref(self.h)) == 0

    def close(self):
        self.lib.gd_destroy(self.h)


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def device(ctx, seqs, count_only=False, cap=None):
    """(rc, tile_off, status, sizes or None).  The buffers start out poisoned: what the call does not write shows."""
    off, start, span, slen = CC.flatten(seqs)
    n = len(seqs)
    toff = np.full(n + 1, -7, np.int64)
    status = np.full(max(n, 1), -7, np.int32)
    rc = ctx.lib.gd_crai_sizes(ctx.h, n, off.ctypes.data, ptr(start), ptr(span), ptr(slen), toff.ctypes.data, status.ctypes.data, None, 0)
    if rc != 0 or count_only:
        return rc, toff, status[:n], None
    total = int(toff[n])
    room = total if cap is None else cap
    sizes = np.full(max(room, 1) + 8, -7, np.int64)                             # (8 words past the end stay as they are)
    toff2 = np.full(n + 1, -7, np.int64)
    rc = ctx.lib.gd_crai_sizes(ctx.h, n, off.ctypes.data, ptr(start), ptr(span), ptr(slen), toff2.ctypes.data, status.ctypes.data,
                               sizes.ctypes.data, room)
    assert np.array_equal(toff, toff2)
    assert (sizes[max(room, 1):] == -7).all() and (rc != 0 or (sizes[total:] == -7).all())
    return rc, toff2, status[:n], sizes[:total] if rc == 0 else sizes


def check(ctx, seqs, names=None):
    want = [CR.make_sizes(s) for s in seqs]
    rc, toff, status, sizes = device(ctx, seqs)
    assert rc == 0, ctx.lib.gd_last_error(ctx.h).decode()
    assert toff[0] == 0
    for k, (w, st) in enumerate(want):
        name = names[k] if names else k
        assert status[k] == st, name
        got = sizes[toff[k]:toff[k + 1]].tolist()
        assert got == w, (name, seqs[k][:4], got[:8], w[:8])
    return want


def test_structural_edges(ctx):
    cases = CC.edge_sequences()
    names = sorted(cases)
    want = dict(zip(names, check(ctx, [cases[k] for k in names], names)))
    # what the cases are there for does happen in them
    assert want["slices_0"] == ([], 0) and len(want["slices_129"][0]) > 129
    for k in (0, 1, 63, 64, 65, 200):
        assert want["full_%d" % k][0][:k] == [int(100000 * 12345.0 / (k * T + 5))] * k
        assert want["backfill_%d" % k][0] == ([9000] + [0] * (k - 1) if k else []) + [18]
        assert want["backfill_zero_%d" % k][0] == [0] * k + [18]
    # a tile of back fill (it takes the pending 10) only at + 1; the last slice's gap flushes the pending 36 in the others
    assert [want["gap_edge_%d" % d][0] for d in (-1, 0, 1)] == [[10, 10, 10, 36, 36]] * 2 + [[10, 10, 10, 10, 36]]
    # after three shifts the slice is skipped (the eleventh 4 is the pending value, flushed by the next gap) ...
    assert want["shift_to_0"][0] == [4] * 11 + [0] * 8 + [12]
    assert want["shift_to_1"][0] == [4] * 10 + [1100000] + [0] * 8 + [12]       # ... or pending, from a span of 1 ...
    assert want["shift_to_T"][0] == [4] * 10 + [67, 67] + [0] * 7 + [12]        # ... or one tile (and pending again)
    assert want["over_mT_100"][0][:4] == [10, 10, 10, 6000] and want["over_mT1_100"][0][:4] == [10] * 4   # - T - 1 shifts
    assert want["pending_flushed"][0] == [9000, 0, 0, 0, 18] and want["pending_dropped"][0] == [30]
    assert want["big_per_base"][0][0] == 100000 * (2 ** 31 - 1) > 2 ** 32
    assert min(want["negative_len"][0]) < 0
    assert all(st == 0 for _, st in want.values())


def test_a_sequence_does_not_depend_on_its_neighbours(ctx):
    cases = CC.edge_sequences()
    names = sorted(cases)
    _, toff, _, sizes = device(ctx, [cases[k] for k in names])
    for k in (names[0], "unsorted", "full_200", names[-1]):
        rc, t1, s1, z1 = device(ctx, [cases[k]])
        i = names.index(k)
        assert rc == 0 and s1[0] == 0 and z1.tolist() == sizes[toff[i]:toff[i + 1]].tolist()
    back = list(reversed(names))
    _, toff2, _, sizes2 = device(ctx, [cases[k] for k in back])
    for i, k in enumerate(back):
        j = names.index(k)
        assert sizes2[toff2[i]:toff2[i + 1]].tolist() == sizes[toff[j]:toff[j + 1]].tolist()


def test_random_sequences(ctx):
    seqs = CC.random_sequences(20240607)
    assert len(seqs) == 300 and min(map(len, seqs)) == 0 and max(map(len, seqs)) == 200
    want = check(ctx, seqs)
    assert sum(len(w) for w, _ in want) > 50000 and all(st == 0 for _, st in want)


@pytest.fixture(scope="module")
def viral():
    refs = CR.read_index(CC.VIRAL)
    return refs, [CR.make_sizes(r) for r in refs]


def test_the_long_read_fixture_in_one_call_and_in_three(ctx, viral):
    refs, want = viral
    rc, toff, status, sizes = device(ctx, refs)
    assert rc == 0 and toff[-1] == 191442 and not status.any()
    flat = [v for w, _ in want for v in w]
    assert sizes.tolist() == flat
    cuts = [0, 7, 1500, len(refs)]
    parts = []
    for a, b in zip(cuts, cuts[1:]):
        rc, t, st, z = device(ctx, refs[a:b])
        assert rc == 0 and not st.any()
        parts.extend(z.tolist())
    assert parts == flat


def test_count_only_capacity_and_empty_calls(ctx, viral):
    refs, want = viral
    rc, toff, status, sizes = device(ctx, refs, count_only=True)
    assert rc == 0 and sizes is None and not status.any()
    assert np.diff(toff).tolist() == [len(w) for w, _ in want] and toff[0] == 0
    # one word short: nothing is written, the counts stand
    rc, toff2, _, sizes = device(ctx, refs, cap=191441)
    assert rc == GD_E_CAPACITY and np.array_equal(toff, toff2) and (sizes == -7).all()
    assert b"191442" in ctx.lib.gd_last_error(ctx.h)
    # no sequence at all; sequences without slices; slices without tiles
    t = np.full(1, -7, np.int64)
    assert ctx.lib.gd_crai_sizes(ctx.h, 0, None, None, None, None, t.ctypes.data, None, None, 0) == 0 and t[0] == 0
    assert ctx.lib.gd_crai_sizes(ctx.h, 0, None, None, None, None, None, None, None, 0) == 0
    rc, toff, status, sizes = device(ctx, [[], [], []])
    assert rc == 0 and toff.tolist() == [0, 0, 0, 0] and not status.any() and sizes.size == 0
    rc, toff, status, sizes = device(ctx, [[(1, 100, 5)], [], [(9, 0, 1), (10, 16383, 4)]])
    assert rc == 0 and toff.tolist() == [0, 0, 0, 0] and not status.any()


def test_refusals(ctx):
    lib, h = ctx.lib, ctx.h
    off, start, span, slen = CC.flatten([CC.plain(3), CC.plain(2)])
    toff, status = np.full(3, -7, np.int64), np.full(2, -7, np.int32)
    sizes = np.full(64, -7, np.int64)

    def call(off=off, start=start, span=span, slen=slen, n=2, toff=toff, status=status):
        return lib.gd_crai_sizes(h, n, ptr(off), ptr(start), ptr(span), ptr(slen), ptr(toff), ptr(status), sizes.ctypes.data, sizes.size)

    assert call() == 0 and toff[-1] > 0 and (sizes[:toff[-1]] > 0).all()
    sizes[:] = -7
    assert call(n=-1) == GD_E_INVALID
    assert call(off=np.array([1, 3, 5], np.int64)) == GD_E_INVALID                        # does not start at 0
    assert call(off=np.array([0, 4, 3], np.int64)) == GD_E_INVALID                        # decreases
    assert call(off=None) == GD_E_INVALID and call(toff=None) == GD_E_INVALID and call(status=None) == GD_E_INVALID
    assert call(start=None) == GD_E_INVALID and call(span=None) == GD_E_INVALID and call(slen=None) == GD_E_INVALID
    assert lib.gd_crai_sizes(None, 2, ptr(off), ptr(start), ptr(span), ptr(slen), ptr(toff), ptr(status), None, 0) == GD_E_INVALID
    for arr, k, v in ((start, 4, 2 ** 31), (start, 0, -(2 ** 31)), (span, 2, 2 ** 31), (span, 3, -1)):
        bad = arr.copy()
        bad[k] = v
        assert (call(start=bad) if arr is start else call(span=bad)) == GD_E_RANGE
        assert (b"slice %d" % k) in lib.gd_last_error(h)
    assert (sizes == -7).all()                                                           # nothing was launched
    ok = start.copy()
    ok[0], ok[4] = -(2 ** 31 - 1), 2 ** 31 - 1                                           # the bounds themselves
    n = [len(CR.make_sizes(list(zip(ok[a:b].tolist(), span[a:b].tolist(), slen[a:b].tolist())))[0]) for a, b in ((0, 3), (3, 5))]
    assert call(start=ok) == GD_E_CAPACITY and toff.tolist() == [0, n[0], n[0] + n[1]] and n[1] > 2 ** 17 - 2   # (more tiles than 64)
    assert lib.gd_crai_sizes(h, 2, ptr(off), ptr(ok), ptr(span), ptr(slen), ptr(toff), ptr(status), None, 0) == 0
