"""-m gpu: gd_commit's host validation of a block the caller filled, below and above the 2^18 records from which the
context's worker threads share it in pieces of 65 536 records: a position out of order and a CSR offset that dips, at
a piece seam and inside a piece, are refused with the status and -- for positions -- the record number of the first
fault, and the context goes on."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PIECE = 1 << 16
L = 1_000_000


def block(n):
    """n sorted records of one 50M op each."""
    pos = (np.arange(n, dtype=np.int64) * (L - 100) // n).astype(np.int32)
    return dict(pos=pos, flag=np.zeros(n, np.uint16), mapq=np.full(n, 60, np.uint8),
                cigar_off=np.arange(n + 1, dtype=np.uint32), cigar=np.full(n, 50 << 4, np.uint32))


def commit(eng, rec, n):
    b = eng.acquire(n, n)
    for name, a in rec.items():
        a = np.ascontiguousarray(a)
        C.memmove(getattr(b, name), a.ctypes.data, a.nbytes)
    eng.commit(b, 0, n, n)


@pytest.mark.parametrize("n", [100_000, 300_000], ids=["below-2^18", "above-2^18"])
def test_bad_blocks_are_refused_where_they_go_wrong(n):
    from goleft_amd.engine import DepthEngine, GdError
    assert (n >= 1 << 18) == (n == 300_000) and n > PIECE + 5000
    good = block(n)
    with DepthEngine(0) as eng:
        eng.set_params(window_size=1000)
        eng.set_contigs([L])
        # (array, index whose entry falls below its predecessor, status, the record the message names)
        for name, k, status in (("pos", PIECE, -7), ("pos", PIECE + 4465, -7),
                                ("cigar_off", PIECE, -1), ("cigar_off", PIECE + 1, -1), ("cigar_off", PIECE + 4465, -1)):
            rec = dict(good)
            rec[name] = good[name].copy()
            rec[name][k] = rec[name][k - 1] - 1
            eng.reset()
            with pytest.raises(GdError) as ei:
                commit(eng, rec, n)
            assert ei.value.status == status, (name, k, ei.value.status)
            if name == "pos":
                assert "contig 0 record %d: pos %d < %d" % (k, rec[name][k], rec[name][k - 1]) in str(ei.value), ei.value
            else:
                assert "cigar_off not monotone" in str(ei.value), ei.value
        eng.reset()
        commit(eng, good, n)
        eng.compute()
        d = eng.perbase(0)
        assert int(d.sum()) == 50 * n and int(d[good["pos"][PIECE]]) >= 1
