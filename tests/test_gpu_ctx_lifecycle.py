"""GPU: what a context owns, over its life.  gd_destroy with every kept state alive at once; adopted records and a
caller's stream, which are the caller's before and after; a second gd_*_begin on a used context; arrays that grow and
keep what they held.  Every call here is one a correct library answers with GD_OK; nothing is freed or read that is
expected to be invalid, and free device memory is never looked at (the device is shared).

The covstats state is compared through gd_covstats_histogram right after gd_covstats_begin (tests/test_gpu_covstats_abi.py
decodes ranges on one context, begin after begin).  tests/test_gpu_soak.py grows a context's arrays from job to job with
random sizes; the growth case here does it with sizes chosen to cross a contig's capacity twice."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from goleft_amd import _lib
from goleft_amd.engine import DepthEngine, PATH_CHUNK
from oracle import pyoracle as po
from tests import helpers as H

pytestmark = pytest.mark.gpu

T = 4096                                                 # reference positions per tile
L2 = 2 * T                                               # the two-tile contig


@pytest.fixture(scope="module")
def two_tiles():
    """The two-tile contig's records and their per-base depth from the oracle, computed once."""
    r = H.random_reads(np.random.default_rng(4101), L2, 300)
    return r, po.perbase_c(r, 1, 0, L2)


def compute_two_tiles(eng, r):
    eng.set_params(window_size=250, min_mapq=1, min_cov=4)
    eng.set_contigs([L2])
    eng.push(0, r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
    eng.compute()
    return eng.perbase(0)


def bgzf(payload: bytes) -> bytes:
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    d = co.compress(payload) + co.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(d) + 25) + d +
            struct.pack("<II", zlib.crc32(payload), len(payload)))


def indexsplit_begin(eng, longest):
    a = np.asarray(longest, np.int32)
    eng._chk(eng._lib.gd_indexsplit_begin(eng._ctx, len(a), a.ctypes.data))


def indexsplit_sums(eng, longest, sizes):
    """One sample whose tiles are `sizes` per reference: begin, add, the cell sums."""
    indexsplit_begin(eng, longest)
    flat = np.ascontiguousarray(np.concatenate(sizes), np.int64)
    cnt = np.array([len(s) for s in sizes], np.int32)
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    soff = np.array([0, len(flat)], np.int64)
    eng._chk(eng._lib.gd_indexsplit_add(eng._ctx, 1, soff.ctypes.data, flat.ctypes.data, off.ctypes.data, cnt.ctypes.data))
    out = np.zeros(int(np.sum(longest)), np.float64)
    eng._chk(eng._lib.gd_indexsplit_sums(eng._ctx, out.ctypes.data, out.size))
    return out


def indexcov_upload(eng):
    """Two samples, two references of a few index tiles."""
    cnt = np.array([3, 2, 2, 2], np.int32)                   # [sample][reference]
    toff = np.array([0, 3, 5, 7], np.int64)
    soff = np.array([0, 5, 9], np.int64)
    sizes = np.arange(1, 10, dtype=np.int64) * 1000
    sex = np.array([0, 1], np.uint8)
    eng._chk(eng._lib.gd_indexcov_upload(eng._ctx, 2, 2, soff.ctypes.data, sizes.ctypes.data, toff.ctypes.data,
                                         cnt.ctypes.data, sex.ctypes.data))


EM_DEPTHS = np.array([[30, 31, 29], [30, 60, 15], [31, 58, 14]], np.float32)      # the 3 x 3 matrix
EM_STARTS = np.array([0, 100, 200], np.uint32)
EM_ENDS = np.array([100, 200, 300], np.uint32)


def emcnv_begin_add(eng, depths=EM_DEPTHS):
    n = len(depths)
    eng._chk(eng._lib.gd_emcnv_begin(eng._ctx, depths.shape[1]))
    eng._chk(eng._lib.gd_emcnv_add(eng._ctx, depths.ctypes.data, n, EM_STARTS[:n].ctypes.data, EM_ENDS[:n].ctypes.data, None))


def test_destroy_with_every_kept_state_alive(two_tiles):
    r, want = two_tiles
    eng = DepthEngine(0)
    eng.set_path(PATH_CHUNK)                                 # the long-read block of the contig exists after this compute
    assert np.array_equal(compute_two_tiles(eng, r), want)
    eng.covstats_begin(10, 0)
    indexcov_upload(eng)
    indexsplit_begin(eng, [3, 2])
    emcnv_begin_add(eng)
    eng.md_begin(L2)
    eng.seq_load(b"ACGTN" * 20)
    held = eng.acquire(16, 16)                               # a staging block that is never committed
    assert held.pos and held.reads_cap >= 16
    eng.ingest_feed_range(bgzf(b"x" * 100) + bgzf(b"y" * 50), 0)      # a range begun and fed, not decoded
    eng.close()
    with DepthEngine(0) as fresh:
        assert np.array_equal(compute_two_tiles(fresh, r), want)


def test_adopted_records_stay_the_callers(two_tiles):
    r, want = two_tiles
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    arrays = [np.ascontiguousarray(a) for a in (r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)]
    with DepthEngine(0) as a:
        ptrs = [a.device_alloc(x.nbytes) for x in arrays]
        for p, x in zip(ptrs, arrays):
            assert hip.hipMemcpy(p, x.ctypes.data, x.nbytes, 1) == 0           # hipMemcpyHostToDevice
        b = DepthEngine(0)
        b.set_contigs([L2])
        batch = _lib.GdBatch(*ptrs, len(r.pos), len(r.cigar), -1)
        b._chk(b._lib.gd_adopt_device(b._ctx, 0, C.byref(batch), len(r.pos), len(r.cigar)))
        b.compute()
        assert np.array_equal(b.perbase(0), want)
        b.close()
        for p, x in zip(ptrs, arrays):                       # the same bytes, through the context that allocated them
            back = np.zeros_like(x)
            a._chk(a._lib.gd_device_read(a._ctx, back.ctypes.data, C.c_void_p(p), x.nbytes))
            assert np.array_equal(back, x)
        for p in ptrs:
            a.device_free(p)                                 # (raises unless GD_OK)


def test_a_callers_stream_survives_the_context(two_tiles):
    import torch
    r, want = two_tiles
    s = torch.cuda.Stream(device=0)
    eng = DepthEngine(0, stream=s.cuda_stream)
    assert np.array_equal(compute_two_tiles(eng, r), want)
    eng.close()
    with torch.cuda.stream(s):
        total = torch.arange(8, device="cuda:0").sum()
    s.synchronize()
    assert int(total) == 28
    # back to a stream of the context's own after a caller's
    with DepthEngine(0, stream=s.cuda_stream) as eng:
        eng._chk(eng._lib.gd_set_stream(eng._ctx, None))
        assert np.array_equal(compute_two_tiles(eng, r), want)
    with torch.cuda.stream(s):
        total = torch.arange(9, device="cuda:0").sum()
    s.synchronize()
    assert int(total) == 36


def kept_state_outputs(eng):
    """What the three states give that a begin starts over, as bytes."""
    sums = indexsplit_sums(eng, [3, 2], [np.array([1, 2, 3]) * 10 ** 9, np.array([5, 7]) * 10 ** 9])
    eng.covstats_begin(10, 0)
    hist = [eng.covstats_histogram(k) for k in range(3)]
    cnv = eng.emdepth_cnvs(EM_DEPTHS, EM_STARTS, EM_ENDS)
    out = [sums.tobytes()] + [struct.pack("<q", lo) + b.tobytes() + o.tobytes() for lo, b, o in hist]
    return out + [cnv[k].tobytes() for k in ("sample", "psize", "emit_row", "member_off", "member_row", "depth", "cn", "log2fc", "site_cn")]


def test_begin_again_on_a_used_context():
    with DepthEngine(0) as fresh:
        want = kept_state_outputs(fresh)
    assert want[0] == np.array([1, 2, 3, 5, 7], np.float64).tobytes()
    with DepthEngine(0) as eng:
        indexsplit_sums(eng, [2, 4, 1], [np.array([9, 9]) * 10 ** 9, np.array([8] * 4) * 10 ** 9, np.array([4]) * 10 ** 9])
        eng.covstats_begin(5, 1)
        emcnv_begin_add(eng, np.ascontiguousarray(EM_DEPTHS[:2] * 2))      # begun and fed, then ended by the next begin
        eng._chk(eng._lib.gd_emcnv_end(eng._ctx))
        emcnv_begin_add(eng)                                 # ... and once more without an end in between
        assert kept_state_outputs(eng) == want
        assert kept_state_outputs(eng) == want


def commit(eng, tid, r, a, b):
    """Records a .. b of r through gd_acquire / gd_commit (the contig's arrays at least double when they grow)."""
    o0, o1 = int(r.cigar_off[a]), int(r.cigar_off[b])
    blk = eng.acquire(b - a, max(o1 - o0, 1))
    for dst, src in ((blk.pos, r.pos[a:b]), (blk.flag, r.flag[a:b]), (blk.mapq, r.mapq[a:b]),
                     (blk.cigar_off, (r.cigar_off[a:b + 1] - o0).astype(np.uint32)), (blk.cigar, r.cigar[o0:o1])):
        src = np.ascontiguousarray(src)
        C.memmove(dst, src.ctypes.data, src.nbytes)
    eng.commit(blk, tid, b - a, o1 - o0)


def test_growth_keeps_what_was_there():
    rng = np.random.default_rng(4102)
    L1 = 5 * T + 17                                          # more tiles than the two-tile contig: the tile tables grow
    r0, r1 = H.random_reads(rng, L2, 650), H.random_reads(rng, L1, 400)
    with DepthEngine(0) as eng:
        eng.set_params(window_size=250, min_mapq=1, min_cov=4)
        eng.set_contigs([L2, L1])
        # 100 records, then 250 (past the capacity of 100), then 650 (past the 250 that took): two growths with a prefix kept
        for a, b in ((0, 100), (100, 250), (250, 650)):
            commit(eng, 0, r0, a, b)
        eng.push(1, r1.pos, r1.flag, r1.mapq, r1.cigar_off, r1.cigar)
        eng.select_contigs([0])
        eng.compute()
        assert np.array_equal(eng.perbase(0), po.perbase_c(r0, 1, 0, L2))
        eng.select_contigs([])                               # both contigs: seven tiles after two
        eng.compute()
        assert np.array_equal(eng.perbase(0), po.perbase_c(r0, 1, 0, L2))
        assert np.array_equal(eng.perbase(1), po.perbase_c(r1, 1, 0, L1))
        sums, mins = eng.windows(1)
        ws, wm = H.oracle_windows(po.perbase_c(r1, 1, 0, L1), 250)
        assert np.array_equal(sums, ws) and np.array_equal(mins, wm)
