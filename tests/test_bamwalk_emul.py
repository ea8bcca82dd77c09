"""CPU: the device BAM record walk (goleft_amd/csrc/gd_bamdecode.hpp) compiled for the HOST and run lane by lane
(tests/emul/bamwalk_emul.cpp), the inflated stream and every output array ending exactly at an inaccessible page -- under
the depth read's policy (the two passes) and under covstats' (every record to a CsRec slot).  On
intact streams the walks deliver what the records say; on damaged streams -- the fields a walk trusts flipped:
block_size, refID, POS, l_read_name, n_cigar_op, l_seq, the CIGAR, the CG tag -- the walk must terminate and never
touch a byte outside the stream or its outputs (a stray access is a segmentation fault of the child process).  The GPU
twin of this test (tests/test_gpu_bamdecode.py::test_device_bam_walker_mutation_fuzz) compares with the host decoder;
a read past the end is silent there."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from oracle import bamio
from tests import helpers as H

EMUL_DIR = os.path.join(H.ROOT, "tests", "emul")
CLANG = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++") or "") if p and os.path.exists(p)), None)

pytestmark = pytest.mark.skipif(CLANG is None, reason="the kernel source is compiled for the host with clang")


def _lib():
    src = os.path.join(EMUL_DIR, "bamwalk_emul.cpp")
    so = os.path.join(EMUL_DIR, "bamwalk_emul.so")
    deps = [src, os.path.join(EMUL_DIR, "emul_machine.hpp"), os.path.join(H.ROOT, "goleft_amd", "csrc", "gd_bamdecode.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call([CLANG, "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = C.CDLL(so)
    lib.emul_bam_walk.argtypes = ([C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32] + [C.c_void_p] * 7 +
                                  [C.c_uint64, C.c_uint64] + [C.c_void_p] * 5)
    lib.emul_bam_walk.restype = C.c_int
    lib.emul_cs_walk.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint64, C.c_void_p]
    lib.emul_cs_walk.restype = C.c_int
    lib.emul_bam_walk_mode(C.c_int(MODE))
    return lib


# how the records are extracted: 1 (what gd_api_ingest.inc does) the counting walk leaves a table of record starts and
# gd_bam_extract_tab_kernel takes a thread per record; 0 the second walk (kept for segments of 4 GB and more)
MODE = 1


@pytest.fixture(params=[1, 0], ids=["record-table", "second-walk"])
def both_extractions(request):
    global MODE
    MODE = request.param
    yield request.param
    MODE = 1


def record_starts(d: bytes):
    """(offset, refID) of every record of an inflated BAM."""
    l_text, = struct.unpack_from("<i", d, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", d, p)
        p += 8 + l_name
    out = []
    while p + 8 <= len(d):
        bs, ref = struct.unpack_from("<ii", d, p)
        out.append((p, ref))
        p += 4 + bs
    return out, n_ref


def walk(data: bytes, anchors, tid, n_ref):
    """The two passes over the segments [anchor_i, anchor_i+1) (the last one to the end of the stream).
    -> (rc, per-segment dict, arrays or None)"""
    lib = _lib()
    raw = np.frombuffer(data, np.uint8)
    beg = np.asarray(anchors, np.uint64)
    end = np.concatenate([beg[1:], [len(data)]]).astype(np.uint64)
    n = len(beg)
    n_rec = np.zeros(n, np.uint32); n_ops = np.zeros(n, np.uint64); first = np.zeros(n, np.int32); last = np.zeros(n, np.int32)
    flags = np.zeros(n, np.uint32)
    N = C.c_uint64(0); M = C.c_uint64(0)
    cap_rec, cap_ops = len(data) // 36 + 1, len(data) // 4 + 1
    pos = np.zeros(cap_rec, np.int32); flag = np.zeros(cap_rec, np.uint16); mapq = np.zeros(cap_rec, np.uint8)
    off = np.zeros(cap_rec + 1, np.uint32); cig = np.zeros(cap_ops, np.uint32)
    rc = lib.emul_bam_walk(raw.ctypes.data, len(data), beg.ctypes.data, end.ctypes.data, n, tid, n_ref, n_rec.ctypes.data,
                           n_ops.ctypes.data, first.ctypes.data, last.ctypes.data, flags.ctypes.data, C.byref(N), C.byref(M),
                           cap_rec, cap_ops, pos.ctypes.data, flag.ctypes.data, mapq.ctypes.data, off.ctypes.data, cig.ctypes.data)
    seg = dict(n_rec=n_rec, n_ops=n_ops, first=first, last=last, flags=flags)
    if rc != 0:
        return rc, seg, None
    off[N.value] = M.value
    return rc, seg, (pos[:N.value], flag[:N.value], mapq[:N.value], off[:N.value + 1], cig[:M.value])


def make_stream(tmp_path, seed, long_cigars=False):
    rng = np.random.default_rng(seed)
    contigs = [("c1", 300_000), ("c2", 120_000), ("c3", 50_000)]
    reads = {0: H.random_reads(rng, 300_000, 2500, max_len=150), 2: H.random_reads(rng, 50_000, 400, max_len=150)}
    if long_cigars:                                          # one CIGAR behind the CG:B,I tag (more than 65 535 ops)
        r = reads[0]
        ops = np.tile(np.asarray([(1 << 4) | 0, (1 << 4) | 2], np.uint32), 33_000)
        cig = np.concatenate([r.cigar, ops])
        off = np.concatenate([r.cigar_off, [r.cigar_off[-1] + len(ops)]]).astype(np.uint32)
        reads[0] = type(r)(np.concatenate([r.pos, [r.pos[-1]]]).astype(np.int32), np.concatenate([r.flag, [0]]).astype(np.uint16),
                           np.concatenate([r.mapq, [60]]).astype(np.uint8), off, cig)
    path = str(tmp_path / ("s%d.bam" % seed))
    bamio.write_bam(path, contigs, reads, unplaced=3)
    return bamio.bgzf_decompress(open(path, "rb").read()), contigs, reads


@pytest.mark.parametrize("long_cigars", [False, True])
def test_walk_delivers_the_records(tmp_path, long_cigars, both_extractions):
    data, contigs, reads = make_stream(tmp_path, 1, long_cigars)
    starts, n_ref = record_starts(data)
    for tid in (0, 2):
        mine = [p for p, ref in starts if ref == tid]
        for step in (1, 7, 64, 100_000):                     # an anchor per record ... one anchor for the whole contig
            rc, seg, arr = walk(data, mine[::step], tid, n_ref)
            assert rc == 0 and not (seg["flags"] & 7).any()
            r = reads[tid]
            assert int(seg["n_rec"].sum()) == r.n
            assert np.array_equal(arr[0], r.pos) and np.array_equal(arr[1], r.flag) and np.array_equal(arr[2], r.mapq)
            assert np.array_equal(arr[3], r.cigar_off) and np.array_equal(arr[4], r.cigar)
            # the contig's walk ends at the first record of another reference: bit 3 on the last segment, no resume
            assert seg["flags"][-1] & 8 and not (seg["flags"] & 16).any()
    # an anchor that is no record start: the walk overruns the next anchor (bit 2) or meets a corrupt record (bit 1)
    mine = [p for p, ref in starts if ref == 0]
    rc, seg, _ = walk(data, [mine[0], mine[5] + 3, mine[9]], 0, n_ref)
    assert rc == 1 and (seg["flags"] & 6).any()


FUZZ = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
from tests import test_bamwalk_emul as T
import pathlib, tempfile
seed = int(sys.argv[1])
tmp = pathlib.Path(tempfile.mkdtemp())
data, contigs, reads = T.make_stream(tmp, 50 + seed, long_cigars=(seed %% 2 == 1))
starts, n_ref = T.record_starts(data)
mine = [p for p, ref in starts if ref == 0]
rng = np.random.default_rng(seed)
clean = refused = 0
for case in range(120):
    d = bytearray(data)
    for _ in range(int(rng.integers(1, 6))):
        s = mine[int(rng.integers(0, len(mine)))]
        # block_size, refID, POS, l_read_name, MAPQ / bin, n_cigar_op, flag, l_seq, the first CIGAR bytes, anywhere in the record
        at = s + [int(rng.integers(0, 4)), 4 + int(rng.integers(0, 4)), 8 + int(rng.integers(0, 4)), 12, 13 + int(rng.integers(0, 3)),
                  16 + int(rng.integers(0, 2)), 18 + int(rng.integers(0, 2)), 20 + int(rng.integers(0, 4)), 36 + int(rng.integers(0, 30)),
                  int(rng.integers(0, 300))][int(rng.integers(0, 10))]
        if at < len(d):
            d[at] = (d[at] ^ (1 << int(rng.integers(0, 8)))) if rng.random() < 0.6 else int(rng.integers(0, 256))
    if case %% 5 == 4:                                        # and the stream cut anywhere (a range that ends inside a record)
        d = d[:int(rng.integers(mine[0] + 1, len(d)))]
    anchors = [a for a in mine[::int(rng.integers(1, 40))] if a < len(d)] or [mine[0]]
    rc, seg, arr = T.walk(bytes(d), anchors, 0, n_ref)
    if rc == 0:
        clean += 1
        pos, flag, mapq, off, cig = arr
        assert len(off) == len(pos) + 1 and (np.diff(off.astype(np.int64)) >= 0).all() and off[-1] == len(cig)
    else:
        refused += 1
print("clean", clean, "refused", refused)
"""


@pytest.mark.parametrize("seed", range(4))
def test_damaged_streams_never_leave_their_buffers(seed):
    r = subprocess.run([sys.executable, "-c", FUZZ % H.ROOT, str(seed)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-2000:])
    clean, refused = int(r.stdout.split()[1]), int(r.stdout.split()[3])
    assert clean + refused == 120 and refused > 20


# ---- the covstats walk (gd_cs_walk_kernel: the same bam_walk under the CsWalk policy) ---------------------------------

CS_REC = np.dtype([("flag", "<u4"), ("pos", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"), ("mlen", "<u4"), ("pad", "<u4"),
                   ("qlen", "<u8")])
CS_NOT_M = 0xffffffff
CORRUPT, OVERRAN = 2, 4                  # gd::BW_CORRUPT, gd::BW_OVERRAN


def cs_walk(data: bytes, anchors, open_end):
    """The covstats walk over the segments [anchor_i, anchor_i+1) (the last one to the end of the stream).
    -> (rc, per-segment dict, records in file order or None)"""
    lib = _lib()
    raw = np.frombuffer(data, np.uint8)
    beg = np.asarray(anchors, np.uint64)
    end = np.concatenate([beg[1:], [len(data)]]).astype(np.uint64)
    n = len(beg)
    n_rec = np.zeros(n, np.uint32); end_off = np.zeros(n, np.uint64); flags = np.zeros(n, np.uint32)
    N = C.c_uint64(0)
    cap = len(data) // 36 + 1
    recs = np.zeros(cap, CS_REC)
    rc = lib.emul_cs_walk(raw.ctypes.data, len(data), beg.ctypes.data, end.ctypes.data, n, open_end, n_rec.ctypes.data,
                          end_off.ctypes.data, flags.ctypes.data, C.byref(N), cap, recs.ctypes.data)
    seg = dict(n_rec=n_rec, end_off=end_off, flags=flags, seg_end=end)
    return rc, seg, (recs[:N.value] if rc == 0 else None)


def parse_cs(d: bytes, starts):
    """What a CsRec must hold for the records at `starts`: a direct parse of the bytes, the STORED CIGAR as it stands."""
    out = np.zeros(len(starts), CS_REC)
    for i, p in enumerate(starts):
        bs, ref, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, next_ref, next_pos, tlen = struct.unpack_from("<iiiBBHHHIiii", d, p)
        ops = struct.unpack_from("<%dI" % n_cigar, d, p + 36 + l_name)
        qlen = sum(op >> 4 for op in ops if (op & 0xf) in (0, 1, 4, 7, 8))
        mlen = ops[0] >> 4 if n_cigar == 1 and (ops[0] & 0xf) == 0 else CS_NOT_M
        out[i] = (flag, pos, next_pos, tlen, mlen, 0, qlen)
    return out


@pytest.mark.parametrize("long_cigars", [False, True])
def test_cs_walk_delivers_every_record(tmp_path, long_cigars):
    data, contigs, reads = make_stream(tmp_path, 1, long_cigars)
    starts, n_ref = record_starts(data)
    every = [p for p, ref in starts]                          # ALL references and the unplaced tail
    assert {ref for p, ref in starts} == {0, 2, -1}
    want = parse_cs(data, every)
    if long_cigars:                                           # the <l_seq>S<ref_len>N placeholder counts as stored: its S is the query length
        ph = [i for i, p in enumerate(every) if struct.unpack_from("<i", data, p)[0] > 4 * 65_535]   # (only a CG:B,I tag is that long)
        assert ph and all(struct.unpack_from("<H", data, every[i] + 16)[0] == 2 and want["mlen"][i] == CS_NOT_M and
                          want["qlen"][i] == struct.unpack_from("<I", data, every[i] + 20)[0] for i in ph)
    for step in (1, 7, 64, len(every)):                       # a segment per record ... one segment for the whole range
        for open_end in (0, 1):
            rc, seg, recs = cs_walk(data, every[::step], open_end)
            assert rc == 0 and not seg["flags"].any()
            assert int(seg["n_rec"].sum()) == len(every)
            assert np.array_equal(seg["end_off"], seg["seg_end"])
            assert np.array_equal(recs, want)


def test_cs_walk_a_stream_cut_inside_a_record(tmp_path):
    data, contigs, reads = make_stream(tmp_path, 1)
    starts, n_ref = record_starts(data)
    every = [p for p, ref in starts]
    k = len(every) - 40
    for inside in (2, 20, every[k + 1] - every[k] - 1):       # in block_size, in the fixed fields, one byte short of whole
        d = data[:every[k] + inside]
        want = parse_cs(d, every[:k])
        for anchors in (every[:k + 1:7], every[:1]):
            # the cut record is the last segment's: the next range begins with it when more of the file follows
            rc, seg, recs = cs_walk(d, anchors, 1)
            assert rc == 0 and not seg["flags"].any()
            assert int(seg["end_off"][-1]) == every[k] and np.array_equal(recs, want)
            rc, seg, recs = cs_walk(d, anchors, 0)
            assert rc == 1 and seg["flags"][-1] & CORRUPT and not seg["flags"][:-1].any()
        # the cut inside a segment that is not the last (its end lies behind the stream's): damaged in both modes
        for open_end in (0, 1):
            rc, seg, recs = cs_walk(d, [every[0], every[k + 5]], open_end)
            assert rc == 1 and seg["flags"][0] & CORRUPT


def test_cs_walk_an_anchor_that_is_no_record_start(tmp_path):
    data, contigs, reads = make_stream(tmp_path, 1)
    starts, n_ref = record_starts(data)
    every = [p for p, ref in starts]
    for open_end in (0, 1):
        # the walk overruns the next anchor (bit 2) or meets a corrupt record (bit 1)
        rc, seg, _ = cs_walk(data, [every[0], every[5] + 3, every[9]], open_end)
        assert rc == 1 and (seg["flags"] & (CORRUPT | OVERRAN)).any()


# The same damage as FUZZ (fields, seeds, cases), the covstats walk over it; every other case with more of the file to follow.
_DEPTH_CALL = FUZZ[FUZZ.index("    rc, seg, arr = T.walk("):FUZZ.index("    else:\n        refused += 1")]
FUZZ_CS = FUZZ.replace(_DEPTH_CALL, """    rc, seg, recs = T.cs_walk(bytes(d), anchors, case %% 2)
    if rc == 0:
        clean += 1
        assert len(recs) == int(seg["n_rec"].sum()) and int(seg["end_off"][-1]) <= len(d)
""")


@pytest.mark.parametrize("seed", range(4))
def test_damaged_streams_never_leave_the_cs_walks_buffers(seed):
    r = subprocess.run([sys.executable, "-c", FUZZ_CS % H.ROOT, str(seed)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-2000:])
    clean, refused = int(r.stdout.split()[1]), int(r.stdout.split()[3])
    # (this walk has no refID or sortedness test and refuses fewer than the depth walk: 73 / 88 / 70 / 76 of 120 for the
    # four seeds, where the depth walk refuses 95 / 103 / 88 / 93)
    assert clean + refused == 120 and refused > 20
