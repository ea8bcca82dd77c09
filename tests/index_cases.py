"""Synthetic BAMs for the indexer's tests (tests/test_gpu_index.py): each holds what a .bai rule or a structural edge of the
device indexer needs, and tests/bai_ref.py says what its index must be.  Written with tests/covstats_ref.py's BAM writer."""
from __future__ import annotations

import struct

from tests import covstats_ref as CR

REFS = [("big", 1 << 30), ("none1", 1000), ("mid", 300000), ("none3", 5000), ("tail", 70000)]


def decoy_tag(n, pad=0):
    """A B:C tag of `pad` filler bytes and then n fake 40-byte record heads, 44 bytes apart, the last one ending with the
    record: each passes the candidate test on its own (block_size 100, reference 0, position 5, a one-byte name that is
    NUL, no mate) and none leads to a record -- the guesses a chain check of 0 falls for."""
    fake = struct.pack("<iiiBBHHHiiii", 100, 0, 5, 1, 0, 4680, 0, 0, 0, -1, -1, 0) + b"\0\0\0\0" + b"\xee" * 4
    assert len(fake) == 44
    body = b"\xee" * pad + fake * n
    return b"zzBC" + struct.pack("<i", len(body)) + body


def edge_records(pad=0):
    """Every content rule of the issue in one record list (file order), over REFS; pad: filler in the long record."""
    R = CR.Rec
    recs = []
    # reference 0: ends that cross 2^14, 2^17, 2^20, 2^23 and 2^26; a read touching five windows; rlen 0; placed-unmapped
    recs.append(R(0, 100, 0, cigar=[(0, 80)]))
    recs.append(R(0, 3 * 16384 + 100, 0, cigar=[(0, 100), (3, 65536), (0, 100)]))        # windows 3 .. 7
    for k in (14, 17, 20, 23, 26):
        recs.append(R(0, (1 << k) - 50, 0, cigar=[(0, 100)]))
        recs.append(R(0, (1 << k) - 50, 16, cigar=[(0, 30)]))                             # the same window, a lower bin level
    recs.append(R(0, (1 << 26) + 5, 0, cigar=[(4, 60)]))                                  # mapped, rlen 0: 60S
    recs.append(R(0, (1 << 26) + 5, 0, cigar=[]))                                         # mapped, no CIGAR at all
    recs.append(R(0, (1 << 26) + 9, 4 | 8, cigar=[]))                                     # placed-unmapped
    recs.append(R(0, (1 << 26) + 9, 4, cigar=[(0, 5000)]))                                # ... with a CIGAR that does not count
    # a CG:B,I placeholder: 10S 50000N stored, the real CIGAR in the tag (not consulted: the N carries the length)
    cg = b"CGBI" + struct.pack("<i", 3) + struct.pack("<3I", (10 << 4) | 4, (49000 << 4) | 0, (1000 << 4) | 2)
    recs.append(R(0, (1 << 26) + 100, 0, cigar=[(4, 10), (3, 50000)], l_seq=10, tags=cg))
    recs.append(R(0, (1 << 29) - 100, 0, cigar=[(0, 100)]))                               # ends exactly at 2^29
    recs.sort(key=lambda r: r.pos)                                                        # (stable: ties keep their order)
    # reference 2: a long record (five fake heads per 256 bytes of it), then plain reads
    recs.append(R(2, 10, 0, cigar=[(0, 50)], tags=decoy_tag(80, pad)))                         # 3.5 kb: longer than two slices of 1 kb
    for i in range(120):
        recs.append(R(2, 1000 + 150 * i, 99 if i % 3 else 0, cigar=[(0, 100)], next_pos=1200 + 150 * i, tlen=300))
    # reference 4: one window; then the unplaced tail
    for i in range(40):
        recs.append(R(4, 16384 * 2 + i, 0, cigar=[(0, 10), (2, 5), (7, 3), (8, 2), (1, 9)]))
    for i in range(25):
        recs.append(R(-1, -1, 4 | (64 if i % 2 else 128), cigar=[]))
    return recs


def write(path, recs, refs=REFS, block=4000, cuts=None):
    CR.write_bam(str(path), refs, recs, block=block, index=False, cuts=cuts)
    return str(path)


def write_edges(path, **kw):
    """edge_records() as a BAM whose long record ends 44 bytes into a 64-byte slice (counted from the first record): the slice
    that holds the next record's start holds a fake head in front of it, so with slices of 64 or 1024 bytes the guess there
    is wrong and the segment it opens holds a true start -- a repair round is certain, not likely."""
    write(path, edge_records(), **kw)
    first, starts, total = layout(path)
    size = [b - a for a, b in zip(starts, starts[1:] + [total])]
    k = max(range(len(size)), key=lambda i: size[i])
    write(path, edge_records((44 - (starts[k + 1] - first)) % 64), **kw)
    first, starts, total = layout(path)
    assert (starts[k + 1] - first) % 64 == 44
    return str(path)


def layout(path):
    """(inflated offset of the first record, inflated offsets of all record starts, inflated size) of a BAM."""
    from oracle import bamio
    d = bamio.bgzf_decompress(open(path, "rb").read())
    l_text, = struct.unpack_from("<i", d, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, p)
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", d, p)[0]
    first, starts = p, []
    while p < len(d):
        starts.append(p)
        p += 4 + struct.unpack_from("<i", d, p)[0]
    return first, starts, len(d)


def member_cuts(special):
    """A `cuts` callable for covstats_ref.write_bam: a member boundary every 3000 bytes, and whatever special(header
    length, record starts, stream length) adds."""
    def cuts(first, starts, total):
        c = set(range(3000, total, 3000)) | set(special(first, starts, total))
        return sorted(x for x in c if 0 < x < total)
    return cuts


# ---- wrong guesses that walk cleanly --------------------------------------------------------------------------------------

FAKE_SIGNATURE = struct.pack("<iiBBHHHiiii", 0, 5, 1, 0, 4680, 0, 0, 0, -1, -1, 0) + b"\0\0\0\0" + b"\xee" * 4   # what follows a fake's block_size


def candidate(d, o, ref_len):
    """gd_bamguess.hpp's bam_candidate in Python: where the record behind a candidate at o would begin, or None."""
    if len(d) - o < 36:
        return None
    bs, ref, pos, l_rn, _mq, _bin, n_cig, _flag, l_seq, mref, mpos = struct.unpack_from("<IiiBBHHHIii", d, o)
    if bs < 32 or not -1 <= ref < len(ref_len) or not -1 <= mref < len(ref_len):
        return None
    if pos < -1 or (ref >= 0 and pos >= ref_len[ref]) or mpos < -1 or (mref >= 0 and mpos >= ref_len[mref]):
        return None
    if l_rn < 1 or 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
        return None
    nul = o + 36 + l_rn - 1
    if nul >= len(d) or d[nul] != 0:
        return None
    return o + 4 + bs


def slice_guesses(d, first, slice_, ref_len):
    """The lowest candidate of every slice (a chain check of 0), slice 0's being `first`; ascending, as the host keeps them."""
    out = [first]
    for beg in range(first + slice_, len(d), slice_):
        g = next((o for o in range(beg, min(beg + slice_, len(d))) if candidate(d, o, ref_len) is not None), None)
        if g is not None and g > out[-1]:
            out.append(g)
    return out


def write_leaps(path, n=160, ahead=250):
    """Reads of about 100 bytes, each with one fake record head in a tag whose block_size lands EXACTLY on a true record start at
    least `ahead` bytes on: a walk that starts on a fake is clean -- one record that is none, then true ones -- and stops
    several slices of 64 bytes later.  -> (path, inflated stream, first record, record starts)."""
    from oracle import bamio
    recs = [CR.Rec(2, 100 + 7 * i, 0, cigar=[(0, 50)], tags=decoy_tag(1, i % 7)) for i in range(n)]
    recs += [CR.Rec(-1, -1, 4, cigar=[]) for _ in range(10)]
    write(path, recs)
    first, starts, total = layout(path)
    d = bytearray(bamio.bgzf_decompress(open(path, "rb").read()))
    at, fakes = 0, []
    while True:
        at = d.find(FAKE_SIGNATURE, at + 1)
        if at < 0:
            break
        fakes.append(at - 4)
    assert len(fakes) == n
    for f in fakes:
        target = next((s for s in starts if s >= f + ahead), None)
        if target is not None:                             # (the last few keep block_size 100 and lead nowhere)
            struct.pack_into("<i", d, f, target - f - 4)
    with open(path, "wb") as fh:
        fh.write(bamio.bgzf_compress(bytes(d), block=4000, level=1))
    return str(path), bytes(d), first, starts
