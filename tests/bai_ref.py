"""A .bai (SAMv1 5.2) from a BAM's records, as htslib's indexer writes it -- the model `goleft-depth index` is held to.

The rules, pinned byte for byte by tests/golden/ref/{t,hla,t-empty}.bam.bai, which htslib wrote:
  1 a record's interval is [pos, pos + rlen) with rlen the reference length of the STORED CIGAR (M D N = X), and
    [pos, pos + 1) when it is unmapped (flag 4) or rlen is 0; its bin is reg2bin of that, not the record's bin field
  2 its virtual offsets: begin = (member, offset) of its first byte, end = the begin of the record behind it; an offset
    on a member boundary names the member that BEGINS there and has bytes; the last record ends at file size << 16
  3 consecutive records of one (reference, bin) form one chunk
  4 htslib's compression: level 5 up to level 1, a bin spanning fewer than 65536 compressed bytes moves into its parent
    when the parent exists; then every bin's chunks are sorted and merged where they meet inside one member
  5 the linear index: the first record to touch a 16 kb window; unset windows inherit from the window behind them
  6 pseudo-bin 37450 per reference with records; n_no_coor behind the last reference
  7 bins ascending, the pseudo-bin last
  8 refusals: Refused(status name, message)
"""
from __future__ import annotations

import bisect
import struct

from oracle import bamio

PSEUDO_BIN = 37450
MAX_END = 1 << 29
UNSET = (1 << 64) - 1
LEVEL_FIRST = (0, 1, 9, 73, 585, 4681)          # the first bin of every level


class Refused(Exception):
    def __init__(self, status, message):
        super().__init__("%s: %s" % (status, message))
        self.status = status


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def bin_level(b):
    return max(l for l in range(6) if LEVEL_FIRST[l] <= b)


def members(raw):
    """[(file offset, inflated offset, inflated size)] of every BGZF member, and the inflated stream."""
    out, data, off, cum = [], [], 0, 0
    while off < len(raw):
        if raw[off:off + 4] != b"\x1f\x8b\x08\x04":
            raise Refused("GD_E_INVALID", "not a BGZF member at %d" % off)
        xlen, = struct.unpack_from("<H", raw, off + 10)
        p, bsize = off + 12, None
        while p < off + 12 + xlen:
            if raw[p] == 66 and raw[p + 1] == 67:
                bsize = struct.unpack_from("<H", raw, p + 4)[0] + 1
            p += 4 + struct.unpack_from("<H", raw, p + 2)[0]
        d = bamio.bgzf_decompress(raw[off:off + bsize])
        out.append((off, cum, len(d)))
        data.append(d)
        cum += len(d)
        off += bsize
    return out, b"".join(data)


def read(path):
    """(reference lengths, records, file size): a record is (ref, pos, flag, rlen, begin, end), the last two virtual."""
    raw = open(path, "rb").read()
    mem, d = members(raw)
    starts = [m[1] for m in mem]

    def voff(o):
        if o >= len(d):
            return len(raw) << 16
        k = bisect.bisect_right(starts, o) - 1           # the last member that begins at or before o: the one with bytes
        return (mem[k][0] << 16) | (o - starts[k])
    if d[:4] != b"BAM\x01":
        raise Refused("GD_E_INVALID", "not a BAM file")
    l_text, = struct.unpack_from("<i", d, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, p)
    p += 4
    lens = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", d, p)
        lens.append(struct.unpack_from("<i", d, p + 4 + l_name)[0])
        p += 8 + l_name
    recs = []
    while p < len(d):
        if p + 4 > len(d):
            raise Refused("GD_E_INVALID", "a record cut by the end of the file")
        bs, = struct.unpack_from("<I", d, p)
        if bs < 32 or p + 4 + bs > len(d):
            raise Refused("GD_E_INVALID", "a damaged record at inflated offset %d" % p)
        ref, pos, l_rn, _mq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", d, p + 4)
        if 32 + l_rn + 4 * n_cig > bs or ref < -1 or ref >= n_ref:
            raise Refused("GD_E_INVALID", "a damaged record at inflated offset %d" % p)
        rlen = sum(c >> 4 for c in struct.unpack_from("<%dI" % n_cig, d, p + 36 + l_rn) if (c & 15) in (0, 2, 3, 7, 8))
        recs.append((ref, pos, flag, rlen, p, p + 4 + bs))
        p += 4 + bs
    return lens, [(r[0], r[1], r[2], r[3], voff(r[4]), voff(r[5])) for r in recs], len(raw)


def interval(pos, flag, rlen):
    return pos, pos + (1 if (flag & 4) or rlen == 0 else rlen)


def scan(n_ref, recs):
    """Rules 1, 3, 5 (before the fill), 6 and 8 -> (runs, linear, meta, n_no_coor): what the device hands the host.
    runs: [(ref, bin, begin, end)] in file order; linear: per reference {window: begin}; meta: per reference
    [first begin, last end, n_mapped, n_unmapped] or None."""
    runs, lin, meta, n_no_coor = [], [dict() for _ in range(n_ref)], [None] * n_ref, 0
    last_ref, last_pos, key = None, 0, None
    for i, (ref, pos, flag, rlen, vb, ve) in enumerate(recs):
        if ref < 0:
            n_no_coor += 1
            last_ref, key = -1, None
            continue
        if last_ref == -1:
            raise Refused("GD_E_UNSORTED", "record %d: a placed record after an unplaced one" % i)
        if last_ref is not None and ref < last_ref:
            raise Refused("GD_E_UNSORTED", "record %d: reference %d resumes after reference %d began" % (i, ref, last_ref))
        if ref == last_ref and pos < last_pos:
            raise Refused("GD_E_UNSORTED", "record %d: positions go backwards on reference %d" % (i, ref))
        beg, end = interval(pos, flag, rlen)
        if beg < 0 or end > MAX_END:
            raise Refused("GD_E_INVALID", "record %d (reference %d, position %d): outside what a .bai can hold" % (i, ref, pos))
        last_ref, last_pos = ref, pos
        b = reg2bin(beg, end)
        if key == (ref, b):
            runs[-1] = (ref, b, runs[-1][2], ve)
        else:
            runs.append((ref, b, vb, ve))
            key = (ref, b)
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            lin[ref].setdefault(w, vb)
        m = meta[ref]
        if m is None:
            m = meta[ref] = [vb, ve, 0, 0]
        m[1] = ve
        m[3 if flag & 4 else 2] += 1
    return runs, lin, meta, n_no_coor


def assemble(n_ref, runs, lin, meta, n_no_coor):
    """Rules 4-7: the file's bytes."""
    out = [b"BAI\x01", struct.pack("<i", n_ref)]
    for t in range(n_ref):
        bins = {}
        for ref, b, vb, ve in runs:
            if ref == t:
                bins.setdefault(b, []).append([vb, ve])
        for level in (5, 4, 3, 2, 1):
            for b in sorted(x for x in bins if bin_level(x) == level):
                ch = bins[b]
                parent = (b - 1) >> 3
                if (ch[-1][1] >> 16) - (ch[0][0] >> 16) < 65536 and parent in bins:
                    bins[parent].extend(ch)
                    del bins[b]
        for b, ch in bins.items():
            ch.sort(key=lambda c: c[0])
            merged = [ch[0]]
            for c in ch[1:]:
                if merged[-1][1] >> 16 >= c[0] >> 16:
                    merged[-1][1] = max(merged[-1][1], c[1])
                else:
                    merged.append(c)
            bins[b] = merged
        has = meta[t] is not None
        out.append(struct.pack("<i", len(bins) + (1 if has else 0)))
        for b in sorted(bins):
            out.append(struct.pack("<Ii", b, len(bins[b])) + b"".join(struct.pack("<QQ", *c) for c in bins[b]))
        if has:
            out.append(struct.pack("<Ii", PSEUDO_BIN, 2) + struct.pack("<QQQQ", *meta[t]))
        n_intv = max(lin[t]) + 1 if lin[t] else 0
        io = [lin[t].get(w, UNSET) for w in range(n_intv)]
        for w in range(n_intv - 2, -1, -1):
            if io[w] == UNSET:
                io[w] = io[w + 1]
        out.append(struct.pack("<i", n_intv) + struct.pack("<%dQ" % n_intv, *io))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def build(path):
    """The .bai of the BAM at `path`."""
    lens, recs, _ = read(path)
    return assemble(len(lens), *scan(len(lens), recs))
