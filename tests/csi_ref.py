"""A .csi (CSI version 1) from a BAM's records -- the model `goleft-depth index -c` is held to.

Rules 1-3, 6 and 8 of tests/bai_ref.py hold, with the binning scheme a parameter (min_shift, depth; a .bai is 14 and 5):
  C1 depth: the smallest d >= 0 with L + 256 <= 2^(min_shift + 3 d), L the header's largest reference length; min_shift is
     14 unless given, 8 to 24
  C2 interval and bin as rule 1 with the general reg2bin; a placed record is refused when pos < 0 or its end exceeds
     min(2^(min_shift + 3 depth), 2^31 - 1)
  C3 chunks are runs (rule 3)
  C4 compression as rule 4 from level `depth` down to 1
  C5 loffset: from the linear array at min_shift granularity (first touch, filled backwards below the last touched window):
     a real bin takes the entry of its first window, 0 when that window is at or beyond the last touched window + 1; the
     pseudo-bin's is 0
  C6 the pseudo-bin is (8^(depth+1) - 1) / 7 + 1; n_no_coor at the end
  C7 bins ascending, the pseudo-bin last
  C8 the file is BGZF: members of at most 65280 payload bytes, then the EOF member
  C9 refusals as rule 8, and min_shift outside 8 .. 24

At (14, 5) the bins, chunks and pseudo-bins are those of the .bai of the same file, and the loffsets a function of its linear
index: tests/golden/ref/{t,hla,t-empty}.bam.bai, which htslib wrote, pin C2-C6 there.  Beyond that geometry this
restatement is the only authority."""
from __future__ import annotations

import random
import struct
import zlib

from tests import bai_ref
from tests.bai_ref import Refused, UNSET, interval, read

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_POS = (1 << 31) - 1


def level_first(level):
    return ((1 << (3 * level)) - 1) // 7


def pseudo_bin(depth):
    return level_first(depth + 1) + 1


def max_end(min_shift, depth):
    return 1 << (min_shift + 3 * depth)


def choose_depth(lens, min_shift=14):
    longest = max(lens, default=0)
    d = 0
    while longest + 256 > max_end(min_shift, d):
        d += 1
    return d


def reg2bin(beg, end, min_shift, depth):
    end -= 1
    s = min_shift
    for level in range(depth, 0, -1):
        if beg >> s == end >> s:
            return level_first(level) + (beg >> s)
        s += 3
    return 0


def bin_level(b, depth):
    return max(l for l in range(depth + 1) if level_first(l) <= b)


def bin_span(b, min_shift, depth):
    """[beg, end) of the positions bin b covers."""
    l = bin_level(b, depth)
    s = min_shift + 3 * (depth - l)
    return (b - level_first(l)) << s, (b - level_first(l) + 1) << s


def first_window(b, depth):
    l = bin_level(b, depth)
    return (b - level_first(l)) << (3 * (depth - l))


def scan(n_ref, recs, min_shift, depth):
    """bai_ref.scan with the scheme a parameter: (runs, linear, meta, n_no_coor)."""
    if not 8 <= min_shift <= 24:
        raise Refused("GD_E_INVALID", "min_shift %d is outside 8 .. 24" % min_shift)
    limit = min(max_end(min_shift, depth), MAX_POS)
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
        if beg < 0 or end > limit:
            raise Refused("GD_E_INVALID", "record %d (reference %d, position %d): outside what min_shift %d and depth %d hold"
                          % (i, ref, pos, min_shift, depth))
        last_ref, last_pos = ref, pos
        b = reg2bin(beg, end, min_shift, depth)
        if key == (ref, b):
            runs[-1] = (ref, b, runs[-1][2], ve)
        else:
            runs.append((ref, b, vb, ve))
            key = (ref, b)
        for w in range(beg >> min_shift, ((end - 1) >> min_shift) + 1):
            lin[ref].setdefault(w, vb)
        m = meta[ref]
        if m is None:
            m = meta[ref] = [vb, ve, 0, 0]
        m[1] = ve
        m[3 if flag & 4 else 2] += 1
    return runs, lin, meta, n_no_coor


def filled(lin_t):
    n_intv = max(lin_t) + 1 if lin_t else 0
    io = [lin_t.get(w, UNSET) for w in range(n_intv)]
    for w in range(n_intv - 2, -1, -1):
        if io[w] == UNSET:
            io[w] = io[w + 1]
    return io


def reference_bins(runs, t, lin_t, depth):
    """{bin: (loffset, [[beg, end]])} of reference t after C4 and the merge."""
    bins = {}
    for ref, b, vb, ve in runs:
        if ref == t:
            bins.setdefault(b, []).append([vb, ve])
    io = filled(lin_t)
    loff = {b: (io[first_window(b, depth)] if first_window(b, depth) < len(io) else 0) for b in bins}     # before compression
    for level in range(depth, 0, -1):
        for b in sorted(x for x in bins if bin_level(x, depth) == level):
            ch = bins[b]
            parent = (b - 1) >> 3
            if (ch[-1][1] >> 16) - (ch[0][0] >> 16) < 65536 and parent in bins:
                bins[parent].extend(ch)
                del bins[b]
    out = {}
    for b, ch in bins.items():
        ch.sort(key=lambda c: c[0])
        merged = [ch[0]]
        for c in ch[1:]:
            if merged[-1][1] >> 16 >= c[0] >> 16:
                merged[-1][1] = max(merged[-1][1], c[1])
            else:
                merged.append(c)
        out[b] = (loff[b], merged)
    return out


def pack(min_shift, depth, refs, n_no_coor, aux=b"", order=None):
    """The payload from per-reference ({bin: (loffset, chunks)}, meta).  order: a function that reorders the list of bin
    records of a reference (the model writes them ascending, the pseudo-bin last); n_no_coor None: left out."""
    out = [b"CSI\x01", struct.pack("<iii", min_shift, depth, len(aux)), aux, struct.pack("<i", len(refs))]
    for bins, meta in refs:
        rows = [(b, bins[b][0], bins[b][1]) for b in sorted(bins)]
        if meta is not None:
            rows.append((pseudo_bin(depth), 0, [meta[:2], meta[2:]]))
        if order:
            rows = order(rows)
        out.append(struct.pack("<i", len(rows)))
        for b, lo, ch in rows:
            out.append(struct.pack("<IQi", b, lo, len(ch)) + b"".join(struct.pack("<QQ", *c) for c in ch))
    if n_no_coor is not None:
        out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def assemble(n_ref, runs, lin, meta, n_no_coor, min_shift, depth, **kw):
    """Rules C4-C7: the uncompressed payload."""
    return pack(min_shift, depth, [(reference_bins(runs, t, lin[t], depth), meta[t]) for t in range(n_ref)], n_no_coor, **kw)


def payload(path, min_shift=14, depth=None, **kw):
    """The payload of the .csi of the BAM at `path`; depth: C1's unless given (the fixtures' references are short: their own
    depth is below 5, and the comparison with htslib's .bai is made at 5)."""
    lens, recs, _ = read(path)
    if depth is None:
        depth = choose_depth(lens, min_shift)
    return assemble(len(lens), *scan(len(lens), recs, min_shift, depth), min_shift, depth, **kw)


def bgzf(data, block=65280):
    """C8: `data` as BGZF members and the EOF member."""
    out = []
    for at in range(0, len(data), block):
        piece = data[at:at + block]
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        c = z.compress(piece) + z.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(c) + 25) + c +
                   struct.pack("<II", zlib.crc32(piece), len(piece)))
    return b"".join(out) + EOF_MEMBER


def build(path, min_shift=14):
    """The .csi of the BAM at `path`, as a file."""
    return bgzf(payload(path, min_shift))


def inflate(raw):
    """(payload, the file ends with the EOF member, the largest member payload) of a BGZF file."""
    out, off, largest = [], 0, 0
    while off < len(raw):
        if raw[off:off + 4] != b"\x1f\x8b\x08\x04" or raw[off + 12:off + 16] != b"BC\x02\0":
            raise ValueError("not a BGZF member at %d" % off)
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        d = zlib.decompress(raw[off + 18:off + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", raw, off + bsize - 8)
        if zlib.crc32(d) != crc or len(d) != isize:
            raise ValueError("a damaged BGZF member at %d" % off)
        out.append(d)
        largest = max(largest, len(d))
        off += bsize
    return b"".join(out), raw.endswith(EOF_MEMBER), largest


def parse(p):
    """A payload -> {"min_shift", "depth", "aux", "refs": [{bin: (loffset, [(beg, end)])}], "n_no_coor" or None, "fields":
    the offsets at which a field begins}."""
    assert p[:4] == b"CSI\x01"
    fields = [0, 4, 8, 12]
    min_shift, depth, l_aux = struct.unpack_from("<iii", p, 4)
    at = 16 + l_aux
    fields.append(at)
    n_ref, = struct.unpack_from("<i", p, at)
    at += 4
    refs = []
    for _ in range(n_ref):
        fields.append(at)
        n_bin, = struct.unpack_from("<i", p, at)
        at += 4
        bins = {}
        for _ in range(n_bin):
            fields += [at, at + 4, at + 12]
            b, lo, n_chunk = struct.unpack_from("<IQi", p, at)
            at += 16
            ch = []
            for _ in range(n_chunk):
                fields += [at, at + 8]
                ch.append(struct.unpack_from("<QQ", p, at))
                at += 16
            bins[b] = (lo, ch)
        refs.append(bins)
    n_no_coor = None
    if at < len(p):
        fields.append(at)
        n_no_coor, = struct.unpack_from("<Q", p, at)
        at += 8
    assert at == len(p)
    return {"min_shift": min_shift, "depth": depth, "aux": p[16:16 + l_aux], "refs": refs, "n_no_coor": n_no_coor, "fields": fields}


def reader_view(p):
    """What the host's .csi reader must deliver from a payload, per reference: (anchors, has_chunks, largest chunk end,
    n_mapped or -1, n_unmapped)."""
    x = parse(p)
    ps = pseudo_bin(x["depth"])
    out = []
    for bins in x["refs"]:
        real = {b: v for b, v in bins.items() if b != ps}
        begs = [c[0] for _, ch in real.values() for c in ch]
        ends = [c[1] for _, ch in real.values() for c in ch]
        vals = set(begs) | {lo for lo, _ in real.values()}
        anchors = sorted(v for v in vals if v != 0 and begs and v >= min(begs))
        meta = bins.get(ps)
        nm, nu = (meta[1][1][0], meta[1][1][1]) if meta and len(meta[1]) == 2 else (-1, 0)
        out.append((anchors, bool(begs), max(ends, default=0), nm, nu))
    return out


def shuffled(seed):
    def order(rows):
        rows = list(rows)
        random.Random(seed).shuffle(rows)
        return rows
    return order


def from_bai(bai):
    """A .bai's bytes -> (n_ref, [({bin: chunks}, pseudo-bin's four numbers or None, linear array)], n_no_coor)."""
    n_ref, = struct.unpack_from("<i", bai, 4)
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", bai, at)
        at += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, at)
            ch = [struct.unpack_from("<QQ", bai, at + 8 + 16 * k) for k in range(n_chunk)]
            at += 8 + 16 * n_chunk
            if b == bai_ref.PSEUDO_BIN:
                meta = [ch[0][0], ch[0][1], ch[1][0], ch[1][1]]
            else:
                bins[b] = ch
        n_intv, = struct.unpack_from("<i", bai, at)
        lin = list(struct.unpack_from("<%dQ" % n_intv, bai, at + 4))
        at += 4 + 8 * n_intv
        refs.append((bins, meta, lin))
    n_no_coor, = struct.unpack_from("<Q", bai, at)
    return n_ref, refs, n_no_coor
