"""A restatement of goleft's covstats/covstats.go in Python -- the yardstick of the covstats tests -- and the helpers
that craft BAM files for them (records in any order, the .bai pseudo-bins that oracle/bamio.write_bai and synth-bam do
not write).

Restated, quirks included: the 100 000 skipped records; unmapped records not counted in k; duplicates and QC failures
"bad" before anything else; nProper counted on the record that breaks the loop; the single-end break; the stored CIGAR
(no CG:B,I resolution); madFilter dropping the largest element when nothing exceeds the bound; the raw counts printed
when no size was sampled; the last -r line without a newline not counted."""
from __future__ import annotations

import bisect
import gzip
import math
import struct
import zlib

import numpy as np

from oracle import bamio

SKIP = 100000
HEADER = ("coverage\tinsert_mean\tinsert_sd\tinsert_5th\tinsert_95th\ttemplate_mean\ttemplate_sd\tpct_unmapped\t"
          "pct_bad_reads\tpct_duplicate\tpct_proper_pair\tread_length\tbam\tsample\n")
PSEUDO_BIN = 37450


class MadFilterPanic(Exception):
    """madFilter on 1 or 2 elements: the reference indexes past an empty slice."""


# ---- the record stream --------------------------------------------------------------------------------------------
class Rec:
    __slots__ = ("ref", "pos", "flag", "next_ref", "next_pos", "tlen", "cigar", "name", "tags", "mapq", "l_seq", "raw")

    def __init__(self, ref=0, pos=0, flag=0, next_pos=-1, tlen=0, cigar=((0, 100),), name="r", tags=b"", mapq=60,
                 next_ref=None, l_seq=0, raw=None):
        self.ref, self.pos, self.flag, self.next_pos, self.tlen = ref, pos, flag, next_pos, tlen
        self.cigar = list(cigar)
        self.name, self.tags, self.mapq, self.l_seq = name, tags, mapq, l_seq
        self.next_ref = ref if next_ref is None else next_ref
        self.raw = raw                                      # the record's bytes as write_bam stores them (raw_rec)


def qlen(cigar):
    """rec.Cigar.Lengths()'s read length: M, I, S, =, X."""
    return sum(n for op, n in cigar if op in (0, 1, 4, 7, 8))


def read_records(path):
    """(header text, [(name, length)], [Rec]) of a BAM, every record in file order with its STORED CIGAR."""
    d = bamio.bgzf_decompress(open(path, "rb").read())
    assert d[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<i", d, 4)
    text = d[8:8 + l_text].split(b"\0")[0].decode("latin-1")
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, p)
    p += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", d, p)
        name = d[p + 4:p + 4 + l_name].split(b"\0")[0].decode()
        l_ref, = struct.unpack_from("<i", d, p + 4 + l_name)
        refs.append((name, l_ref))
        p += 8 + l_name
    recs = []
    while p < len(d):
        bs, = struct.unpack_from("<i", d, p)
        ref, pos, l_rn, _mq, _bin, n_cig, flag, _l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", d, p + 4)
        q = p + 36 + l_rn
        cig = [(int(c) & 0xF, int(c) >> 4) for c in struct.unpack_from("<%dI" % n_cig, d, q)]
        recs.append(Rec(ref, pos, flag, npos, tlen, cig, next_ref=nref))
        p += 4 + bs
    return text, refs, recs


# ---- covstats.go ----------------------------------------------------------------------------------------------------
def mad_filter(arr, nmads=10):
    arr = sorted(arr)
    med = arr[len(arr) // 2]
    upper_mads = sorted(a - med for a in arr[len(arr) // 2 + 1:])
    if not upper_mads:
        raise MadFilterPanic(len(arr))
    umad = upper_mads[len(upper_mads) // 2]
    upper = med + nmads * umad
    i = 0
    for i, a in enumerate(arr):
        if a > upper:
            break
    return arr[:i]


def mean_std(arr):
    l = float(len(arr))
    mean = 0.0
    for a in arr:
        mean += float(a) / l
    std = 0.0
    for a in arr:
        d = float(a) - mean
        std += d * d / l
    return mean, math.sqrt(std)


def bam_stats(recs, n, skip=SKIP):
    """BamStats (:122-220) over the records in file order.  A dict of the Stats fields, the counts and the arrays."""
    it = iter(recs)
    skipped = 0
    for _ in range(skip):
        if next(it, None) is None:
            break
        skipped += 1
    sizes, ins, tl = [], [], []
    n_bad = n_unmapped = k = 0
    dup = proper = 0.0
    stopped = skipped == skip                               # false: the stream ran out (in the skip or in the loop)
    while len(ins) < n:
        rec = next(it, None)
        if rec is None:
            stopped = False
            break
        if rec.flag & 0x4:
            n_unmapped += 1
            continue
        k += 1
        if rec.flag & (0x400 | 0x200):
            if rec.flag & 0x400:
                dup += 1
            n_bad += 1
            continue
        if rec.flag & 0x2:
            proper += 1
        if len(sizes) < 2 * n:
            sizes.append(qlen(rec.cigar))
        elif len(ins) == 0:
            break
        if (rec.pos < rec.next_pos and rec.flag & 0x2 and len(rec.cigar) == 1 and rec.cigar[0][0] == 0):
            ins.append(rec.next_pos - (rec.pos + rec.cigar[0][1]))
            tl.append(rec.tlen)
    s = dict(insert_mean=0.0, insert_sd=0.0, pct5=0, pct95=0, template_mean=0.0, template_sd=0.0, rl_mean=0.0,
             bad=0.0, unmapped=0.0, proper=proper, dup=dup, max_rl=0, counts=(n_unmapped, k, n_bad, int(dup), int(proper)),
             sizes=list(sizes), ins=list(ins), tl=list(tl), skip_short=skipped < skip, stopped=stopped)
    sizes.sort()
    if sizes:
        tot = float(k + n_unmapped)
        s["bad"] = float(n_bad) / tot
        s["dup"] = dup / tot
        s["proper"] = proper / tot
        s["unmapped"] = float(n_unmapped) / tot
        s["rl_mean"] = mean_std(sizes)[0]
        s["max_rl"] = sizes[-1]
    if ins:
        ins = sorted(ins)
        l = float(len(ins) - 1)
        s["pct5"] = ins[int(0.05 * l + 0.5)]
        s["pct95"] = ins[int(0.95 * l + 0.5)]
        try:
            s["insert_mean"], s["insert_sd"] = mean_std(mad_filter(ins))
            s["template_mean"], s["template_sd"] = mean_std(mad_filter(tl))
        except MadFilterPanic:
            s["panic"] = True
    return s


def gof(fmt, v):
    """fmt.Sprintf's %.Nf, NaN and the infinities included."""
    if math.isnan(v):
        return "NaN"
    if math.isinf(v):
        return "+Inf" if v > 0 else "-Inf"
    return fmt % v


def format_row(s, mapped, genome_bases, bam, names):
    gb = float(genome_bases)
    num = (1 - s["bad"]) * float(mapped) * s["rl_mean"]
    if gb == 0.0:
        coverage = math.nan if num == 0 or math.isnan(num) else math.copysign(math.inf, num)
    else:
        coverage = num / gb
    return "\t".join([gof("%.2f", coverage), gof("%.2f", s["insert_mean"]), gof("%.2f", s["insert_sd"]),
                      "%d" % s["pct5"], "%d" % s["pct95"], gof("%.2f", s["template_mean"]), gof("%.2f", s["template_sd"]),
                      gof("%.2f", 100 * s["unmapped"]), gof("%.1f", 100 * s["bad"]), gof("%.1f", 100 * s["dup"]),
                      gof("%.1f", 100 * s["proper"]), "%d" % s["max_rl"], bam, names]) + "\n"


def sample_names(text):
    """samplename.Names, as a list in order of first appearance (the reference's order is Go's map order)."""
    rgs = [ln for ln in text.split("\n") if ln.startswith("@RG\t")]
    sms = []
    for ln in rgs:
        sm = ""
        for f in ln.split("\t")[1:]:
            if f.startswith("SM:"):
                sm = f[3:]
                break
        sms.append(sm)
    if len(rgs) == 1:
        return [sms[0]] if sms[0] else []
    out = []
    for sm in sms:
        if sm and sm not in out:
            out.append(sm)
    return out


def read_coverage(path):
    """readCoverage (:36-55)."""
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    cov = 0
    lines = raw.decode().split("\n")
    for line in lines[:-1]:                                 # the piece after the last newline is not counted
        toks = line.split("\t", 4)
        cov += int(toks[2]) - int(toks[1])                  # (a ValueError / IndexError: the reference panics)
    return cov


def bai_mapped(path):
    """n_mapped of every reference's pseudo-bin, None for a reference without one."""
    d = open(path, "rb").read()
    assert d[:4] == b"BAI\x01"
    n_ref, = struct.unpack_from("<i", d, 4)
    p = 8
    out = []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", d, p)
        p += 4
        m = None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", d, p)
            if b == PSEUDO_BIN and n_chunk == 2:
                m, = struct.unpack_from("<Q", d, p + 8 + 16)
            p += 8 + 16 * n_chunk
        n_intv, = struct.unpack_from("<i", d, p)
        p += 4 + 8 * n_intv
        out.append(m)
    return out


def index_path(bam):
    import os
    if os.path.exists(bam + ".bai"):
        return bam + ".bai"
    return bam[:-4] + ".bai"


def covstats_rows(bams, n=1000000, skip=SKIP, regions=None):
    """Main (:222-284): the header and one row per BAM; the names of a row as printed in first-appearance order."""
    out = [HEADER]
    for bam in bams:
        text, refs, recs = read_records(bam)
        names = ",".join(sample_names(text)) or "<no-read-groups>"
        mapped = 0
        stats = bam_stats(recs, n, skip)
        if stats.get("panic"):
            raise MadFilterPanic(bam)
        genome = sum(l for _, l in refs)
        if bam.endswith(".bam"):
            for m in bai_mapped(index_path(bam))[:len(refs)]:
                if m is not None:
                    mapped += m
        if regions:
            genome = read_coverage(regions)
        out.append(format_row(stats, mapped, genome, bam, names))
    return "".join(out)


# ---- crafting BAM files ------------------------------------------------------------------------------------------------
def raw_rec(ref=0, pos=0, flag=0, next_pos=-1, tlen=0, cigar=(), name=b"", tags=b"", l_seq=0, next_ref=None, mapq=60,
            block_size=None, l_read_name=None, n_cigar=None):
    """A Rec whose bytes are fixed here: `name` is stored as given (no index appended, no NUL added; empty: a 36-byte
    record), and block_size / l_read_name / n_cigar may lie about what follows (a damaged record)."""
    cig = np.asarray([(ln << 4) | op for op, ln in cigar], "<u4").tobytes()
    seq = b"\0" * ((l_seq + 1) // 2) + b"\xff" * l_seq
    nref = ref if next_ref is None else next_ref
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name) if l_read_name is None else l_read_name, mapq, 4680,
                       len(cigar) if n_cigar is None else n_cigar, flag, l_seq, nref, next_pos, tlen) + name + cig + seq + tags
    raw = struct.pack("<i", len(body) if block_size is None else block_size) + body
    return Rec(ref, pos, flag, next_pos, tlen, cigar, name="", tags=tags, mapq=mapq, next_ref=nref, l_seq=l_seq, raw=raw)


def bgzf_cut(data, cuts, level=1, sizes=None):
    """BGZF of `data` with a member boundary at every offset of `cuts` (ascending; an offset given twice: an empty
    member there) and the EOF marker; sizes: the compressed size of every data member."""
    def member(chunk):
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        c = co.compress(chunk) + co.flush()
        return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(c) + 25) + c
                + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
    edges = [0] + [int(c) for c in cuts] + [len(data)]
    assert all(a <= b and b - a < 0x10000 for a, b in zip(edges, edges[1:])), "cuts: ascending, members below 64 KB"
    out = [member(data[a:b]) for a, b in zip(edges, edges[1:])]
    if sizes is not None:
        sizes.extend(len(m) for m in out)
    out.append(member(b""))
    return b"".join(out), edges[:-1]


def write_bam(path, refs, recs, header_text=None, block=0xff00, level=1, index=True, pseudo=True, cuts=None):
    """A BAM of `recs` in the order given (Rec: ref -1 for unplaced), BGZF members of `block` uncompressed bytes, and
    (index) a .bai whose linear index holds the first record of every 16 kb window of every reference and (pseudo) a
    pseudo-bin per reference with records: n_mapped = its records without flag 0x4.  cuts: a callable that is given
    (the header's length, the start of every record, the stream's length) and returns the offsets of the inflated
    stream at which members begin (bgzf_cut), instead of `block`."""
    if header_text is None:
        header_text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    ht = header_text.encode()
    out = [b"BAM\x01", struct.pack("<i", len(ht)), ht, struct.pack("<i", len(refs))]
    for name, length in refs:
        nb = name.encode() + b"\0"
        out.append(struct.pack("<i", len(nb)) + nb + struct.pack("<i", length))
    cur = sum(len(x) for x in out)
    offs = []
    for i, r in enumerate(recs):
        if r.raw is not None:
            ref_len = min(sum(ln for op, ln in r.cigar if op in (0, 2, 3, 7, 8)), 1 << 24)   # (the index's windows)
            out.append(r.raw)
            offs.append((cur, cur + len(r.raw), max(ref_len, 1)))
            cur += len(r.raw)
            continue
        name = (r.name + str(i)).encode() + b"\0"
        cig = np.asarray([(ln << 4) | op for op, ln in r.cigar], "<u4").tobytes()
        ref_len = sum(ln for op, ln in r.cigar if op in (0, 2, 3, 7, 8))
        seq = b"\0" * ((r.l_seq + 1) // 2) + b"\xff" * r.l_seq
        body = struct.pack("<iiBBHHHiiii", r.ref, r.pos, len(name), r.mapq, 4680, len(r.cigar), r.flag, r.l_seq,
                           r.next_ref, r.next_pos, r.tlen) + name + cig + seq + r.tags
        out.append(struct.pack("<i", len(body)) + body)
        offs.append((cur, cur + 4 + len(body), max(ref_len, 1)))
        cur += 4 + len(body)
    sizes = []
    if cuts is None:
        with open(path, "wb") as fh:
            fh.write(bamio.bgzf_compress(b"".join(out), block=block, level=level, sizes=sizes))
    else:
        data = b"".join(out)
        raw, starts = bgzf_cut(data, cuts(offs[0][0] if offs else len(data), [o[0] for o in offs], len(data)), level, sizes)
        with open(path, "wb") as fh:
            fh.write(raw)
    if not index:
        return
    coff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if cuts is None:
        voff = lambda o: (int(coff[o // block]) << 16) | (o % block)
    else:                                                   # the last member that begins at or before o (never an empty one)
        def voff(o):
            k = bisect.bisect_right(starts, o) - 1
            return (int(coff[k]) << 16) | (o - starts[k])
    lin = [dict() for _ in refs]
    chunks = [None] * len(refs)
    mapped = [0] * len(refs)
    unmapped = [0] * len(refs)
    for r, (o0, o1, rl) in zip(recs, offs):
        if r.ref < 0:
            continue
        v0, v1 = voff(o0), voff(o1)
        c = chunks[r.ref]
        chunks[r.ref] = (v0, v1) if c is None else (min(c[0], v0), max(c[1], v1))
        if r.flag & 0x4:
            unmapped[r.ref] += 1
        else:
            mapped[r.ref] += 1
        if r.pos >= 0:
            for w in range(r.pos >> 14, ((r.pos + rl - 1) >> 14) + 1):
                lin[r.ref].setdefault(w, v0)
    bai = [b"BAI\x01", struct.pack("<i", len(refs))]
    for t in range(len(refs)):
        bins = []
        if chunks[t] is not None:
            bins.append(struct.pack("<Ii", 0, 1) + struct.pack("<QQ", *chunks[t]))
            if pseudo:
                bins.append(struct.pack("<Ii", PSEUDO_BIN, 2) + struct.pack("<QQ", *chunks[t])
                            + struct.pack("<QQ", mapped[t], unmapped[t]))
        bai.append(struct.pack("<i", len(bins)) + b"".join(bins))
        n_intv = max(lin[t]) + 1 if lin[t] else 0
        bai.append(struct.pack("<i", n_intv))
        last = 0
        for w in range(n_intv):
            last = lin[t].get(w, last)
            bai.append(struct.pack("<Q", last))
    with open(path + ".bai", "wb") as fh:
        fh.write(b"".join(bai))


def add_pseudo_bins(bam):
    """Rewrites the .bai next to `bam` (one without pseudo-bins, as synth-bam writes) with a pseudo-bin per reference
    that has bins: n_mapped / n_unmapped counted from the BAM's records."""
    _, refs, recs = read_records(bam)
    mapped = [0] * len(refs)
    unmapped = [0] * len(refs)
    for r in recs:
        if r.ref >= 0:
            if r.flag & 0x4:
                unmapped[r.ref] += 1
            else:
                mapped[r.ref] += 1
    path = index_path(bam)
    d = open(path, "rb").read()
    n_ref, = struct.unpack_from("<i", d, 4)
    out = [d[:8]]
    p = 8
    for t in range(n_ref):
        n_bin, = struct.unpack_from("<i", d, p)
        q = p + 4
        bins = []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", d, q)
            if b != PSEUDO_BIN:
                bins.append(d[q:q + 8 + 16 * n_chunk])
            q += 8 + 16 * n_chunk
        if bins:
            bins.append(struct.pack("<Ii", PSEUDO_BIN, 2) + struct.pack("<QQ", 0, 0)
                        + struct.pack("<QQ", mapped[t], unmapped[t]))
        out.append(struct.pack("<i", len(bins)) + b"".join(bins))
        n_intv, = struct.unpack_from("<i", d, q)
        out.append(d[q:q + 4 + 8 * n_intv])
        p = q + 4 + 8 * n_intv
    with open(path, "wb") as fh:
        fh.write(b"".join(out))
