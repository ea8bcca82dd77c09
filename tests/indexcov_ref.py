"""Restatement of `goleft indexcov` (indexcov/indexcov.go and indexcov/types.go of the reference; line numbers below are
those files') in Python + numpy: the decompressed BED matrix, the .roc table and the .ped file, plus a writer for
synthetic .bai files.  float32 steps are numpy.float32 operations, one rounding each, as Go on amd64 performs them.

Readings of the three implementation-defined spots: uint8() of a float32 above 255 truncates to
an integer and keeps the low 8 bits; the exclude pattern is matched by Python's `re` (the default pattern means the
same in RE2); a principal component whose singular value is 0 up to rounding prints 0.00."""
import glob as _glob
import gzip
import math
import os
import re
import struct

import numpy as np

PSEUDO_BIN = 37450
SLOTS = 70
F32 = np.float32
DEFAULT_EXCLUDE = r"^chrEBV$|^NC|_random$|Un_|^HLA\-|_alt$|hap\d$"


class Fatal(Exception):
    """log.Fatal / panic of the reference: the CLI exits non-zero and names str(e) on stderr."""


# ---- .bai ---------------------------------------------------------------------------------------------------------------
def write_bai(path, refs):
    """refs: per reference (intervals, stats): intervals = virtual offsets of the linear index as they are stored
    (repeats and zeros included), stats = (mapped, unmapped) of the pseudo-bin or None."""
    out = [b"BAI\x01", struct.pack("<i", len(refs))]
    for intervals, stats in refs:
        if stats is None:
            out.append(struct.pack("<i", 0))
        else:
            out.append(struct.pack("<iIi", 1, PSEUDO_BIN, 2))
            out.append(struct.pack("<QQQQ", 0, 0, stats[0], stats[1]))
        out.append(struct.pack("<i", len(intervals)))
        out.append(np.asarray(intervals, np.uint64).astype("<u8").tobytes())
    with open(path, "wb") as f:
        f.write(b"".join(out))


def read_bai(path):
    """getSizes (types.go:45-82): per reference the differences of consecutive raw intervals; mapped, unmapped."""
    d = open(path, "rb").read()
    if d[:4] != b"BAI\x01":
        raise Fatal(path)
    n_ref, = struct.unpack_from("<i", d, 4)
    p = 8
    sizes, mapped, unmapped = [], 0, 0
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", d, p)
        p += 4
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", d, p)
            if b == PSEUDO_BIN and n_chunk == 2:
                m, u = struct.unpack_from("<QQ", d, p + 8 + 16)
                mapped += m
                unmapped += u
            p += 8 + 16 * n_chunk
        n_intv, = struct.unpack_from("<i", d, p)
        p += 4
        iv = np.frombuffer(d, "<u8", n_intv, p).astype(np.int64)   # vOffset: File << 16 | Block, as int64
        p += 8 * n_intv
        if n_intv < 2:
            sizes.append(np.zeros(0, np.int64))
            continue
        s = iv[1:] - iv[:-1]
        if (s < 0).any():
            raise Fatal(path)                                # "expected positive change in vOffset"
        sizes.append(s)
    return sizes, mapped, unmapped


def bam_header(path):
    with gzip.open(path, "rb") as f:
        assert f.read(4) == b"BAM\x01"
        l_text, = struct.unpack("<i", f.read(4))
        text = f.read(l_text).split(b"\0")[0].decode()
        n_ref, = struct.unpack("<i", f.read(4))
        refs = []
        for _ in range(n_ref):
            l_name, = struct.unpack("<i", f.read(4))
            name = f.read(l_name)[:-1].decode()
            refs.append((name, struct.unpack("<i", f.read(4))[0]))
    return text, refs


def short_name(path, is_index):
    """GetShortName (:213-246)."""
    if not is_index:
        text, _ = bam_header(path)
        sms = []
        for ln in text.split("\n"):
            if ln.startswith("@RG"):
                sm = ""
                for f in ln.split("\t")[1:]:
                    if f.startswith("SM:"):
                        sm = f[3:]
                if sm not in sms:
                    sms.append(sm)
        if len(sms) > 1:
            raise Fatal(path)
        if sms:
            return sms[0]
    vs = path.split("/")[-1].split(".")
    if len(vs) <= 2:
        return vs[0]
    return "-".join(vs[:-1])


def read_fai(path):
    """ReadFai (:278-318): the records sorted by their offset."""
    recs = []
    for ln in open(path):
        t = ln.rstrip("\n").split("\t")
        if len(t) >= 3:
            recs.append((int(t[2]), t[0], int(t[1])))
    recs.sort(key=lambda r: r[0])
    return [(n, l) for _, n, l in recs]


# ---- the numbers --------------------------------------------------------------------------------------------------------
def median_size(sizes):
    """Index.init (:83-125)."""
    s = np.sort(np.concatenate(sizes) if len(sizes) else np.zeros(0, np.int64), kind="stable")
    if len(s) < 1:
        raise Fatal("no usable chromsomes")
    n98 = s[int(0.98 * float(len(s)))]
    cum = np.cumsum(np.minimum(s, n98))
    total = int(cum[-1])
    idx = int(np.searchsorted(cum, total // 2, side="right"))     # the first cumsum > total / 2
    if idx >= len(s):
        idx = len(s) - 1
    return int(s[idx])


def normalized_depth(sizes, ref_id, median):
    """NormalizedDepth (:129-151)."""
    if ref_id >= len(sizes) or median == 0:
        return np.zeros(0, F32)
    d = (sizes[ref_id].astype(np.float64) / float(median)).astype(F32)
    return np.minimum(d, F32(50000))


SLOT_C = F32(F32(70) * F32(2.0 / 3.0))


def slots_of(depths):
    """CountsAtDepth (:170-177) with tint (:159-167)."""
    f = (depths * SLOT_C).astype(F32) + F32(0.5)
    v = np.clip(f.astype(np.int64), 0, SLOTS - 1)
    return np.bincount(v, minlength=SLOTS).astype(np.int64)


def counts_roc(counts):
    """CountsROC (:181-193), float32."""
    totals = np.cumsum(counts[::-1])[::-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return totals.astype(F32) / F32(totals[0])


def pca8_bytes(dp):
    f = (F32(65535) / F32(8) * dp).astype(F32) + F32(0.5)
    return (f.astype(np.int64) & 0xff).astype(np.uint8)


def get_cn(depths):
    """GetCN (:957-991)."""
    out = []
    for d in depths:
        tmp = np.sort(d[d != 0])
        lows = int((tmp < F32(0.02)).sum())
        if len(tmp) == 0:
            out.append(-0.1)
            continue
        if float(lows) / float(len(d)) > 0.3:
            tmp = tmp[lows:]
        out.append(float(F32(2) * tmp[int(float(len(tmp)) * 0.4)]) if len(tmp) else 0.0)
    return out


def normalize_across_samples(depths):
    """normalizeAcrossSamples (:549-597), in place."""
    if len(depths) < 5:
        return
    max_len = max(len(d) for d in depths)
    for j in range(max_len):
        m = 0.0
        n = 0.0
        for d in depths:
            if len(d) > j:
                m += float(d[j]); n += 1
                if j > 0:
                    m += float(d[j - 1]); n += 1
                if j < len(d) - 1:
                    m += float(d[j + 1]); n += 1
        if int(n) < 3 * len(depths) - 4:
            continue
        m /= n
        if m < 0.1:
            continue
        fm = F32(m)
        for d in depths:
            if len(d) > j:
                d[j] = d[j] / fm
                if j > 2 and j < len(d) - 3:
                    # Go evaluates 1.0 / 7.0 as an exact constant rounded to float32, then the sum left to right
                    t = d[j - 3] + d[j - 2]
                    t = t + d[j - 1]
                    t = t + d[j]
                    t = t + d[j + 1] / fm
                    t = t + d[j + 2] / fm
                    t = t + d[j + 3] / fm
                    d[j] = F32(1.0 / 7.0) * t


def same_chrom(sex, b):
    """sameChrom (:530-547)."""
    for a in sex:
        if a == b:
            return True
        na = a
        if a.startswith("chr"):
            na = a[3:]
        elif b.startswith("chr"):
            na = "chr" + a
        if na == b:
            return True
    return False


def gof(fmt, v):
    v = float(v)
    if math.isnan(v):
        return "NaN"
    if math.isinf(v):
        return "+Inf" if v > 0 else "-Inf"
    return fmt % v


def fmt3g(x):
    return "%.3g" % float(x)


def principal_components(X):
    """pca (:773-807): gonum's stat.PC on the float64 matrix -- the columns centred, a thin SVD -- and the UNCENTRED
    rows projected onto the first k right singular vectors.  Returns (proj [N, k] or None, singular values)."""
    A = X.astype(np.float64)
    N, M = A.shape
    k = min(5, N, M)
    if k < 3:
        return None, None
    Ac = A - A.mean(axis=0, keepdims=True)
    _, sv, vt = np.linalg.svd(Ac, full_matrices=False)
    proj = A @ vt[:k].T
    for c in range(k):
        if sv[c] <= 1e-6 * sv[0]:
            proj[:, c] = 0.0
    return proj, sv


class Result:
    pass


def expand(paths):
    out = []
    for p in paths:
        out.extend(sorted(_glob.glob(p)) if _glob.has_magic(p) else ([p] if os.path.exists(p) else []))
    return out


def indexcov(paths, directory, sex="X,Y", exclude=DEFAULT_EXCLUDE, fai=None, extra_normalize=False, include_gl=False):
    """Main (:392-456) + run (:599-734) + writeIndex (:815-893).  Returns a Result with .bed, .roc, .ped (text),
    .pcs (the PC columns as floats, [N, k], or None), .sv, .names."""
    first = paths[0]
    if first.endswith(".bam"):
        refs = bam_header(first)[1]
    elif fai:
        refs = read_fai(fai)
    else:
        raise Fatal(first)
    paths = expand(paths)
    sexes_wanted = [s for s in sex.strip().split(",")] if len(sex) > 0 else []
    rx = re.compile(exclude) if exclude else None
    names, all_sizes, medians, mapped, unmapped = [], [], [], [], []
    for b in paths:
        if b.endswith(".crai") or b.endswith(".cram"):
            raise Fatal(b)
        ip = b if b.endswith(".bai") else (b + ".bai" if os.path.exists(b + ".bai") else b[:-4] + ".bai")
        if not os.path.exists(ip):
            raise Fatal(b)
        try:
            sizes, m, u = read_bai(ip)
        except Fatal:
            raise Fatal(b)
        if sum(len(s) for s in sizes) < 1:
            raise Fatal(b)                                   # "no usable chromsomes in bam"
        medians.append(median_size(sizes))
        all_sizes.append(sizes)
        names.append(short_name(b, b.endswith(".bai")))
        mapped.append(m)
        unmapped.append(u)
    N = len(paths)
    bed = ["#chrom\tstart\tend\t%s\n" % "\t".join(names)]
    roc = []
    sexes = {}
    counters = np.zeros((N, 4), np.int64)                    # out, low, hi, in
    pca8 = [[] for _ in range(N)]
    slopes = np.zeros(N, F32)
    n_slopes = 0
    for ref_id, (chrom, ref_len) in enumerate(refs):
        if rx is not None and rx.search(chrom):
            continue
        depths = [normalized_depth(all_sizes[k], ref_id, medians[k]).copy() for k in range(N)]
        longest, longesti = 0, 0
        for k in range(N):
            if len(depths[k]) > longest:
                longest, longesti = len(depths[k]), k
        is_sex = same_chrom(sexes_wanted, chrom)
        if extra_normalize and not is_sex:
            normalize_across_samples(depths)
        counts = [slots_of(d) for d in depths]
        rows = []
        for i in range(longest):
            rows.append("%s\t%d\t%d\t%s\n" % (chrom, i * 16384, (i + 1) * 16384,
                                               "\t".join("0" if i >= len(d) else fmt3g(d[i]) for d in depths)))
        bed.append("".join(rows))
        if is_sex:
            if longest > 0:
                sexes[chrom] = get_cn(depths)
        else:
            for k in range(N):
                dp = np.minimum(depths[k], F32(8))
                n_missing = longest - len(dp)
                pca8[k].append(pca8_bytes(dp))
                # the padding loop starts at the last tile's index (or -1) and runs to `longest`: longest + 1 bytes in all
                pca8[k].append(np.zeros(longest + 1 - len(dp), np.uint8))
                out = (dp < F32(0.85)) | (dp > F32(1.15))
                hi = dp > F32(1.15)
                low = out & ~hi & (dp < F32(0.15))
                counters[k] += (int(out.sum()) + n_missing, int(low.sum()) + n_missing, int(hi.sum()), int((~out).sum()))
        if longest > 0:
            rocs = [counts_roc(c) for c in counts]
            roc.append("#chrom\tcov\t%s\n" % "\t".join(names))
            for i in range(SLOTS):
                roc.append("%s\t%.2f\t%s\n" % (chrom, float(i) / (70 * (2.0 / 3.0)),
                                              "\t".join(gof("%.2f", r[i]) for r in rocs)))
            if (include_gl or not chrom.startswith("GL")) and longest > 2:
                if not is_sex and longest > 100:
                    scalar = F32(ref_len) / F32(1e6)
                    for k in range(N):
                        with np.errstate(invalid="ignore"):
                            slopes[k] = slopes[k] + F32(rocs[k][40] - rocs[k][54]) * scalar
                    n_slopes += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        slopes = slopes / F32(n_slopes)
    res = Result()
    res.names = names
    res.bed = "".join(bed)
    res.roc = "".join(roc)
    if len(sexes) != len(sexes_wanted) and len(sexes) == 0 and sexes_wanted != ["X", "Y"]:
        raise Fatal("(FATAL)")
    X = np.stack([np.concatenate(p) if p else np.zeros(0, np.uint8) for p in pca8])
    res.pca8 = X
    if X.shape[1] == 0:
        raise Fatal("(FATAL)")                               # mat.NewDense panics on a matrix without columns
    pcs, sv = principal_components(X)
    res.pcs, res.sv = pcs, sv
    keys = sorted(sexes)
    hdr = ["CN" + k for k in keys] + ["bins.out", "bins.lo", "bins.hi", "bins.in", "slope", "p.out"]
    n_pc = 0 if pcs is None else pcs.shape[1]
    hdr += ["PC%d" % (i + 1) for i in range(n_pc)]
    anygt = any(m > 0 or u > 0 for m, u in zip(mapped, unmapped))
    if anygt:
        hdr += ["mapped", "unmapped"]
    ped = ["#family_id\tsample_id\tpaternal_id\tmaternal_id\tsex\tphenotype\t%s\n" % "\t".join(hdr)]
    for i, s in enumerate(names):
        inferred = int(0.5 + sexes[keys[0]][i]) if keys else -9
        cells = ["%.2f" % sexes[k][i] for k in keys]
        o, lo, hi, inn = (int(v) for v in counters[i])
        pout = float(o) / float(inn) if inn else (math.nan if o == 0 else math.inf)
        cells += ["%d" % o, "%d" % lo, "%d" % hi, "%d" % inn, gof("%.3f", slopes[i]), gof("%.2f", pout)]
        cells += ["%.2f" % pcs[i, c] for c in range(n_pc)]
        if anygt:
            cells += ["%d" % mapped[i], "%d" % unmapped[i]]
        ped.append("unknown\t%s\t-9\t-9\t%d\t-9\t%s\n" % (s, inferred, "\t".join(cells)))
    res.ped = "".join(ped)
    res.n_pc = n_pc
    res.n_front = 6 + len(keys) + 6                          # columns in front of the PCs
    return res


def strip_pcs(ped_text, n_front, n_pc):
    """The .ped without its PC columns, and the PC columns as floats per row."""
    rows, pcs = [], []
    for i, ln in enumerate(ped_text.splitlines()):
        t = ln.split("\t")
        rows.append("\t".join(t[:n_front] + t[n_front + n_pc:]))
        if i:
            pcs.append([float(v) for v in t[n_front:n_front + n_pc]])
    return "\n".join(rows) + "\n", np.array(pcs)
