"""Restatement of `goleft indexsplit` (indexsplit/indexsplit.go of the reference; line numbers below are that file's)
in plain Python floats -- IEEE doubles, one rounding per operation, as Go on amd64 performs them -- with
depth.ReadTree / depth.Overlaps (depth/intervals.go) and the row format.  The index and reference readers are
tests/indexcov_ref.py's.

gonum's stat.MeanStdDev and floats.Sum are restated from memory: the mean is the sequential sum
over n, the variance the corrected two-pass form, the sum a sequential loop."""
import math
import os
import re

from tests import indexcov_ref as IR

TILE = 16384
SCALAR = 1000000000.0
Fatal = IR.Fatal
_REGION = re.compile(r"(.+?)[:\t](\d+)([\-\t])(\d+).*?")                   # depth/depth.go:73


def chrom_start_end(line):
    """chromStartEndFromLine (depth/depth.go:75-94)."""
    m = _REGION.search(line)
    if m is None:
        raise Fatal(line)
    start = int(m.group(2))
    if m.group(3) == "-":
        start -= 1
    return m.group(1), max(start, 0), int(m.group(4))


def read_tree(path):
    """ReadTree (intervals.go:42-79) of one path: {chrom: [(start, end)]}.  ReadBytes returns io.EOF together with a
    last line that has no newline, and the loop leaves before it looks at it."""
    tree = {}
    if not path:
        return tree
    data = open(path).read()
    for line in data.split("\n")[:-1]:
        chrom, start, end = chrom_start_end(line + "\n")
        if start >= end:
            continue
        tree.setdefault(chrom, []).append((start, end))
    return tree


def overlaps(ivs, start, end):
    """Overlaps (intervals.go:16-39): half-open; no tree, no overlap."""
    if not ivs:
        return False
    return any(e > start and s < end for s, e in ivs)


def mean_std(x):
    """stat.MeanStdDev(x, nil)."""
    n = len(x)
    if n == 0:
        return math.nan, math.nan                            # 0 / 0
    s = 0.0
    for v in x:
        s += v
    m = s / n
    if n == 1:
        return m, math.nan                                   # (0 - 0 / 1) / 0
    ss = c = 0.0
    for v in x:
        d = v - m
        ss += d * d
        c += d
    var = (ss - c * c / n) / (n - 1)
    return m, (math.sqrt(var) if var >= 0 else math.nan)


def chop(sizes):
    """chop (:38-49), in place."""
    for size in sizes:
        m, std = mean_std(size)
        mx = m + 3 * std
        for i, s in enumerate(size):
            if s > mx:
                size[i] = 8 * m


def get_percents(sizes):
    """getPercents (:52-66)."""
    chop(sizes)
    tot = 0.0
    sums = []
    for s in sizes:
        t = 0.0
        for v in s:
            t += v
        sums.append(t)
        tot += t
    if tot == 0:
        raise Fatal("no data")                               # (the reference goes on with int(NaN): DESIGN.md section 5)
    return [s / tot for s in sums], sums


def cohort_sizes(all_sizes, n_refs):
    """Split (:89-114): per reference the sum over the indexes, in their order, of float64(size) / 1e9."""
    sizes = []
    for osz in all_sizes:
        for i in range(n_refs):
            while i >= len(sizes):
                sizes.append([])
            if i >= len(osz):
                break
            s, o = sizes[i], osz[i]
            m = min(len(s), len(o))
            for j in range(m):
                s[j] += float(int(o[j])) / SCALAR
            for j in range(m, len(o)):
                s.append(float(int(o[j])) / SCALAR)
    return sizes


def row(chrom, start, end, total, splits):
    return "%s\t%d\t%d\t%.2f\t%d" % (chrom, start, end, total, splits)


def split(all_sizes, refs, N, probs=None):
    """Split (:82-194): the Chunks as (chrom, start, end, sum, splits)."""
    sizes = cohort_sizes(all_sizes, len(refs))
    percents, sums = get_percents(sizes)
    out = []
    for ri, (name, ref_len) in enumerate(refs):
        if ri >= len(sizes) or len(sizes[ri]) == 0:
            out.append((name, 0, ref_len, 0.0, 0))
            continue
        n = int(percents[ri] * float(N))
        if n == 0 and percents[ri] > 0:
            n = 1
        elif n == 0:
            out.append((name, 0, ref_len, 0.0, 0))
            continue
        chunk = sums[ri] / float(n)
        size = sizes[ri]
        total = 0.0
        lasti = 0
        tree = probs.get(name) if probs is not None else None
        for i in range(len(size)):
            ovl = overlaps(tree, i * TILE, (i + 1) * TILE)
            if size[i] > chunk or (size[i] >= 0.05 * chunk and ovl):
                if i > lasti:
                    out.append((name, lasti * TILE, i * TILE, total, 1))
                total = size[i]
                nsplits = int(0.5 + (total / (chunk / 2)))
                if nsplits > 8:
                    nsplits = 8
                elif nsplits < 1:
                    nsplits = 1
                    if ovl:
                        nsplits = 3
                start = i * TILE
                ln = int(float(TILE) / float(nsplits) + 1)
                for k in range(nsplits):
                    if i + k == len(size) + 1:
                        out.append((name, start, ref_len, total / float(nsplits), nsplits))
                    else:
                        out.append((name, start, min(start + ln, (i + 1) * TILE), total / float(nsplits), nsplits))
                    start += ln
                lasti, total = i + 1, 0.0
                continue
            total += size[i]
            if total >= chunk or i == len(size) - 1 or (total >= 0.2 * chunk and ovl):
                if i == len(size) - 1:
                    out.append((name, lasti * TILE, ref_len, total, 1))
                else:
                    out.append((name, lasti * TILE, (i + 1) * TILE, total, 1))
                lasti = i + 1
                total = 0.0
    return out


def partition_gaps(text, refs):
    """The check of the reference's functional-tests.sh: [] when the rows of every reference, in the order they were
    written, start at 0, each begin where the one before ended, and end at the reference's length -- no gap, no overlap,
    nothing outside; else the offending (chrom, start, end, expected start)."""
    bad = []
    at = {}
    order = []
    for ln in text.splitlines():
        chrom, start, end = ln.split("\t")[:3]
        start, end = int(start), int(end)
        if chrom not in at:
            at[chrom] = 0
            order.append(chrom)
        if start != at[chrom] or end <= start:
            bad.append((chrom, start, end, at[chrom]))
        at[chrom] = end
    if order != [n for n, _ in refs]:
        bad.append(("references", order))
    for name, length in refs:
        if at.get(name) != length:
            bad.append((name, "ends at", at.get(name), length))
    return bad


def index_path(b):
    if b.endswith(".bai"):
        return b
    return b + ".bai" if os.path.exists(b + ".bai") else b[:-4] + ".bai"


def indexsplit(paths, N, fai=None, problematic=None):
    """Main (:197-216): the text of stdout.  Fatal(str) names the argument at fault."""
    for b in paths:
        if b.endswith(".crai") or b.endswith(".cram"):
            raise Fatal(b)
    probs = None
    if problematic:
        try:
            probs = read_tree(problematic)
        except (OSError, Fatal):
            raise Fatal(problematic)
    first = paths[0]
    if first.endswith(".bam"):
        refs = IR.bam_header(first)[1]
    elif fai:
        refs = IR.read_fai(fai)
    else:
        raise Fatal(first)
    all_sizes = []
    for b in paths:
        ip = index_path(b)
        if not os.path.exists(ip):
            raise Fatal(b)
        try:
            sizes = IR.read_bai(ip)[0]
        except Fatal:
            raise Fatal(b)
        if sum(len(s) for s in sizes) < 1:
            raise Fatal(b)                                   # Index.init: "no usable chromsomes in bam"
        all_sizes.append(sizes)
    try:
        chunks = split(all_sizes, refs, N, probs)
    except Fatal:
        raise Fatal(first)
    return "".join(row(*c) + "\n" for c in chunks)
