"""A plain, sequential restatement of the reference's emdepth.Cache, for the tests alone (nothing under goleft_amd/
imports it).  It sits on tests/emdepth_ref.py, which restates EMDepth, Type and Log2FC.

Written from reading emdepth/emdepth.go:208-398 of goleft; the line numbers below are that file's.  Kept as written:

  * Same (:227-247) against lower = -0.80 and upper = 0.40, NaN falling through to `changed`;
  * Add (:330-346): the first Add sets last = e BEFORE Same, so row 0 is compared with itself;
  * Clear (:348-373): positions are uint32 and `p.Start - last.End` wraps; `keys := make([]int, len(c.cnvs))` holds
    len zeros in front of the appended keys, so key 0 is deleted in every Clear that finds a list; Clear(nil) tests
    against last.Start + 100000;
  * makecnvs (:376-398) with its -0.5 < fc < 0.3 filter (which a member never meets).

The reference returns the CNVs of one Clear in Go's map order; here they are sorted by sample, and every CNV carries the
row whose Add emitted it (the row count for Clear(nil)).

parallel_form() is the same result computed without the walk, the form the device kernels follow."""
import math

import numpy as np

from tests import emdepth_ref as R

LOWER = -0.80
UPPER = 0.40
GAP = 30000
FINAL = 100000
M32 = 0xFFFFFFFF
NEAR = 1e-9              # a cell whose float64 fc is this close to a threshold may fall on the other side on a device


def log2_quotient(d, lam2):
    """math.Log2(float64(d) / lambda[2]) as Go computes it (:256): Log2(0) = -Inf, Log2(+Inf) = +Inf, NaN stays"""
    try:
        q = d / lam2
    except ZeroDivisionError:
        q = math.nan if d == 0 or math.isnan(d) else math.copysign(math.inf, d)
    if math.isnan(q) or q < 0:
        return math.nan
    if q == 0:
        return -math.inf
    if math.isinf(q):
        return math.inf
    return math.log2(q)


class EMD:
    """What Cache needs of an EMD (:209-214): the depths, the position, Log2FC() and Type()."""

    def __init__(self, row, depths, start, end, fc=None, cn=None, lam2=None):
        self.row, self.depths, self.start, self.end = row, depths, start & M32, end & M32
        self._l2 = fc if fc is not None else [log2_quotient(float(d), lam2) for d in depths]
        self._cn = cn

    def log2fc(self):
        return self._l2

    def type(self, s):
        return self._cn[s]


def same(e, o):
    """e.Same(o) (:227-247): (non2, changed, pct)"""
    ofc = o.log2fc()
    n_same = 0.0
    non2, changed = [], []
    for i, ee in enumerate(e.log2fc()):
        oo = ofc[i]
        if ee > LOWER and ee < UPPER and oo > LOWER and oo < UPPER:
            n_same += 1
            continue
        if (oo >= UPPER and ee >= UPPER) or (oo <= LOWER and ee <= LOWER):
            non2.append(i)
            n_same += 1
        else:
            changed.append(i)
    return non2, changed, n_same / float(len(e.depths))


class CNV:
    def __init__(self, sample):
        self.sample, self.psize, self.emit_row = sample, 0, None
        self.rows, self.depth, self.cn, self.log2fc = [], [], [], []

    def key(self):
        return (self.sample, self.psize, self.emit_row, tuple(self.rows))


def makecnvs(es, sample):
    """:376-398"""
    cnv = None
    for e in es:
        fc = e.log2fc()[sample]
        if fc > -0.5 and fc < 0.3:
            continue
        if cnv is None:
            cnv = CNV(sample)
        cnv.cn.append(e.type(sample))
        cnv.depth.append(np.float32(e.depths[sample]))
        cnv.rows.append(e.row)
        cnv.log2fc.append(np.float32(fc))
    return cnv


class Cache:
    def __init__(self):
        self.last = None
        self.cnvs = None

    def add(self, e):
        """:330-346"""
        if self.last is None:
            if self.cnvs is None:
                self.cnvs = {}
            self.last = e
        ret = self.clear((e.start, e.end))
        noncn2, _, _ = same(self.last, e)
        for si in noncn2:
            self.cnvs.setdefault(si, []).append(e)
        self.last = e
        return ret

    def clear(self, p):
        """:348-373; p: (start, end) or None"""
        if p is None:
            if self.last is None:
                return []
            p = ((self.last.start + FINAL) & M32, (self.last.end + FINAL) & M32)
        cnvs = []
        d = self.cnvs
        keys = [0] * len(d)
        for si, emd in d.items():
            if ((p[0] - emd[-1].end) & M32) < GAP:       # not a big enough gap yet
                continue
            putative = makecnvs(emd, si)
            if putative is not None:
                cnvs.append(putative)
                cnvs[-1].psize = len(d)
                keys.append(si)
        for key in keys:
            d.pop(key, None)
        return sorted(cnvs, key=lambda c: c.sample)


def run_cache(emds):
    """Add for every EMD in order, Clear(nil) after the last: the CNVs in (emit_row, sample) order."""
    c = Cache()
    out = []
    for r, e in enumerate(emds):
        for cnv in c.add(e):
            cnv.emit_row = r
            out.append(cnv)
    for cnv in c.clear(None):
        cnv.emit_row = len(emds)
        out.append(cnv)
    return out


class Result:
    """cnvs: the CNVs; rows: the emdepth restatement's rows; near: the cells (row, sample) whose float64 fc lies
    within NEAR of a threshold; fc: float64 [rows][samples]"""


def run(depths, starts, ends, em_rows=None):
    """The whole chain on a [rows][samples] matrix (narrowed to float32 first)."""
    d32 = np.ascontiguousarray(depths, np.float32)
    res = Result()
    res.rows = em_rows if em_rows is not None else R.em_matrix(d32)
    emds, res.near, res.fc = [], [], []
    for r, (row, d) in enumerate(zip(res.rows, d32)):
        e = EMD(r, d, int(starts[r]), int(ends[r]), cn=row.cn, lam2=row.lam[2])
        emds.append(e)
        res.fc.append(e.log2fc())
        res.near += [(r, s) for s, f in enumerate(e.log2fc()) if abs(f - LOWER) <= NEAR or abs(f - UPPER) <= NEAR]
    res.cnvs = run_cache(emds)
    return res


def state_of(fc):
    if fc >= UPPER:
        return "U"
    if fc <= LOWER:
        return "D"
    if fc > LOWER and fc < UPPER:
        return "N"
    return "X"


def parallel_form(fc, starts, ends):
    """The CNVs as (sample, psize, emit_row, rows) tuples in (emit_row, sample) order, without the walk:
    members, F per row, runs per column, PSize per emit row."""
    R_, n = len(fc), (len(fc[0]) if len(fc) else 0)
    st = [[state_of(f) for f in row] for row in fc]
    member = [[st[r][s] in "UD" and st[r][s] == st[r - 1 if r else 0][s] for s in range(n)] for r in range(R_)]
    F = []
    for a in range(R_):
        f = R_ if ((starts[R_ - 1] + FINAL - ends[a]) & M32) >= GAP else R_ + 1
        for r in range(a + 1, R_):
            if ((starts[r] - ends[a]) & M32) >= GAP:
                f = r
                break
        F.append(f)
    out = []                                     # (emit_row, sample, rows)
    for s in range(1, n):
        cur = []
        for r in range(R_):
            if not member[r][s]:
                continue
            if cur and not F[cur[-1]] > r:
                if F[cur[-1]] <= R_:
                    out.append((F[cur[-1]], s, cur))
                cur = []
            cur = cur + [r]
        if cur and F[cur[-1]] <= R_:
            out.append((F[cur[-1]], s, cur))
    if n:
        for a in range(R_):
            if member[a][0] and F[a] == a + 1:
                out.append((a + 1, 0, [a]))

    def psize(e):
        k = 1 if e >= 1 and member[e - 1][0] else 0
        for s in range(1, n):
            latest = next((a for a in range(e - 1, -1, -1) if member[a][s]), None)
            if latest is not None and F[latest] >= e:
                k += 1
        return k

    return [(s, psize(e), e, tuple(rows)) for e, s, rows in sorted(out, key=lambda t: (t[0], t[1]))]
