"""The numpy restatement of gd_perbase_runs (include/goleft_depth.h): the yardstick of the perbase
tests.  It is applied to the CPU oracle's per-base vector, never to the engine's own."""
import numpy as np


def values(depth, cuts=None):
    """v(p): the depth, or with cuts the number of cuts <= the depth (its bin, 0 .. len(cuts))."""
    d = np.asarray(depth, np.int64)
    if cuts is None or len(cuts) == 0:
        return d
    c = np.asarray(cuts, np.int64)
    assert c.ndim == 1 and (c >= 1).all() and (np.diff(c) > 0).all()
    return np.searchsorted(c, d, side="right").astype(np.int64)


def runs(depth, start, end, cuts=None):
    """(starts uint32, values int32) of region [start, end) of the contig whose per-base vector is `depth`: position p
    starts a run iff p == start or v(p) != v(p - 1)."""
    assert 0 <= start <= end <= len(depth)
    v = values(np.asarray(depth)[start:end], cuts)
    if v.size == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.int32)
    at = np.concatenate([[0], np.flatnonzero(np.diff(v)) + 1])
    return (at + start).astype(np.uint32), v[at].astype(np.int32)


def labels(cuts):
    """--quantize's labels: bin b is lo:hi, lo = 0 or a cut, hi = the next cut or inf."""
    c = [int(x) for x in cuts]
    return ["%s:%s" % (c[b - 1] if b else 0, c[b] if b < len(c) else "inf") for b in range(len(c) + 1)]


def lines(chrom, depth, start, end, cuts=None):
    """What `goleft-depth perbase` prints for the region."""
    s, v = runs(depth, start, end, cuts)
    e = np.append(s[1:], end)
    lab = labels(cuts) if cuts is not None and len(cuts) else None
    return "".join("%s\t%d\t%d\t%s\n" % (chrom, a, b, lab[x] if lab else x) for a, b, x in zip(s.tolist(), e.tolist(), v.tolist()))
