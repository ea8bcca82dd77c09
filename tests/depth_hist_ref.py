"""The numpy restatement of gd_depth_hist, gd_region_bins and of the files `goleft-depth dist` writes
(include/goleft_depth.h, include/goleft_depth_host.h): the yardstick of the dist tests.  It is
applied to the CPU oracle's per-base vectors, never to the engine's own."""
import numpy as np

from tests import perbase_runs_ref as R


def hist(depth, regions, n_bins):
    """(bins uint64 [n_bins], sum, min, max) over the multiset of the positions of `regions`, a list of (tid, start, end),
    `depth` being the list of the contigs' vectors: bins[k] counts the positions with min(d, n_bins - 1) == k; sum, min
    and max are unclamped, and 0 without a position."""
    assert 1 <= n_bins <= 65536
    for tid, s, e in regions:
        assert 0 <= s <= e <= len(depth[tid])
    d = np.concatenate([np.zeros(0, np.int64)] + [np.asarray(depth[tid][s:e], np.int64) for tid, s, e in regions])
    if d.size == 0:
        return np.zeros(n_bins, np.uint64), 0, 0, 0
    return np.bincount(np.minimum(d, n_bins - 1), minlength=n_bins).astype(np.uint64), int(d.sum()), int(d.min()), int(d.max())


def bins(depth, s, e, cuts=None):
    """The row of gd_region_bins for [s, e) of the contig whose vector is `depth`: the positions in each depth bin (the
    number of cuts <= the depth), uint64 [len(cuts) + 1]."""
    assert 0 <= s <= e <= len(depth)
    n = 1 + (len(cuts) if cuts is not None else 0)
    if n == 1:
        return np.array([e - s], np.uint64)
    return np.bincount(R.values(np.asarray(depth)[s:e], cuts), minlength=n).astype(np.uint64)


class Scope:
    """What the command knows of a scope: name, length, and the histogram with its scalars."""

    def __init__(self, name, length, h):
        self.name, self.length = name, length
        self.bins, self.bases, self.min, self.max = h


def dist_text(scopes):
    """PREFIX.dist.txt / PREFIX.region.dist.txt: per scope `name depth fraction` from min(N, its highest depth) down to 0;
    nothing for a scope without positions."""
    out = []
    for s in scopes:
        n = int(s.bins.sum())
        if n == 0:
            continue
        top = min(len(s.bins) - 1, s.max)
        above = np.cumsum(s.bins[::-1].astype(np.int64))[::-1]
        out += ["%s\t%d\t%.6f\n" % (s.name, d, float(above[d]) / float(n)) for d in range(top, -1, -1)]
    return "".join(out)


def summary_row(s):
    return "%s\t%d\t%d\t%.2f\t%d\t%d\n" % (s.name, s.length, s.bases, s.bases / s.length if s.length else 0.0, s.min, s.max)


def files(contigs, depth, max_depth=65535, only=None, bed=None, thresholds=None):
    """{suffix: text} of `goleft-depth dist`: contigs is [(name, length)], depth the list of their vectors, bed a list of
    (tid, start, end, name) already clipped, in file order."""
    n_bins = max_depth + 1
    wanted = [t for t, (c, _) in enumerate(contigs) if only in (None, c)]
    if bed is not None and only is not None:
        bed = [b for b in bed if contigs[b[0]][0] == only]
    scopes, rscopes = [], []
    summary = ["chrom\tlength\tbases\tmean\tmin\tmax\n"]
    for t in wanted:
        name, L = contigs[t]
        s = Scope(name, L, hist(depth, [(t, 0, L)], n_bins))
        scopes.append(s)
        summary.append(summary_row(s))
        mine = [(b[0], b[1], b[2]) for b in (bed or []) if b[0] == t]
        if mine:
            r = Scope(name, sum(e - a for _, a, e in mine), hist(depth, mine, n_bins))
            rscopes.append(r)
            r2 = Scope(name + "_region", r.length, (r.bins, r.bases, r.min, r.max))
            summary.append(summary_row(r2))
    scopes.append(Scope("total", sum(contigs[t][1] for t in wanted), hist(depth, [(t, 0, contigs[t][1]) for t in wanted], n_bins)))
    summary.append(summary_row(scopes[-1]))
    out = {".dist.txt": dist_text(scopes)}
    if bed is not None:
        allr = [(b[0], b[1], b[2]) for b in bed]
        tot = Scope("total", sum(e - a for _, a, e in allr), hist(depth, allr, n_bins))
        out[".region.dist.txt"] = dist_text(rscopes + [tot])
        summary.append(summary_row(Scope("total_region", tot.length, (tot.bins, tot.bases, tot.min, tot.max))))
    out[".summary.txt"] = "".join(summary)
    if thresholds is not None:
        rows = ["#chrom\tstart\tend\tregion" + "".join("\t%dX" % t for t in thresholds) + "\n"]
        for tid, s, e, name in bed:
            row = bins(depth[tid], s, e, thresholds)
            ge = [int(row[k + 1:].sum()) for k in range(len(thresholds))]
            rows.append("%s\t%d\t%d\t%s" % (contigs[tid][0], s, e, name) + "".join("\t%d" % g for g in ge) + "\n")
        out[".thresholds.bed"] = "".join(rows)
    return out
