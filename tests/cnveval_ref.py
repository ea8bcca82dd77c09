"""Restatement of goleft's cnveval (cnveval/cnveval.go) in plain Python: the judge of the device kernels.

Two forms.  evaluate_literal() is the reference's walk as written: the cursor `i` with its `i--`, the `used` map
of the truth copy, the `counted` flag, the fpfound / tpfound / found flags, and the samples in map order (any order:
nothing is carried from one sample to the next).  evaluate_order_free() is what goleft_amd/csrc/gd_cnveval.hpp
computes: every (sample, truth) pair on its own.  tests/test_cnveval_ref.py holds the two to each other count for count.

A CNV is (chrom, start, end, cn, sample), a truth (chrom, start, end, cn, [samples]); chromosomes and samples are
strings (bytes order is Python's str order for ASCII names).  Go's sort.Slice is unstable; here, as in the project,
CNVs of one sample with equal (chrom, start) keep their input order (a stable sort).
Counts: {(sample, class): [FP, FN, TP, TN]}, class 0 / 1 / 2 for a length below 20000 / below 100000 / the rest."""
import math

FP, FN, TP, TN = 0, 1, 2, 3
SMALL, MEDIUM = 20000, 100000
CLASS_NAMES = ("0-20000", "20000-100000", ">=100000", "all")


def size_class(start, end):
    l = end - start
    return 0 if l < SMALL else 1 if l < MEDIUM else 2


def same_cn(a, b):
    return min(a, 3) == min(b, 3)


def poverlap(c, t):
    """cnveval.go:378-389; one float64 division, NaN for a zero-length interval"""
    if c[0] != t[0]:
        return 0.0
    total = min(float(c[2] - c[1]), float(t[2] - t[1]))
    ovl = min(c[2], t[2]) - max(c[1], t[1])
    if ovl < 0:
        return 0.0
    if total == 0.0:
        return math.nan                  # Go: 0 / 0 (ovl is 0 here: it cannot exceed the shorter length)
    return float(ovl) / total


def match(c, t, po):
    return poverlap(c, t) >= po and same_cn(c[3], t[3])


def _sorted(items):
    return sorted(items, key=lambda x: (x[0], x[1]))       # stable


def _get(stat, sample, cls):
    return stat.setdefault((sample, cls), [0, 0, 0, 0])


def _update_positive(stat, truths, cnvs, counted, po):
    """cnveval.go:289-341"""
    if not cnvs:
        return
    sample = cnvs[0][4]
    i = 0
    for t in truths:
        val = _get(stat, sample, size_class(t[1], t[2]))
        found = False
        used = None                                        # the map of the loop's copy of t: fresh for every t
        while i < len(cnvs) and (cnvs[i][0] < t[0] or (cnvs[i][0] == t[0] and cnvs[i][2] < t[1])):
            i += 1
        if i > 0:
            i -= 1
        for k in range(i, len(cnvs)):
            cnv = cnvs[k]
            if cnv[0] > t[0] or (t[0] == cnv[0] and cnv[1] > t[2]):
                break
            if poverlap(cnv, t) >= po and same_cn(cnv[3], t[3]):
                if used is None or cnv[4] not in used:
                    val[TP] += 1
                    counted[k] = True
                    found = True
                    if used is None:
                        used = {}
                    used[cnv[4]] = True
        if not found:
            val[FN] += 1
    for k, cnv in enumerate(cnvs):
        if not counted[k]:
            _get(stat, cnv[4], size_class(cnv[1], cnv[2]))[FP] += 1


def _update_fp(stat, others, cnvs, truths, counted, po):
    """cnveval.go:231-285"""
    if not cnvs or not others:
        return
    i = 0
    for o in others:
        val = _get(stat, cnvs[0][4], size_class(o[1], o[2]))
        while i < len(cnvs) and (cnvs[i][0] < o[0] or (cnvs[i][0] == o[0] and cnvs[i][2] < o[1])):
            i += 1
        if i > 0:
            i -= 1
        tpfound = fpfound = found = False
        for k in range(i, len(cnvs)):
            cnv = cnvs[k]
            if cnv[0] > o[0] or (o[0] == cnv[0] and cnv[1] > o[2]):
                break
            if poverlap(cnv, o) >= po and same_cn(cnv[3], o[3]):
                fpfound = True
                for t in truths:
                    if t[0] != cnv[0]:
                        continue
                    if poverlap(cnv, t) >= po and same_cn(cnv[3], t[3]):
                        tpfound = True
                        break
            if fpfound and not tpfound:
                val[FP] += 1
                found = True
                counted[k] = True
        if not (found or tpfound):
            val[TN] += 1


def evaluate_literal(cnvs, truths, po):
    """cnveval.go:163-212 Evaluate"""
    stat = {}
    all_samples = {}
    for t in truths:
        for s in t[4]:
            all_samples[s] = True
    for c in cnvs:
        all_samples[c[4]] = True
    sample_list = list(all_samples)
    truth_by_sample, truth_without_sample = {}, {}
    for t in truths:
        for s in t[4]:
            truth_by_sample.setdefault(s, []).append(t)
        named = set(t[4])                                  # notin(), as a set
        for s in sample_list:
            if s not in named:
                truth_without_sample.setdefault(s, []).append(t)
    cnv_by_sample = {}
    for c in cnvs:
        cnv_by_sample.setdefault(c[4], []).append(c)
    for sample in sample_list:
        ts = _sorted(truth_by_sample.get(sample, []))
        cs = _sorted(cnv_by_sample.get(sample, []))
        counted = [False] * len(cs)
        _update_positive(stat, ts, cs, counted, po)
        others = _sorted(truth_without_sample.get(sample, []))
        _update_fp(stat, others, cs, ts, counted, po)
    return stat


def evaluate_order_free(cnvs, truths, po):
    """The four steps of DESIGN.md section 3.18, a pair at a time."""
    stat = {}
    cnv_by_sample = {}
    for c in cnvs:
        cnv_by_sample.setdefault(c[4], []).append(c)
    for sample, cs in cnv_by_sample.items():
        cs = _sorted(cs)
        mine = [t for t in truths for s in t[4] if s == sample]          # one entry per naming
        own = [any(match(c, t, po) for t in mine) for c in cs]
        counted = [False] * len(cs)
        for t in mine:
            first = next((k for k, c in enumerate(cs) if match(c, t, po)), None)
            if first is None:
                _get(stat, sample, size_class(t[1], t[2]))[FN] += 1
            else:
                _get(stat, sample, size_class(t[1], t[2]))[TP] += 1
                counted[first] = True
        for k, c in enumerate(cs):
            if not counted[k]:
                _get(stat, sample, size_class(c[1], c[2]))[FP] += 1
        for o in truths:
            if sample in o[4]:
                continue
            val = _get(stat, sample, size_class(o[1], o[2]))
            first = next((k for k, c in enumerate(cs) if match(c, o, po)), None)
            if first is None:
                val[TN] += 1
                continue
            for k in range(first, len(cs)):
                c = cs[k]
                if c[0] != o[0] or c[1] > o[2]:
                    break
                if own[k] and match(c, o, po):
                    break
                val[FP] += 1
    return stat


def sample_names(cnvs, truths):
    """The union of the truth and the test samples, sorted: the ids of the device call"""
    names = {c[4] for c in cnvs}
    for t in truths:
        names.update(t[4])
    return sorted(names)


def as_array(stat, names):
    """[n_samples][3][4] nested lists, FP FN TP TN"""
    return [[list(stat.get((s, k), (0, 0, 0, 0))) for k in range(3)] for s in names]


def tabulate(stat):
    """cnveval.go:118-133 Tabulate: four [FP, FN, TP, TN]"""
    tabs = [[0, 0, 0, 0] for _ in range(4)]
    for (_, cls), st in stat.items():
        for f in range(4):
            tabs[cls][f] += st[f]
    for cls in range(3):
        for f in range(4):
            tabs[3][f] += tabs[cls][f]
    return tabs


def _ratio(a, b):
    """Go's %.4f of float64(a) / float64(b): 0 / 0 prints NaN"""
    return "NaN" if b == 0 else "%.4f" % (float(a) / float(b))


def stat_string(st):
    """cnveval.go:93-96 Stat.String; '-' overrides '0' in %-04d: left-justified, space-padded"""
    return "precision: %s (%-4d / (%-4d + %-4d)) recall: %s (%-4d / (%-4d + %-4d))" % (
        _ratio(st[TP], st[TP] + st[FP]), st[TP], st[TP], st[FP], _ratio(st[TP], st[TP] + st[FN]), st[TP], st[TP], st[FN])


def report(stat):
    """the four lines the command prints"""
    tabs = tabulate(stat)
    return "".join("size-class: %-12s | %s\n" % (CLASS_NAMES[k], stat_string(tabs[k])) for k in range(4))
