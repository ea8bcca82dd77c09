"""The cases the cnveval tests run, hand-made and seeded, with the restatement's counts computed once a process.

CPU tests (tests/test_cnveval_ref.py) hold the literal walk and the order-free form to each other on every case; the GPU
tests (tests/test_gpu_cnveval.py) run the same cases through the C ABI.  Shapes follow the kernels' structure
(goleft_amd/csrc/gd_cnveval.hpp): 256 work items a workgroup; the pairs kernel gives a workgroup one sample and 256
truths a pass, and a launch min(ceil(truths / 256), max(1, 1024 / samples with calls)) workgroups a sample, which
stride over the rest; the membership bitmap holds 32 samples a word."""
import functools

import numpy as np

from tests import cnveval_ref as R

WG = 256                 # work items of a workgroup, truths of one pass of it (CE_WG)
TARGET_BLOCKS = 1024     # workgroups of a pairs launch, about (CE_TARGET_BLOCKS)
WORD = 32                # samples of a membership word
PO = 0.4


class Case:
    def __init__(self, cnvs, truths, po=PO):
        self.cnvs = [tuple(c) for c in cnvs]
        self.truths = [(t[0], t[1], t[2], t[3], list(t[4])) for t in truths]
        self.po = po


WORKED_TRUTH = "1\t1000\t6000\t1\ta,b\n1\t50000\t90000\t3\ta\n10\t0\t150000\t0\tb\n2\t100\t200\t1\tc\n"
WORKED_TEST = ("1\t1200\t5800\t1\ta\n1\t1300\t5000\t1\ta\n1\t52000\t95000\t4\tb\n1\t60000\t61000\t2\tb\n"
               "10\t10\t140000\t0\tb\n2\t100\t200\t1\ta\n")
WORKED_OUT = (
    "size-class: 0-20000      | precision: 0.2000 (1    / (1    + 4   )) recall: 0.5000 (1    / (1    + 1   ))\n"
    "size-class: 20000-100000 | precision: 0.0000 (0    / (0    + 3   )) recall: 0.0000 (0    / (0    + 1   ))\n"
    "size-class: >=100000     | precision: 1.0000 (1    / (1    + 0   )) recall: 1.0000 (1    / (1    + 0   ))\n"
    "size-class: all          | precision: 0.2222 (2    / (2    + 7   )) recall: 0.5000 (2    / (2    + 2   ))\n")


def parse_bed(text, test):
    """the lines of a truth or a test file as tuples (a test line's sample is the first of its list)"""
    out = []
    for line in text.splitlines():
        if line.startswith("#"):
            continue
        f = line.split("\t")
        names = f[4].split(",")
        out.append((f[0], int(f[1]), int(f[2]), int(f[3]), names[0] if test else names))
    return out


def bed_text(items):
    return "".join("%s\t%d\t%d\t%d\t%s\n" % (x[0], x[1], x[2], x[3], x[4] if isinstance(x[4], str) else ",".join(x[4]))
                   for x in items)


def hand_cases():
    c = {}
    c["worked"] = Case(parse_bed(WORKED_TEST, True), parse_bed(WORKED_TRUTH, False))
    # poverlap == po exactly, and one base short of it
    c["exact_2_of_5"] = Case([("1", 3, 8, 1, "a")], [("1", 0, 5, 1, ["a"])], 0.4)
    c["short_of_2_of_5"] = Case([("1", 301, 801, 1, "a")], [("1", 1, 500, 1, ["a"])], 0.4)      # 199 of 499
    c["exact_5_of_10"] = Case([("1", 5, 15, 1, "a")], [("1", 0, 10, 1, ["b"])], 0.5)
    c["short_of_5_of_10"] = Case([("1", 50, 150, 1, "a")], [("1", 0, 99, 1, ["b"])], 0.5)       # 49 of 99
    c["po_1_inside"] = Case([("1", 10, 20, 1, "a"), ("1", 10, 21, 1, "a")], [("1", 0, 20, 1, ["a"]), ("1", 5, 30, 1, ["b"])], 1.0)
    c["abutting"] = Case([("1", 10, 20, 1, "a"), ("1", 20, 30, 1, "b")], [("1", 20, 30, 1, ["a"]), ("1", 10, 20, 1, ["b"])])
    c["zero_length_call"] = Case([("1", 15, 15, 1, "a"), ("1", 12, 18, 1, "a")], [("1", 10, 20, 1, ["a"]), ("1", 10, 20, 1, ["b"])])
    c["zero_length_truth"] = Case([("1", 10, 20, 1, "a"), ("1", 15, 15, 1, "b")], [("1", 15, 15, 1, ["a"]), ("1", 15, 15, 1, ["c"])])
    c["cn_3_is_7"] = Case([("1", 0, 10, 3, "a"), ("1", 0, 10, 7, "b")], [("1", 0, 10, 7, ["a"]), ("1", 0, 10, 3, ["c"])])
    c["cn_2_is_not_3"] = Case([("1", 0, 10, 2, "a"), ("1", 0, 10, 3, "b")], [("1", 0, 10, 3, ["a"]), ("1", 0, 10, 2, ["b"])])
    c["cn_negative"] = Case([("1", 0, 10, -1, "a"), ("1", 0, 10, -2, "b")], [("1", 0, 10, -1, ["a", "b"]), ("1", 0, 10, -2, ["c"])])
    c["class_edges"] = Case(
        [("1", 0, 19999, 1, "a"), ("1", 100000, 120000, 1, "a"), ("1", 200000, 299999, 1, "b"), ("1", 400000, 500000, 1, "b"),
         ("1", 600000, 600001, 1, "b")],
        [("1", 0, 19999, 1, ["a"]), ("1", 100000, 120000, 1, ["a"]), ("1", 200000, 299999, 1, ["a"]), ("1", 400000, 500000, 1, ["a"]),
         ("2", 0, 20000, 1, ["b"]), ("2", 0, 99999, 1, ["b"]), ("2", 0, 100000, 1, ["c"])])
    c["chromosomes"] = Case(
        [("1", 0, 100, 1, "a"), ("10", 0, 100, 1, "a"), ("2", 0, 100, 1, "a"), ("X", 0, 100, 1, "a"), ("10", 50, 150, 1, "b")],
        [("2", 0, 100, 1, ["a"]), ("10", 0, 100, 1, ["b"]), ("1", 0, 100, 1, ["b"]), ("MT", 0, 100, 1, ["a"]), ("10", 20, 120, 1, ["c"])])
    # two calls of equal (chrom, start) that both match one truth: the first in input order is counted
    c["tie_input_order"] = Case([("1", 1000, 150000, 1, "a"), ("1", 1000, 90000, 1, "a")], [("1", 1000, 200000, 1, ["a"])])
    c["tie_input_order_swapped"] = Case([("1", 1000, 90000, 1, "a"), ("1", 1000, 150000, 1, "a")], [("1", 1000, 200000, 1, ["a"])])
    c["sample_named_twice"] = Case([("1", 0, 100, 1, "a"), ("1", 500, 600, 1, "a")], [("1", 0, 100, 1, ["a", "a"]), ("1", 900, 950, 1, ["a", "b", "a"])])
    c["sample_only_in_truths"] = Case([("1", 0, 100, 1, "a")], [("1", 0, 100, 1, ["zz"]), ("1", 0, 100, 1, ["a", "zz"])])
    c["sample_only_in_calls"] = Case([("1", 0, 100, 1, "a"), ("1", 0, 100, 1, "q")], [("1", 0, 100, 1, ["a"])])
    c["truth_names_everyone"] = Case([("1", 0, 100, 1, "a"), ("1", 0, 100, 1, "b"), ("1", 300, 400, 1, "c")], [("1", 0, 100, 1, ["a", "b", "c"])])
    c["no_truths"] = Case([("1", 0, 100, 1, "a"), ("1", 0, 30000, 1, "a"), ("2", 0, 100000, 1, "b")], [])
    c["no_calls"] = Case([], [("1", 0, 100, 1, ["a"]), ("1", 0, 100, 1, ["b"])])
    c["nothing"] = Case([], [])
    # step 4: the first match is own / a later own match stops the run / calls that do not match inside the run
    c["walk_first_is_own"] = Case([("1", 0, 100, 1, "a"), ("1", 50, 150, 1, "a")], [("1", 0, 100, 1, ["a"]), ("1", 0, 160, 1, ["b"])])
    c["walk_later_own_stops"] = Case(
        [("1", 0, 100, 1, "a"), ("1", 10, 120, 1, "a"), ("1", 200, 300, 1, "a"), ("1", 250, 400, 1, "a")],
        [("1", 200, 300, 1, ["a"]), ("1", 0, 400, 1, ["b"])], 0.2)
    c["walk_non_matching_inside"] = Case(
        [("1", 0, 100, 1, "a"), ("1", 10, 12, 0, "a"), ("1", 20, 21, 1, "a"), ("1", 30, 130, 1, "a"), ("1", 401, 500, 1, "a")],
        [("1", 0, 400, 1, ["b"]), ("1", 0, 30000, 1, ["c"])])
    return c


CHROMS = ("1", "10", "2", "X")


def seeded(seed, n_samples, n_truths, calls, span=4000, max_len=1500, po=PO, huge=False, with_calls=None):
    """n_samples samples s000 .., calls a sample for the first with_calls of them (all by default), n_truths truths with
    long-tailed sample lists.  Coordinates are drawn small: overlaps, equal starts and shared intervals are common."""
    rng = np.random.default_rng(seed)
    names = ["s%03d" % i for i in range(n_samples)]
    with_calls = n_samples if with_calls is None else with_calls

    def interval():
        start = int(rng.integers(0, span))
        length = int(rng.choice([0, 1, 7, 100, int(rng.integers(1, max_len)), int(rng.integers(1, max_len))]))
        return str(rng.choice(CHROMS)), start, start + length, int(rng.integers(0, 5))

    truths = []
    for _ in range(n_truths):
        k = min(n_samples, int(rng.choice([1, 1, 1, 2, 3, max(1, n_samples // 2), n_samples])))
        who = [names[i] for i in rng.choice(n_samples, size=k, replace=False)]
        if rng.random() < 0.05:
            who.append(who[0])
        truths.append(interval() + (who,))
    if huge:
        truths[0] = ("1", 0, 10 * span, 1, [names[-1]])
        truths.append(("1", 0, 10 * span, 1, [names[0]]))
    cnvs = []
    for s in range(with_calls):
        for _ in range(calls):
            chrom, start, end, cn = interval()
            if huge and s == 0:
                chrom, cn = "1", 1
            # half of the calls sit on a truth, moved a little
            if truths and rng.random() < 0.5:
                t = truths[int(rng.integers(0, len(truths)))]
                if not (huge and s == 0):
                    chrom = t[0]
                    cn = t[3] if rng.random() < 0.8 else cn
                start, end = max(0, t[1] + int(rng.integers(-20, 21))), max(0, t[2] + int(rng.integers(-20, 21)))
                end = max(end, start)
            cnvs.append((chrom, start, end, cn, names[s]))
    order = rng.permutation(len(cnvs))
    return Case([cnvs[i] for i in order], truths, po)


def seeded_cases():
    c = {}
    for t in (1, 63, 64, 65, WG - 1, WG, WG + 1):
        c["truths_%d" % t] = seeded(1000 + t, 5, t, 6)
    for k in (1, 64, 65):
        c["calls_%d" % k] = seeded(1100 + k, 3, 40, k)
    c["longest_window"] = seeded(1200, 4, 50, 130, huge=True)
    for s in (WORD - 1, WORD, WORD + 1, 2 * WORD, 2 * WORD + 1):
        c["samples_%d" % s] = seeded(1300 + s, s, 70, 2)
    c["half_without_calls"] = seeded(1400, 40, 90, 3, with_calls=20)
    c["po_half"] = seeded(1500, 6, 120, 8, po=0.5)
    c["po_one"] = seeded(1501, 6, 120, 8, po=1.0)
    # a launch of the pairs kernel: TARGET_BLOCKS / 256 samples = 4 workgroups a sample, 1024 truths a pass
    per_launch = (TARGET_BLOCKS // 256) * WG
    for t in (per_launch - 1, per_launch, per_launch + 1):
        c["launch_%d" % t] = seeded(1600 + t, 256, t, 1, span=20000)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    c = {"hand_" + k: v for k, v in hand_cases().items()}
    c.update(seeded_cases())
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """(sample names, the literal walk's [n_samples][3][4] counts) of a case, computed once"""
    case = cases()[name]
    names = R.sample_names(case.cnvs, case.truths)
    stat = R.evaluate_literal(case.cnvs, case.truths, case.po)
    return names, np.array(R.as_array(stat, names), np.int64).reshape(len(names), 3, 4)


def device_inputs(case):
    """What gd_cnveval takes: names, and a dict of arrays -- the calls grouped by sample and stably sorted by (chromosome
    rank, start), the truths with a CSR of sample ids.  Chromosomes are ranked in byte order over both sets."""
    names = R.sample_names(case.cnvs, case.truths)
    sid = {s: i for i, s in enumerate(names)}
    chroms = sorted({c[0] for c in case.cnvs} | {t[0] for t in case.truths}, key=lambda s: s.encode())
    rank = {c: i for i, c in enumerate(chroms)}
    by = [[] for _ in names]
    for c in case.cnvs:
        by[sid[c[4]]].append(c)
    rows, off = [], [0]
    for cs in by:
        rows += sorted(cs, key=lambda c: (rank[c[0]], c[1]))
        off.append(len(rows))
    i32 = lambda xs: np.array(xs, np.int32).reshape(-1)
    t_off, t_ids = [0], []
    for t in case.truths:
        t_ids += [sid[s] for s in t[4]]
        t_off.append(len(t_ids))
    return names, dict(
        cnv_off=np.array(off, np.int64), cnv_chrom=i32([rank[c[0]] for c in rows]), cnv_start=i32([c[1] for c in rows]),
        cnv_end=i32([c[2] for c in rows]), cnv_cn=i32([c[3] for c in rows]),
        t_chrom=i32([rank[t[0]] for t in case.truths]), t_start=i32([t[1] for t in case.truths]),
        t_end=i32([t[2] for t in case.truths]), t_cn=i32([t[3] for t in case.truths]),
        t_off=np.array(t_off, np.int64), t_samples=i32(t_ids))
