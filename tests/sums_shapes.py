"""Shapes for gd_sums_stream_kernel (and the fallback gd_tile_sums_kernel) at the kernel's own thresholds, with the
two things a test needs to trust them: a second reference that is independent of the C oracle, and a plain model
of the kernel's routing that says whether a shape reaches the edge it is named for.

Test infrastructure only, no pytest marks: tests/test_sums_shapes.py (CPU) shows that every case hits its edge and
that both references agree; tests/test_gpu_sums_stream_shapes.py runs every case on the device under both kernels.

The routing model is written from the comments of goleft_amd/csrc/gd_sums_stream.hpp:
  * a wave takes 4096 consecutive reads of one contig, 16 groups of 256, four consecutive reads per lane;
  * a read is kept when no flag bit of the mask is set, MAPQ >= Q and it has ops;
  * a kept read of at most two ops with ONE counted op (M = X) and nothing that consumes the reference before it is
    that op; it FITS when the op has fewer than 2^22 bases, POS >= 0, and it ends (clipped to the contig) at or before
    the end of the lane's third window, the lane's first window being the one of its first read;
  * a kept read of three ops at POS >= 0 is queued WITH its ops when its group's ops are fetched -- one read per lane
    and round, a round is refused as a whole when the 256-slot queue has no room for it, and what is refused stays an
    ordinary odd read;
  * every other kept read is ODD: queued by index when its group is worked on, one read per lane and round; when a
    round would take the queue past 256 it is drained first;
  * the ops of group g + 1 are fetched before group g is worked on (the software pipeline);
  * the wave has 256 window accumulators from the window of its first read on.
The model's constants are restated here, not read from the header; kernel_constants() reads the header's and
tests/test_sums_shapes.py holds the two against each other (GD_SUMS_DRAIN_AT can be overridden with -D: the product
build does not, and the model describes the product build).
"""
import os
import re
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from oracle import pyoracle as po
from tests import helpers as H

WAVE_READS, GROUP_READS, QUEUE_SLOTS, N_ACC, FIT_BASES = 4096, 256, 256, 256, 1 << 22
COUNTED, CONSUMING = (0, 7, 8), (0, 2, 3, 7, 8)
LMAX = 0x7fff0000
OPS = "MIDNSHP=X"


def kernel_constants():
    """The constants of goleft_amd/csrc/gd_sums_stream.hpp that the model restates, read from the header's text."""
    with open(os.path.join(H.ROOT, "goleft_amd", "csrc", "gd_sums_stream.hpp")) as f:
        text = f.read()
    def num(pattern):
        return int(re.search(pattern, text).group(1))
    u = num(r"constexpr int U = (\d+);")
    return {"reads_per_lane": u, "group": 64 * u, "wave": 64 * u * num(r"constexpr uint32_t GPW = (\d+);"),
            "queue": num(r"constexpr int SQ_CAP = (\d+);"), "drain_at": num(r"#define GD_SUMS_DRAIN_AT (\d+)"),
            "accumulators": num(r"constexpr uint32_t NACC = (\d+);"),
            "fit_bases": 1 << num(r"\(len < \(1u << (\d+)\)\)")}


def unit_contigs(c):
    """Contig of every 4096-read unit of a case's job, in unit order (contigs without reads own none)."""
    return [t for t in range(len(c.lengths)) for _ in range((c.get(t).n + WAVE_READS - 1) // WAVE_READS)]


# ---- the second reference -------------------------------------------------------------------------------------------

def counted_intervals(r, Q, flag_mask, length):
    """(s, e) int64: every counted interval (M, =, X with at least one base) of every kept read, clipped to
    [0, length); empty ones removed.  D and N advance the reference, I S H P and the codes 9-15 do nothing."""
    nops = np.diff(r.cigar_off.astype(np.int64))
    op = (r.cigar & 15).astype(np.int64)
    ln = (r.cigar >> 4).astype(np.int64)
    adv = np.where(np.isin(op, CONSUMING), ln, 0)
    before = np.cumsum(adv) - adv                                   # reference bases consumed by earlier ops, all reads
    owner = np.repeat(np.arange(r.n), nops)
    first = r.cigar_off[:-1].astype(np.int64)
    at_first = before[np.minimum(first, max(len(before) - 1, 0))] if len(before) else np.zeros(r.n, np.int64)
    start = r.pos.astype(np.int64)[owner] + before - at_first[owner]
    kept = ((r.flag.astype(np.int64) & int(flag_mask)) == 0) & (r.mapq.astype(np.int64) >= Q)
    use = kept[owner] & np.isin(op, COUNTED)
    s = np.clip(start[use], 0, length)
    e = np.clip(start[use] + ln[use], 0, length)
    ok = e > s
    return s[ok], e[ok]


def interval_window_sums(reads, Q, flag_mask, length, W):
    """int64[ceil(length / W)]: the sum over all counted intervals of their overlap with each window.  With
    F(x) = the covered bases below x = sum_i (min(e_i, x) - min(s_i, x)), the overlap total of the window [a, b) is
    F(b) - F(a); sum_i min(v_i, x) comes from the sorted v and their running sum.  Exact int64 throughout, and no
    per-base vector: a contig of 0x7fff0000 positions costs as much as one of 1000."""
    nwin = (length + W - 1) // W
    s, e = counted_intervals(reads, Q, flag_mask, length)
    edges = np.minimum(np.arange(nwin + 1, dtype=np.int64) * W, length)

    def sum_of_min(v):
        v = np.sort(v)
        run = np.concatenate([[0], np.cumsum(v)])
        k = np.searchsorted(v, edges, "right")                       # v[:k] <= edge: they count in full
        return run[k] + edges * (len(v) - k)

    F = sum_of_min(e) - sum_of_min(s)
    return np.diff(F)


# ---- the routing model ----------------------------------------------------------------------------------------------

@dataclass
class Wave:
    first_read: int
    n_fit: int = 0
    n_three: int = 0
    n_odd: int = 0
    occupancy: list = field(default_factory=list)    # the queue after every round of insertions
    refused: bool = False                            # a three-op read found no room and stayed an odd read
    drains: list = field(default_factory=list)       # (three-op items, odd items) of every drain, the final one included
    first_window: int = 0
    lo_window: int = -1                              # lowest / highest window a kept read's counted bases touch
    hi_window: int = -1


@dataclass
class Routing:
    kept: np.ndarray          # bool[n]: the read filter
    route: list               # per read: "drop", "none" (kept, nothing counted), "fit", "three", "odd"
    end: np.ndarray           # int64[n]: clipped end of a read that is ONE counted op, else -1
    nb2: np.ndarray           # int64[n]: end of the third window of the read's lane
    waves: list


def _single_op(ops):
    """A read of at most two ops as one counted op: its length; 0 when nothing is counted; None for the general walk."""
    if len(ops) == 1:
        return ops[0][0] if ops[0][1] in COUNTED else 0
    (la, a), (lb, b) = ops
    if a in COUNTED and b not in COUNTED:
        return la
    if a not in CONSUMING and b in COUNTED:
        return lb
    if a not in COUNTED and b not in COUNTED:
        return 0
    return None


def classify(reads, Q, flag_mask, length, W):
    n = reads.n
    pos = reads.pos.astype(np.int64).tolist()
    off = reads.cigar_off.astype(np.int64).tolist()
    cig = reads.cigar.astype(np.int64).tolist()
    flag, mapq = reads.flag.astype(np.int64).tolist(), reads.mapq.astype(np.int64).tolist()
    kept = np.zeros(n, bool)
    route = ["drop"] * n
    end = np.full(n, -1, np.int64)
    nb2 = np.zeros(n, np.int64)
    want3 = [False] * n
    waves = []
    for w0 in range(0, n, WAVE_READS):
        wv = Wave(w0, first_window=max(pos[w0], 0) // W)
        w1 = min(n, w0 + WAVE_READS)
        for i in range(w0, w1):
            ops = [(c >> 4, c & 15) for c in cig[off[i]:off[i + 1]]]
            lane_first = i - (i - w0) % 4
            nb2[i] = min((max(pos[lane_first], 0) // W + 3) * W, 0xffffffff)
            if (flag[i] & flag_mask) or mapq[i] < Q or not ops:
                continue
            kept[i] = True
            x = pos[i]
            for l, o in ops:                                         # the windows its counted bases touch
                if o in COUNTED and l:
                    s, e = min(max(x, 0), length), min(max(x + l, 0), length)
                    if e > s:
                        wv.lo_window = s // W if wv.lo_window < 0 else min(wv.lo_window, s // W)
                        wv.hi_window = max(wv.hi_window, (e - 1) // W)
                if o in CONSUMING:
                    x += l
            one = _single_op(ops) if len(ops) <= 2 else None
            if one == 0:
                route[i] = "none"
            elif one is not None:
                end[i] = min(max(pos[i], 0) + one, length)
                route[i] = "fit" if one < FIT_BASES and pos[i] >= 0 and end[i] <= nb2[i] else "odd"
            else:
                route[i] = "odd"
                want3[i] = len(ops) == 3 and pos[i] >= 0
        # the queue, in the pipeline's order: the ops of group g + 1 are fetched before group g is worked on
        qn, q3, qo = 0, 0, 0

        def rounds(idx):
            """Reads of one group that want a slot -> one read per lane and round."""
            by_lane = {}
            for i in idx:
                by_lane.setdefault((i - w0) // 4, []).append(i)
            k = 0
            while True:
                r_ = [v[k] for v in by_lane.values() if len(v) > k]
                if not r_:
                    return
                yield r_
                k += 1

        groups = list(range(w0, w1, GROUP_READS))

        def fetch(g):
            nonlocal qn, q3
            full = False
            for r_ in rounds([i for i in range(g, min(w1, g + GROUP_READS)) if want3[i]]):
                if full or qn + len(r_) > QUEUE_SLOTS:
                    full = wv.refused = True
                    continue
                for i in r_:
                    route[i] = "three"
                qn += len(r_)
                q3 += len(r_)
                wv.occupancy.append(qn)

        def work(g):
            nonlocal qn, q3, qo
            for r_ in rounds([i for i in range(g, min(w1, g + GROUP_READS)) if route[i] == "odd"]):
                if qn + len(r_) > QUEUE_SLOTS:
                    wv.drains.append((q3, qo))
                    qn = q3 = qo = 0
                qn += len(r_)
                qo += len(r_)
                wv.occupancy.append(qn)

        fetch(groups[0])
        for k, g in enumerate(groups):
            if k + 1 < len(groups):
                fetch(groups[k + 1])
            work(g)
        if qn:
            wv.drains.append((q3, qo))
        for i in range(w0, w1):
            wv.n_fit += route[i] == "fit"
            wv.n_three += route[i] == "three"
            wv.n_odd += route[i] == "odd"
        waves.append(wv)
    return Routing(kept, route, end, nb2, waves)


# ---- building records -----------------------------------------------------------------------------------------------

def cig(text):
    """'50M3D60M' -> [(50, 0), (3, 2), (60, 0)]"""
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num), OPS.index(ch)))
            num = ""
    return out


def make_reads(pos, cigars, flag=None, mapq=None):
    """Reads from positions (sorted) and one op list [(len, op), ...] or CIGAR text per read."""
    cigars = [cig(c) if isinstance(c, str) else c for c in cigars]
    pos = np.asarray(pos, np.int64)
    assert len(pos) == len(cigars) and (np.diff(pos) >= 0).all(), "records must be coordinate sorted"
    off = np.zeros(len(pos) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in cigars])
    flat = np.array([(l << 4) | o for c in cigars for l, o in c], np.int64)
    return po.Reads(pos.astype(np.int32), np.zeros(len(pos), np.uint16) if flag is None else flag,
                    np.full(len(pos), 60, np.uint8) if mapq is None else mapq, off.astype(np.uint32),
                    flat.astype(np.uint32))


@dataclass
class Case:
    name: str
    W: int
    lengths: list
    reads: dict                     # tid -> po.Reads (contigs without an entry have no reads)
    Q: int = 1
    flag_mask: int = 0x704
    huge: tuple = ()                # contigs too long for a per-base vector: the interval reference, oracle on ranges
    guarded: bool = False           # the device test hands the records over inside arenas whose neighbours look alive

    def get(self, tid):
        return self.reads.get(tid, H.empty_reads())


A_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 1023, 1024, 1025, 4095, 4096, 4351, 8191,
            8192)
A_PLACED = {63: 4097, 64: 12289, 65: 8193, 127: 4353, 128: 769}
A_EMPTY = (0, 62, 66, 126, 129, 130)
A_UNIT = 67                          # length 1, one `1M` read


def a_contig(rng, n):
    """n reads `<len>M`, every length once; every third read dropped by one of five reasons in turn (period 15);
    the last read and the first read of every group of 256 kept."""
    L = 3 * n + 50
    pos = np.sort(rng.integers(0, L, size=n))
    lens = 1 + rng.permutation(n)
    flag, mapq = np.zeros(n, np.uint16), np.full(n, 60, np.uint8)
    i = np.arange(n)
    drop = (i % 3 == 2) & (i % GROUP_READS != 0) & (i != n - 1)
    kind = (i // 3) % 5
    for k, f in enumerate((0x4, 0x100, 0x200, 0x400)):
        flag[drop & (kind == k)] = f
    mapq[drop & (kind == 4)] = 0
    return L, make_reads(pos, [[(int(l), 0)] for l in lens], flag, mapq)


def case_a(n_ctgs):
    rng = np.random.default_rng(131)
    lengths, reads = [0] * 131, {}
    counts = dict(A_PLACED)
    free = [t for t in range(1, 62) if t not in counts]
    counts.update(zip(free, A_COUNTS))
    for t in range(131):
        if t in A_EMPTY:
            lengths[t] = 1000 + t
        elif t == A_UNIT:
            lengths[t], reads[t] = 1, make_reads([0], ["1M"])
        elif t in counts:
            lengths[t], reads[t] = a_contig(rng, counts[t])
        else:
            lengths[t] = 2000 + 7 * t
            reads[t] = H.random_reads(rng, lengths[t], 40 + t % 9, max_len=150)
    return Case("a%d" % n_ctgs, 100, lengths[:n_ctgs], {t: r for t, r in reads.items() if t < n_ctgs})


B_LENS = (0, 1, 37)


def case_b():
    """Every CIGAR of one, two and three ops.  The op lengths come from {0, 1, 37}: the one- and two-op CIGARs are
    repeated once per combination of lengths (3 and 9 passes), the 4096 three-op ones -- one full wave -- walk through
    the 27 combinations as they go."""
    def stream(n_ops, passes):
        combos = 16 ** n_ops
        cigars = []
        for i in range(combos * passes):
            ops = [(i // 16 ** (n_ops - 1 - j)) % 16 for j in range(n_ops)]
            turn = i // combos if passes > 1 else i
            ls = [B_LENS[(turn // 3 ** j) % 3] for j in range(n_ops)]
            if n_ops == 2 and ops == [4, 3] and ls[0] == 0:
                ls[0] = 1                                            # `0S <n>N`: SAM's placeholder of a CG-tag CIGAR
            cigars.append(list(zip(ls, ops)))
        n = len(cigars)
        return 29 * n + 10, make_reads(29 * np.arange(n), cigars)
    parts = [stream(1, 3), stream(2, 9), stream(3, 1)]
    return Case("b", 64, [p[0] for p in parts], {t: p[1] for t, p in enumerate(parts)})


THREE, FIVE = "50M3D60M", "30M2I30M4D30M"


def case_c():
    """One wave of `150M` reads per contig, with odd reads at chosen indices."""
    def wave(odd):
        return 7 * WAVE_READS + 300, make_reads(7 * np.arange(WAVE_READS), [odd.get(i, "150M") for i in range(WAVE_READS)])
    lanes64 = lambda g: [g * GROUP_READS + 4 * lane + g % 4 for lane in range(64)]       # one read per lane of group g
    five256 = [i for g in range(4) for i in lanes64(g)]
    parts = [wave({i: THREE for i in range(256)}),
             wave({i: THREE for i in range(257)}),
             wave({i: FIVE for i in five256}),
             wave({i: FIVE for i in five256 + [4 * GROUP_READS + 9]}),
             wave({i: FIVE for i in range(WAVE_READS)}),
             wave({i: (THREE, FIVE)[i % 2] for i in range(WAVE_READS)}),
             wave({WAVE_READS - 1: FIVE})]
    return Case("c", 250, [p[0] for p in parts], {t: p[1] for t, p in enumerate(parts)})


D_FORMS = ("%dM", "20S%dM", "%dM50S", "%dM3I", "%dM2D", "5H%dM")


def case_d(W):
    """Hand-placed lanes of four reads around the end of the lane's third window, then plain reads, then the
    contig's end.  Lane j starts in window 10 + 8 j: the lanes stay sorted and do not touch each other."""
    # position 0: a plain read, one from boundary to boundary, the five two-op forms
    pos, cigars = [0] * 7 + [1], ["%dM" % min(W, 150), "%dM" % W] + [f % 30 for f in D_FORMS[1:]] + ["7M"]
    k = 10
    for form in D_FORMS:
        for delta in (0, 1, W - 1):
            for over in (-1, 0, 1):
                s = k * W + delta
                pos += [s, s, s + 1, s + 2]
                cigars += ["5M", form % ((k + 3) * W + over - s), "3M", "4M"]
                k += 8
    s = k * W                                                        # boundary to boundary, inside a lane
    pos += [s, s, s + W, s + W]
    cigars += ["3M", "%dM" % W, "%dM" % W, "1M"]
    plain = 150 if W >= 100 else 40
    n_pad = WAVE_READS - len(pos)
    p0 = (k + 8) * W
    pos += [p0 + 5 * i for i in range(n_pad)]
    cigars += ["%dM" % plain] * n_pad
    length = p0 + 5 * n_pad + 10 * W + 1000
    for at, bases in ((length - 150, 150), (length - 149, 150), (length - 1, 77)):     # to the end, 1 past it, at length - 1
        pos += [at] * len(D_FORMS)
        cigars += [f % bases for f in D_FORMS]
    pos += [length - 1, length - 1]
    cigars += ["77M", "1M"]
    return Case("d%d" % W, W, [length], {0: make_reads(pos, cigars)})


E_KW0 = 40


def case_e():
    """W = 32.  The accumulators of a wave cover the windows kw0 .. kw0 + 255."""
    W, base = 32, E_KW0 * 32
    def spread(reach, bases, n=WAVE_READS):
        """n reads of `<bases>M` from window kw0 on, the last one ending at base + reach."""
        room = reach - bases
        return [base + (i * room) // (n - 1) for i in range(n)], ["%dM" % bases] * n
    parts = [spread(N_ACC * W, 150), spread(N_ACC * W + 1, 150),
             ([base + 300 * W * i for i in range(700)], ["150M"] * 700),
             ([base + 2 * i for i in range(2000)] + [base + 10_000 * W + 2 * i for i in range(2096)], ["150M"] * WAVE_READS),
             spread(N_ACC * W, 20), spread(N_ACC * W + 1, 20)]       # the same two edges on the fitting path
    lengths = [p[0][-1] + 5000 for p in parts]
    return Case("e", W, lengths, {t: make_reads(*p) for t, p in enumerate(parts)})


def case_e_short():
    """A contig shorter than one window, two waves of reads on it."""
    n = WAVE_READS + 1
    return Case("e-short", 4096, [3000], {0: make_reads((np.arange(n) * 2990) // n, ["150M"] * n)})


def case_f_len(W):
    """One-op reads of 2^22 - 1, 2^22 and 2^22 + 1 bases in one lane, then plain reads."""
    pos = [10, 11, 12, 13] + [5000 + 3 * i for i in range(300)]
    cigars = ["%dM" % (FIT_BASES - 1), "%dM" % FIT_BASES, "%dM" % (FIT_BASES + 1), "150M"] + ["150M"] * 300
    return Case("f-len-%d" % W, W, [1 << 24], {0: make_reads(pos, cigars)})


def case_f_sum():
    """4096 reads of 2^22 - 1 bases at one position: a group's prefix sum is 2^30, the window's total 2^34."""
    return Case("f-sum", 1 << 23, [1 << 24], {0: make_reads([77] * WAVE_READS, ["%dM" % (FIT_BASES - 1)] * WAVE_READS)})


def case_f_sum_wide():
    """4096 reads of 2^24 bases at position 0 of a 2^24 contig, one window: were they folded in the lanes (the 2^22
    bound is what keeps them out), a group's 32-bit prefix sum would be 2^32 exactly."""
    return Case("f-sum-wide", 1 << 24, [1 << 24], {0: make_reads([0] * WAVE_READS, ["%dM" % (1 << 24)] * WAVE_READS)})


def case_f_w(W):
    rng = np.random.default_rng(5)
    return Case("f-w-%d" % W, W, [5003, 1], {0: H.random_reads(rng, 5003, 700, max_len=200),
                                              1: make_reads([0], ["1M"])})


def case_f_huge():
    """W = 2^30 + 1 on the longest contig: two reads across the window boundary, twenty in the last 70 000 positions,
    the last of them hanging over the end."""
    W = (1 << 30) + 1
    pos = [W - 75, W - 1] + [LMAX - 70_000 + 3600 * i for i in range(19)] + [LMAX - 60]
    cigars = ["150M", "50M3D60M"] + [("150M", "20S130M", "30M2I30M4D30M", "70M900N80M")[i % 4] for i in range(19)] + ["150M"]
    return Case("f-huge", W, [LMAX], {0: make_reads(pos, cigars)}, huge=(0,))


def case_guard():
    """Read counts around multiples of 2 and 4 (the flag and MAPQ loads are rounded up to whole dwords) and one read
    past a full wave.  The device test adopts these records as the front of larger tensors of its own whose next
    elements look like live records (flag 0, MAPQ 60, a whole-contig `M` op).  The kernel's rounded-up flag and MAPQ
    loads do reach those bytes, by design; what it must not do is count them.  A tripwire for the unmodified kernel,
    over memory the test owns -- not a way to run a kernel that was edited to read past its records."""
    rng = np.random.default_rng(9)
    counts = (1, 2, 3, 5, 6, 7, 258, 4097, 4098, 4099)
    lengths, reads = [], {}
    for t, n in enumerate(counts):
        L = 5 * n + 400
        lengths.append(L)
        reads[t] = make_reads(np.sort(rng.integers(0, L, size=n)), ["%dM" % (20 + i % 131) for i in range(n)])
    return Case("guard", 100, lengths, reads, guarded=True)


BUILDERS = {
    "a131": lambda: case_a(131), "a64": lambda: case_a(64), "a65": lambda: case_a(65),
    "b": case_b, "c": case_c,
    "d32": lambda: case_d(32), "d100": lambda: case_d(100), "d4096": lambda: case_d(4096),
    "e": case_e, "e-short": case_e_short,
    "f-len-4096": lambda: case_f_len(4096), "f-len-2m": lambda: case_f_len(1 << 21), "f-sum": case_f_sum,
    "f-sum-wide": case_f_sum_wide,
    "f-w-max": lambda: case_f_w((1 << 31) - 1), "f-w-2^30+1": lambda: case_f_w((1 << 30) + 1), "f-huge": case_f_huge,
    "guard": case_guard,
}
NAMES = tuple(BUILDERS)


@lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def busy_ranges(r, length, pad=1000):
    """[(a, b)]: the ranges of a huge contig that hold every base a read can cover, merged."""
    ends = po.read_ends(r)
    out = []
    for a, b in sorted(zip((np.maximum(r.pos.astype(np.int64) - pad, 0)).tolist(), np.minimum(ends + pad, length).tolist())):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b) for a, b in out]


def window_sums_from_ranges(r, Q, flag_mask, length, W, depth_of):
    """Window sums of a huge contig from per-base vectors of its busy ranges (depth_of(a, b) -> depths of [a, b)):
    every counted base lies in one of them."""
    sums = np.zeros((length + W - 1) // W, np.int64)
    for a, b in busy_ranges(r, length):
        d = np.asarray(depth_of(a, b)).astype(np.int64)
        p = np.arange(a, b, dtype=np.int64)
        np.add.at(sums, p // W, d)
    return sums


@lru_cache(maxsize=None)
def oracle_sums(name):
    """tuple of int64 window sums per contig of a case, from the C oracle's per-base vector (on a huge contig: from its
    vectors over the ranges around the reads).  Computed once; do not write to it."""
    c = case(name)
    out = []
    for t, L in enumerate(c.lengths):
        r = c.get(t)
        if t in c.huge:
            s = window_sums_from_ranges(r, c.Q, c.flag_mask, L, c.W, lambda a, b: po.perbase_c(r, c.Q, a, b, c.flag_mask))
        else:
            d = po.perbase_c(r, c.Q, 0, L, c.flag_mask, diff=name.startswith("f-sum"))      # (2^34 increments one by one otherwise)
            s = H.oracle_windows(d, c.W)[0]
        s.setflags(write=False)
        out.append(s)
    return tuple(out)
