"""Shared by the .crai tests: writers of small .crai files, the host reader through its C entry, the sequences (lists of
(alnStart, alnSpan, sliceLen)) that pin gd_crai_sizes at its structural edges, and the twin .bai of a .crai -- a .bai
whose linear index holds the running sums of the restatement's tile sizes, so that both tools see exactly those sizes."""
import ctypes as C
import gzip
import os

import numpy as np

from tests import crai_ref as CR
from tests import indexcov_ref as IR
from tests.helpers import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", "ref")
VIRAL = os.path.join(GOLD, "viral.crai")
VIRAL_FAI = os.path.join(GOLD, "viral.fa.fai")
T = CR.T


def write_crai(path, text, members=1):
    """text (bytes) as `members` concatenated gzip members, cut at arbitrary bytes."""
    cuts = [len(text) * k // members for k in range(members + 1)]
    with open(path, "wb") as f:
        for a, b in zip(cuts, cuts[1:]):
            f.write(gzip.compress(text[a:b], mtime=0))
    return str(path)


def line(seq, start, span, slen, container=0, slice_start=0):
    return b"%d\t%d\t%d\t%d\t%d\t%d\n" % (seq, start, span, container, slice_start, slen)


def host_read(path):
    """gdh_crai_read -> per reference a list of (alnStart, alnSpan, sliceLen); raises CraiError(line) when refused."""
    from goleft_amd import _hostlib
    lib = _hostlib.load()
    nr, ns, ln = C.c_size_t(), C.c_size_t(), C.c_int64(-1)
    msg = C.create_string_buffer(256)
    rc = lib.gdh_crai_read(str(path).encode(), 0, 0, None, None, None, None, C.byref(nr), C.byref(ns), C.byref(ln), msg, 256)
    if rc == -2:
        raise CR.CraiError(ln.value, msg.value.decode())
    assert rc in (0, -3), rc
    off = np.zeros(nr.value + 1, np.int64)
    start, span = np.zeros(ns.value, np.int64), np.zeros(ns.value, np.int64)
    slen = np.zeros(ns.value, np.int32)
    rc = lib.gdh_crai_read(str(path).encode(), nr.value, ns.value, off.ctypes.data, start.ctypes.data, span.ctypes.data,
                           slen.ctypes.data, C.byref(nr), C.byref(ns), C.byref(ln), msg, 256)
    assert rc == 0, rc
    return [[(int(start[i]), int(span[i]), int(slen[i])) for i in range(off[r], off[r + 1])] for r in range(nr.value)]


# ---- sequences for gd_crai_sizes -----------------------------------------------------------------------------------------
def plain(n, step=20000, span=20000):
    return [(1 + i * step, span, 1000 + 7 * i) for i in range(n)]


def edge_sequences():
    """name -> sequence.  The slices of a sequence are loaded 64 at a time and a fill is stored 64 tiles at a time."""
    out = {}
    for n in (0, 1, 63, 64, 65, 128, 129):
        out["slices_%d" % n] = plain(n)
    for k in (0, 1, 63, 64, 65, 200):
        out["full_%d" % k] = [(1, k * T + 5, 12345)] + [(k * T + 10, T, 3)]
        # a small slice leaves a pending value; the next one starts k tiles on: k tiles of back fill, the first holds it
        out["backfill_%d" % k] = [(5, 100, 9), (k * T + 1 if k else T, T, 3)]
        out["backfill_zero_%d" % k] = [(k * T + 1 if k else T, T, 3)]            # nothing pending at the start: zeros
    for d in (-1, 0, 1):
        out["gap_edge_%d" % d] = [(1, 3 * T, 5), (3 * T + T + d, T, 6), (3 * T + T + d + 30000, 100, 2)]
    for name, off in (("T", T), ("mT", -T), ("mT1", -T - 1)):
        for span in (100, T, 2 * T + 1):
            out["over_%s_%d" % (name, span)] = [(1, 3 * T, 5), (3 * T + off, span, 6), (9 * T, T, 1)]
    for name, span in (("0", 3 * T), ("1", 3 * T + 1), ("T", 4 * T)):
        out["shift_to_%s" % name] = [(1, 10 * T, 7), (10 * T - 3 * T - 5, span, 11), (20 * T, T, 2)]
    out["pending_flushed"] = [(5, 100, 9), (70000, 16384, 3)]
    out["pending_dropped"] = [(1, T, 5), (T + 10, 100, 77)]
    out["big_per_base"] = [(1, 1, 2 ** 31 - 1), (5 * T, T, 1)]                  # 100000 * (2^31 - 1): above 2^32
    out["negative_len"] = [(1, 2 * T, -5), (2 * T + 1, 10, -(2 ** 31)), (6 * T, T, 1)]
    out["negative_start"] = [(-5, T, 3), (T, T, 4)]
    out["negative_start_shifted"] = [(-40000, 3 * T, 10), (-100, 2 * T, 4)]
    out["most_negative_start"] = [(-(2 ** 31 - 1), 2 ** 31 - 1, 1000), (1, 5 * T, 8)]
    out["largest_start"] = [(2 ** 31 - 1 - 70 * T, 3 * T, 2)]
    out["unsorted"] = [(20 * T, 2 * T, 5), (1, 4 * T, 6), (10 * T, 30 * T, 7), (2 * T, 5, 8), (50 * T, 5, 9), (60 * T, T, 1)]
    out["hand_1"] = [(10000, 20000, 100), (40000, 10000, 50)]
    out["hand_2"] = [(1, 16384, 16384), (100000, 40000, 7)]
    out["hand_3"] = [(1, 100000, 1000), (20000, 30000, 999), (120000, 20000, 40)]
    out["hand_4"] = [(1, 100000, 1000), (50000, 100000, 3000)]
    out["hand_6"] = [(16384, 16384, 1), (49152, 16383, 5), (65536, 16384, 2)]
    out["hand_7"] = [(1, 0, 5), (20000, 16384, 8)]
    return out


def random_sequences(seed, n=300):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = int(rng.integers(0, 201))
        at = int(rng.integers(-20000, 100000))
        seq = []
        for _ in range(k):
            at += int(rng.integers(-60000, 120000))                            # overlapping and unsorted
            kind = rng.integers(0, 10)
            span = 0 if kind == 0 else int(rng.integers(1, 300)) if kind == 1 else int(rng.integers(1, 200000))
            if kind == 2:
                span = int(rng.integers(1, 40)) * T                            # whole tiles
            slen = int(rng.integers(-1000, 2 ** 31 - 1)) if kind == 3 else int(rng.integers(0, 500000))
            seq.append((at, span, slen))
        out.append(seq)
    return out


def flatten(seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    for i, s in enumerate(seqs):
        off[i + 1] = off[i] + len(s)
    flat = [x for s in seqs for x in s]
    start = np.array([x[0] for x in flat], np.int64)
    span = np.array([x[1] for x in flat], np.int64)
    slen = np.array([x[2] for x in flat], np.int32)
    return off, start, span, slen


# ---- the twin ------------------------------------------------------------------------------------------------------------
def write_twin_bai(crai, bai):
    """A .bai with the references of `crai` whose tile sizes are the restatement's; returns them (per reference)."""
    sizes = CR.index_sizes(crai)
    refs = []
    at = 1 << 16
    for s in sizes:
        if len(s) == 0:
            refs.append((np.zeros(0, np.uint64), None))
            continue
        iv = at + np.concatenate([[0], np.cumsum(np.array(s, np.int64))])
        assert (np.diff(iv) >= 0).all()
        refs.append((iv.astype(np.uint64), None))
        at = int(iv[-1])
    IR.write_bai(bai, refs)
    return sizes


def viral_variants(d, seed=11):
    """viral.crai and three files derived from it: slice lengths changed, slices dropped, and in one of them a reference
    left without slices.  Returns the .crai paths; d/twin/<same base>.bai are their twins."""
    text = gzip.open(VIRAL, "rb").read()
    lines = text.split(b"\n")[:-1]
    rng = np.random.default_rng(seed)
    d = str(d)
    os.makedirs(os.path.join(d, "twin"), exist_ok=True)
    paths = [os.path.join(d, "viral.crai")]
    write_crai(paths[0], text)
    for v in range(1, 4):
        keep = []
        for ln in lines:
            t = ln.split(b"\t")
            if t[0] != b"-1":
                if rng.random() < 0.05 or (v == 2 and t[0] == b"20"):
                    continue
                t[5] = b"%d" % max(1, int(int(t[5]) * rng.uniform(0.4, 2.5) * (0.5 + 0.5 * v)))
            keep.append(b"\t".join(t))
        p = os.path.join(d, "v%d.crai" % v)
        write_crai(p, b"\n".join(keep) + b"\n", members=v)
        paths.append(p)
    for p in paths:
        write_twin_bai(p, os.path.join(d, "twin", os.path.basename(p)[:-5] + ".bai"))
    return paths
