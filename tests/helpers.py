"""Shared helpers for the tests (test infrastructure; may use oracle/)."""
import functools
import json
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HIPCC = next((p for p in ("/opt/rocm/bin/hipcc", shutil.which("hipcc") or "") if p and os.path.exists(p)), None)


@functools.lru_cache(maxsize=None)
def api_asm():
    """goleft_amd/csrc/gd_api.hip as hipcc compiles it for gfx950, as assembly text.  The resource tests all read this one
    compile: it runs once a process."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "api.s")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                               "-I", os.path.join(ROOT, "include"), "-o", path,
                               os.path.join(ROOT, "goleft_amd", "csrc", "gd_api.hip")], stderr=subprocess.DEVNULL)
        with open(path) as f:
            return f.read()


def kernel_metadata(asm):
    """{mangled name: dict(lds, scratch, vgpr, sgpr, spill, sgpr_spill, wg)} from the amdhsa.kernels: list of an assembly
    text; the dicts are the caller's"""
    meta = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for k in re.split(r"\n  - \.", meta)[1:]:
        g = lambda key: re.search(r"\.%s:\s+(\S+)" % key, "." + k).group(1)
        out[g("name")] = dict(lds=int(g("group_segment_fixed_size")), scratch=int(g("private_segment_fixed_size")),
                              vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")), spill=int(g("vgpr_spill_count")),
                              sgpr_spill=int(g("sgpr_spill_count")), wg=int(g("max_flat_workgroup_size")))
    return out


def load_golden_bam(name):
    """-> (contigs[(name,len)], {tid: Reads}, npz)"""
    z = np.load(os.path.join(GOLDEN, name + "_bam.npz"))
    contigs = list(zip([str(x) for x in z["contig_names"]], [int(x) for x in z["contig_lens"]]))
    reads = {}
    for tid in range(len(contigs)):
        if "pos_%d" % tid in z:
            reads[tid] = po.Reads(z["pos_%d" % tid], z["flag_%d" % tid], z["mapq_%d" % tid],
                                  z["cigar_off_%d" % tid], z["cigar_%d" % tid])
    return contigs, reads, z


def golden_beds():
    return json.load(open(os.path.join(GOLDEN, "fixture_beds.json")))


def empty_reads():
    return po.Reads(np.zeros(0, np.int32), np.zeros(0, np.uint16), np.zeros(0, np.uint8),
                    np.zeros(1, np.uint32), np.zeros(0, np.uint32))


def random_reads(rng, length, n, max_ops=6, max_len=300, long_reads=False):
    """Random record stream with every CIGAR op, including zero-length ops,
    leading/trailing clips, N skips and reads hanging over the contig end."""
    pos = np.sort(rng.integers(0, max(1, length), size=n)).astype(np.int32)
    nops = rng.integers(0, max_ops + 1, size=n)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum(nops)
    m = int(off[-1])
    ops = rng.choice(9, size=m, p=[0.55, 0.08, 0.1, 0.04, 0.08, 0.02, 0.01, 0.06, 0.06])
    lens = rng.integers(0, max_len, size=m)
    if long_reads:
        lens = np.where(rng.random(m) < 0.02, lens * 50, lens)
    cigar = ((lens.astype(np.uint32) << 4) | ops.astype(np.uint32)).astype(np.uint32)
    flag = rng.choice([0, 16, 99, 147, 0x400, 0x100, 0x200, 0x4, 0x800, 0x410], size=n).astype(np.uint16)
    mapq = rng.choice([0, 1, 5, 60], size=n).astype(np.uint8)
    return po.Reads(pos, flag, mapq, off, cigar)


def long_cigar_reads(rng, length, n_ops_list, max_step=40, skip_every=0):
    """One read per entry of n_ops_list with exactly that many CIGAR ops: M runs
    interleaved with I / D (and S / = / X / P / zero-length ops), the shape of long-read
    alignments; every skip_every-th read also carries one long N skip.  Reads start
    at sorted random positions in the first half of the contig."""
    n = len(n_ops_list)
    pos = np.sort(rng.integers(0, max(1, length // 2), size=n)).astype(np.int32)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum(n_ops_list)
    m = int(off[-1])
    ops = rng.choice(9, size=m, p=[0.5, 0.2, 0.2, 0.0, 0.02, 0.0, 0.02, 0.03, 0.03])
    lens = rng.integers(0, max_step, size=m)
    if skip_every:
        for i in range(0, n, skip_every):
            if n_ops_list[i] > 2:
                k = int(off[i]) + int(rng.integers(1, n_ops_list[i] - 1))
                ops[k], lens[k] = 3, int(rng.integers(5000, 40000))
    cigar = ((lens.astype(np.uint32) << 4) | ops.astype(np.uint32)).astype(np.uint32)
    flag = rng.choice([0, 16, 0x800, 0x400], size=n, p=[0.5, 0.3, 0.1, 0.1]).astype(np.uint16)
    mapq = rng.choice([0, 20, 60], size=n, p=[0.05, 0.25, 0.7]).astype(np.uint8)
    return po.Reads(pos, flag, mapq, off, cigar)


# MAPQ bytes where a kernel's byte handling goes wrong: the sign bit of a byte (127 / 128 / 129) and SAM's
# "MAPQ unavailable" (255), which `samtools depth -Q` still compares as a number
EDGE_MAPQ = (0, 1, 127, 128, 129, 254, 255)
# flag_mask values no longer than the 16-bit flag field (0x8000: its sign bit)
EDGE_FLAG_MASKS = (0x704, 0, 0x8000, 0x800, 0xFFFF, 0xFFFFFFFF)
# op codes that consume no reference, none of them counted: I S H P and the unassigned codes 9-15
NON_CONSUMING_OPS = (1, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15)


def edge_reads(rng, length, n, max_ops=7, max_len=300, long_ops=0):
    """Records that reach the edges of the read filter and of the CIGAR encoding: MAPQ over 0-255 with weight on
    EDGE_MAPQ; flags over the whole 16-bit field (every single bit, 0xFFFF, the subsets of 0x704, uniform values);
    every op code 0-15, zero-length ops, and non-consuming ops (I S H P, 9-15) of up to 2^28 - 1 bases; reads of
    0, 1, 2 and up to max_ops ops, at sorted positions over the whole contig (some hang over its end).
    long_ops > 0 adds one more read of that many ops (every code, lengths 0-3) at a position in the first half.
    No two-op read is `0S <n>N`: with SEQ '*' that is SAM's placeholder of a CIGAR stored in the CG tag."""
    n_long = 1 if long_ops else 0
    pos = np.sort(rng.integers(0, max(1, length), size=n + n_long)).astype(np.int32)
    nops = rng.choice(np.arange(max_ops + 1), size=n + n_long,
                      p=[0.02, 0.38, 0.3] + [0.3 / (max_ops - 2)] * (max_ops - 2))
    if n_long:
        k = int(np.searchsorted(pos, length // 2))
        nops[int(rng.integers(0, max(1, k)))] = long_ops
    off = np.zeros(n + n_long + 1, np.uint32)
    off[1:] = np.cumsum(nops)
    m = int(off[-1])
    p = np.array([0.35, 0.05, 0.06, 0.03, 0.08, 0.04, 0.03, 0.06, 0.06] + [0.24 / 7] * 7)
    ops = rng.choice(16, size=m, p=p / p.sum())
    lens = rng.integers(0, max_len, size=m)
    lens[rng.random(m) < 0.05] = 0
    huge = np.isin(ops, NON_CONSUMING_OPS) & (rng.random(m) < 0.15)
    lens[huge] = rng.choice([(1 << 28) - 1, (1 << 28) - 2, 1 << 27, 1 << 22], size=int(huge.sum()))
    if n_long:
        i = int(np.flatnonzero(nops == long_ops)[0])
        a, b = int(off[i]), int(off[i + 1])
        ops[a:b] = np.arange(b - a) % 16
        rng.shuffle(ops[a:b])
        lens[a:b] = rng.integers(0, 4, size=b - a)
    two = np.flatnonzero(nops == 2)
    first = off[two].astype(np.int64)
    ph = first[(ops[first] == 4) & (lens[first] == 0) & (ops[first + 1] == 3)]
    lens[ph] = 1
    cigar = ((lens.astype(np.uint32) << 4) | ops.astype(np.uint32)).astype(np.uint32)

    N = n + n_long
    kind = rng.choice(5, size=N, p=[0.2, 0.4, 0.15, 0.1, 0.15])
    single = (1 << rng.integers(0, 16, size=N)).astype(np.int64)
    sub704 = np.array([sum(b for j, b in enumerate((0x4, 0x100, 0x200, 0x400)) if (s >> j) & 1)
                       for s in range(16)], np.int64)[rng.integers(0, 16, size=N)]
    anyf = rng.integers(0, 1 << 16, size=N)
    flag = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                     [0, single, sub704, np.where(rng.random(N) < 0.5, 0xFFFF, 0x8000)], anyf).astype(np.uint16)
    mapq = np.where(rng.random(N) < 0.5, rng.choice(EDGE_MAPQ, size=N), rng.integers(0, 256, size=N)).astype(np.uint8)
    return po.Reads(pos, flag, mapq, off, cigar)


def oracle_windows(depth, W, start=0):
    """(sums, mins) of W-anchored windows clipped to [start, start+len(depth))."""
    end = start + len(depth)
    sums, mins = [], []
    for k in range(start // W, (end - 1) // W + 1 if end > start else 0):
        s, e = max(start, k * W), min(end, (k + 1) * W)
        seg = depth[s - start:e - start]
        sums.append(int(seg.astype(np.int64).sum()))
        mins.append(int(seg.min()))
    return np.asarray(sums, np.int64), np.asarray(mins, np.int32)


def oracle_runs(depth, mincov, maxmean, step, start=0):
    """[(start,end,cls)] with breaks at class changes and at multiples of step."""
    cls = np.where(depth == 0, 0, np.where(depth < mincov, 1,
                   np.where((maxmean > 0) & (depth >= maxmean), 3, 2)))
    n = len(depth)
    if n == 0:
        return np.zeros((0, 3), np.int32)
    p = np.arange(start, start + n)
    brk = np.ones(n, bool)
    brk[1:] = (cls[1:] != cls[:-1]) | (p[1:] % step == 0)
    s = p[brk]
    e = np.append(s[1:], start + n)
    return np.stack([s, e, cls[brk]], 1).astype(np.int32)


def depthwed_tie_grid():
    """(sums, lens) int64: window sums whose mean sits exactly on (or one unit of the sum away from) a 4-digit
    rounding tie or a x.5 boundary of the depthwed cell, for every magnitude and a range of window lengths."""
    sums, lens = [], []
    for l in (1, 2, 4, 5, 8, 10, 20, 40, 125, 250, 1000, 2000, 16384):
        for e in range(-1, 7):
            for d in (1000, 1001, 1234, 1235, 4999, 5000, 5001, 9998, 9999):
                for half in (0, 1):
                    # mean ~ (d + half/2) * 10^(e-3)
                    num = (2 * d + half) * 10 ** max(e, 0) * l
                    den = 2 * 10 ** 3 * 10 ** max(-e, 0)
                    base = num // den
                    for delta in (-1, 0, 1):
                        if base + delta >= 0:
                            sums.append(base + delta)
                            lens.append(l)
    return np.array(sums, np.int64), np.array(lens, np.int64)


def window_sum_reads(rng, length, W, sums, n_filtered=0):
    """Records on one contig of `length` bases whose W-window sums (min_mapq 1, flag mask 0x704) are `sums`.
    Every record stays inside its window: sum // len reads of `<len>M` at the window's start plus one of
    `<sum % len>M`, len being the window's length (the last window is shorter).  n_filtered more records that
    the filters drop (unmapped, secondary, QC-failed, duplicate, MAPQ 0) land at random places inside windows."""
    sums = np.asarray(sums, np.int64)
    nw = (length + W - 1) // W
    assert sums.shape == (nw,) and (sums >= 0).all()
    start = np.arange(nw, dtype=np.int64) * W
    wlen = np.minimum(start + W, length) - start
    assert (sums <= wlen * 200000).all()            # keeps the record count (about the mean) bounded
    full, rem = sums // wlen, sums % wlen
    pos = [np.repeat(start, full), start[rem > 0]]
    span = [np.repeat(wlen, full), rem[rem > 0]]
    flag = [np.zeros(int(full.sum()) + int((rem > 0).sum()), np.uint16)]
    mapq = [np.full(flag[0].shape[0], 60, np.uint8)]
    if n_filtered:
        w = rng.integers(0, nw, size=n_filtered)
        off = rng.integers(0, wlen[w])
        pos.append(start[w] + off)
        span.append(rng.integers(1, wlen[w] - off + 1))
        kind = rng.integers(0, 5, size=n_filtered)
        flag.append(np.array([0x4, 0x100, 0x200, 0x400, 0], np.uint16)[kind])
        mapq.append(np.where(kind == 4, 0, 60).astype(np.uint8))
    pos, span = np.concatenate(pos), np.concatenate(span)
    flag, mapq = np.concatenate(flag), np.concatenate(mapq)
    order = np.argsort(pos, kind="stable")
    n = pos.shape[0]
    return po.Reads(pos[order].astype(np.int32), flag[order], mapq[order], np.arange(n + 1, dtype=np.uint32),
                    (span[order].astype(np.uint32) << 4))             # one M op per record


def ref_span(r):
    """Reference bases each record's CIGAR consumes (M, D, N, =, X), per read."""
    consumes = np.array([1, 0, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0], np.int64)
    c = r.cigar.astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(consumes[c & 15] * (c >> 4))])
    off = r.cigar_off.astype(np.int64)
    return cs[off[1:]] - cs[off[:-1]]


def device_arrays(r, misaligned=()):
    """The records as device tensors; the arrays named in `misaligned` are contiguous slices at element offset 1 of
    larger tensors (what a host that slices one device arena per contig hands over)."""
    import torch
    dev = torch.device("cuda", 0)
    out = []
    for name, a, dt in (("pos", r.pos, np.int32), ("flag", r.flag, np.int16), ("mapq", r.mapq, np.uint8),
                        ("off", r.cigar_off, np.int32), ("cigar", r.cigar, np.int32)):
        a = np.ascontiguousarray(a).view(dt)
        if name in misaligned:
            big = torch.zeros(a.shape[0] + 9, dtype=torch.from_numpy(a[:0]).dtype, device=dev)
            t = big[1:1 + a.shape[0]]
            t.copy_(torch.from_numpy(a))
            assert t.is_contiguous() and t.data_ptr() % {"pos": 16, "flag": 8, "mapq": 4, "off": 16, "cigar": 4}[name]
        else:
            t = torch.from_numpy(a).to(dev)
        out.append(t)
    return out
