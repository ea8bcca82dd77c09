"""CPU: the .csi model (tests/csi_ref.py) against the indexes htslib wrote -- at (14, 5) a .csi holds the bins and chunks of
the .bai of the same file, and its loffsets are a function of that .bai's linear index --, the general reg2bin and the depth
selection, the host's assembler (gdh_csi_assemble) against the model on crafted runs, and the host's .csi reader
(host/csi_reader.hpp through gdh_csi_read, and under sanitizers as a stand-alone program) on whole and damaged files.
No device."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import bai_ref
from tests import csi_ref
from tests import helpers as H

REF = os.path.join(H.GOLDEN, "ref")
UNSET = bai_ref.UNSET
GD_MAX_CONTIG_LENGTH = 0x7fff0000
FIXTURES = ["t", "hla", "t-empty"]


@pytest.fixture(scope="module")
def payloads():
    """The fixtures' payloads at C1's own depth (their references are short: below 5)."""
    return {name: csi_ref.payload(os.path.join(REF, name + ".bam")) for name in FIXTURES}


# ---- 1: pinned to the htslib fixtures -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_at_14_5_the_model_holds_what_htslibs_bai_holds(payloads, name):
    bam = os.path.join(REF, name + ".bam")
    raw = csi_ref.build(bam)
    got, eof, largest = csi_ref.inflate(raw)
    assert got == payloads[name] and eof and largest <= 65280
    lens, recs, _ = bai_ref.read(bam)
    own = csi_ref.parse(got)
    assert (own["min_shift"], own["depth"]) == (14, csi_ref.choose_depth(lens)) and own["depth"] < 5
    # the geometry of a .bai: C1 gives these short references less, so the depth is given
    parts = csi_ref.scan(len(lens), recs, 14, 5)
    got = csi_ref.payload(bam, depth=5)
    assert got == csi_ref.assemble(len(lens), *parts, 14, 5)
    assert assemble(len(lens), parts[0], parts[1], parts[2], parts[3], 14, 5, windows=max(max(l, default=0) for l in parts[1]) + 2) == got
    x = csi_ref.parse(got)
    n_ref, refs, n_no_coor = csi_ref.from_bai(open(bam + ".bai", "rb").read())
    assert (x["min_shift"], x["depth"], x["aux"]) == (14, 5, b"")
    assert len(x["refs"]) == n_ref and x["n_no_coor"] == n_no_coor
    n_real = 0
    for bins, (want_bins, meta, lin) in zip(x["refs"], refs):
        real = {b: v for b, v in bins.items() if b != bai_ref.PSEUDO_BIN}
        assert {b: ch for b, (_, ch) in real.items()} == want_bins
        if meta is None:
            assert bai_ref.PSEUDO_BIN not in bins
        else:
            lo, ch = bins[bai_ref.PSEUDO_BIN]
            assert lo == 0 and [ch[0][0], ch[0][1], ch[1][0], ch[1][1]] == meta
            assert list(bins)[-1] == bai_ref.PSEUDO_BIN                              # C7: the pseudo-bin last
        assert list(real) == sorted(real)                                            # C7: ascending
        for b, (lo, _) in real.items():
            w = csi_ref.first_window(b, 5)
            assert lo == (lin[w] if w < len(lin) else 0), (b, w)
            n_real += 1
    assert n_real > 0 or name == "t-empty"


# ---- 2: the general reg2bin -------------------------------------------------------------------------------------------------------

def test_reg2bin_at_14_5_is_the_bais():
    edges = sorted({(1 << k) + d for k in range(13, 30) for d in (-1, 0, 1)})
    n = 0
    for beg in edges:
        for end in edges:
            if beg < end <= 1 << 29:
                assert csi_ref.reg2bin(beg, end, 14, 5) == bai_ref.reg2bin(beg, end), (beg, end)
                n += 1
    assert n > 1000
    assert csi_ref.pseudo_bin(5) == bai_ref.PSEUDO_BIN and [csi_ref.level_first(l) for l in range(6)] == list(bai_ref.LEVEL_FIRST)


@pytest.mark.parametrize("min_shift, depth", [(14, 6), (8, 8)])
def test_reg2bin_gives_the_smallest_bin_that_contains_the_interval(min_shift, depth):
    top = csi_ref.max_end(min_shift, depth)
    edges = sorted({(1 << k) + d for k in range(min_shift - 1, min_shift + 3 * depth + 1) for d in (-1, 0, 1)} | {0, 1})
    edges = [e for e in edges if 0 <= e <= top]
    levels = set()
    for beg in edges:
        for end in edges + [top]:
            if not beg < end:
                continue
            b = csi_ref.reg2bin(beg, end, min_shift, depth)
            assert 0 <= b < csi_ref.pseudo_bin(depth) - 1
            lo, hi = csi_ref.bin_span(b, min_shift, depth)
            assert lo <= beg and end <= hi, (beg, end, b)
            level = csi_ref.bin_level(b, depth)
            levels.add(level)
            if level < depth:                                # no child holds it: the child that holds beg ends before `end`
                s = min_shift + 3 * (depth - level - 1)
                assert beg >> s != (end - 1) >> s, (beg, end, b)
    assert levels == set(range(depth + 1))
    assert csi_ref.reg2bin(top - 1, top, min_shift, depth) == csi_ref.pseudo_bin(depth) - 2       # the last real bin
    assert csi_ref.reg2bin(0, top, min_shift, depth) == 0


# ---- 3: C1 ----------------------------------------------------------------------------------------------------------------------

def test_depth_selection():
    assert csi_ref.choose_depth([1000, (1 << 29) - 256]) == 5
    assert csi_ref.choose_depth([(1 << 29) - 255, 5]) == 6
    assert csi_ref.choose_depth([GD_MAX_CONTIG_LENGTH], 14) == 6
    assert csi_ref.choose_depth([GD_MAX_CONTIG_LENGTH], 8) == 8
    assert csi_ref.choose_depth([0, 0, 0]) == 0 and csi_ref.choose_depth([]) == 0
    assert csi_ref.choose_depth([(1 << 14) - 256]) == 0 and csi_ref.choose_depth([(1 << 14) - 255]) == 1
    for min_shift in range(8, 25):                           # every bin of every accepted geometry lies below bit 30
        d = csi_ref.choose_depth([GD_MAX_CONTIG_LENGTH], min_shift)
        assert d <= 8 and csi_ref.pseudo_bin(d) < 1 << 30


# ---- 4: gdh_csi_assemble ---------------------------------------------------------------------------------------------------------

def assemble(n_ref, runs, lin, meta, n_no_coor, min_shift, depth, windows=40):
    """gdh_csi_assemble on the model's inputs: `windows` windows per reference, untouched ones all ones."""
    from goleft_amd import _hostlib, _lib
    lib = _hostlib.load()
    r = (_lib.GdIndexRun * max(1, len(runs)))()
    for k, (ref, b, vb, ve) in enumerate(runs):
        r[k] = _lib.GdIndexRun(ref, b, vb, ve)
    lin_off = np.arange(n_ref + 1, dtype=np.uint64) * np.uint64(windows)
    flat = np.full(n_ref * windows + 1, UNSET, np.uint64)
    for t in range(n_ref):
        for w, v in lin[t].items():
            flat[t * windows + w] = v
    refs = (_lib.GdIndexRef * max(1, n_ref))()
    for t in range(n_ref):
        if meta[t] is not None:
            refs[t] = _lib.GdIndexRef(*meta[t])
    args = (n_ref, C.addressof(r), len(runs), lin_off.ctypes.data, flat.ctypes.data, C.addressof(refs), n_no_coor, min_shift, depth)
    need = lib.gdh_csi_assemble(*args, None, 0)
    if need < 0:
        return None
    out = np.zeros(need, np.uint8)
    assert lib.gdh_csi_assemble(*args, out.ctypes.data, need) == need
    return out.tobytes()


def V(coff, uoff=0):
    return (coff << 16) | uoff


def _meta(runs, n_ref):
    meta = [None] * n_ref
    for ref, _b, vb, ve in runs:
        if meta[ref] is None:
            meta[ref] = [vb, ve, 3, 1]
        meta[ref][1] = ve
    return meta


F = csi_ref.level_first
# (depth, runs, linear of reference 0, the real bins of reference 0 afterwards: {bin: (loffset, chunk count)})
CASES = {
    # a deepest-level bin moves into its parent, which is there; the parent keeps its own loffset (window 0's entry)
    "moves-5": (5, [(0, F(4), V(10), V(20)), (0, F(5) + 3, V(1000), V(1000 + 65535, 7))], {0: V(10), 3: V(1000)},
                {F(4): (V(10), 2)}),
    # ... and one whose parent is absent stays, with the entry of ITS first window (9): filled backwards from window 11
    "orphan-5": (5, [(0, F(5) + 9, V(10), V(20)), (0, F(5), V(1000), V(1001))], {0: V(1000), 11: V(10)},
                 {F(5): (V(1000), 1), F(5) + 9: (V(10), 1)}),
    # two children meet in one parent and merge into one chunk there (they touch inside one member)
    "meet": (5, [(0, F(4), V(5), V(6)), (0, F(5) + 1, V(6), V(7, 9)), (0, F(5) + 2, V(7, 9), V(8))], {0: V(5), 1: V(6), 2: V(7, 9)},
             {F(4): (V(5), 1)}),
    # a bin whose first window lies beyond the last touched window: loffset 0 (bin F(4) + 1 begins at window 8)
    "beyond": (5, [(0, F(5) + 2, V(5), V(6)), (0, F(4) + 1, V(6), V(70000))], {2: V(5), 5: V(6)},
               {F(5) + 2: (V(5), 1), F(4) + 1: (0, 1)}),
    # depth 6: bins above 65535, one moving into a level-5 parent that is itself above the .bai's range
    "deep": (6, [(0, F(5) + 4096, V(10), V(20)), (0, F(6) + 8 * 4096 + 1, V(22), V(30)), (0, F(6) + 40000, V(30), V(40))],
             {1: V(20)}, {F(5) + 4096: (0, 2), F(6) + 40000: (0, 1)}),
    # depth 6, too wide to move: it stays, with its own first window (8)
    "deep-wide": (6, [(0, F(5) + 1, V(10), V(20)), (0, F(6) + 8, V(20), V(20 + 65536))], {8: V(20), 9: V(10)},
                  {F(5) + 1: (V(20), 1), F(6) + 8: (V(20), 1)}),
    # depth 0: everything is bin 0
    "flat": (0, [(0, 0, V(10), V(20))], {0: V(10)}, {0: (V(10), 1)}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_assemble_matches_the_model(name):
    depth, runs, lin0, expect = CASES[name]
    runs = runs + [(2, 0, V(90000), V(90001))]                       # and a reference without records between two with some
    n_ref = 3
    meta = _meta(runs, n_ref)
    lin = [dict(lin0), {}, {0: V(90000)}]
    want = csi_ref.assemble(n_ref, runs, lin, meta, 7, 14, depth)
    assert assemble(n_ref, runs, lin, meta, 7, 14, depth) == want
    x = csi_ref.parse(want)
    ps = csi_ref.pseudo_bin(depth)
    assert {b: (lo, len(ch)) for b, (lo, ch) in x["refs"][0].items() if b != ps} == expect
    assert x["refs"][1] == {} and x["refs"][0][ps][0] == 0 and x["n_no_coor"] == 7 and (x["min_shift"], x["depth"]) == (14, depth)
    if name == "deep":
        assert max(expect) > 65535


def test_assemble_shares_the_bais_arithmetic():
    """At (14, 5), on every case of tests/test_bai_ref.py: the bins and chunks of gdh_bai_assemble's output."""
    from tests import test_bai_ref as TB
    for name, runs in TB.CASES.items():
        meta = _meta(runs, 3)
        lin = [dict() for _ in range(3)]
        for ref, _b, vb, _ve in runs:
            lin[ref].setdefault(0, vb)
        got = assemble(3, runs, lin, meta, 7, 14, 5, windows=12)
        assert got == csi_ref.assemble(3, runs, lin, meta, 7, 14, 5), name
        _n, refs, _ = csi_ref.from_bai(TB.assemble(3, runs, lin, meta, 7))
        for bins, (want_bins, want_meta, _lin) in zip(csi_ref.parse(got)["refs"], refs):
            assert {b: ch for b, (_, ch) in bins.items() if b != bai_ref.PSEUDO_BIN} == want_bins, name


def test_assemble_refuses_what_is_no_input():
    runs = [(0, 0, V(1), V(2))]
    assert assemble(1, runs, [{}], _meta(runs, 1), 0, 7, 5) is None and assemble(1, runs, [{}], _meta(runs, 1), 0, 25, 5) is None
    assert assemble(1, runs, [{}], _meta(runs, 1), 0, 14, 9) is None
    bad = [(0, csi_ref.pseudo_bin(6), V(1), V(2))]                   # no bin of the scheme
    assert assemble(1, bad, [{}], _meta(bad, 1), 0, 14, 6) is None
    bad = [(1, 0, V(1), V(2)), (0, 0, V(2), V(3))]                   # references out of order
    assert assemble(2, bad, [{}, {}], _meta(bad, 2), 0, 14, 6) is None


# ---- 5: the host's reader ---------------------------------------------------------------------------------------------------------

def read_csi(data):
    """gdh_csi_read -> ((min_shift, depth, n_no_coor or None), per reference what csi_ref.reader_view gives), or the refusal."""
    from goleft_amd import _hostlib
    lib = _hostlib.load()
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    info = (C.c_int64 * 9)()
    err = C.create_string_buffer(256)
    n = C.c_size_t()
    if lib.gdh_csi_read(buf, len(data), -1, info, None, 0, C.byref(n), err, len(err)) != 0:
        return "refused: " + err.value.decode()
    head = (info[0], info[1], info[4] if info[3] else None)
    refs = []
    for r in range(info[2]):
        assert lib.gdh_csi_read(buf, len(data), r, info, None, 0, C.byref(n), err, len(err)) == 0
        a = np.zeros(max(1, n.value), np.uint64)
        assert lib.gdh_csi_read(buf, len(data), r, info, a.ctypes.data, n.value, C.byref(n), err, len(err)) == 0
        refs.append(([int(v) for v in a[:n.value]], bool(info[5]), info[6], info[7], info[8]))
    return head, refs


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("min_shift", [14, 9])
def test_reader_delivers_the_models_derivation(name, min_shift):
    bam = os.path.join(REF, name + ".bam")
    lens, recs, _ = bai_ref.read(bam)
    depth = csi_ref.choose_depth(lens, min_shift)
    parts = csi_ref.scan(len(lens), recs, min_shift, depth)
    plain = csi_ref.assemble(len(lens), *parts, min_shift, depth)
    want = csi_ref.reader_view(plain)
    n_no_coor = parts[3]
    variants = {"file": csi_ref.bgzf(plain), "payload": plain, "small-members": csi_ref.bgzf(plain, 700),
                "shuffled": csi_ref.bgzf(csi_ref.assemble(len(lens), *parts, min_shift, depth, order=csi_ref.shuffled(5))),
                "aux": csi_ref.bgzf(csi_ref.assemble(len(lens), *parts, min_shift, depth, aux=b"\xff" * 12))}
    for what, data in variants.items():
        assert read_csi(data) == ((min_shift, depth, n_no_coor), want), what
    short = csi_ref.assemble(len(lens), parts[0], parts[1], parts[2], None, min_shift, depth)
    assert read_csi(csi_ref.bgzf(short)) == ((min_shift, depth, None), want)
    # the anchors are record starts of their reference, the first of them its first record
    starts = [set() for _ in lens]
    for ref, _pos, _flag, _rlen, vb, _ve in recs:
        if ref >= 0:
            starts[ref].add(vb)
    for t, (anchors, has, end, nm, nu) in enumerate(want):
        assert set(anchors) <= starts[t] and has == bool(starts[t])
        if has:
            assert anchors[0] == min(starts[t]) and parts[2][t][2:] == [nm, nu] and end == parts[2][t][1]
        else:
            assert anchors == [] and nm == -1
    if name == "t" and min_shift == 9:
        assert max(len(a) for a, *_ in want) > 20


def _damaged(p):
    """(what, bytes) of hla's payload cut at every field boundary and one byte into every field, and with bad counts."""
    x = csi_ref.parse(p)
    tail = x["fields"][-1]                                     # n_no_coor: a file may end in front of it
    out = []
    for f in x["fields"]:
        if f != tail:
            out.append(("cut at %d" % f, p[:f]))
        out.append(("cut at %d + 1" % f, p[:f + 1]))
    n_bin_at = x["fields"][5]
    n_chunk_at = n_bin_at + 4 + 12
    for what, at in (("n_ref", 16), ("n_bin", n_bin_at), ("n_chunk", n_chunk_at), ("l_aux", 12)):
        for v in (-1, -(1 << 31), 1 << 30, {"n_ref": (len(p) - at) // 4, "l_aux": len(p) - at - 3}.get(what, (len(p) - at - 4) // 16 + 1)):
            out.append(("%s = %d" % (what, v), p[:at] + struct.pack("<i", v) + p[at + 4:]))
    out.append(("depth 13", p[:8] + struct.pack("<i", 13) + p[12:]))
    out.append(("min_shift -1", p[:4] + struct.pack("<i", -1) + p[8:]))
    out.append(("another magic", b"CSI\x02" + p[4:]))
    return out


def test_reader_refuses_damaged_payloads(payloads):
    p = payloads["hla"]
    assert not isinstance(read_csi(p), str)
    assert not isinstance(read_csi(p[:-8]), str)                # without n_no_coor
    cases = _damaged(p)
    assert len(cases) > 40
    for what, data in cases:
        assert isinstance(read_csi(data), str), what
        assert isinstance(read_csi(csi_ref.bgzf(data)), str) or not data, what
    raw = csi_ref.bgzf(p, 3000)
    for n in (0, 1, 10, 17, 18, len(raw) // 2, len(raw) - 29, len(raw) - 1):
        assert isinstance(read_csi(raw[:n]), str), n
    broken = bytearray(raw)
    broken[40] ^= 0x55
    assert isinstance(read_csi(bytes(broken)), str)


def test_reader_under_sanitizers(payloads, tmp_path):
    """tests/emul/csi_asan_main.cpp: the reader built with -fsanitize=address,undefined and run on its own over the same
    whole and damaged inputs; its answers are the library's."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "csi_asan")
    r = subprocess.run([gxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-I",
                        os.path.join(H.ROOT, "goleft_amd", "csrc", "host"), "-o", exe,
                        os.path.join(H.ROOT, "tests", "emul", "csi_asan_main.cpp"), "-lz"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("this toolchain has no sanitizer run time: " + r.stderr[-300:])
    p = payloads["hla"]
    inputs = [p, csi_ref.bgzf(p), csi_ref.bgzf(p, 500), p[:-8], csi_ref.bgzf(payloads["t"]), payloads["t-empty"]]
    inputs += [d for _, d in _damaged(p)]
    inputs += [csi_ref.bgzf(d) for _, d in _damaged(p)[::7]]
    raw = csi_ref.bgzf(p, 3000)
    inputs += [raw[:n] for n in range(0, len(raw), 97)]
    rng = np.random.default_rng(3)
    for _ in range(40):
        z = bytearray(raw if rng.integers(0, 2) else p)
        for _ in range(int(rng.integers(1, 6))):
            z[int(rng.integers(0, len(z)))] = int(rng.integers(0, 256))
        inputs.append(bytes(z))
    # one file: [u32 size, bytes] per input
    blob = tmp_path / "inputs.bin"
    blob.write_bytes(b"".join(struct.pack("<I", len(d)) + d for d in inputs))
    r = subprocess.run([exe, str(blob)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert got[-1] == "ok" and len(got) == len(inputs) + 1
    for line, data in zip(got, inputs):
        want = read_csi(data)
        if isinstance(want, str):
            assert line == "refused", data[:40]
        else:
            (ms, d, nnc), refs = want
            assert line == "%d %d %d %d %d" % (ms, d, len(refs), sum(len(a) for a, *_ in refs), sum(sum(a) % 1000003 for a, *_ in refs) % 1000003)
