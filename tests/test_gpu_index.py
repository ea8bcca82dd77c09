"""-m gpu: `goleft-depth index` -- a BAM's .bai made on the device -- through the host library's
entry (goleft_amd.index, which drives gd_index_begin / _decode / _result) and through the command line.

The yardsticks: the three indexes htslib wrote (tests/golden/ref/*.bam.bai), byte for byte; and for synthetic files
tests/bai_ref.py, which those three pin.  Guess quality (slice size, chain checks) and the cut into ranges must not
change a byte.  `goleft depth` on a BAM without an index takes the device path under GOLEFT_GPU_INDEX=1 and only then."""
import json
import os
import shutil
import struct
import subprocess

import pytest

from tests import bai_ref
from tests import covstats_ref as CR
from tests import helpers as H
from tests import index_cases as IC

pytestmark = pytest.mark.gpu
EXE = os.path.join(H.ROOT, "goleft_amd", "goleft-depth")
REF = os.path.join(H.GOLDEN, "ref")
KNOBS = ("GOLEFT_INDEX_SLICE", "GOLEFT_INDEX_GUESS_CHECKS", "GOLEFT_INDEX_REPAIR_ROUNDS", "GOLEFT_INDEX_RANGE_BYTES", "GOLEFT_GPU_INDEX", "GOLEFT_INDEX_TIMING",
         "GOLEFT_INGEST_TIMING")


def build(path, monkeypatch, **knobs):
    """(bytes, stats) from the library, with the test knobs set for this call only."""
    from goleft_amd import index
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv("GOLEFT_INDEX_" + k.upper(), str(v))
    return index.build_stats(str(path))


def cli(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, env=e, timeout=120)


@pytest.fixture(scope="module")
def edge_bam(tmp_path_factory):
    """Every content rule in one file; members of 4000 inflated bytes, so records end in, start in and span members."""
    return IC.write_edges(tmp_path_factory.mktemp("index") / "edges.bam")


@pytest.fixture(scope="module")
def edge_want(edge_bam):
    return bai_ref.build(edge_bam)


# ---- the fixtures htslib indexed ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["t", "hla", "t-empty"])
def test_cli_writes_the_fixture_indexes_byte_for_byte(tmp_path, name):
    out = tmp_path / (name + ".bai")
    r = cli(["index", "-o", out, os.path.join(REF, name + ".bam")])
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == open(os.path.join(REF, name + ".bam.bai"), "rb").read()
    assert [p.name for p in tmp_path.iterdir()] == [name + ".bai"]               # (the temporary file is gone)


def test_cli_default_output_is_next_to_the_bam(tmp_path):
    shutil.copy(os.path.join(REF, "hla.bam"), tmp_path / "hla.bam")
    r = cli(["index", tmp_path / "hla.bam"], GOLEFT_INDEX_TIMING=1)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "hla.bam.bai").read_bytes() == open(os.path.join(REF, "hla.bam.bai"), "rb").read()
    t = json.loads(r.stderr.strip().splitlines()[-1])
    assert t["records"] == 482 and t["repair_rounds"] == 0 and t["ranges"] == 1
    for key in ("read_s", "wait_inflate_s", "guess_s", "walks_s", "runs_linear_s", "device_read_back_s", "assemble_s"):
        assert key in t


def test_library_twin_and_defaults_need_no_repair_on_hla(monkeypatch):
    got, st = build(os.path.join(REF, "hla.bam"), monkeypatch)
    assert got == open(os.path.join(REF, "hla.bam.bai"), "rb").read()
    assert st == {"records": 482, "rounds": 0, "ranges": 1}


# ---- synthetic files against the model -----------------------------------------------------------------------------------------

def test_every_content_rule_in_one_file(edge_bam, edge_want, monkeypatch):
    got, st = build(edge_bam, monkeypatch)
    assert st["records"] == len(IC.edge_records()) and st["ranges"] == 1
    assert got == edge_want
    # the file holds what it is meant to hold: five windows of one read, empty references, the unplaced tail
    lens, recs, _ = bai_ref.read(edge_bam)
    runs, lin, meta, n_no_coor = bai_ref.scan(len(lens), recs)
    assert meta[1] is None and meta[3] is None and meta[0] and meta[2] and meta[4] and n_no_coor == 25
    assert all(lin[0][w] == lin[0][3] for w in range(3, 8)) and meta[0][3] == 2
    assert {bai_ref.bin_level(b) for r, b, _, _ in runs if r == 0} == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("slice_, checks", [(64, 0), (64, 3), (1024, 0), (1024, 3), (70000, 3)])
def test_guess_quality_does_not_change_a_byte(edge_bam, edge_want, monkeypatch, slice_, checks):
    got, st = build(edge_bam, monkeypatch, slice=slice_, guess_checks=checks)
    assert got == edge_want
    if checks == 0:
        assert st["rounds"] > 0                               # a fake record head in front of a true start was fallen for (IC.write_edges)


def test_a_slice_without_a_record_start_and_a_start_on_a_slice_boundary(edge_bam, edge_want, monkeypatch):
    first, starts, total = IC.layout(edge_bam)
    size = [b - a for a, b in zip(starts, starts[1:] + [total])]
    k = max(range(len(size)), key=lambda i: size[i])
    assert size[k] > 2 * 1024                                 # with slices of 1 kb, one lies inside this record whatever the phase
    got, _ = build(edge_bam, monkeypatch, slice=1024)
    assert got == edge_want
    # slices of exactly the distance to a record start: slice 1 begins on it (and slice 2 on whatever follows)
    for j in (5, k + 1, len(starts) - 3):
        assert starts[j] - first >= 64
        got, _ = build(edge_bam, monkeypatch, slice=starts[j] - first)
        assert got == edge_want


def test_records_that_end_with_a_member_and_span_three(tmp_path, monkeypatch):
    recs = IC.edge_records()

    def special(first, starts, total):
        k = next(i for i in range(len(starts) - 1) if starts[i + 1] - starts[i] > 3000)     # the long record
        s = starts[k]
        # a member ends with record 3's last byte; the long record lies in three members; an EMPTY member inside the stream
        # is not pinned by any htslib index and is left out
        return [starts[4], s + 1000, s + 2000, starts[k + 1], starts[-1]]
    path = IC.write(tmp_path / "cuts.bam", recs, cuts=IC.member_cuts(special))
    want = bai_ref.build(path)
    for knobs in ({}, {"slice": 64, "guess_checks": 0}, {"range_bytes": 700}):
        got, st = build(path, monkeypatch, **knobs)
        assert got == want, knobs
    assert st["ranges"] > 2


def test_two_ranges_with_a_run_a_window_and_a_record_across_the_cut(tmp_path, monkeypatch):
    # one reference, one bin, every record in window 0 .. 2: whatever the cut, a run and a window straddle it; members of
    # 700 bytes and records of about 90, so that records straddle member -- and range -- boundaries
    recs = [CR.Rec(0, 20 * i, 0, cigar=[(0, 60)]) for i in range(2000)] + [CR.Rec(-1, -1, 4, cigar=[]) for _ in range(30)]
    path = IC.write(tmp_path / "two.bam", recs, refs=[("one", 100000)], block=700)
    want = bai_ref.build(path)
    one, st1 = build(path, monkeypatch)
    assert one == want and st1["ranges"] == 1
    two, st2 = build(path, monkeypatch, range_bytes=os.path.getsize(path) // 2 + 1500)
    assert st2["ranges"] == 2 and two == want
    many, st3 = build(path, monkeypatch, range_bytes=3000, slice=200, guess_checks=0)
    assert st3["ranges"] > 5 and many == want
    # the cut fell inside a record: the first range's last member holds the start of a record it does not hold whole
    first, starts, total = IC.layout(path)
    assert any(s % 700 > 620 for s in starts)


def test_clean_wrong_guesses_that_leap_a_true_start(tmp_path, monkeypatch):
    """Fake record heads whose block_size lands exactly on a true record start several slices on: a walk from such a guess is
    CLEAN (one record that is none, then true ones) and stops far behind the next guesses.  Two such guesses in a row, the
    second leaping a segment that begins on a true start, is where a loop that believed unconfirmed walks lost records or never
    ended.  The bytes must be the model's below the merge into one segment (it never comes), at it, and when it comes at once."""
    path, d, first, starts = IC.write_leaps(tmp_path / "leaps.bam")
    want = bai_ref.build(path)
    ref_len = [n for _, n in IC.REFS]
    true = set(starts)
    for slice_ in (64, 128):
        g = IC.slice_guesses(d, first, slice_, ref_len)
        leap = lambda o: IC.candidate(d, o, ref_len)
        assert any(g[i] not in true and g[i + 1] not in true and g[i + 2] in true and leap(g[i + 1]) in true and leap(g[i + 1]) >= g[i + 3]
                   for i in range(len(g) - 3)), slice_
        seen = {}
        for repair_rounds in (1000, 4, 1, 0):
            for checks in (0, 3):                             # (a leap leaves the slice, so the chain check passes it either way)
                got, st = build(path, monkeypatch, slice=slice_, guess_checks=checks, repair_rounds=repair_rounds)
                assert got == want, (slice_, repair_rounds, checks)
                assert st["rounds"] > 0 and st["records"] == len(starts)
                seen[repair_rounds] = st["rounds"]
        assert seen[0] == 1                                   # everything unconfirmed walked as one segment, at once
        assert seen[1000] >= 1                                # ... and repaired round by round when the merge never comes
    got, st = build(path, monkeypatch)
    assert got == want


def test_a_read_that_hangs_far_over_its_references_end(tmp_path, monkeypatch):
    # reference "tail" is 70 000 long: five windows and four to spare.  A read that ends a megabase behind it touches 66, in a
    # later range than the reads that set the first windows: the linear array grows and keeps what it held
    recs = [CR.Rec(2, 50 * i, 0, cigar=[(0, 40)]) for i in range(300)]
    recs += [CR.Rec(4, 100 * i, 0, cigar=[(0, 80)]) for i in range(400)]
    recs += [CR.Rec(4, 69000, 0, cigar=[(0, 100), (3, 1000000), (0, 100)]), CR.Rec(4, 69500, 0, cigar=[(0, 2000000)])]
    recs += [CR.Rec(-1, -1, 4, cigar=[]) for _ in range(5)]
    path = IC.write(tmp_path / "over.bam", recs, block=1500)
    want = bai_ref.build(path)
    assert max(bai_ref.scan(5, bai_ref.read(path)[1])[1][4]) == (69500 + 2000000 - 1) >> 14
    for knobs in ({}, {"range_bytes": 2000}, {"range_bytes": 1200, "slice": 100}):
        got, st = build(path, monkeypatch, **knobs)
        assert got == want, knobs
    assert st["ranges"] > 3


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def _refused(tmp_path, monkeypatch, name, recs, refs, status, exit_code, damage=None):
    from goleft_amd import index
    path = IC.write(tmp_path / (name + ".bam"), recs, refs=refs, block=2000)
    if damage:
        damage(path)
    with pytest.raises(index.Refused) as e:
        build(path, monkeypatch)
    assert e.value.status == status, str(e.value)
    r = cli(["index", path])
    assert r.returncode == exit_code and r.stderr.strip(), (r.returncode, r.stderr)
    assert sorted(p.name for p in tmp_path.iterdir()) == [name + ".bam"]          # no index, no temporary file
    return str(e.value)


UNSORTED, INVALID = -7, -1
TWO = [("a", 1 << 30), ("b", 50000)]
PLAIN = [CR.Rec(0, 100 * i, 0, cigar=[(0, 50)]) for i in range(300)]


def test_refused_positions_go_backwards(tmp_path, monkeypatch):
    recs = PLAIN[:200] + [CR.Rec(0, 5, 0, cigar=[(0, 50)])] + PLAIN[200:]
    msg = _refused(tmp_path, monkeypatch, "back", recs, TWO, UNSORTED, 2)
    assert "record 200" in msg and "backwards" in msg


def test_refused_a_reference_resumes(tmp_path, monkeypatch):
    recs = PLAIN[:100] + [CR.Rec(1, 10, 0, cigar=[(0, 50)])] + PLAIN[100:]
    msg = _refused(tmp_path, monkeypatch, "resume", recs, TWO, UNSORTED, 2)
    assert "record 101" in msg and "resumes" in msg


def test_refused_placed_after_unplaced(tmp_path, monkeypatch):
    recs = PLAIN + [CR.Rec(-1, -1, 4, cigar=[]), CR.Rec(1, 10, 0, cigar=[(0, 50)])]
    msg = _refused(tmp_path, monkeypatch, "placed", recs, TWO, UNSORTED, 2)
    assert "record 301" in msg and "unplaced" in msg


def test_refused_an_end_beyond_what_a_bai_holds(tmp_path, monkeypatch):
    recs = PLAIN + [CR.Rec(0, (1 << 29) - 10, 0, cigar=[(0, 11)])]
    msg = _refused(tmp_path, monkeypatch, "span", recs, TWO, INVALID, 1)
    assert "record 300" in msg and "position %d" % ((1 << 29) - 10) in msg


def test_refused_a_negative_position_on_a_reference(tmp_path, monkeypatch):
    recs = [CR.Rec(0, -1, 4, cigar=[])] + PLAIN
    msg = _refused(tmp_path, monkeypatch, "neg", recs, TWO, INVALID, 1)
    assert "record 0" in msg


def test_refused_a_damaged_record(tmp_path, monkeypatch):
    bad = CR.raw_rec(ref=0, pos=20000, cigar=[(0, 50)], name=b"x\0", n_cigar=60000)       # its CIGAR would leave the record
    _refused(tmp_path, monkeypatch, "record", PLAIN[:150] + [bad] + PLAIN[150:], TWO, INVALID, 1)


def test_refused_a_record_cut_by_the_end_of_the_file(tmp_path, monkeypatch):
    bad = CR.raw_rec(ref=0, pos=40000, cigar=[(0, 50)], name=b"x\0", block_size=5000)     # the file ends inside it
    _refused(tmp_path, monkeypatch, "cut", PLAIN + [bad], TWO, INVALID, 1)


def test_refused_a_damaged_member(tmp_path, monkeypatch):
    def damage(path):
        raw = bytearray(open(path, "rb").read())
        size = struct.unpack_from("<H", raw, 16)[0] + 1                                    # the first member
        raw[size + 18 + 40] ^= 0x10                                                        # a bit of the second one's deflate stream
        open(path, "wb").write(bytes(raw))
    _refused(tmp_path, monkeypatch, "member", PLAIN, TWO, INVALID, 1, damage)


# ---- `goleft depth` on a BAM without an index -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def depth_dirs(tmp_path_factory):
    """with/: t.bam and hla.bam with htslib's indexes; without/: the BAMs alone; ours/: with the indexes `index` writes."""
    from oracle import bamio
    d = tmp_path_factory.mktemp("depth")
    fai = {}
    for name in ("t", "hla"):
        raw = bamio.bgzf_decompress(open(os.path.join(REF, name + ".bam"), "rb").read())
        l_text, = struct.unpack_from("<i", raw, 4)
        p = 8 + l_text
        n_ref, = struct.unpack_from("<i", raw, p)
        p += 4
        rows = []
        for _ in range(n_ref):
            l_name, = struct.unpack_from("<i", raw, p)
            rows.append("%s\t%d\t6\t60\t61\n" % (raw[p + 4:p + 4 + l_name - 1].decode(), struct.unpack_from("<i", raw, p + 4 + l_name)[0]))
            p += 8 + l_name
        fai[name] = "".join(rows)
    for sub in ("with", "without", "ours"):
        (d / sub).mkdir()
        for name in ("t", "hla"):
            shutil.copy(os.path.join(REF, name + ".bam"), d / sub / (name + ".bam"))
            (d / sub / (name + ".fa.fai")).write_text(fai[name])
            if sub == "with":
                shutil.copy(os.path.join(REF, name + ".bam.bai"), d / sub / (name + ".bam.bai"))
            if sub == "ours":
                assert cli(["index", d / sub / (name + ".bam")]).returncode == 0
    return d


def _depth(d, sub, name, **env):
    prefix = d / sub / (name + "_out" + "".join(sorted(env)))
    r = cli(["depth", "-w", 1000, "-r", d / sub / (name + ".fa"), "--prefix", prefix, d / sub / (name + ".bam")],
            GOLEFT_INGEST_TIMING=1, **env)
    assert r.returncode == 0, r.stderr
    return open(str(prefix) + ".depth.bed", "rb").read(), open(str(prefix) + ".callable.bed", "rb").read(), r.stderr


@pytest.mark.parametrize("name", ["t", "hla"])
def test_depth_reads_an_unindexed_bam_on_the_device_when_asked(depth_dirs, name):
    want_d, want_c, err = _depth(depth_dirs, "with", name)
    assert "ingest_call_s" in err                                                # the device read ran
    got_d, got_c, err = _depth(depth_dirs, "without", name, GOLEFT_GPU_INDEX=1)
    assert "ingest_call_s" in err and (got_d, got_c) == (want_d, want_c)
    assert not os.path.exists(depth_dirs / "without" / (name + ".bam.bai"))      # the index is not written
    host_d, host_c, err = _depth(depth_dirs, "without", name)
    assert "ingest_call_s" not in err and (host_d, host_c) == (want_d, want_c)   # as before: the host decoder


@pytest.mark.parametrize("name", ["t", "hla"])
def test_an_index_written_here_serves_the_device_read(depth_dirs, name):
    want_d, want_c, _ = _depth(depth_dirs, "with", name)
    got_d, got_c, err = _depth(depth_dirs, "ours", name)
    assert "ingest_call_s" in err and (got_d, got_c) == (want_d, want_c)
    assert (depth_dirs / "ours" / (name + ".bam.bai")).read_bytes() == open(os.path.join(REF, name + ".bam.bai"), "rb").read()
