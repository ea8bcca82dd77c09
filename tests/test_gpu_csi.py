"""-m gpu: `goleft-depth index -c` -- a BAM's .csi made on the device -- and the device BAM read
through a .csi alone.

The yardstick is tests/csi_ref.py, which the htslib-written .bai fixtures pin at (14, 5) (tests/test_csi_ref.py); files are
compared by their inflated payload and the presence of the EOF member, never by their compressed bytes.  Guess quality and the
cut into ranges must not change a byte of the payload.  `depth`, `covstats` and `multidepth` read on the device with only a
.csi next to the BAM and write what they write with htslib's .bai; a contig beyond 2^29 -- which no .bai can hold -- is
indexed, and read on the device."""
import os
import shutil
import struct
import subprocess

import pytest

from tests import bai_ref
from tests import covstats_ref as CR
from tests import csi_ref
from tests import helpers as H
from tests import index_cases as IC

pytestmark = pytest.mark.gpu
EXE = os.path.join(H.ROOT, "goleft_amd", "goleft-depth")
REF = os.path.join(H.GOLDEN, "ref")
KNOBS = ("GOLEFT_INDEX_SLICE", "GOLEFT_INDEX_GUESS_CHECKS", "GOLEFT_INDEX_REPAIR_ROUNDS", "GOLEFT_INDEX_RANGE_BYTES", "GOLEFT_GPU_INDEX",
         "GOLEFT_INDEX_TIMING", "GOLEFT_INGEST_TIMING", "GOLEFT_GPU_DECODE", "GOLEFT_COVSTATS_TIMING")
INVALID = -1


def build(path, monkeypatch, min_shift=14, **knobs):
    """(payload, stats) from the library, with the test knobs set for this call only; the file ends with the EOF member."""
    from goleft_amd import index
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv("GOLEFT_INDEX_" + k.upper(), str(v))
    raw, st = index.build_stats(str(path), csi=True, min_shift=min_shift)
    payload, eof, largest = csi_ref.inflate(raw)
    assert eof and largest <= 65280
    return payload, st


def cli(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, env=e, timeout=120)


def payload_of(path):
    payload, eof, largest = csi_ref.inflate(open(path, "rb").read())
    assert eof and largest <= 65280
    return payload


# ---- 7: the fixtures --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["t", "hla", "t-empty"])
def test_cli_and_library_write_the_models_csi_for_the_fixtures(tmp_path, monkeypatch, name):
    bam = tmp_path / (name + ".bam")
    shutil.copy(os.path.join(REF, name + ".bam"), bam)
    want = csi_ref.payload(str(bam))
    r = cli(["index", "-c", bam])
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == [name + ".bam", name + ".bam.csi"]      # the default name; no temporary file
    assert payload_of(tmp_path / (name + ".bam.csi")) == want
    got, st = build(bam, monkeypatch)
    assert got == want and (st["min_shift"], st["depth"]) == (14, csi_ref.choose_depth(bai_ref.read(str(bam))[0]))
    from goleft_amd import index
    out = index.write(str(bam), str(tmp_path / "twin.csi"), csi=True)
    assert open(out, "rb").read() == (tmp_path / (name + ".bam.csi")).read_bytes()                # the library twin: the same bytes
    r = cli(["index", "--csi", "-o", tmp_path / "named.csi", bam])
    assert r.returncode == 0 and payload_of(tmp_path / "named.csi") == want


# ---- 8: every content rule, and positions beyond 2^29 ----------------------------------------------------------------------------------

def deep_records(pad=0):
    R = CR.Rec
    recs = IC.edge_records(pad)
    big = [r for r in recs if r.ref == 0]
    rest = [r for r in recs if r.ref != 0]
    big += [R(0, (1 << 29) - (1 << 14), 0, cigar=[(0, 10), (3, (1 << 15) - 20), (0, 10)]),      # an N across 2^29 - 2^14 .. 2^29 + 2^14
            R(0, (1 << 29) - 50, 0, cigar=[(0, 100)]),                                            # crosses 2^29: bin 0 at depth 6
            R(0, 1 << 29, 0, cigar=[(0, 30)]),
            R(0, (1 << 30) - 100, 0, cigar=[(0, 100)])]                                           # ends exactly at the reference's end
    big.sort(key=lambda r: r.pos)
    return big + rest


@pytest.fixture(scope="module")
def deep_bam(tmp_path_factory):
    """IC.write_edges' layout (the long record ends 44 bytes into a 64-byte slice: a repair round is certain) with the records
    beyond 2^29 added."""
    path = str(tmp_path_factory.mktemp("csi") / "deep.bam")
    IC.write(path, deep_records(), block=1000)                                   # fifteen members or so: a dozen ranges can be cut
    first, starts, total = IC.layout(path)
    size = [b - a for a, b in zip(starts, starts[1:] + [total])]
    k = max(range(len(size)), key=lambda i: size[i])
    IC.write(path, deep_records((44 - (starts[k + 1] - first)) % 64), block=1000)
    first, starts, total = IC.layout(path)
    assert (starts[k + 1] - first) % 64 == 44
    return path


@pytest.fixture(scope="module")
def deep_want(deep_bam):
    return csi_ref.payload(deep_bam)


def test_every_content_rule_at_depth_6(deep_bam, deep_want, monkeypatch):
    got, st = build(deep_bam, monkeypatch)
    assert st["records"] == len(deep_records()) and st["depth"] == 6 and st["ranges"] == 1
    assert got == deep_want
    x = csi_ref.parse(got)
    lens, recs, _ = bai_ref.read(deep_bam)
    runs, _lin, _meta, _n = csi_ref.scan(len(lens), recs, 14, 6)
    assert {csi_ref.bin_level(b, 6) for r, b, _, _ in runs if r == 0} == {0, 1, 2, 3, 4, 5, 6}
    # (at depth 6 a level-1 bin spans 2^29: the read across 2^29 lies in bin 0, the one that begins there in a level-6 bin above 65535)
    assert csi_ref.reg2bin((1 << 29) - 50, (1 << 29) + 50, 14, 6) == 0 and csi_ref.reg2bin(1 << 29, (1 << 29) + 30, 14, 6) > 65535
    assert any(b > 65535 for _, b, _, _ in runs)
    assert x["refs"][1] == {} and x["refs"][3] == {} and x["n_no_coor"] == 25


def test_guess_quality_and_ranges_do_not_change_a_byte(deep_bam, deep_want, monkeypatch):
    got, st = build(deep_bam, monkeypatch, slice=64, guess_checks=0)
    assert got == deep_want and st["rounds"] > 0
    size = os.path.getsize(deep_bam)
    got, st = build(deep_bam, monkeypatch, range_bytes=size * 3 // 5)           # (a range begins with the last member of the one before)
    assert got == deep_want and st["ranges"] in (2, 3)
    got, st = build(deep_bam, monkeypatch, range_bytes=size // 12)
    assert got == deep_want and st["ranges"] >= 8


# ---- 9: other geometries ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_shift", [8, 12, 17])
def test_min_shift_on_hla(tmp_path, monkeypatch, min_shift):
    bam = os.path.join(REF, "hla.bam")
    depth = csi_ref.choose_depth(bai_ref.read(bam)[0], min_shift)
    assert depth == {8: 3, 12: 1, 17: 0}[min_shift]
    r = cli(["index", "-m", min_shift, "-o", tmp_path / "x.csi", bam])
    assert r.returncode == 0, r.stderr
    got = payload_of(tmp_path / "x.csi")
    assert got == csi_ref.payload(bam, min_shift)
    assert struct.unpack_from("<ii", got, 4) == (min_shift, depth)
    assert build(bam, monkeypatch, min_shift=min_shift)[0] == got


def test_min_shift_24_on_the_deep_file(deep_bam, monkeypatch):
    got, st = build(deep_bam, monkeypatch, min_shift=24)
    assert st["depth"] == 3 and got == csi_ref.payload(deep_bam, 24)


@pytest.mark.parametrize("flag, value", [("-m", 7), ("-m", 25), ("--min-shift", "x"), ("--min-shift=0", None)])
def test_min_shift_outside_8_to_24_is_refused(tmp_path, flag, value):
    bam = tmp_path / "hla.bam"
    shutil.copy(os.path.join(REF, "hla.bam"), bam)
    r = cli(["index", flag] + ([value] if value is not None else []) + [bam])
    assert r.returncode == 255 and "min_shift" in r.stderr
    assert [p.name for p in tmp_path.iterdir()] == ["hla.bam"]


def test_min_shift_outside_8_to_24_is_refused_by_the_library(monkeypatch):
    from goleft_amd import index
    for m in (7, 25):
        with pytest.raises(index.Refused) as e:
            index.build(os.path.join(REF, "hla.bam"), csi=True, min_shift=m)
        assert e.value.status == INVALID


def test_a_read_far_over_its_references_end_grows_the_windows_at_min_shift_8(tmp_path, monkeypatch):
    # reference "tail" is 70 000 long: 274 windows of 256 and four to spare; a read that ends 200 000 behind it touches 1055
    recs = [CR.Rec(2, 50 * i, 0, cigar=[(0, 40)]) for i in range(300)]
    recs += [CR.Rec(4, 100 * i, 0, cigar=[(0, 80)]) for i in range(400)]
    recs += [CR.Rec(4, 69000, 0, cigar=[(0, 100), (3, 100000), (0, 100)]), CR.Rec(4, 69500, 0, cigar=[(0, 200000)])]
    recs += [CR.Rec(-1, -1, 4, cigar=[]) for _ in range(5)]
    refs = [(n, min(l, 1 << 20)) for n, l in IC.REFS]                            # (a gigabase at 256 per window is 4 M windows)
    path = IC.write(tmp_path / "over.bam", recs, refs=refs, block=1500)
    want = csi_ref.payload(path, 8)
    lens, rr, _ = bai_ref.read(path)
    assert max(csi_ref.scan(5, rr, 8, csi_ref.choose_depth(lens, 8))[1][4]) == (69500 + 200000 - 1) >> 8
    for knobs in ({}, {"range_bytes": 2000}, {"range_bytes": 1200, "slice": 100}):
        got, st = build(path, monkeypatch, min_shift=8, **knobs)
        assert got == want, knobs
    assert st["ranges"] > 3


# ---- 10: the span limit is the geometry's ----------------------------------------------------------------------------------------------

def test_an_end_beyond_the_geometrys_limit_is_refused(tmp_path, monkeypatch):
    """A longest reference of 2^20 - 256 gives depth 2 at min_shift 14 (C1 adds 256 to the length: 2^20 itself would give 3):
    positions up to 2^20.  A record that ends at 2^20 + 1 is refused, one that ends at 2^20 is indexed."""
    from goleft_amd import index
    refs = [("a", (1 << 20) - 256), ("b", 50000)]
    assert csi_ref.choose_depth([l for _, l in refs]) == 2 and csi_ref.max_end(14, 2) == 1 << 20
    plain = [CR.Rec(0, 100 * i, 0, cigar=[(0, 50)]) for i in range(300)]
    (tmp_path / "bad").mkdir()
    bad = IC.write(tmp_path / "bad" / "x.bam", plain + [CR.Rec(0, (1 << 20) - 10, 0, cigar=[(0, 11)])], refs=refs, block=2000)
    with pytest.raises(index.Refused) as e:
        build(bad, monkeypatch)
    assert e.value.status == INVALID
    msg = str(e.value)
    assert "record 300" in msg and "position %d" % ((1 << 20) - 10) in msg and "min_shift 14" in msg and "depth 2" in msg and ".bai" not in msg
    r = cli(["index", "-c", bad])
    assert r.returncode == 1 and "record 300" in r.stderr
    assert [p.name for p in (tmp_path / "bad").iterdir()] == ["x.bam"]
    with pytest.raises(bai_ref.Refused):
        csi_ref.payload(bad)
    good = IC.write(tmp_path / "good.bam", plain + [CR.Rec(0, (1 << 20) - 10, 0, cigar=[(0, 10)])], refs=refs, block=2000)
    got, st = build(good, monkeypatch)
    assert got == csi_ref.payload(good) and st["depth"] == 2 and st["records"] == 301
    # without -c nothing changes: the same file is a .bai's, and 2^29 is a .bai's limit with its own words
    assert index.build(bad) == bai_ref.build(bad)


# ---- 11: `goleft depth` through a .csi alone -----------------------------------------------------------------------------------------

def _fai(bam):
    lens_names = []
    from oracle import bamio
    raw = bamio.bgzf_decompress(open(bam, "rb").read())
    l_text, = struct.unpack_from("<i", raw, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, p)
        lens_names.append((raw[p + 4:p + 4 + l_name - 1].decode(), struct.unpack_from("<i", raw, p + 4 + l_name)[0]))
        p += 8 + l_name
    return lens_names


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """bai/: t.bam and hla.bam with htslib's .bai; csi/: with the .csi `index -c` writes; csi12/: with one at -m 12; both/:
    with the two of them."""
    d = tmp_path_factory.mktemp("csidepth")
    for sub in ("bai", "csi", "csi12", "both"):
        (d / sub).mkdir()
        for name in ("t", "hla"):
            bam = d / sub / (name + ".bam")
            shutil.copy(os.path.join(REF, name + ".bam"), bam)
            (d / sub / (name + ".fa.fai")).write_text("".join("%s\t%d\t6\t60\t61\n" % r for r in _fai(str(bam))))
            if sub in ("bai", "both"):
                shutil.copy(os.path.join(REF, name + ".bam.bai"), str(bam) + ".bai")
            if sub in ("csi", "both"):
                assert cli(["index", "-c", bam]).returncode == 0
            if sub == "csi12":
                assert cli(["index", "-m", 12, bam]).returncode == 0
            assert os.path.exists(str(bam) + ".bai") == (sub in ("bai", "both")) and os.path.exists(str(bam) + ".csi") == (sub != "bai")
    return d


def _depth(d, sub, name, **env):
    prefix = d / sub / (name + "_out" + "".join(sorted(env)))
    r = cli(["depth", "-w", 1000, "-r", d / sub / (name + ".fa"), "--prefix", prefix, d / sub / (name + ".bam")], GOLEFT_INGEST_TIMING=1, **env)
    assert r.returncode == 0, r.stderr
    return open(str(prefix) + ".depth.bed", "rb").read(), open(str(prefix) + ".callable.bed", "rb").read(), r.stderr


@pytest.fixture(scope="module")
def depth_want(dirs):
    out = {}
    for name in ("t", "hla"):
        d_, c_, err = _depth(dirs, "bai", name)
        assert "ingest_call_s" in err
        out[name] = (d_, c_)
    return out


@pytest.mark.parametrize("sub", ["csi", "csi12", "both"])
@pytest.mark.parametrize("name", ["t", "hla"])
def test_depth_reads_on_the_device_through_a_csi(dirs, depth_want, name, sub):
    got_d, got_c, err = _depth(dirs, sub, name)
    assert "ingest_call_s" in err                                                 # the device read ran
    assert (got_d, got_c) == depth_want[name]


# ---- 12: a contig no .bai can hold ------------------------------------------------------------------------------------------------------

LONG = (1 << 29) + (1 << 20)
LONG_REFS = [("long", LONG), ("b", 50000)]


def long_records():
    R = CR.Rec
    recs = [R(0, 1000 + 37 * i, 0, cigar=[(0, 100)]) for i in range(12)]
    recs += [R(0, (1 << 29) - 400 + 53 * i, 0, cigar=[(0, 100)]) for i in range(14)]          # round 2^29, some crossing it
    recs += [R(0, (1 << 29) - 30, 0, cigar=[(0, 20), (2, 30), (0, 50)]), R(0, (1 << 29) + 5000, 16, cigar=[(0, 80)])]
    recs += [R(0, LONG - 2000 + 150 * i, 0, cigar=[(0, 100)]) for i in range(12)]             # near the end of `long`
    recs += [R(0, LONG - 100, 0, cigar=[(0, 100)])]                                           # ... and exactly at it
    recs.sort(key=lambda r: r.pos)
    recs += [R(1, 200 + 90 * i, 0, cigar=[(0, 100)]) for i in range(20)]
    recs += [R(-1, -1, 4, cigar=[]) for _ in range(6)]
    return recs


@pytest.fixture(scope="module")
def long_dirs(tmp_path_factory):
    d = tmp_path_factory.mktemp("long")
    bed = "".join("long\t%d\t%d\n" % (a, a + 16384) for a in (0, (1 << 29) - 16384, 1 << 29, LONG - 16384)) + "b\t0\t16384\n"
    for sub in ("csi", "none"):
        (d / sub).mkdir()
        IC.write(d / sub / "x.bam", long_records(), refs=LONG_REFS, block=3000)
        (d / sub / "x.fa.fai").write_text("".join("%s\t%d\t6\t60\t61\n" % r for r in LONG_REFS))
        (d / sub / "w.bed").write_text(bed)
    return d


def _long_depth(d, sub, tag, **env):
    prefix = d / sub / ("out_" + tag)
    r = cli(["depth", "-w", 16384, "--bed", d / sub / "w.bed", "-r", d / sub / "x.fa", "--prefix", prefix, d / sub / "x.bam"],
            GOLEFT_INGEST_TIMING=1, **env)
    return r, prefix


def test_a_contig_beyond_2_to_29_is_indexed_and_read_on_the_device(long_dirs, monkeypatch):
    d = long_dirs
    bam = d / "csi" / "x.bam"
    # no .bai can hold it ...
    r = cli(["index", bam])
    assert r.returncode == 1 and ".bai" in r.stderr and not os.path.exists(str(bam) + ".bai")
    # ... a .csi does, at depth 6
    r = cli(["index", "-c", bam])
    assert r.returncode == 0, r.stderr
    got = payload_of(str(bam) + ".csi")
    assert got == csi_ref.payload(str(bam)) and struct.unpack_from("<ii", got, 4) == (14, 6)
    # the host decoder is the yardstick
    r, prefix = _long_depth(d, "csi", "host", GOLEFT_GPU_DECODE=0)
    assert r.returncode == 0 and "ingest_call_s" not in r.stderr, r.stderr
    want = (open(str(prefix) + ".depth.bed", "rb").read(), open(str(prefix) + ".callable.bed", "rb").read())
    assert want[0].count(b"\n") >= 5 and b"long\t536870912\t" in want[0]
    # with the .csi: the device read
    r, prefix = _long_depth(d, "csi", "dev")
    assert r.returncode == 0 and "ingest_call_s" in r.stderr, r.stderr
    assert (open(str(prefix) + ".depth.bed", "rb").read(), open(str(prefix) + ".callable.bed", "rb").read()) == want
    # without any index, asked to make one: the device read, the same output, no file
    r, prefix = _long_depth(d, "none", "made", GOLEFT_GPU_INDEX=1)
    assert r.returncode == 0 and "ingest_call_s" in r.stderr, r.stderr
    assert (open(str(prefix) + ".depth.bed", "rb").read(), open(str(prefix) + ".callable.bed", "rb").read()) == want
    assert not [p.name for p in (d / "none").iterdir() if p.name.endswith((".csi", ".bai"))]


# ---- 13: covstats and multidepth with only a .csi ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["t", "hla"])
def test_covstats_with_only_a_csi(dirs, name):
    want = cli(["covstats", dirs / "bai" / (name + ".bam")], GOLEFT_COVSTATS_SKIP=0)
    assert want.returncode == 0, want.stderr
    for sub in ("csi", "csi12"):
        got = cli(["covstats", dirs / sub / (name + ".bam")], GOLEFT_COVSTATS_SKIP=0, GOLEFT_COVSTATS_TIMING=1)
        assert got.returncode == 0, got.stderr
        assert got.stdout.replace("/%s/" % sub, "/bai/") == want.stdout
        assert "lib_wait_inflate_s" in got.stderr and "lib_walk_scan_hist_s" in got.stderr      # the device read's timing line


def test_multidepth_with_only_a_csi(dirs):
    def run(sub, **env):
        return cli(["multidepth", "--chrom", "chr22", "--mincov", 1, "--minsize", 1, dirs / sub / "t.bam", dirs / sub / "hla.bam"],
                   GOLEFT_INGEST_TIMING=1, **env)
    want = run("bai")
    assert want.returncode == 0 and "ingest_call_s" in want.stderr, want.stderr
    assert want.stdout.startswith("#chrom")
    for sub in ("csi", "csi12"):
        got = run(sub)
        assert got.returncode == 0 and got.stdout == want.stdout, got.stderr
        assert got.stderr.count("ingest_call_s") == want.stderr.count("ingest_call_s") >= 1    # as many device reads as with the .bai


# ---- 14: the commands that want a linear index's tiles ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cmd", ["indexcov", "indexsplit"])
def test_indexcov_and_indexsplit_say_what_a_csi_lacks(dirs, tmp_path, cmd):
    fai = dirs / "csi" / "t.fa.fai"
    for given in (dirs / "csi" / "t.bam.csi", dirs / "csi" / "t.bam"):
        args = ["indexcov", "-d", tmp_path / "out", "-f", fai, given] if cmd == "indexcov" else ["indexsplit", "-n", 10, "--fai", fai, given]
        r = cli(args)
        assert r.returncode != 0
        assert "a .csi holds no 16 kb tiles" in r.stderr and "no usable index" not in r.stderr, r.stderr
