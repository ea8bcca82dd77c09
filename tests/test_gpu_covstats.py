"""GPU: `goleft-depth covstats` byte for byte against the restatement of covstats.go (tests/covstats_ref.py): the
reference fixtures, multi-BAM invocations, synth-bam files cut into many ranges, crafted BAMs for every quirk, the error
paths and the sample names.  Every CLI call runs under its own timeout; nothing is retried."""
import os
import shutil
import subprocess

import pytest

from tests import covstats_ref as R
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
SYNTH = os.path.join(ROOT, "goleft_amd", "synth-bam")
GOLD = os.path.join(ROOT, "tests", "golden", "ref")
FIXTURES = ["t.bam", "hla.bam", "t-empty.bam", "sample_issue_27_0001.bam"]
M, I, S, N_ = 0, 1, 4, 3


def cli(args, skip=None, range_kb=None, timeout=300):
    env = dict(os.environ)
    env.pop("GOLEFT_COVSTATS_SKIP", None)
    env.pop("GOLEFT_COVSTATS_RANGE_KB", None)
    if skip is not None:
        env["GOLEFT_COVSTATS_SKIP"] = str(skip)
    if range_kb is not None:
        env["GOLEFT_COVSTATS_RANGE_KB"] = str(range_kb)
    r = subprocess.run([EXE, "covstats"] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=env)
    return r.returncode, r.stdout, r.stderr


def check(bams, n=1000000, skip=None, range_kb=None, regions=None):
    args = (["-n", n] if n != 1000000 else []) + (["-r", regions] if regions else []) + list(bams)
    rc, out, err = cli(args, skip=skip, range_kb=range_kb)
    try:
        want = R.covstats_rows([str(b) for b in bams], n=n, skip=R.SKIP if skip is None else skip, regions=regions)
    except R.MadFilterPanic as e:                           # 1 or 2 inserts: an error naming the BAM
        assert rc != 0 and str(e) in err, err
        return None
    assert rc == 0, err
    assert out == want, err
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixtures_at_the_default_skip(name):
    check([os.path.join(GOLD, name)])


@pytest.mark.parametrize("n", [1, 3, 100, 5000, 39000, 1000000])
def test_reference_fixtures_without_skip(n):
    # t.bam: both references and the 64 unplaced records at its end are crossed once n is large
    for name in FIXTURES:
        check([os.path.join(GOLD, name)], n=n, skip=0)


def test_multi_bam_invocation_in_argument_order(tmp_path):
    bams = [os.path.join(GOLD, f) for f in ("hla.bam", "t.bam", "t-empty.bam", "t.bam")]
    out = check(bams, n=2000, skip=5)
    assert out.startswith(R.HEADER) and len(out.splitlines()) == 5


def test_regions(tmp_path):
    bed = tmp_path / "r.bed"
    bed.write_text("chr1\t0\t1000\nchr1\t5000\t7000")      # the last line has no newline: not counted
    check([os.path.join(GOLD, "t.bam")], n=500, skip=0, regions=str(bed))


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    if not os.path.exists(SYNTH):
        pytest.fail("synth-bam was not built")
    d = tmp_path_factory.mktemp("synth")
    p = d / "s.bam"
    env = dict(os.environ, SYNTH_BAM_AUX="1", SYNTH_BAM_LEVEL="6")
    subprocess.run([SYNTH, str(p), "chrS", "1500000,700000,300000", "30", "11", "16"], check=True, env=env, timeout=300,
                   capture_output=True)
    R.add_pseudo_bins(str(p))
    return str(p)


@pytest.mark.parametrize("n", [1000000, 60000, 1])
def test_synth_bam_every_range_size_gives_the_same_row(synth, n):
    rows = {kb: check([synth], n=n, range_kb=kb) for kb in (64, 257, 4096, None)}
    assert len(set(rows.values())) == 1


def test_synth_bam_without_skip_many_ranges(synth):
    check([synth], n=250000, skip=0, range_kb=96)


# ---- crafted BAMs -----------------------------------------------------------------------------------------------------
def pe(pos, ins, rl=100, flag=0x3, tlen=None, ref=0):
    return R.Rec(ref, pos, flag, pos + rl + ins, (ins + 2 * rl) if tlen is None else tlen, ((M, rl),))


def crafted(tmp_path, name, recs, refs=(("c1", 1 << 20), ("c2", 1 << 19)), **kw):
    p = str(tmp_path / name)
    R.write_bam(p, list(refs), recs, **kw)
    return p


def test_single_end_break(tmp_path):
    recs = [R.Rec(0, 10 * i, 0x0, -1, 0, ((M, 100 + i % 3),)) for i in range(3000)]
    p = crafted(tmp_path, "se.bam", recs, block=4096)
    for n in (1, 10, 1000, 2000):
        check([p], n=n, skip=0, range_kb=64)


def test_interleaved_unmapped_dups_qcfail_secondary(tmp_path):
    recs = []
    for i in range(6000):
        f = [0x3, 0x4 | 0x1, 0x403, 0x203, 0x103, 0x803, 0x1, 0x13][i % 8]
        recs.append(pe(20 * i, 150 + (i * 7) % 90, flag=f))
    recs += [R.Rec(-1, -1, 0x4, -1, 0, ()) for _ in range(50)]
    p = crafted(tmp_path, "mix.bam", recs, block=2000)
    for n in (1, 4, 700, 2999, 3000, 100000):
        check([p], n=n, skip=0, range_kb=64)
    check([p], n=1000, skip=777, range_kb=64)


def test_long_cigar_placeholder_and_no_cigar(tmp_path):
    recs = []
    for i in range(2000):
        if i % 5 == 0:                                      # CG:B,I: the stored <l_seq>S<ref_len>N placeholder counts
            real = [(M, 50), (I, 2), (M, 48)] * 30
            tag = b"CGBI" + len(real).to_bytes(4, "little") + b"".join(((ln << 4) | op).to_bytes(4, "little") for op, ln in real)
            recs.append(R.Rec(0, 30 * i, 0x3, 30 * i + 500, 700, ((S, 3000), (N_, 2940)), tags=tag, l_seq=3000))
        elif i % 5 == 1:
            recs.append(R.Rec(0, 30 * i, 0x3, 30 * i + 500, 700, ()))
        else:
            recs.append(pe(30 * i, 100 + i % 50))
    p = crafted(tmp_path, "cg.bam", recs, block=8192)
    for n in (3, 500, 1200):
        check([p], n=n, skip=0, range_kb=64)


def test_overlapping_mates_and_outliers_beyond_the_window(tmp_path):
    recs = []
    for i in range(5000):
        ins = [-80, -5, 0, 300, 310, 320, 70000, 1 << 29][i % 8]
        tl = [-(1 << 30), 400, 400, 500, 520, 99999, -70000, 1 << 30][(i * 3) % 8]
        recs.append(pe(100 * i, ins, tlen=tl, ref=0 if i < 3000 else 1))
    p = crafted(tmp_path, "ol.bam", recs, block=3000)
    for n in (3, 100, 4000, 5000):
        check([p], n=n, skip=0, range_kb=64)


def test_exactly_n_eligible_records_ending_the_file_and_ranges(tmp_path):
    recs = [pe(50 * i, 200 + i % 17) for i in range(4000)]
    p = crafted(tmp_path, "exact.bam", recs, block=1000)
    rows = {kb: check([p], n=4000, skip=0, range_kb=kb) for kb in (64, 65, 70, 80, None)}
    assert len(set(rows.values())) == 1
    check([p], n=4001, skip=0, range_kb=64)


# ---- error paths ------------------------------------------------------------------------------------------------------
def test_missing_index_is_an_error_naming_the_bam_and_earlier_rows_stay(tmp_path):
    good = crafted(tmp_path, "good.bam", [pe(100 * i, 300) for i in range(10)])
    bad = crafted(tmp_path, "noidx.bam", [pe(100 * i, 300) for i in range(10)], index=False)
    rc, out, err = cli([good, bad], skip=0)
    assert rc != 0 and "noidx.bam" in err
    assert out == R.covstats_rows([good], skip=0)


def test_x_bai_beside_x_bam_is_found(tmp_path):
    p = crafted(tmp_path, "alt.bam", [pe(100 * i, 300 + i) for i in range(10)])
    os.rename(p + ".bai", str(tmp_path / "alt.bai"))
    check([p], skip=0)


def test_path_without_bam_suffix_has_no_index(tmp_path):
    p = crafted(tmp_path, "plain.bam", [pe(100 * i, 300 + i) for i in range(10)])
    q = str(tmp_path / "plain.data")
    shutil.copy(p, q)
    check([q], skip=0)


def test_cram_is_refused(tmp_path):
    good = crafted(tmp_path, "g.bam", [pe(100 * i, 300) for i in range(10)])
    rc, out, err = cli([good, str(tmp_path / "x.cram")], skip=0)
    assert rc == 1 and "CRAM" in err and out == R.covstats_rows([good], skip=0)


@pytest.mark.parametrize("k", [1, 2])
def test_one_or_two_inserts_are_an_error(tmp_path, k):
    p = crafted(tmp_path, "few.bam", [pe(100 * i, 300) for i in range(k)] + [R.Rec(0, 5000, 0x1, -1, 0)])
    rc, out, err = cli([p], skip=0)
    assert rc != 0 and "few.bam" in err and out == R.HEADER


# ---- sample names -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rgs,want", [
    (["@RG\tID:a\tSM:one"], {"one"}),
    ([], set()),
    (["@RG\tID:a"], set()),
    (["@RG\tID:a\tSM:x", "@RG\tID:b\tSM:y", "@RG\tID:c\tSM:x", "@RG\tID:d"], {"x", "y"}),
])
def test_sample_names(tmp_path, rgs, want):
    refs = [("c1", 100000)]
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:100000\n" + "".join(r + "\n" for r in rgs)
    p = crafted(tmp_path, "sm.bam", [pe(100 * i, 300 + i) for i in range(20)], refs=refs, header_text=text)
    rc, out, err = cli([p], skip=0)
    assert rc == 0, err
    names = out.splitlines()[1].split("\t")[-1]
    assert (set(names.split(",")) if want else {"<no-read-groups>"}) == (want or {"<no-read-groups>"})
    assert out.splitlines()[1].split("\t")[:-1] == R.covstats_rows([p], skip=0).splitlines()[1].split("\t")[:-1]


def test_python_entry(tmp_path):
    from goleft_amd import covstats
    out = tmp_path / "rows.txt"
    assert covstats.Main(["-n", "300", os.path.join(GOLD, "hla.bam")], out_path=str(out)) == 0
    assert out.read_text() == R.covstats_rows([os.path.join(GOLD, "hla.bam")], n=300)
