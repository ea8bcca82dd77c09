"""CPU: the .crai reader (host/crai_reader.hpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone
program: the reference's fixture, written files with every kind of bad line (what it returns is held to the restatement),
and gzip bytes that are damaged or cut short (it must end cleanly).  tests/test_crai.py calls the same reader in the plain
build, where a stray read only shows if it crashes."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import crai_cases as CC
from tests import crai_ref as CR
from tests import helpers as H

GXX = shutil.which("g++")
HOST = os.path.join(H.ROOT, "goleft_amd", "csrc", "host")


@pytest.fixture(scope="module")
def asan_reader(tmp_path_factory):
    if GXX is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("asan") / "crai_asan")
    r = subprocess.run([GXX, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-I", HOST, "-o", exe,
                        os.path.join(H.ROOT, "tests", "emul", "crai_asan_main.cpp"), "-lz"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("this toolchain has no sanitizer run time: " + r.stderr[-300:])
    return exe


def summary(path):
    try:
        refs = CR.read_index(path)
    except CR.CraiError as e:
        return "refused %d" % e.line
    return "%d %d %d" % (len(refs), sum(len(r) for r in refs), sum(sum(s) for r in refs for s in r))


def test_reader_stays_inside_its_buffers(asan_reader, tmp_path):
    good = CC.line(0, 1, 20000, 100) + CC.line(-1, 0, 0, 55) + CC.line(2, 5, 70000, 9) + CC.line(0, 20001, 30000, 7)
    texts = [good, good * 300, b"", b"\n", b"\t\t\t\t\t\n", good + b"0\t1\t2\t3\t4\n", good + b"0\t1\t2\t3\t4\t5\t6\t7\n",
             good + b"0\t1\t2\t3\t4\t5", b" \t " + good, good + b"x\t1\t2\t3\t4\t5\n", good + b"0\t1\t-2\t3\t4\t5\n" + good,
             good + CC.line(-2, 1, 2, 3), CC.line(1 << 20, 1, 2, 3), CC.line(0, 1 << 31, 2, 3), CC.line(0, 1, 1 << 31, 3),
             CC.line(0, 1, 2, 1 << 31), b"0\t-\t2\t3\t4\t5\n", b"0\t+\t2\t3\t4\t5\n", b"0\t9223372036854775808\t2\t3\t4\t5\n",
             b"0\t-9223372036854775808\t2\t3\t4\t5\n", b"-9223372036854775808\t1\t2\t3\t4\t5\n", b"\t" * 70000 + b"\n", b"1" * 70000 + b"\n"]
    exact = [CC.VIRAL]
    for k, t in enumerate(texts):
        exact.append(CC.write_crai(tmp_path / ("t%d.crai" % k), t, members=1 + k % 3))
    # the text damaged byte by byte: still gzip, so the restatement reads the same bytes
    rng = np.random.default_rng(77)
    text = bytearray(gzip.open(CC.VIRAL, "rb").read()[:40000])
    for k in range(30):
        t = bytearray(text)
        for _ in range(int(rng.integers(1, 8))):
            t[int(rng.integers(0, len(t)))] = int(rng.choice(list(b"\t\n -+x0919")))
        exact.append(CC.write_crai(tmp_path / ("d%d.crai" % k), bytes(t), members=1 + k % 4))
    r = subprocess.run([asan_reader] + exact, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert got[-1] == "ok" and got[:-1] == [summary(p) for p in exact]
    # the gzip bytes damaged or cut short: whatever it makes of them, it stays inside its buffers
    raw = open(CC.VIRAL, "rb").read()
    loose = []
    for k in range(30):
        z = bytearray(raw)
        for _ in range(int(rng.integers(1, 6))):
            z[int(rng.integers(0, len(z)))] = int(rng.integers(0, 256))
        p = str(tmp_path / ("z%d.crai" % k))
        open(p, "wb").write(bytes(z) if k % 2 else raw[:int(rng.integers(0, len(raw)))])
        loose.append(p)
    loose.append(str(tmp_path / "missing.crai"))
    r = subprocess.run([asan_reader] + loose, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]
    assert r.stdout.count("refused 0") >= 15                 # (a cut file never passes)
