"""CPU: goleft_amd/csrc/gd_eigh.hpp -- the tred2 / tql2 solver indexcov's principal components and the SVD debiaser share --
compiled as it is into a stand-alone program (tests/emul/eigh_emul.cpp, g++) and compared with numpy.linalg.eigh at
N = 2, 3, 64, 65 and 257, a repeated eigenvalue and a rank-deficient matrix among them: eigenvalues within
N 2^-50 |w|max, residuals |G v - w v| within N 2^-48 |w|max, eigenvectors orthonormal.  The same program is built and run
once more with -fsanitize=address,undefined: a host-only check, nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H

EMUL_DIR = os.path.join(H.ROOT, "tests", "emul")
SRC = os.path.join(EMUL_DIR, "eigh_emul.cpp")
HDR = os.path.join(H.ROOT, "goleft_amd", "csrc", "gd_eigh.hpp")
GXX = shutil.which("g++")

pytestmark = pytest.mark.skipif(GXX is None, reason="the header is compiled for the host with g++")


def matrices():
    rng = np.random.default_rng(11)
    out = []
    for n in (2, 3, 64, 65, 257):
        X = rng.poisson(30, (3 * n + 5, n)).astype(np.float64)
        out.append(("gram_%d" % n, X.T @ X))
    Q, _ = np.linalg.qr(rng.standard_normal((64, 64)))
    w = np.concatenate([[9.0, 4.0, 4.0, 4.0], np.linspace(3, 1, 60)])
    G = (Q * w) @ Q.T
    out.append(("repeated_64", (G + G.T) / 2))
    X = rng.poisson(30, (40, 65)).astype(np.float64)                                   # rank 40 of 65
    out.append(("rank_deficient_65", X.T @ X))
    out.append(("diagonal_3", np.diag([2.0, 0.0, 5.0])))
    out.append(("zero_5", np.zeros((5, 5))))
    out.append(("one_1", np.array([[7.0]])))
    return out


def build(tmp, flags, name):
    exe = str(tmp / name)
    subprocess.check_call([GXX, "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off"] + flags + ["-o", exe, SRC])
    return exe


def solve(exe, tmp, mats):
    src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(src, "wb") as f:
        for _, G in mats:
            f.write(np.int64(G.shape[0]).tobytes())
            f.write(np.ascontiguousarray(G, np.float64).tobytes())
    subprocess.check_call([exe, src, dst], timeout=120)
    raw = open(dst, "rb").read()
    at, res = 0, []
    for _, G in mats:
        n = G.shape[0]
        rc = int(np.frombuffer(raw, np.int64, 1, at)[0])
        w = np.frombuffer(raw, np.float64, n, at + 8)
        V = np.frombuffer(raw, np.float64, n * n, at + 8 + 8 * n).reshape(n, n)       # row c: eigenvector c
        at += 8 + 8 * n + 8 * n * n
        res.append((rc, w, V))
    assert at == len(raw)
    return res


def held(mats, res):
    for (name, G), (rc, w, V) in zip(mats, res):
        n = G.shape[0]
        assert rc == 0, name
        want = np.linalg.eigh(G)[0]
        top = np.abs(want).max()
        assert (np.abs(np.sort(w) - want) <= n * 2.0 ** -50 * top).all(), (name, float(np.abs(np.sort(w) - want).max()), top)
        resid = np.linalg.norm(G @ V.T - V.T * w, axis=0)
        assert (resid <= n * 2.0 ** -48 * top).all(), (name, float(resid.max()), top)
        assert np.abs(V @ V.T - np.eye(n)).max() <= n * 2.0 ** -50, name


def test_the_solver_against_numpy(tmp_path):
    mats = matrices()
    held(mats, solve(build(tmp_path, [], "eigh_emul"), tmp_path, mats))


def test_the_solver_under_the_sanitizers(tmp_path):
    mats = matrices()
    exe = build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "eigh_emul_san")
    held(mats, solve(exe, tmp_path, mats))
