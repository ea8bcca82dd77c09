"""What `goleft-depth` refuses before it opens the device, byte for byte: every case of tools/record_cli_cases.py run as a
fresh child process in a fresh working directory, its exit code, whole stdout and whole stderr held to
tests/cli_refusals.json.  The recorded values are those of a build of the commit before the command-line scaffold was
shared (host/cli.hpp): they are a reference and are not regenerated from the tree under test.  No case reaches gd_create
(the recorder refuses one that does), so the same expectations hold with and without a device."""
import importlib.util
import json
import os

import pytest

from tests.helpers import ROOT

EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")


def _recorder():
    spec = importlib.util.spec_from_file_location("record_cli_cases", os.path.join(ROOT, "tools", "record_cli_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
with open(os.path.join(ROOT, "tests", "cli_refusals.json")) as _f:
    RECORDED = json.load(_f)


def test_the_recorded_cases_are_the_table():
    """the JSON was recorded from this table: same cases, same argvs, same inputs, in the same order"""
    assert [(r["name"], r["cmd"], r["argv"], r["files"], r["env"]) for r in RECORDED] == [tuple(c) for c in REC.CASES]
    for r in RECORDED:
        assert "no usable MI355X device" not in r["stderr"], r["name"]
        assert r["exit"] in (1, 2, 255) or (r["exit"] == 0 and ("-h" in r["argv"] or "--help" in r["argv"])), r["name"]
    # every subcommand: help twice, an unknown flag written both ways
    for cmd in REC.SUBCOMMANDS:
        mine = [r for r in RECORDED if r["cmd"] == cmd]
        assert sum(r["exit"] == 0 and r["stdout"] != "" for r in mine) == 2, cmd
        assert sum("unknown argument --bogus" in r["stderr"] for r in mine) >= 2, cmd


@pytest.mark.parametrize("rec", RECORDED, ids=[r["name"] for r in RECORDED])
def test_refusal(rec):
    code, out, err, left = REC.run_case(EXE, (rec["name"], rec["cmd"], rec["argv"], rec["files"], rec["env"]), timeout=60)
    assert err == rec["stderr"]
    assert out == rec["stdout"]
    assert code == rec["exit"]
    assert left == [], "the run left files behind"
