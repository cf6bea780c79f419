"""The carve helper (csrc/carve.hpp: one description of a block, walked once to measure and once to place) exercised on the host by
tests/emu/carve_emu.cpp, a program of its own (its header lists the properties): built once plain and once with
-fsanitize=address,undefined, and run.  No GPU, nothing loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "carve_emu.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _build_and_run(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / "carve_emu")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.rstrip().endswith("all checks passed") and "FAIL" not in r.stdout
    return r.stdout


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    return _build_and_run(tmp_path_factory, "plain", ["-O2"])


def test_carve_under_sanitizers(tmp_path_factory):
    out = _build_and_run(tmp_path_factory, "san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "runtime error" not in out


def test_random_descriptions(report):
    m = re.search(r"^(\d+) random descriptions, (\d+) of them 256-aligned throughout, (\d+) empty arrays", report, re.M)
    assert m and int(m.group(1)) >= 300 and int(m.group(2)) >= 50 and int(m.group(3)) >= 50, report[:400]


def test_library_blocks_keep_their_offsets(report):
    """every block the library carves, at its smallest, an odd and its largest shape, against the offset chain it replaced"""
    for what in ("PnPsolver set (1, 4)", "PnPsolver set (2, 65)", "PnPsolver set (64, 16384)", "Sim3Solver set (1, 4)", "Sim3Solver set (2, 65)",
                 "Sim3Solver set (64, 16384)", "Initializer (8)", "Initializer (65)", "Initializer (16384)", "PnP scratch (5)", "PnP scratch (4096)",
                 "findFundamentalMat scratch", "keyframe database, pinned (1, 1, 1)", "keyframe database, pinned (65536, 4096, 4096)"):
        assert re.search(r"^%s\s+\d+ arrays, \d+ bytes$" % re.escape(what), report, re.M), what
