"""The band schedule of k_resize_level_rows (csrc/resize_rows.hpp) walked on the host by tests/emu/resize_rows_emu.cpp, a program of its own
(its header lists the properties): built once plain and once with -fsanitize=address,undefined, and run.  No GPU, nothing loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "resize_rows_emu.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _build_and_run(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / "resize_rows_emu")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.rstrip().endswith("all checks passed") and "FAIL" not in r.stdout
    return r.stdout


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    return _build_and_run(tmp_path_factory, "plain", ["-O2"])


def test_schedule_under_sanitizers(tmp_path_factory):
    out = _build_and_run(tmp_path_factory, "san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "runtime error" not in out


def _rows(report, what, ring):
    m = re.search(r"^%s\s+ring\s+%d:\s+(\d+) bands, ([\d.]+) source rows filtered per output row \(([\d.]+) on the monotone part" % (re.escape(what), ring), report, re.M)
    assert m, "no line for %s ring %d" % (what, ring)
    return int(m.group(1)), float(m.group(2)), float(m.group(3))


def test_rows_filtered_per_output_row(report):
    """scale + 1 / band on the monotone part is the schedule's promise; the whole launch adds the reflected pad rows, where the sequence
    turns round"""
    m = re.search(r"^band (\d+), (\d+) rows ahead", report, re.M)
    band = int(m.group(1))
    for what, scale in (("640x512 scale 1.20 level 1 in place", 1.2), ("640x512 scale 1.20 level 7", 1.2), ("1920x1080 scale 1.20 level 1 in place", 1.2),
                        ("200x180 scale 1.10 level 1 in place", 1.1), ("333x222 scale 1.33 level 1", 1.33)):
        bands, total, mono = _rows(report, what, 4)
        print(what, bands, total, mono)
        assert abs(mono - scale) < 0.02, (what, mono)                  # inside a band: one row on a step of one, two on a step of two
        assert scale <= total <= scale + 1.0 / band + 0.06, (what, total)     # + the band's first row, + the turn in the four pad rows


def test_held_rows_filtered_again_only_in_the_pad(report):
    """the kernel filters the lower row always: the program asserts per level that this repeats a held row only where the table clamps or turns
    round, at most 2 x pad rows + 4 times; here the printed counts: ring 4 (the hot path) has 8 pad rows"""
    counts = [int(m) for m in re.findall(r"ring  4: .*?; (\d+) re-filtered", report)]
    assert len(counts) > 40 and max(counts) <= 12, counts


def test_byte_gather_levels_keep_the_old_kernel(report):
    for what in ("400x300 scale 1.50 level 1 in place", "512x384 scale 2.00 level 2"):
        assert re.search(r"^%s\s+keeps k_resize_level" % re.escape(what), report, re.M)
    assert "ring" not in "".join(l for l in report.splitlines() if l.startswith(("400x300", "512x384")))
