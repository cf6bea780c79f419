"""USLAM::KeyFrameDatabase (include/uvo/compat/KeyFrameDatabase.h) driven from a C++ program with stand-ins for the reference's KeyFrame
and FrameKTL, the way Tracking::Relocalisation and LoopClosing::DetectLoop call it: add / erase / clear and the three Detect* with
their signatures.  Held to the literal model on the whole case table of tests/kfdb_cases.py, in both refresh modes of the covisible
rows: every key frame in front of every query (the default), and only those named through NotifyCovisibilityChanged."""
import os
import subprocess

import pytest

import host_build
import kfdb_cases as kc

NAMES = sorted(kc.cases())


def build_driver():
    return host_build.build("compat_kfdb")


def test_kfdb_driver_compiles_as_cxx11(uvo):
    """The adaptor instantiates over key frame / frame stand-ins in the reference's dialect, warnings as errors."""
    assert os.path.exists(build_driver())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["every_keyframe", "hook"])
@pytest.mark.parametrize("name", NAMES)
def test_adaptor_equals_the_model(uvo, tmp_path, name, mode):
    case, want = kc.cases()[name], kc.expected(name)
    script = tmp_path / "case.txt"
    script.write_text(kc.to_script(case))
    r = subprocess.run([build_driver()] + (["--hook"] if mode == "hook" else []) + [str(script)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = kc.parse_output(r.stdout)
    assert got == want, kc.explain(got, want, case)
