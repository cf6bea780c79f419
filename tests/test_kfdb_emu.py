"""The keyframe database without a GPU: the host build of csrc/kfdb_core.hpp (tests/emu/kfdb_emu.cpp: the functions the kernels of
csrc/kfdb.hip call, run by a serial loop over the slots) against the literal model (tests/kfdb_model.py) on the whole case table of
tests/kfdb_cases.py -- candidate lists and their order, the table of listed keyframes, every float as its bits, all six stored
fields of every slot after every query.  The closed-form list order (first common word, add sequence) is the host build's and the
kernels'; the model walks an inverted file.  The same program runs once more built with the address and undefined-behaviour sanitizers."""
import ctypes
import subprocess

import pytest

import host_build
import kfdb_cases as kc

NAMES = sorted(kc.cases())


def run_emu(exe, case, tmp_path):
    script = tmp_path / "case.txt"
    script.write_text(kc.to_script(case))
    r = subprocess.run([exe, str(script)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return kc.parse_output(r.stdout)


@pytest.fixture(scope="module")
def emu():
    return host_build.build("kfdb_emu")


@pytest.fixture(scope="module")
def emu_sanitized():
    return host_build.build("kfdb_emu", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"), "_san")


def test_new_symbols_are_declared_and_exported(uvo):
    names = ("uvo_kfdb_create", "uvo_kfdb_destroy", "uvo_kfdb_add", "uvo_kfdb_erase", "uvo_kfdb_clear", "uvo_kfdb_set_covisibles", "uvo_kfdb_detect_reloc",
             "uvo_kfdb_detect_loop", "uvo_kfdb_detect_loop_haloc", "uvo_kfdb_last_query", "uvo_kfdb_last_haloc", "uvo_kfdb_state", "uvo_kfdb_size")
    lib = ctypes.CDLL(uvo.LIB_PATH)
    for n in names:
        assert n in uvo.ABI_SYMBOLS and hasattr(lib, n), n
    assert uvo.KFDB_STATE_DTYPE.itemsize == 32 and uvo.KFDB_ROW_DTYPE.itemsize == 24


@pytest.mark.parametrize("name", NAMES)
def test_host_build_equals_the_model(emu, tmp_path, name):
    case, want = kc.cases()[name], kc.expected(name)
    got = run_emu(emu, case, tmp_path)
    assert got == want, kc.explain(got, want, case)


@pytest.mark.parametrize("name", NAMES)
def test_host_build_under_sanitizers(emu_sanitized, tmp_path, name):
    case, want = kc.cases()[name], kc.expected(name)
    got = run_emu(emu_sanitized, case, tmp_path)
    assert got == want, kc.explain(got, want, case)
