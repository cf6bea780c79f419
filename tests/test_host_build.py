"""tests/host_build.py on a throw-away tree: a two-line source, a header it includes, and a second header only that one includes.  What
makes an artefact stale is the compiler's own dependency list and the recorded command, never a list written by hand; a failed compile
leaves what was there.  Mtimes are set, not waited for.  The last test holds the real table to the files it names."""
import ctypes
import os
import subprocess

import pytest

import host_build

ENTRY = host_build.Artefact("out/libthing.so", "src/thing.cpp", host_build.CXX, ["-O0", "-fPIC", "-shared"], [])
SOURCE = '#include "outer.hpp"\nextern "C" int thing() { return INNER + VALUE; }\n'


@pytest.fixture
def tree(tmp_path):
    (tmp_path / "src").mkdir()
    (tmp_path / "out").mkdir()
    (tmp_path / "src" / "thing.cpp").write_text(SOURCE)
    (tmp_path / "src" / "outer.hpp").write_text('#include "inner.hpp"\n#ifndef VALUE\n#define VALUE 0\n#endif\n')
    (tmp_path / "src" / "inner.hpp").write_text("#define INNER 40\n")
    return tmp_path


def build(tree, **kw):
    return host_build.compile_artefact(ENTRY, root=str(tree), **kw)


def age(tree, lib, seconds):
    """Every file of the tree `seconds` older than the artefact."""
    t = os.stat(lib).st_mtime_ns - seconds * 10 ** 9
    for f in ("thing.cpp", "outer.hpp", "inner.hpp"):
        os.utime(str(tree / "src" / f), ns=(t, t))


def stamp(lib):
    s = os.stat(lib)
    return s.st_mtime_ns, s.st_ino


def thing(lib):
    return ctypes.CDLL(lib).thing()


def test_built_when_missing_and_left_alone_when_fresh(tree, monkeypatch):
    lib = build(tree)
    assert lib == str(tree / "out" / "libthing.so") and thing(lib) == 40
    lines = (tree / "out" / "libthing.so.d").read_text().splitlines()
    assert lines[0].startswith("# %s " % host_build.CXX) and lines[1:] == ["src/inner.hpp", "src/outer.hpp", "src/thing.cpp"]     # no system header, no absolute path
    age(tree, lib, 0)                                               # not newer: as old as the artefact is still fresh
    before = stamp(lib)
    monkeypatch.setattr(subprocess, "run", lambda *a, **k: pytest.fail("a fresh artefact started a process"))
    assert build(tree) == lib and stamp(lib) == before


def test_header_behind_a_header_rebuilds(tree):
    lib = build(tree)
    age(tree, lib, 10)
    inner = tree / "src" / "inner.hpp"                              # thing.cpp does not name it: only the compiler knows
    inner.write_text("#define INNER 41\n")
    t = os.stat(lib).st_mtime_ns + 10 ** 9
    os.utime(str(inner), ns=(t, t))
    before = stamp(lib)
    assert build(tree) == lib and stamp(lib) != before and thing(lib) == 41


def test_another_define_rebuilds_files_untouched(tree):
    lib = build(tree, extra=["-DVALUE=1"], suffix="_one")
    assert lib == str(tree / "out" / "libthing_one.so") and thing(lib) == 41
    age(tree, lib, 10)
    before = stamp(lib)
    assert build(tree, extra=["-DVALUE=1"], suffix="_one") == lib and stamp(lib) == before
    assert build(tree, extra=["-DVALUE=2"], suffix="_one") == lib and stamp(lib) != before
    assert "-DVALUE=2" in (tree / "out" / "libthing_one.so.d").read_text().splitlines()[0]


def test_sidecar_missing_or_naming_a_lost_file_rebuilds(tree):
    lib = build(tree)
    age(tree, lib, 10)
    sidecar = tree / "out" / "libthing.so.d"
    before = stamp(lib)
    sidecar.unlink()                                                # an artefact from before there were sidecars
    assert build(tree) == lib and stamp(lib) != before and sidecar.exists()
    age(tree, lib, 10)
    before = stamp(lib)
    sidecar.write_text(sidecar.read_text() + "src/gone.hpp\n")
    assert build(tree) == lib and stamp(lib) != before
    assert "gone.hpp" not in sidecar.read_text()


def test_failed_compile_raises_and_keeps_what_was_there(tree):
    lib = build(tree)
    age(tree, lib, 10)
    before, sidecar = stamp(lib), (tree / "out" / "libthing.so.d").read_text()
    (tree / "src" / "thing.cpp").write_text(SOURCE + "this is not C++\n")
    with pytest.raises(RuntimeError) as e:
        build(tree)
    assert host_build.CXX in str(e.value) and "src/thing.cpp" in str(e.value) and "error" in str(e.value)      # the command and the compiler's message
    assert stamp(lib) == before and (tree / "out" / "libthing.so.d").read_text() == sidecar and thing(lib) == 40
    assert sorted(os.listdir(str(tree / "out"))) == ["libthing.so", "libthing.so.d"]                    # no temporary file left behind


def test_table_names_existing_sources_and_distinct_outputs():
    outs = [e.out for e in host_build.ARTEFACTS.values()]
    assert len(set(outs)) == len(outs)
    for name, e in host_build.ARTEFACTS.items():
        assert os.path.isfile(os.path.join(host_build.ROOT, e.src)), name
        assert e.cc in (host_build.CXX, "hipcc") and not os.path.isabs(e.out) and not os.path.isabs(e.src), name
    assert set(host_build.PREBUILT) <= set(host_build.ARTEFACTS)
