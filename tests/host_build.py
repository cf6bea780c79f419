"""Every host artefact the tests and __graft_entry__.build() compile: the tests/emu host builds the kernels are held to, their
stand-alone programs, and the C++11 compat drivers of tests/cpp.  One table, one function.  Test infrastructure only.

build(name) returns the artefact's path and compiles first unless it is fresh.  The compiler runs at the repository root with relative
paths and writes the dependencies it saw (-MMD); they are kept next to the artefact as <out>.d, the command in a first comment line, the
project's own files below it as root-relative paths.  An artefact is fresh when it and its .d exist, the recorded command is the one
that would run now, and every listed file exists and is not newer than the artefact.  No header is listed by hand anywhere.

The drivers link -luvo: the library has to be there before a driver is asked for (build() of __graft_entry__.py, or the uvo fixture)."""
import collections
import importlib.util
import os
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# out and src relative to the root; cc "g++" or "hipcc" (build.py's HIPCC); flags stand in front of -o, libs behind the source
Artefact = collections.namedtuple("Artefact", "out src cc flags libs")

CXX = "g++"
SHARED = ["-O2", "-std=c++17", "-fPIC", "-shared"]
NO_FMA = ["-ffp-contract=off"]                          # the library's contract, where device and host are held bit for bit
PROGRAM = ["-O2", "-std=c++17", "-ffp-contract=off"]
HIP = ["-x", "hip", "--offload-arch=gfx950"]            # csrc/extractor_geom.cpp runs on the host, but its headers need HIP's
CXX11 = ["-std=c++11", "-O2", "-Wall", "-Werror", "-Iinclude"]
UVO = ["-Lu-vip-slam_amd", "-luvo", "-Wl,-rpath,$ORIGIN/../../u-vip-slam_amd"]


def _emu(name, flags, cc=CXX, libs=()):
    return Artefact("tests/emu/lib%s.so" % name, "tests/emu/%s.cpp" % name, cc, flags, list(libs))


def _program(name, flags):
    return Artefact("tests/emu/" + name, "tests/emu/%s.cpp" % name, CXX, PROGRAM + flags, [])


def _driver(name, flags=CXX11):
    return Artefact("tests/cpp/" + name, "tests/cpp/%s.cpp" % name, CXX, flags, UVO)


ARTEFACTS = {}
ARTEFACTS.update({n: _emu(n, SHARED) for n in ("octree_emu", "pyr_tiles_emu", "strip_plan_emu", "blur_plan_emu")})
# the same quad-tree body with the phases run by 1024 "threads", as k_octree<1024> runs them (tests/octree_cases.py)
ARTEFACTS["octree_emu_1024"] = Artefact("tests/emu/liboctree_emu_1024.so", "tests/emu/octree_emu.cpp", CXX, SHARED + ["-DOCT_THREADS=1024"], [])
ARTEFACTS.update({n: _emu(n, SHARED + HIP, "hipcc") for n in ("geom_emu", "grider_geom_emu")})
ARTEFACTS.update({n: _emu(n, SHARED + NO_FMA) for n in ("pnp_emu", "pnpsolver_emu", "sim3solver_emu", "initializer_emu", "poseopt_emu",
                                                        "sim3opt_emu", "ba_emu", "navopt_emu", "navba_emu")})
ARTEFACTS["math_host"] = _emu("math_host", SHARED + NO_FMA, libs=["-lpthread"])
ARTEFACTS["kfdb_emu"] = _program("kfdb_emu", ["-Wall", "-Werror"])
ARTEFACTS.update({n + "_main": _program(n, ["-D%s_MAIN" % n.upper()]) for n in ("poseopt_emu", "sim3opt_emu", "ba_emu", "navopt_emu", "navba_emu")})
ARTEFACTS.update({n: _driver(n) for n in ("compat_scenes", "compat_newpoints", "compat_pnp", "compat_pnpsolver", "compat_sim3solver",
                                          "compat_kfdb", "compat_poseopt", "compat_sim3opt", "compat_ba", "compat_navopt", "compat_navba")})
ARTEFACTS["compat_initializer"] = _driver("compat_initializer", CXX11 + ["-Itests/cpp/opencv_decl_stub"])
ARTEFACTS["compat_driver"] = _driver("compat_driver", [f for f in CXX11 if f != "-Werror"])

# what __graft_entry__.build() compiles ahead of the tests, in its order
PREBUILT = ("octree_emu", "octree_emu_1024", "pyr_tiles_emu", "strip_plan_emu", "geom_emu", "grider_geom_emu", "pnp_emu", "pnpsolver_emu", "sim3solver_emu",
            "initializer_emu", "kfdb_emu")


def _compiler(cc):
    if cc != "hipcc":
        return cc
    spec = importlib.util.spec_from_file_location("uvo_build", os.path.join(ROOT, "u-vip-slam_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC


def _listed(dep_text, root):
    """The files of a compiler-written dependency file that lie under root, as sorted root-relative paths."""
    files = set()
    for rule in dep_text.replace("\\\n", " ").splitlines():
        for f in rule.partition(":")[2].split():
            rel = os.path.relpath(os.path.join(root, f), root)
            if not rel.startswith(".."):
                files.add(rel)
    return sorted(files)


def _fresh(out, sidecar, header, root):
    try:
        built = os.path.getmtime(os.path.join(root, out))
        with open(os.path.join(root, sidecar)) as fh:
            lines = fh.read().splitlines()
        return lines[:1] == [header] and all(os.path.getmtime(os.path.join(root, f)) <= built for f in lines[1:])
    except OSError:                                     # no artefact, no sidecar (an artefact from before there were any), a listed file gone
        return False


def compile_artefact(entry, extra=(), suffix="", force=False, root=ROOT):
    """entry, with `extra` flags added and `suffix` put in front of the output's extension -> the artefact's absolute path."""
    stem, ext = os.path.splitext(entry.out)
    out = stem + suffix + ext
    command = [entry.cc] + entry.flags + list(extra) + ["-MMD", "-MF", out + ".d", "-o", out, entry.src] + entry.libs
    header = "# " + " ".join(shlex.quote(a) for a in command)
    if force or not _fresh(out, out + ".d", header, root):
        tmp = "%s.%d.tmp" % (out, os.getpid())          # same directory: os.replace() is atomic, a concurrent build keeps its own
        run = [_compiler(entry.cc)] + [{out: tmp, out + ".d": tmp + ".d"}.get(a, a) for a in command[1:]]
        try:
            r = subprocess.run(run, cwd=root, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("%s failed:\n%s\n%s" % (entry.cc, " ".join(shlex.quote(a) for a in run), r.stderr[-6000:]))
            sys.stderr.write(r.stderr)
            with open(os.path.join(root, tmp + ".d")) as fh:
                files = _listed(fh.read(), root)
            with open(os.path.join(root, tmp + ".d"), "w") as fh:
                fh.write("\n".join([header] + files) + "\n")
            os.replace(os.path.join(root, tmp), os.path.join(root, out))
            os.replace(os.path.join(root, tmp + ".d"), os.path.join(root, out + ".d"))
        finally:
            for leftover in (tmp, tmp + ".d"):
                if os.path.exists(os.path.join(root, leftover)):
                    os.remove(os.path.join(root, leftover))
    return os.path.join(root, out)


def build(name, extra=(), suffix="", force=False):
    return compile_artefact(ARTEFACTS[name], extra, suffix, force)
