"""The C++ adaptors with the reference's class signatures (include/uvo/compat/) driven from a C++ program, the way
src/Tracking.cc drives USLAM::ORBextractor / USLAM::ORBmatcher; results checked against the oracle."""
import os
import struct
import subprocess

import numpy as np
import pytest

import host_build
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver():
    return host_build.build("compat_driver")


def test_adaptor_headers_compile_as_cxx11():
    """The reference is built as C++11 (CMakeLists.txt:16); the adaptors must compile in that dialect with plain g++."""
    assert os.path.exists(build_driver())


def test_opencv_signature_branches_type_check():
    """The UVO_COMPAT_WITH_OPENCV branches -- USLAM::ORBextractor::operator() with the reference's signature
    (include/ORBextractor.h:56-58), the cv::Mat overloads and every search member of the ORBmatcher adaptor instantiated with types
    that declare what the reference's FrameKTL / KeyFrame / MapPoint declare, Grider_FAST::perform_griding -- must compile as C++11 at
    the reference's own call sites (src/Tracking.cc:946, :2228, :2500, :2561; src/LocalMapping.cc:1080, :1236, :1261; the loop-closing
    calls).  OpenCV and Eigen are declaration-only stand-ins (tests/cpp/opencv_decl_stub/: no behaviour, nothing linked or run, they
    pin nothing); the check is g++ -fsyntax-only."""
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "opencv_decl_stub"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "compile_opencv_branch.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    # and the branch is really there: without the macro the cv:: members do not exist
    probe = "#include \"uvo/compat/ORBextractor.h\"\nint f(USLAM::ORBextractor* e) { return sizeof(&USLAM::ORBextractor::operator()); }\n"
    r2 = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-x", "c++", "-"], input=probe, capture_output=True, text=True)
    assert r2.returncode != 0


@pytest.mark.gpu
def test_cpp_adaptors_match_oracle(tmp_path, oracle, synth):
    w, h = 752, 480
    img = synth.make_frame(31337, w, h)
    oe = oracle.extractor(1000, 1.2, 8, 7)
    kp_o, de_o = oe(img)
    n = len(kp_o)
    rng = np.random.default_rng(2)
    M = 3000
    src = rng.integers(0, n, M)
    mp_desc = rng.integers(0, 256, (M, 32), dtype=np.uint8)
    true = rng.random(M) < 0.5
    flips = rng.random((M, 256)) < 0.05
    mp_desc[true] = np.packbits(np.unpackbits(de_o[src], axis=1) ^ flips, axis=1)[true]
    px = (kp_o["x"][src] + rng.normal(0, 1.5, M)).astype(np.float32)
    py = (kp_o["y"][src] + rng.normal(0, 1.5, M)).astype(np.float32)
    level = np.clip(kp_o["octave"][src] + rng.integers(-1, 2, M), 0, 7).astype(np.int32)
    vc = np.where(rng.random(M) < 0.5, 0.999, 0.9).astype(np.float32)
    inview = (rng.random(M) < 0.9).astype(np.uint8)
    img_p, mp_p, out_p = tmp_path / "img.raw", tmp_path / "mp.bin", tmp_path / "out.bin"
    img.tofile(img_p)
    with open(mp_p, "wb") as f:
        for i in range(M):
            f.write(struct.pack("<ffifB", px[i], py[i], level[i], vc[i], inview[i]) + mp_desc[i].tobytes())
    r = subprocess.run([build_driver(), str(img_p), str(w), str(h), str(mp_p), str(out_p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out_p, "rb").read()
    n_g = struct.unpack_from("<i", raw, 0)[0]
    assert n_g == n
    kp_g = np.frombuffer(raw, oracle_lib.KP, n, 4)
    de_g = np.frombuffer(raw, np.uint8, n * 32, 4 + 28 * n).reshape(n, 32)
    nm_g = struct.unpack_from("<i", raw, 4 + 60 * n)[0]
    a_g = np.frombuffer(raw, np.int32, n, 8 + 60 * n)
    assert kp_g.tobytes() == kp_o.tobytes() and (de_g == de_o).all()
    a_o = np.full(n, -1, np.int32)
    nm_o = oracle.search_by_projection(kp_o, de_o, (0, 0, w, h), a_o, px, py, level, vc, inview, mp_desc, oe.scale, 1.0, 0.8)
    assert nm_g == nm_o and (a_g == a_o).all() and nm_g > 200
