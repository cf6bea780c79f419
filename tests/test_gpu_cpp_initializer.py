"""USLAM::Initializer (include/uvo/compat/Initializer.h) driven from a C++ program through the C ABI, the way Tracking::Initialize would
drive it, compiled against the declaration-only OpenCV stand-in (tests/cpp/opencv_decl_stub, unchanged; the driver defines what it
calls): what it returns equals what the Python binding gives for the same calls on one generator, which tests/test_gpu_initializer.py
holds to the host build and the model."""
import os
import struct
import subprocess

import numpy as np
import pytest

import host_build
import initializer_checks as ic


def build_driver():
    return host_build.build("compat_initializer")


def test_initializer_driver_compiles_as_cxx11(uvo):
    """The adaptor instantiates over a frame stand-in in the reference's dialect, warnings as errors."""
    assert os.path.exists(build_driver())


@pytest.mark.gpu
def test_cpp_initialize_equals_the_c_abi(uvo, tmp_path):
    """Two scenes on one reference frame and one generator: a general one (accepted) and its pure-rotation twin (rejected)."""
    k1, k2a, m12, _ = ic.scene(0, 64, 0.1)
    _, k2b, _, _ = ic.scene(0, 64, 0.1, "rotation")
    blob = struct.pack("<ii4f", len(k1), 2, *ic.CAM) + k1.tobytes()
    for k2 in (k2a, k2b):
        blob += struct.pack("<i", len(k2)) + k2.tobytes() + m12.tobytes()
    scene_p, out_p = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    with open(scene_p, "wb") as f:
        f.write(blob)
    r = subprocess.run([build_driver(), scene_p, out_p], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out_p, "rb").read()
    klt = uvo.KLT(64, 64, max_points=256)
    ini = uvo.Initializer(klt, 2048)
    ini.set_reference(k1, ic.CAM, 1.0, 200)
    g, off, oks = uvo.GlibcRand(1), 0, []
    for k2 in (k2a, k2b):
        res = ini.initialize(k2, m12, g)
        n = len(k2)
        ok, r_empty, t_empty, n2 = struct.unpack_from("<4i", raw, off)
        pose = np.frombuffer(raw, np.float32, 12, off + 16)
        p3d = np.frombuffer(raw, np.float32, 3 * n, off + 64).reshape(n, 3)
        tri = np.frombuffer(raw, np.uint8, n, off + 64 + 12 * n)
        off += 64 + 13 * n
        assert (bool(ok), n2) == (res.initialized, n) and r_empty == t_empty == (0 if res.initialized else 1), r.stdout
        assert pose.tobytes() == np.concatenate([res.R21.reshape(9), res.t21]).astype(np.float32).tobytes()
        assert p3d.tobytes() == res.p3d.tobytes() and (tri == res.triangulated).all()
        oks.append(res.initialized)
    ini.close()
    klt.close()
    assert off == len(raw) and oks == [True, False]
