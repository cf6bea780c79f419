"""USLAM::solvePnPRansac (include/uvo/compat/SolvePnPRansac.h) driven from a C++ program through the C ABI, the way
Tracking::TrackWithPnP would drive it; checked byte for byte against the Python binding of the same entry point (same library, same
inputs) and, through it, against everything tests/test_gpu_pnp.py holds that entry point to."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import host_build
import pnp_model as pm


def build_driver():
    return host_build.build("compat_pnp")


def test_pnp_driver_compiles_as_cxx11(uvo):
    """The adaptor instantiates over Point3f / Point2f stand-ins in the reference's dialect, warnings as errors."""
    assert os.path.exists(build_driver())


@pytest.mark.gpu
@pytest.mark.parametrize("sc", [(31, 400, 0.7, 1.0, pm.EUROC), (32, 64, 0.5, 0.3, pm.PLAIN), (33, 5, 1.0, 0.3, pm.EUROC), (34, 4, 1.0, 0.3, pm.PLAIN),
                                (35, 20, 0.3, 1.0, pm.EUROC)], ids=lambda s: "n%d_r%.2f" % (s[1], s[2]))
def test_cpp_solve_pnp_ransac(uvo, tmp_path, sc):
    cam, obj, img, _, _, _ = pm.scene(*sc)
    scene_p, out_p = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    with open(scene_p, "wb") as f:
        f.write(struct.pack("<ii4f8f", len(obj), cam.n_dist, cam.fx, cam.fy, cam.cx, cam.cy, *cam.k))
        f.write(obj.astype(np.float32).tobytes() + img.astype(np.float32).tobytes())
    r = subprocess.run([build_driver(), scene_p, out_p], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    said = json.loads(r.stdout.strip().splitlines()[-1])
    raw = open(out_p, "rb").read()
    ok, k = struct.unpack_from("<ii", raw, 0)
    rvec, tvec = np.frombuffer(raw, np.float64, 3, 8), np.frombuffer(raw, np.float64, 3, 32)
    Tcw, inl = np.frombuffer(raw, np.float32, 16, 56).reshape(4, 4), np.frombuffer(raw, np.int32, k, 120)
    klt = uvo.KLT(64, 64, max_points=max(len(obj), 16))
    prvec, ptvec, pTcw, pinl, info = klt.solve_pnp_ransac(obj, img, uvo.CameraModel.make(cam.fx, cam.fy, cam.cx, cam.cy, cam.k[:cam.n_dist]))
    klt.close()
    assert (ok, k) == (info.ok, info.inliers) == (said["ok"], said["inliers"])
    assert rvec.tobytes() == prvec.tobytes() and tvec.tobytes() == ptvec.tobytes() and Tcw.tobytes() == pTcw.tobytes()
    np.testing.assert_array_equal(inl, pinl)
    if sc[1] >= 64:
        assert ok == 1 and k > 0.4 * sc[1] * sc[2]
    if sc[1] < 5:
        assert ok == 0 and k == 0
