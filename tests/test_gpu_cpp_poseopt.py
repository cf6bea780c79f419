"""USLAM::Optimizer::PoseOptimization (include/uvo/compat/Optimizer.h) driven from a C++11 program through the C ABI, over a frame
whose mvpMapPoints has gaps: its pose, flags and count have to equal the Python binding's for the gathered correspondences (which
tests/test_gpu_poseopt.py holds to the host build and the model), mvbOutlier has to be cleared and rewritten exactly at the indices
with a map point, and the indices without one stay as they were."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import host_build
import poseopt_model as pm

INV_LEVELS = (1.0 / (1.2 ** np.arange(8)) ** 2).astype(np.float32)


def build_driver():
    return host_build.build("compat_poseopt")


def test_poseopt_driver_compiles_as_cxx11(uvo):
    """The adaptor instantiates over frame / map point stand-ins in the reference's dialect, warnings as errors."""
    assert os.path.exists(build_driver())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["shift_100_2", "thin_12", "few_9"])
def test_cpp_pose_optimization(uvo, tmp_path, name):
    p3d, p2d, w, K, Tcw = pm.make(name)
    n = len(p3d)
    g = np.random.default_rng(5)
    nkeys = n + n // 3 + 4
    idx = np.sort(g.choice(nkeys, n, replace=False))                # where the map points are; the rest are gaps
    keys = np.zeros(nkeys, [("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4"), ("class_id", "i4")])
    keys["x"], keys["y"] = g.uniform(0, 700, nkeys), g.uniform(0, 400, nkeys)
    keys["x"][idx], keys["y"][idx] = p2d[:, 0], p2d[:, 1]
    keys["octave"][idx] = np.argmin(np.abs(INV_LEVELS[None, :] - w[:, None]), 1)
    assert (INV_LEVELS[keys["octave"][idx]] == w).all()
    rec = np.zeros(nkeys, [("has", "i4"), ("p", "f4", 3)])
    rec["has"][idx], rec["p"][idx] = 1, p3d
    before = g.integers(0, 2, nkeys).astype(np.uint8)               # a pattern the call must clear where there is a map point, and only there
    blob = struct.pack("<i4f", nkeys, *[float(v) for v in K]) + INV_LEVELS.tobytes() + np.ascontiguousarray(Tcw, np.float32).tobytes()
    blob += keys.tobytes() + rec.tobytes() + before.tobytes()
    scene_p, out_p = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    with open(scene_p, "wb") as f:
        f.write(blob)
    r = subprocess.run([build_driver(), scene_p, out_p], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    said = json.loads(r.stdout.strip().splitlines()[-1])
    raw = open(out_p, "rb").read()
    assert len(raw) == 4 + 64 + nkeys
    ret, T, after = struct.unpack_from("<i", raw, 0)[0], np.frombuffer(raw, np.float32, 16, 4).reshape(4, 4), np.frombuffer(raw, np.uint8, nkeys, 68)
    assert said["ret"] == ret
    # the same problem through the Python binding
    klt = uvo.KLT(64, 64, max_points=16)
    opt = uvo.PoseOptimizer(klt, 1, nkeys)
    res, = opt.optimize([(p3d, p2d, w, K, Tcw)])
    opt.close()
    klt.close()
    assert ret == res.n_inliers and T.tobytes() == res.Tcw.tobytes()
    assert after[idx].tobytes() == res.outlier.tobytes()
    gaps = np.setdiff1d(np.arange(nkeys), idx)
    assert after[gaps].tobytes() == before[gaps].tobytes() and before[gaps].any()
    assert res.outlier.any() and not res.outlier.all()               # the flags were really scattered, not just cleared
