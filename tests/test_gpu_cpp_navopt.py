"""The two IMU overloads of USLAM::Optimizer::PoseOptimization (include/uvo/compat/Optimizer.h) driven from a C++11 program through the
C ABI, over frames whose mvpMapPoints have gaps: the NavState, pose, flags of both frames, mMargCovInv, mNavStatePrior and the count
have to equal the Python binding's for the gathered problem (which tests/test_gpu_navopt.py holds to the host build and the model),
mvbOutlier has to be cleared and rewritten exactly at the indices with a map point, the indices without one stay as they were, and
in the frame form the prior one call writes is the prior the next call reads."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import host_build
import navopt_model as nm

INV_LEVELS = (1.0 / (1.2 ** np.arange(8)) ** 2).astype(np.float32)
DEPTH_COV = 0.05


def build_driver():
    return host_build.build("compat_navopt")


def test_navopt_driver_compiles_as_cxx11(uvo):
    """Both overloads instantiate over frame / key frame / NavState / preintegration stand-ins in the reference's dialect, warnings as errors."""
    assert os.path.exists(build_driver())


def depth_info(sc, last):
    """The adaptor's: 1 / cov1^2, cov1 = shi^2 depth_cov^2 + e3^T Rwb^T CovPos Rwb e3 over the 3 x 3 position block, in its order."""
    R, C = nm.rot(last["q"]), np.asarray(sc["cov"], np.float64).reshape(9, 9)
    cov3 = 0.0
    for i in range(3):
        for j in range(3):
            cov3 = cov3 + (R[i, 2] * C[i, j]) * R[j, 2]
    cov1 = (sc["shi"] * sc["shi"] * DEPTH_COV * DEPTH_COV) + cov3
    return 1 / (cov1 * cov1)


def frame_blob(g, edges):
    """A frame whose map points sit at sorted random indices among gaps -> (bytes, idx, before)."""
    n = len(edges)
    nkeys = n + n // 3 + 4
    idx = np.sort(g.choice(nkeys, n, replace=False))
    keys = np.zeros(nkeys, [("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4"), ("class_id", "i4")])
    keys["x"], keys["y"] = g.uniform(0, 700, nkeys), g.uniform(0, 400, nkeys)
    keys["x"][idx], keys["y"][idx] = edges[:, 3], edges[:, 4]
    keys["octave"][idx] = np.argmin(np.abs(INV_LEVELS[None, :] - edges[:, 5][:, None]), 1)
    assert (INV_LEVELS[keys["octave"][idx]] == edges[:, 5]).all()
    rec = np.zeros(nkeys, [("has", "i4"), ("p", "f4", 3)])
    rec["has"][idx], rec["p"][idx] = 1, edges[:, :3]
    before = g.integers(0, 2, nkeys).astype(np.uint8)
    return struct.pack("<i", nkeys) + keys.tobytes() + rec.tobytes() + before.tobytes(), idx, before


def read_call(raw, off, nk, nk_last):
    ret = struct.unpack_from("<i", raw, off)[0]
    ns = np.frombuffer(raw, np.float64, 22, off + 4)
    T = np.frombuffer(raw, np.float32, 16, off + 180).reshape(4, 4)
    inv = np.frombuffer(raw, np.float64, 225, off + 244).reshape(15, 15)
    prior = np.frombuffer(raw, np.float64, 22, off + 2044)
    after = np.frombuffer(raw, np.uint8, nk, off + 2220)
    after_last = np.frombuffer(raw, np.uint8, nk_last, off + 2220 + nk)
    return (ret, ns, T, inv, prior, after, after_last), off + 2220 + nk + nk_last


def check_call(got, res, idx, before, idx_l, before_l, marg):
    ret, ns, T, inv, prior, after, after_last = got
    assert ret == res.n_inliers and ns.tobytes() == nm.state_vec(res.ns).tobytes() and T.tobytes() == res.Tcw.tobytes()
    assert after[idx].tobytes() == res.outlier.tobytes()
    gaps = np.setdiff1d(np.arange(len(after)), idx)
    assert after[gaps].tobytes() == before[gaps].tobytes() and before[gaps].any()            # untouched indices stay as they were
    if idx_l is not None:
        assert after_last[idx_l].tobytes() == res.outlier_last.tobytes()
        gaps = np.setdiff1d(np.arange(len(after_last)), idx_l)
        assert after_last[gaps].tobytes() == before_l[gaps].tobytes()
    if marg:
        assert res.marg_ok == 1 and inv.tobytes() == res.marg_cov_inv.tobytes() and prior.tobytes() == ns.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kf_shift_300", "fr_shift_300", "fr_shift_60"])
def test_cpp_nav_pose_optimization(uvo, tmp_path, name):
    sc = nm.make(name)
    frame = sc["form"] == nm.FRAME
    # what the adaptor reads through float members: the intrinsics and gw
    sc["K"] = tuple(float(np.float32(v)) for v in sc["K"])
    sc["gw"] = np.asarray(sc["gw"], np.float32).astype(np.float64)
    sc["depth_info"] = depth_info(sc, sc["last"]) if sc["has_depth"] else 0.0
    if not sc["has_depth"]:
        sc["shi"], sc["depth_meas"] = 0.0, 0.0               # the adaptor leaves them zero without a depth edge
    g = np.random.default_rng(5)
    blob_c, idx, before = frame_blob(g, sc["edges"])
    last_edges = sc["edges_last"] if frame else np.zeros((0, 6), np.float32)
    blob_l, idx_l, before_l = frame_blob(g, last_edges)
    scene_p, out_p = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    with open(scene_p, "wb") as f:
        f.write(nm.record(sc).tobytes() + struct.pack("<d", DEPTH_COV) + INV_LEVELS.tobytes() + blob_c + blob_l)
    r = subprocess.run([build_driver(), scene_p, out_p], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    said = json.loads(r.stdout.strip().splitlines()[-1])
    raw = open(out_p, "rb").read()
    nk, nkl = len(before), len(before_l)
    first, off = read_call(raw, 0, nk, nkl if frame else 0)
    # the same problem through the Python binding
    klt = uvo.KLT(64, 64, max_points=16)
    opt = uvo.NavOptimizer(klt, 1, max(nk, nkl))
    try:
        res, = opt.optimize([sc])
        assert said["ret"] == res.n_inliers and res.outlier.any() and not res.outlier.all()  # the flags were really scattered, not just cleared
        check_call(first, res, idx, before, idx_l if frame else None, before_l, sc["compute_marg"])
        if frame:
            # the next call: the frame just optimised is the last frame, with the prior and the information the first call wrote
            second, off = read_call(raw, off, nk, nk)
            # (without bComputeMarg nothing was written: the frame's prior is still what it held before, here its own start and no information)
            marg = sc["compute_marg"]
            nxt = dict(sc, last=res.ns, prior=res.ns if marg else sc["cur"], prior_info=res.marg_cov_inv if marg else np.zeros((15, 15)), edges_last=sc["edges"])
            nxt["depth_info"] = depth_info(sc, res.ns) if sc["has_depth"] else 0.0
            res2, = opt.optimize([nxt])
            assert said["ret2"] == res2.n_inliers
            # the last frame's flags start from what the first call left there
            check_call(second, res2, idx, before, idx, first[5], sc["compute_marg"])
        assert off == len(raw)
    finally:
        opt.close()
        klt.close()
