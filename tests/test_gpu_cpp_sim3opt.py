"""USLAM::Optimizer::OptimizeSim3 (include/uvo/compat/Optimizer.h) driven from a C++11 program through the C ABI, over stub key-frame
and map-point types and a vpMatches1 that holds every kind of entry the reference's walk distinguishes: its return value, its Sim3 and
the entries it nulls have to equal the Python binding's for the gathered pairs (which tests/test_gpu_sim3opt.py holds to the host build
and the model).  Checked besides: a skipped match keeps its entry; e21 is weighted with GetSigma2 (the variance); S12 is untouched on
the early return; the list overload (one device call) equals the single calls."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import host_build
import sim3opt_model as sm

_SIG = np.float32(1.2) ** np.arange(8)
SIGMA2 = (_SIG * _SIG).astype(np.float32)
INV_SIGMA2 = (1.0 / (_SIG * _SIG)).astype(np.float32)
REC = np.dtype([("kind", "<i4"), ("xw", "<f4", 3), ("kp", "<f4", 2), ("octave", "<i4")])


def build_driver():
    return host_build.build("compat_sim3opt")


def test_sim3opt_driver_compiles_as_cxx11(uvo):
    """The adaptor instantiates over key-frame / map-point stand-ins in the reference's dialect, warnings as errors."""
    assert os.path.exists(build_driver())


def kf_bytes(kf):
    return np.ascontiguousarray(kf[0], np.float32).tobytes() + np.ascontiguousarray(kf[1], np.float32).tobytes() + np.asarray(kf[2], np.float32).tobytes()


@pytest.mark.gpu
def test_cpp_optimize_sim3(uvo, tmp_path):
    base = sm.scene(seed=700, n=40, shifted2=6)
    n = 40
    # candidate 0: the scene; 1: the same pairs from another start and with other pairs shifted; 2: key frame 2 of an unrelated scene --
    # nothing fits, every pair is bad, the early return
    other, far = dict(base), sm.scene(seed=701, n=n)
    other["obs2"] = base["obs2"].copy()
    other["obs2"][20:25] += np.float32(9.0)
    other["R12"], other["t12"], other["s12"] = (sm.rot_of_vec(np.array([0.01, -0.02, 0.01])) @ base["R12"]).astype(np.float32), base["t12"] + np.float32(0.02), base["s12"] * np.float32(0.98)
    unrelated = dict(base)
    for k in ("x2w", "obs2", "info2", "kf2"):
        unrelated[k] = far[k]
    cands = [base, other, unrelated]
    g = np.random.default_rng(5)
    N = n + 10
    idx = np.sort(g.choice(N, n, replace=False))                    # where the pairs are
    extra = np.setdiff1d(np.arange(N), idx)
    kinds = [(2, 1), (3, 1), (1, 4), (1, 5), (1, 0)]                # (kind in key frame 1, kind in the candidate): five ways to be skipped
    k1 = np.zeros(N, REC)
    k1["kind"], k1["xw"], k1["kp"] = 1, g.normal(size=(N, 3)), g.uniform(0, 400, (N, 2))
    k1["xw"][idx], k1["kp"][idx] = base["x1w"], base["obs1"]
    k1["octave"][idx] = np.argmin(np.abs(INV_SIGMA2[None, :] - base["info1"][:, None]), 1)
    assert (INV_SIGMA2[k1["octave"][idx]] == base["info1"]).all()
    for e, i in enumerate(extra):
        k1["kind"][i] = kinds[e % 5][0]
    blob = struct.pack("<if", len(cands), float(base["th2"])) + SIGMA2.tobytes() + INV_SIGMA2.tobytes() + kf_bytes(base["kf1"]) + struct.pack("<i", N) + k1.tobytes()
    before = []
    for c in cands:
        k2 = np.zeros(N, REC)
        k2["kind"], k2["xw"], k2["kp"] = 1, g.normal(size=(N, 3)), g.uniform(0, 400, (N, 2))
        k2["xw"][idx], k2["kp"][idx] = c["x2w"], c["obs2"]
        k2["octave"][idx] = np.argmin(np.abs(SIGMA2[None, :] - c["info2"][:, None]), 1)
        assert (SIGMA2[k2["octave"][idx]] == c["info2"]).all() and (c["info2"] != INV_SIGMA2[k2["octave"][idx]]).any()     # the variance, and it matters
        for e, i in enumerate(extra):
            k2["kind"][i] = kinds[e % 5][1]
        before.append((k2["kind"] == 0).astype(np.uint8))
        blob += kf_bytes(c["kf2"]) + np.ascontiguousarray(c["R12"], np.float32).tobytes() + np.ascontiguousarray(c["t12"], np.float32).tobytes()
        blob += struct.pack("<f", float(c["s12"])) + k2.tobytes()
    scene_p, out_p = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    with open(scene_p, "wb") as f:
        f.write(blob)
    r = subprocess.run([build_driver(), scene_p, out_p], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1])["candidates"] == 3
    raw = open(out_p, "rb").read()
    rec = 4 + 64 + N
    assert len(raw) == 2 * len(cands) * rec
    got = []
    for j in range(2 * len(cands)):
        o = j * rec
        got.append((struct.unpack_from("<i", raw, o)[0], np.frombuffer(raw, np.float64, 8, o + 4), np.frombuffer(raw, np.uint8, N, o + 68)))
    # the same problems through the Python binding, one call
    m = uvo.ORBmatcher(0.8)
    opt = uvo.Sim3Optimizer(m, 3, N)
    res = opt.optimize(cands)
    opt.close()
    for j, (c, want) in enumerate(zip(cands, res)):
        for ret, est, null in (got[j], got[len(cands) + j]):                 # the list overload, then the single call
            assert ret == want.n_inliers, j
            assert null[idx].tobytes() == want.removed.tobytes(), j          # exactly the bad pairs are nulled
            assert null[extra].tobytes() == before[j][extra].tobytes(), j    # a skipped match keeps its entry; a null one stays null
            if want.more_iterations:
                assert est.tobytes() == np.concatenate([want.q, want.t, [want.s]]).tobytes(), j
            else:
                start = sm.sim_from_floats(c["R12"], c["t12"], c["s12"]).vec()
                assert ret == 0 and est.tobytes() == start.tobytes() == np.concatenate([want.q, want.t, [want.s]]).tobytes(), j   # S12 untouched
    assert res[0].n_inliers >= 30 and res[0].removed.any() and res[1].n_inliers >= 25 and res[2].more_iterations == 0
    assert (res[0].removed != res[1].removed).any()
