"""USLAM::Sim3Solver (include/uvo/compat/Sim3Solver.h) driven from a C++ program through the C ABI, the way LoopClosing::ComputeSim3
would drive it: the reference's loop as it stands (iterate(5) solver by solver) and the same loop as one library call per stretch of
candidates (USLAM::IterateCandidates) have to give the same candidate, transform, inliers and discards -- and what the Python binding
gives for the same session, which tests/test_gpu_sim3solver.py holds to the host build and the model."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import host_build
import sim3_model as sm

LEVELS = (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)


def build_driver():
    return host_build.build("compat_sim3solver")


def test_sim3solver_driver_compiles_as_cxx11(uvo):
    """The adaptor instantiates over key frame / map point stand-ins in the reference's dialect, warnings as errors."""
    assert os.path.exists(build_driver())


def _scene(spec, accept):
    """Every candidate on nkeys slots of its own pair of key frames: a missing match, two bad points and a slot where the first key
    frame has no point in front of the candidate's correspondences, which keep their order."""
    cands = [sm.candidate(seed, n, ratio, noise) for seed, n, ratio, noise in spec]
    nkeys = max(len(c[0]) for c in cands) + 4
    blob = struct.pack("<iii", nkeys, len(cands), accept) + LEVELS.tobytes()
    out = []
    for (x1w, x2w, sg1, sg2, _, _, kf1, kf2, _) in cands:
        n = len(x1w)
        rec = np.zeros(nkeys, [("flag", "i4"), ("x1", "f4", 3), ("x2", "f4", 3), ("o1", "i4"), ("o2", "i4")])
        rec["flag"][:4] = [0, 2, 3, 4]
        rec["x1"][:4], rec["x2"][:4] = x1w[0], x2w[0]
        idx = 4 + np.arange(n)
        rec["flag"][idx], rec["x1"][idx], rec["x2"][idx] = 1, x1w, x2w
        rec["o1"][idx] = np.argmin(np.abs(LEVELS[None, :] - sg1[:, None]), 1)
        rec["o2"][idx] = np.argmin(np.abs(LEVELS[None, :] - sg2[:, None]), 1)
        for kf in (kf1, kf2):
            blob += np.concatenate([kf[0].reshape(9), kf[1].reshape(3), np.float32(kf[2])]).astype(np.float32).tobytes()
        blob += rec.tobytes()
        out.append((x1w, x2w, LEVELS[rec["o1"][idx]], LEVELS[rec["o2"][idx]], idx.astype(np.int32), nkeys, kf1, kf2))
    return out, nkeys, blob


@pytest.mark.gpu
@pytest.mark.parametrize("spec,accept", [(((41, 5, 0.0, 0.5), (42, 2, 1.0, 0.0), (43, 40, 1.0, 0.0), (44, 64, 0.9, 0.5)), 3),     # the third returns
                                         (((41, 5, 0.0, 0.5), (43, 12, 1.0, 0.0), (44, 64, 0.9, 0.5)), 30),                      # a transform rejected on the way
                                         (((51, 3, 0.0, 0.5), (52, 4, 0.0, 0.5)), 1000),                                         # nobody is accepted: all discarded
                                         (((61, 64, 0.8, 0.5),), 3)], ids=("third_returns", "rejected_then_accepted", "all_exhausted", "single"))
def test_cpp_compute_sim3_loop(uvo, tmp_path, spec, accept):
    cands, nkeys, blob = _scene(spec, accept)
    scene_p, out_p = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    with open(scene_p, "wb") as f:
        f.write(blob)
    r = subprocess.run([build_driver(), scene_p, out_p], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    said = json.loads(r.stdout.strip().splitlines()[-1])
    raw = open(out_p, "rb").read()
    C, size = len(cands), 16 + 116 + nkeys + len(cands)
    assert len(raw) == 2 * size
    modes = []
    for m in range(2):
        b = raw[m * size:(m + 1) * size]
        modes.append((struct.unpack_from("<4i", b, 0), np.frombuffer(b, np.float32, 29, 16), np.frombuffer(b, np.uint8, nkeys, 132),
                      np.frombuffer(b, np.uint8, C, 132 + nkeys)))
    (ha, Ta, ma, da), (hb, Tb, mb, db) = modes
    assert ha == hb and Ta.tobytes() == Tb.tobytes() and (ma == mb).all() and (da == db).all(), (said, ha, hb)
    assert said["by_solver"] == list(ha[:3]) and said["one_call"] == list(hb[:3])
    # the same session through the Python binding
    matcher = uvo.ORBmatcher(0.8)
    sset = uvo.Sim3SolverSet(matcher, C, nkeys)
    for c in cands:
        sset.add(*c, uvo.Sim3SolverParams())
    rng, discarded, res, rounds, match = uvo.GlibcRand(1), [False] * C, None, 0, False
    while discarded.count(False) > 0 and not match and rounds < 100:
        rounds += 1
        first = 0
        while True:
            ids = [i for i in range(first, C) if not discarded[i]]
            if not ids:
                break
            res = sset.iterate(ids, 5, rng)
            for j, i in enumerate(ids):
                if res.status[j][0] and res.status[j][1]:
                    discarded[i] = True
            if res.returned < 0:
                break
            if res.n_inliers >= accept:
                match = True
                break
            first = res.solver + 1
    sset.close()
    matcher.close()
    got = (res.solver, res.n_inliers) if match else (-1, 0)
    assert got + (rounds, discarded.count(False)) == ha, (got, rounds, discarded, ha)
    np.testing.assert_array_equal(np.array(discarded, np.uint8), da)
    if match:
        assert np.concatenate([res.T12.reshape(16), res.R.reshape(9), res.t, [res.s]]).astype(np.float32).tobytes() == Ta.tobytes()
        np.testing.assert_array_equal(res.inliers, ma)
    else:
        assert not Ta.any() and not ma.any()
    if len(spec) == 4:
        assert ha[0] == 2
    if accept == 30:
        assert ha[0] == 2
    if accept == 1000:
        assert ha[0] == -1 and ha[3] == 0 and da.all()
