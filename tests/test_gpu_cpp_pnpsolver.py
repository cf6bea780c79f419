"""USLAM::PnPsolver (include/uvo/compat/PnPsolver.h) driven from a C++ program through the C ABI, the way Tracking::Relocalisation
would drive it: the reference's loop as it stands (iterate(5) solver by solver) and the same loop as one library call per round
(USLAM::IterateCandidates) have to give the same candidate, pose, inliers and discards -- and the pose the Python binding gives for the
same session, which tests/test_gpu_pnpsolver.py holds to the host build and the model."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import host_build
import pnpsolver_model as psm

LEVELS = (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)


def build_driver():
    return host_build.build("compat_pnpsolver")


def test_pnpsolver_driver_compiles_as_cxx11(uvo):
    """The adaptor instantiates over frame / map point stand-ins in the reference's dialect, warnings as errors."""
    assert os.path.exists(build_driver())


def _scene(spec):
    """Candidates on disjoint key ranges of one frame, with a null and a bad match in front of each range's points."""
    cands = [psm.candidate(seed, n, ratio) for seed, n, ratio in spec]
    nkeys = sum(len(c[0]) + 2 for c in cands)
    keys = np.zeros(nkeys, [("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4"), ("class_id", "i4")])
    flags, xyz = np.zeros((len(cands), nkeys), np.int32), np.zeros((len(cands), nkeys, 3), np.float32)
    K, off, out = cands[0][5], 0, []
    for j, (p3d, p2d, sigma2, _, _, _, R, t) in enumerate(cands):
        n = len(p3d)
        flags[j, off + 1] = 2                                   # a bad map point; off + 0 stays null
        xyz[j, off + 1] = p3d[0]
        idx = off + 2 + np.arange(n)
        keys["x"][idx], keys["y"][idx] = p2d[:, 0], p2d[:, 1]
        keys["octave"][idx] = np.argmin(np.abs(LEVELS[None, :] - sigma2[:, None]), 1)
        flags[j, idx], xyz[j, idx] = 1, p3d
        out.append((p3d, p2d, LEVELS[keys["octave"][idx]], idx.astype(np.int32), nkeys, K, R, t))
        off += n + 2
    blob = struct.pack("<ii4f", nkeys, len(cands), *K) + LEVELS.tobytes() + keys.tobytes()
    for j in range(len(cands)):
        rec = np.zeros(nkeys, [("flag", "i4"), ("p", "f4", 3)])
        rec["flag"], rec["p"] = flags[j], xyz[j]
        blob += rec.tobytes()
    return out, nkeys, blob


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [((41, 15, 0.2), (42, 9, 1.0), (43, 40, 0.7), (44, 64, 0.9)),      # the third returns
                                  ((51, 15, 0.2), (52, 20, 0.2), (53, 10, 0.3)),                    # nobody does: all discarded
                                  ((61, 64, 0.8),)], ids=("third_returns", "all_exhausted", "single"))
def test_cpp_relocalisation_loop(uvo, tmp_path, spec):
    cands, nkeys, blob = _scene(spec)
    scene_p, out_p = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    with open(scene_p, "wb") as f:
        f.write(blob)
    r = subprocess.run([build_driver(), scene_p, out_p], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    said = json.loads(r.stdout.strip().splitlines()[-1])
    raw = open(out_p, "rb").read()
    C, size = len(cands), 16 + 64 + nkeys + len(cands)
    assert len(raw) == 2 * size
    modes = []
    for m in range(2):
        b = raw[m * size:(m + 1) * size]
        modes.append((struct.unpack_from("<4i", b, 0), np.frombuffer(b, np.float32, 16, 16).reshape(4, 4), np.frombuffer(b, np.uint8, nkeys, 80),
                      np.frombuffer(b, np.uint8, C, 80 + nkeys)))
    (ha, Ta, ma, da), (hb, Tb, mb, db) = modes
    assert ha == hb and Ta.tobytes() == Tb.tobytes() and (ma == mb).all() and (da == db).all(), (said, ha, hb)
    assert said["by_solver"] == list(ha[:3]) and said["one_call"] == list(hb[:3])
    # the same session through the Python binding
    klt = uvo.KLT(64, 64, max_points=16)
    pset = uvo.PnPsolverSet(klt, C, nkeys)
    for (p3d, p2d, sigma2, kp, nm, K, _, _) in cands:
        pset.add(p3d, p2d, sigma2, kp, nm, K)
    rng, alive, res, rounds = uvo.GlibcRand(1), list(range(C)), None, 0
    while alive and (res is None or res.returned < 0):
        res = pset.iterate(alive, 5, rng)
        rounds += 1
        alive = [i for j, i in enumerate(alive) if not (res.status[j][0] and res.status[j][1])]
    pset.close()
    klt.close()
    assert (res.solver, res.n_inliers, rounds, len(alive)) == ha, (res.solver, res.n_inliers, rounds, len(alive), ha)
    assert res.Tcw.tobytes() == Ta.tobytes()
    if res.returned >= 0:
        np.testing.assert_array_equal(res.inliers, ma)
    if len(spec) == 4:
        assert ha[0] == 2
    if len(spec) == 3:
        assert ha[0] == -1 and ha[3] == 0 and da.all()
