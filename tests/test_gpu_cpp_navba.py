"""USLAM::Optimizer::LocalBundleAdjustmentNavState (include/uvo/compat/Optimizer.h) driven from a C++11 program through the C ABI over a
hand-built map -- a window of 3, the key frame before it, a covisible fixed key frame, a bad observer, a point flagged after the
gathering, one forward and one backward depth entry and one entry that yields no edge -- against the Python binding on the problem the
gathering must produce (which tests/test_gpu_navba.py holds to the host build and the model): lists, marks, states, poses, points,
erasures of the final check only, the mutex and the map-update flag."""
import os
import struct
import subprocess

import numpy as np
import pytest

import navba_checks as pc
import navba_model as vm
import navopt_model as nm

INV_LEVELS = (1.0 / (1.2 ** np.arange(8)) ** 2).astype(np.float32)
INI_DEPTH, DEPTH_COV = 0.25, 0.05
IDS = (11, 12, 13, 10, 5, 6)          # mnId: the window, the key frame before it, the covisible one, the bad observer
UNMARKED = 1000000
CUR = 13                             # pCurKF->mnId, the mark of the gathering


def build_driver():
    return pc.build("compat_navba")


def test_navba_driver_compiles_as_cxx11(uvo):
    assert os.path.exists(build_driver())


def the_map():
    """tests/navba_model.py's scene of 3 + 1 + 2 key frames and 12 points seen by all, as a map: key frame 5 is bad, point 7 reports bad once
    the gathering has marked it and carries a gross outlier, point 9 is bad from the start, key frame 1 (mnId 12) has a depth entry near its
    own time (forward) and one near key frame 0's (backward in time, but minKFID + 1 < pKF0->mnId fails: no edge), key frame 2 (mnId 13)
    one near key frame 1's time (backward)."""
    sc = vm.scene(41, 3, 2, 12, vm.sees_all, shifted=0.15)
    sc["edge_obs"][int(sc["begin"][7])] += np.float32(50.0)
    T = np.zeros(6)
    T[3] = 0.0
    T[0], T[1], T[2] = np.cumsum(sc["links"]["dT"])
    T[4], T[5] = -1.0, -2.0
    depth = {1: [(0.7, T[1] - 0.1 * (T[1] - T[0])), (0.6, T[0] + 0.1 * (T[1] - T[0]))], 2: [(0.8, T[1] + 0.1 * (T[2] - T[1]))]}
    return sc, T, depth


def write_scene(path, sc, T, depth, stop=0, fixed_id=-1, prev_of_first=3):
    a = vm.arrays(sc)
    K, P = len(a["st"]), len(a["pts"])
    Tbc = np.eye(4)
    Tbc[:3, :3], Tbc[:3, 3] = a["Rbc"], a["Pbc"]
    out = [struct.pack("<6i", 2, K, P, 3, fixed_id, stop), np.array([INI_DEPTH, DEPTH_COV] + list(Tbc.reshape(16)) + [a["gyr_rw2"], a["acc_rw2"]], np.float64).tobytes(),
           a["gw"].astype(np.float32).tobytes(), INV_LEVELS.tobytes(), np.array([0, 1, 2], np.int32).tobytes()]
    prev = {0: prev_of_first, 1: 0, 2: 1}
    keys = {k: [] for k in range(K)}
    for e in range(len(a["ekf"])):
        octave = int(round(np.log(1.0 / a["w"][e]) / (2 * np.log(1.2))))
        assert INV_LEVELS[octave] == a["w"][e]
        keys[int(a["ekf"][e])].append((a["obs"][e], octave, int(a["ept"][e])))
    for k in range(K):
        pre = np.zeros(142)
        if k < 3:
            lk = a["links"][k]
            pre = np.concatenate([[lk["dT"]], lk["dP"], lk["dV"], lk["dR"], lk["JPg"], lk["JPa"], lk["JVg"], lk["JVa"], lk["JRg"], lk["cov"]])
        d = depth.get(k, [])
        out += [struct.pack("<3i", IDS[k], 1 if k == 5 else 0, prev.get(k, -1)), a["st"][k].tobytes(), struct.pack("<d", T[k]), a["cams"][k % 2].tobytes(),
                pre.astype(np.float64).tobytes(), struct.pack("<i", len(d)), np.array([x[0] for x in d], np.float64).tobytes(), np.array([x[1] for x in d], np.float64).tobytes(),
                struct.pack("<i", len(keys[k]) + 1), struct.pack("<2f2i", 5.0, 5.0, 0, -1)]        # key 0 of every key frame has no map point
        out += [struct.pack("<2f2i", float(o[0]), float(o[1]), oc, j) for o, oc, j in keys[k]]
    for j in range(P):
        out.append(struct.pack("<2i3f", 1 if j == 9 else 0, 1 if j == 7 else 0, *[float(v) for v in a["pts"][j]]))
    with open(path, "wb") as fh:
        fh.write(b"".join(out))
    return keys


def read_out(path, sc, keys):
    K, P = len(sc["states"]), len(sc["points"])
    with open(path, "rb") as fh:
        b = fh.read()
    o = dict(zip(("ret", "flag", "locks", "K", "P", "E", "L", "D"), struct.unpack_from("<8i", b, 0)))
    pos = 32
    if o["ret"] == 0:
        for name, dt, n in (("begin", np.int32, o["P"] + 1), ("edge_kf", np.int32, o["E"]), ("edge_index", np.int32, o["E"]), ("excluded", np.uint8, o["E"]),
                            ("erased", np.uint8, o["E"]), ("links", np.int32, 2 * o["L"]), ("depth", vm.DEPTH_DTYPE, o["D"])):
            o[name] = np.frombuffer(b, dt, n, pos).copy()
            pos += o[name].nbytes
    o["kf"] = []
    for k in range(K):
        marks = struct.unpack_from("<4i", b, pos)
        ns = np.frombuffer(b, np.float64, 22, pos + 16)
        Tcw = np.frombuffer(b, np.float32, 16, pos + 16 + 176).reshape(4, 4)
        n = len(keys[k]) + 1
        mp = np.frombuffer(b, np.int32, n, pos + 16 + 176 + 64)
        pos += 16 + 176 + 64 + 4 * n
        o["kf"].append(dict(marks=marks, ns=ns, T=Tcw, mp=mp))
    o["mp"] = []
    for j in range(P):
        marks = struct.unpack_from("<3i", b, pos)
        p = np.frombuffer(b, np.float32, 3, pos + 12)
        n = struct.unpack_from("<i", b, pos + 24)[0]
        obs = np.frombuffer(b, np.int32, n, pos + 28)
        pos += 28 + 4 * n
        o["mp"].append(dict(marks=marks, pos=p, obs=obs))
    assert pos == len(b)
    return o


def run(tmp_path, sc, T, depth, **kw):
    scene, out = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    keys = write_scene(scene, sc, T, depth, **kw)
    r = subprocess.run([build_driver(), scene, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return read_out(out, sc, keys), keys


def expected_problem(sc, T, depth):
    """What the gathering must hand to the library: key frames 0..4 (the bad observer is no vertex), points 0..8, 10, 11 (point 9 is bad),
    point 7 flagged, every point's edges in key-frame order, the links of the window in list order, and the depth entries by the rule."""
    keep_pt = [j for j in range(12) if j != 9]
    a = vm.arrays(sc)
    keep = np.array([a["ekf"][e] != 5 and a["ept"][e] != 9 for e in range(len(a["ekf"]))])
    q = vm.prune(sc, keep)
    counts = np.diff(q["begin"])[keep_pt]
    q["begin"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    q["points"], q["point_bad"] = sc["points"][keep_pt], np.array([1 if j == 7 else 0 for j in keep_pt], np.uint8)
    q["states"], q["fixed"], q["has_bias"] = sc["states"][:5], sc["fixed"][:5], sc["has_bias"][:5]
    dep = np.zeros(2, vm.DEPTH_DTYPE)

    def info(shi, link, kf_rot):
        R, C = nm.rot(nm.qnorm(a["st"][kf_rot][6:10])), a["links"][link]["cov"].reshape(9, 9)
        cov3 = 0.0
        for i in range(3):
            for j in range(3):
                cov3 = cov3 + (R[i, 2] * C[i, j]) * R[j, 2]
        cov1 = (shi * shi * DEPTH_COV * DEPTH_COV) + cov3
        return 1 / (cov1 * cov1)

    (m0, t0), _ = depth[1]                                  # forward: (pKF1 = 1, pKF0 = 0, pKF0), pKF1's preintegration
    shi = (T[1] - T[0]) / (t0 - T[0])
    dep[0] = (1, 0, 0, 1, shi, m0 - INI_DEPTH, info(shi, 1, 0))
    (m1, t1), = depth[2]                                    # backward: (pKF0 = 1, pKF_1 = 0, pKF_1), pKF_1's preintegration
    shi = (T[1] - T[0]) / (t1 - T[0])
    dep[1] = (1, 0, 0, 0, shi, m1 - INI_DEPTH, info(shi, 0, 0))
    q["depth"] = dep
    q["gw"] = np.asarray(sc["gw"], np.float32).astype(np.float64)       # Converter::toVector3d of the float cv::Mat
    return q, keep_pt


@pytest.mark.gpu
def test_cpp_local_bundle_adjustment_nav_state(uvo, tmp_path):
    sc, T, depth = the_map()
    got, keys = run(tmp_path, sc, T, depth)
    q, keep_pt = expected_problem(sc, T, depth)
    assert (got["ret"], got["flag"], got["locks"]) == (0, 1, 10) and (got["K"], got["P"], got["L"], got["D"]) == (5, 11, 3, 2)
    assert np.array_equal(got["begin"], q["begin"]) and np.array_equal(got["edge_kf"], q["edge_kf"]) and got["links"].tolist() == [3, 0, 0, 1, 1, 2]
    for f in vm.DEPTH_DTYPE.names:
        assert np.array_equal(got["depth"][f], q["depth"][f]), f
    m = uvo.ORBmatcher(0.8)
    adj = uvo.NavBundleAdjuster(m, 8, 16, 512, 4096, 16)
    want = adj.adjust(q)
    adj.close()
    assert want.n_excluded > 0 and want.n_erased > 0
    assert np.array_equal(got["excluded"], want.excluded) and np.array_equal(got["erased"], want.erased)
    flagged = int(q["begin"][keep_pt.index(7)])
    assert want.excluded[flagged] == 0 and want.erased[flagged] == 0
    for k in range(6):
        kf = got["kf"][k]
        local, fixed = (CUR if k < 3 else UNMARKED), (CUR if k >= 3 else UNMARKED)
        assert kf["marks"][:2] == (local, fixed), k
        if k < 3:
            assert kf["marks"][2:] == (1, 5) and pc.same_bits(kf["T"], want.kf_Tcw[k])
            w = want.kf_state[k]
            assert pc.same_bits(kf["ns"][:10], w[:10]) and pc.same_bits(kf["ns"][16:], w[16:]) and pc.same_bits(kf["ns"][10:16], np.asarray(sc["states"])[k][10:16])
        else:
            assert kf["marks"][2:] == (0, 0) and pc.same_bits(kf["ns"], np.asarray(sc["states"], np.float64)[k])
    # erasures: the final check's only, in the key frame and in the point
    e = 0
    for jj, j in enumerate(keep_pt):
        for e in range(int(q["begin"][jj]), int(q["begin"][jj + 1])):
            k = int(q["edge_kf"][e])
            idx = [i for i, (_, _, p) in enumerate(keys[k]) if p == j][0] + 1
            assert got["edge_index"][e] == idx
            assert (got["kf"][k]["mp"][idx] == -1) == bool(want.erased[e]) and (k not in got["mp"][j]["obs"]) == bool(want.erased[e]), (j, k)
    for jj, j in enumerate(keep_pt):
        assert got["mp"][j]["marks"] == (CUR, 1, 1) and pc.same_bits(got["mp"][j]["pos"], want.points[jj]), j
    assert got["mp"][9]["marks"] == (UNMARKED, 0, 0) and 5 in got["mp"][0]["obs"]      # the bad observer keeps its observations


@pytest.mark.gpu
def test_cpp_stop_flag_fixed_id_and_missing_previous_key_frame(uvo, tmp_path):
    sc, T, depth = the_map()
    got, _ = run(tmp_path, sc, T, depth, stop=1)
    assert (got["ret"], got["flag"], got["locks"]) == (1, 0, 0) and got["kf"][0]["marks"] == (CUR, UNMARKED, 0, 0) and got["mp"][0]["marks"] == (CUR, 0, 0)
    got, _ = run(tmp_path, sc, T, depth, prev_of_first=-1)
    assert (got["ret"], got["flag"], got["locks"]) == (-1, 0, 0) and got["kf"][0]["marks"][2:] == (0, 0)
    got, _ = run(tmp_path, sc, T, depth, fixed_id=11)           # window key frame 0 fixed by its id: its state comes back as it went in
    assert got["ret"] == 0 and pc.same_bits(got["kf"][0]["ns"][:6], np.asarray(sc["states"], np.float64)[0][:6]) and got["kf"][0]["marks"][2:] == (1, 5)
    assert not pc.same_bits(got["kf"][1]["ns"][:6], np.asarray(sc["states"], np.float64)[1][:6])
