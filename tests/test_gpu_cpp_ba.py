"""USLAM::Optimizer::LocalBundleAdjustment / BundleAdjustment / GlobalBundleAdjustemnt / RecoveryBundleAdjustemnt
(include/uvo/compat/Optimizer.h) driven from a C++11 program through the C ABI, over stub key-frame, map-point, map and local-mapper
types.  Three things are checked: the adaptor's gathering, against a literal Python restatement of src/Optimizer.cc:2149-2198 (and of
:1914-1978 for the full mode) on the same graph -- the marks, the order of key frames, points and edges; the erasures of both checks;
and the write-back (SetPose on the local key frames only, SetWorldPos and UpdateNormalAndDepth once per point, under the map's mutex,
the map-update flag).  The numbers have to equal the Python binding's for the gathered problem, which tests/test_gpu_ba.py holds to the
host build and the model."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ba_model as bm
import host_build

INV_SIGMA2 = (1.0 / (np.float32(1.2) ** np.arange(8)) ** 2).astype(np.float32)
UNSET = 1000000
IDS = [3, 0, 5, 6, 7, 8, 9, 10, 11]        # mnId of key frame k: key frame 1, a local one, is the map's first


def build_driver():
    return host_build.build("compat_ba")


def test_ba_driver_compiles_as_cxx11(uvo):
    """The adaptors instantiate over key-frame / map-point / map stand-ins in the reference's dialect, warnings as errors."""
    assert os.path.exists(build_driver())


def graph():
    """Key frames 0..4 are the current one and its covisibles, 5..7 see local points without being covisible, 8 is a BAD covisible that
    also observes points; 60 points from the model's generator, a bad point seen by key frames 0 and 1, a point seen only by 5 and 6;
    null matches in between; the keys of a key frame in shuffled order."""
    sc = bm.scene(41, 5, 3, 60, bm.sees_random(4, 41), shifted=0.1)
    g = np.random.RandomState(5)
    K, P = 9, 62
    T = np.concatenate([sc["Tcw"], sc["Tcw"][:1]]).reshape(K, 3, 4)
    keys = [[] for _ in range(K)]
    ept = np.repeat(np.arange(60), np.diff(sc["begin"]))
    for e, k in enumerate(sc["edge_kf"]):
        keys[k].append((float(sc["edge_obs"][e, 0]), float(sc["edge_obs"][e, 1]), int(g.randint(0, 4)), int(ept[e])))
    for k in (0, 1):
        keys[k].append((100.0 + k, 120.0, 1, 60))                 # the bad point
    for k in (5, 6):
        keys[k].append((200.0 + k, 220.0, 0, 61))                 # seen by no local key frame
    for j in (3, 7, 11):
        keys[8].append((50.0 + j, 60.0, 2, j))                    # the bad key frame observes local points
    for k in range(K):
        for n in range(3):
            keys[k].append((10.0 * n, 5.0, 0, -1))                # no map point
        order = g.permutation(len(keys[k]))
        keys[k] = [keys[k][i] for i in order]
    kfs = [dict(mnId=IDS[k], bad=k == 8, R=T[k][:, :3].copy(), t=T[k][:, 3].copy(), K=sc["cameras"][k % 2].copy(), keys=keys[k],
                cov=[2, 8, 1, 4, 3] if k == 0 else []) for k in range(K)]
    pos = np.concatenate([sc["points"], np.float32([[0.1, 0.2, 5.0], [0.3, -0.2, 6.0]])])
    mps = [dict(bad=j == 60, pos=pos[j].copy()) for j in range(P)]
    return kfs, mps


def write_scene(path, kfs, mps, what, current=0, other=1, n_iterations=0, stop=0):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<7i", what, current, other, n_iterations, stop, len(kfs), len(mps)) + INV_SIGMA2.tobytes())
        for kf in kfs:
            fh.write(struct.pack("<2i", kf["mnId"], int(kf["bad"])) + kf["R"].astype(np.float32).tobytes() + kf["t"].astype(np.float32).tobytes() +
                     kf["K"].astype(np.float32).tobytes() + struct.pack("<i", len(kf["keys"])))
            for x, y, o, mp in kf["keys"]:
                fh.write(struct.pack("<2f2i", x, y, o, mp))
            fh.write(struct.pack("<i", len(kf["cov"])) + struct.pack("<%di" % len(kf["cov"]), *kf["cov"]))
        for mp in mps:
            fh.write(struct.pack("<i", int(mp["bad"])) + mp["pos"].astype(np.float32).tobytes())


def read_out(path, kfs, mps):
    buf = open(path, "rb").read()
    off = [0]

    def take(dtype, n):
        a = np.frombuffer(buf, dtype, n, off[0])
        off[0] += a.nbytes
        return a
    o = {}
    o["ret"], o["flag"], o["locks"], K, P, E = [int(v) for v in take("<i4", 6)]
    o["K"], o["P"], o["E"] = K, P, E
    if o["ret"] == 0:
        o["begin"], o["edge_kf"], o["edge_index"], o["removed1"], o["removed2"] = take("<i4", P + 1), take("<i4", E), take("<i4", E), take("u1", E), take("u1", E)
    o["kf"] = []
    for kf in kfs:
        local, fixed, n_set = [int(v) for v in take("<i4", 3)]
        o["kf"].append(dict(local=local, fixed=fixed, n_set=n_set, T=take("<f4", 16).reshape(4, 4), mp=take("<i4", len(kf["keys"]))))
    o["mp"] = []
    for _ in mps:
        local, n_set, n_up = [int(v) for v in take("<i4", 3)]
        pos = take("<f4", 3)
        o["mp"].append(dict(local=local, n_set=n_set, n_up=n_up, pos=pos, obs=take("<i4", int(take("<i4", 1)[0])).tolist()))
    assert off[0] == len(buf)
    return o


def observations(kfs, j):
    """GetObservations() of point j: a std::map keyed by the key frame's address, so it iterates in key-frame order."""
    return [(k, i) for k, kf in enumerate(kfs) for i, key in enumerate(kf["keys"]) if key[3] == j]


def problem_of(kfs, mps, vertices, fixed, points):
    """The edges of :2261-2307 / :1934-1978 for the given vertices and points -> the library's scene, every edge's key frame and key."""
    cams, begin, ekf, obs, w, ecam, where = [], [0], [], [], [], [], []
    for j in points:
        for k, i in observations(kfs, j):
            if kfs[k]["bad"] or k not in vertices:
                continue
            x, y, o, _ = kfs[k]["keys"][i]
            cam = tuple(np.float32(kfs[k]["K"]).tolist())
            if cam not in cams:
                cams.append(cam)
            ekf.append(vertices.index(k)), obs.append((x, y)), w.append(INV_SIGMA2[o]), ecam.append(cams.index(cam)), where.append((k, i))
        begin.append(len(ekf))
    T = np.stack([np.concatenate([kfs[k]["R"], kfs[k]["t"][:, None]], 1).reshape(12) for k in vertices]).astype(np.float32)
    sc = dict(Tcw=T, fixed=np.uint8(fixed), points=np.float32([mps[j]["pos"] for j in points]), point_bad=np.uint8([mps[j]["bad"] for j in points]),
              begin=np.int32(begin), edge_kf=np.int32(ekf), edge_obs=np.float32(obs).reshape(-1, 2), edge_inv_sigma2=np.float32(w), edge_camera=np.int32(ecam),
              cameras=np.float32(cams))
    return sc, where


def gather_local(kfs, mps, cur):
    """src/Optimizer.cc:2149-2198, line for line, on dictionaries."""
    for d in kfs + mps:
        d["local"], d["fixedmark"] = UNSET, UNSET
    pKF = kfs[cur]
    lLocalKeyFrames = [cur]
    pKF["local"] = pKF["mnId"]
    for i in pKF["cov"]:
        kfs[i]["local"] = pKF["mnId"]
        if not kfs[i]["bad"]:
            lLocalKeyFrames.append(i)
    lLocalMapPoints = []
    for k in lLocalKeyFrames:
        for key in kfs[k]["keys"]:
            j = key[3]
            if j >= 0:
                if not mps[j]["bad"]:
                    if mps[j]["local"] != pKF["mnId"]:
                        lLocalMapPoints.append(j)
                        mps[j]["local"] = pKF["mnId"]
    lFixedCameras = []
    for j in lLocalMapPoints:
        for k, _ in observations(kfs, j):
            if kfs[k]["local"] != pKF["mnId"] and kfs[k]["fixedmark"] != pKF["mnId"]:
                kfs[k]["fixedmark"] = pKF["mnId"]
                if not kfs[k]["bad"]:
                    lFixedCameras.append(k)
    return lLocalKeyFrames, lLocalMapPoints, lFixedCameras


def run(tmp_path, kfs, mps, **kw):
    scene, out = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    write_scene(scene, kfs, mps, **kw)
    r = subprocess.run([build_driver(), scene, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-1000:])
    return read_out(out, kfs, mps)


@pytest.fixture(scope="module")
def adjuster(uvo):
    m = uvo.ORBmatcher(0.8)
    a = uvo.BundleAdjuster(m, 16, 16, 512, 4096)
    yield a
    a.close()


@pytest.mark.gpu
def test_cpp_local_bundle_adjustment(uvo, adjuster, tmp_path):
    kfs, mps = graph()
    got = run(tmp_path, kfs, mps, what=0)
    loc, pts, fix = gather_local(kfs, mps, 0)
    assert loc == [0, 2, 1, 4, 3] and sorted(fix) == [5, 6, 7] and 60 not in pts and 61 not in pts and len(pts) == 57      # the graph is what it is meant to be
    vertices = loc + fix
    sc, where = problem_of(kfs, mps, vertices, [kfs[k]["mnId"] == 0 for k in loc] + [1] * len(fix), pts)
    assert sc["fixed"].tolist() == [0, 0, 1, 0, 0, 1, 1, 1]
    # the gathering
    assert got["ret"] == 0 and (got["K"], got["P"], got["E"]) == (len(vertices), len(pts), len(where))
    assert np.array_equal(got["begin"], sc["begin"]) and np.array_equal(got["edge_kf"], sc["edge_kf"]) and got["edge_index"].tolist() == [i for _, i in where]
    for k, kf in enumerate(kfs):
        assert (got["kf"][k]["local"], got["kf"][k]["fixed"]) == (kf["local"], kf["fixedmark"]), k
    assert [m["local"] for m in got["mp"]] == [m["local"] for m in mps]
    assert got["kf"][8]["local"] == 3 and got["mp"][60]["local"] == UNSET and got["kf"][5]["fixed"] == 3
    # the numbers: the Python binding on the gathered problem
    want = adjuster.adjust(sc)
    assert np.array_equal(got["removed1"], want.removed1) and np.array_equal(got["removed2"], want.removed2)
    assert want.n_removed1 > 0 and want.iterations[0] == 5
    # the erasures of both checks
    erased = {where[e] for e in np.flatnonzero(want.removed1 | want.removed2)}
    for k, kf in enumerate(kfs):
        for i, key in enumerate(kf["keys"]):
            assert got["kf"][k]["mp"][i] == (-1 if (k, i) in erased else key[3]), (k, i)
    for j in range(len(mps)):
        assert got["mp"][j]["obs"] == [k for k, i in observations(kfs, j) if (k, i) not in erased], j
    # the write-back
    for n, k in enumerate(vertices):
        if n < len(loc):
            assert got["kf"][k]["n_set"] == 1 and np.array_equal(got["kf"][k]["T"], want.kf_Tcw[n]), k
        else:
            assert got["kf"][k]["n_set"] == 0 and np.array_equal(got["kf"][k]["T"][:3].reshape(12), sc["Tcw"][n]), k
    assert got["kf"][8]["n_set"] == 0
    for n, j in enumerate(pts):
        assert (got["mp"][j]["n_set"], got["mp"][j]["n_up"]) == (1, 1) and np.array_equal(got["mp"][j]["pos"], want.points[n]), j
    for j in (60, 61):
        assert (got["mp"][j]["n_set"], got["mp"][j]["n_up"]) == (0, 0) and np.array_equal(got["mp"][j]["pos"], mps[j]["pos"])
    assert got["flag"] == 1 and got["locks"] == 10              # locked once, released


@pytest.mark.gpu
def test_cpp_stop_flag_is_read_before_the_call(uvo, tmp_path):
    kfs, mps = graph()
    got = run(tmp_path, kfs, mps, what=0, stop=1)
    gather_local(kfs, mps, 0)
    assert got["ret"] == 1 and got["flag"] == 0 and got["locks"] == 0
    assert [k["local"] for k in got["kf"]] == [k["local"] for k in kfs] and [k["fixed"] for k in got["kf"]] == [k["fixedmark"] for k in kfs]
    assert all(k["n_set"] == 0 for k in got["kf"]) and all(m["n_set"] == 0 and m["n_up"] == 0 for m in got["mp"])
    assert all(got["kf"][k]["mp"].tolist() == [key[3] for key in kf["keys"]] for k, kf in enumerate(kfs))


@pytest.mark.gpu
@pytest.mark.parametrize("what", [1, 2, 3])
def test_cpp_full_bundle_adjustment(uvo, adjuster, tmp_path, what):
    """BundleAdjustment and GlobalBundleAdjustemnt over the whole map, RecoveryBundleAdjustemnt over (key frame 1, key frame 0) and
    key frame 0's matches, 20 iterations: bad key frames and points are no vertices, mnId 0 is fixed, nothing is erased."""
    kfs, mps = graph()
    got = run(tmp_path, kfs, mps, what=what, current=0, other=1, n_iterations=20)
    if what == 3:
        vertices, cand = [1, 0], [key[3] for key in kfs[0]["keys"] if key[3] >= 0]
    else:
        vertices, cand = [k for k in range(len(kfs)) if not kfs[k]["bad"]], list(range(len(mps)))
    pts = [j for j in cand if not mps[j]["bad"]]
    sc, where = problem_of(kfs, mps, vertices, [kfs[k]["mnId"] == 0 for k in vertices], pts)
    assert got["ret"] == 0 and (got["K"], got["P"], got["E"]) == (len(vertices), len(pts), len(where))
    assert np.array_equal(got["begin"], sc["begin"]) and np.array_equal(got["edge_kf"], sc["edge_kf"]) and sum(sc["fixed"]) == 1
    want = adjuster.adjust(sc, uvo.UVO_BA_FULL, 20)
    assert not got["removed1"].any() and not got["removed2"].any() and want.iterations[0] >= 2
    for k, kf in enumerate(kfs):
        assert got["kf"][k]["mp"].tolist() == [key[3] for key in kf["keys"]]                       # nothing is erased
        if k in vertices:
            assert got["kf"][k]["n_set"] == 1 and np.array_equal(got["kf"][k]["T"], want.kf_Tcw[vertices.index(k)]), k
        else:
            assert got["kf"][k]["n_set"] == 0
    for j in range(len(mps)):
        if j in pts:
            assert (got["mp"][j]["n_set"], got["mp"][j]["n_up"]) == (1, 1) and np.array_equal(got["mp"][j]["pos"], want.points[pts.index(j)]), j
        else:
            assert got["mp"][j]["n_set"] == 0
    assert got["flag"] == 0 and got["locks"] == 0
