"""USLAM::Optimizer::OptimizeEssentialGraph (include/uvo/compat/Optimizer.h) driven from a C++11 program through the C ABI, over stub
key-frame, map-point and map types.  Three things are checked: the adaptor's gathering, against a literal Python restatement of the walk
of src/Optimizer.cc:2437-2598 on the same graph -- the vertices in ascending mnId, the edge list in the reference's order of insertion,
the similarities the two kinds of edges measure from, nIDr of every point; the departures (a bad key frame is no vertex and its edges
are skipped, a point whose reference is bad keeps its place, a bad loop key frame ends the call with -1 and nothing touched); and the
write-back, whose numbers have to equal the Python binding's for the gathered problem, which tests/test_gpu_essential.py holds to the
host build and the model."""
import os
import struct
import subprocess

import numpy as np
import pytest

import essential_model as em
import host_build

pytestmark = pytest.mark.gpu

DRIVER = host_build.Artefact("tests/cpp/compat_essential", "tests/cpp/compat_essential.cpp", host_build.CXX, host_build.CXX11, host_build.UVO)
K, LOOP, CUR, BAD = 14, 1, 12, 6


def build_driver():
    return host_build.compile_artefact(DRIVER)


def test_essential_driver_compiles_as_cxx11(uvo):
    """The adaptor instantiates over key-frame / map-point / map stand-ins in the reference's dialect, warnings as errors."""
    assert os.path.exists(build_driver())


def graph(bad_loop=False):
    """14 key frames listed by the map in shuffled order, mnId with gaps; key frame 6 is BAD and is a parent, a loop edge and a covisible of
    others; the current key frame 12 and its neighbours 10, 11 carry CorrectedSim3 / NonCorrectedSim3; LoopConnections joins them to 1, 2
    with weights below and above 100 (the pair (12, 1) passes whatever its weight); covisibles that are the parent, a child, a loop edge,
    an inserted pair, of larger id or below the weight are there to be refused."""
    g = np.random.default_rng(12)
    sc = em._scene(np.random.default_rng(3), K, [(CUR, LOOP)], n_corrected=3, correction=(0.05, 0.3, 1.15))
    kfs = []
    for k in range(K):
        R = em.rotmat(sc["Scwn"][k, :4]).reshape(3, 3).astype(np.float32)
        kfs.append(dict(mnId=3 * k + (k > 7) * 4, bad=(k == BAD) or (bad_loop and k == LOOP), parent=k - 1 if k else -1, R=R, t=sc["Scwn"][k, 4:7].astype(np.float32),
                        loop=[], cov=[], child=[k + 1] if k + 1 < K else [], corrected=None, noncorrected=None, conn=[]))
    for k in (10, 11, 12):
        kfs[k]["corrected"], kfs[k]["noncorrected"] = sc["Scw"][k].copy(), sc["Scwn"][k].copy()
    kfs[9]["loop"], kfs[3]["loop"] = [3, BAD], [9]                      # an older loop: 9 -> 3 is added from 9 only; 9 -> 6 reaches a bad key frame
    kfs[12]["conn"], kfs[11]["conn"], kfs[1]["conn"] = [1, 2], [1, 2], [12]
    kfs[12]["cov"] = [(11, 300), (1, 40), (2, 150), (9, 120), (BAD, 200), (8, 99)]
    kfs[11]["cov"] = [(12, 300), (10, 250), (1, 90), (2, 130), (8, 160)]
    kfs[1]["cov"] = [(12, 40), (2, 400), (0, 350)]
    kfs[9]["cov"] = [(8, 500), (3, 300), (7, 220), (12, 120), (5, 101)]
    kfs[7]["cov"] = [(BAD, 300), (5, 180), (8, 170), (4, 100)]
    kfs[5]["cov"] = [(4, 150), (3, 140)]
    pos = g.normal(size=(24, 3)).astype(np.float32) * 3
    mps = [dict(bad=j == 5, ref=int(g.integers(0, K)) if j not in (7, 8) else BAD, pos=pos[j], by=kfs[CUR]["mnId"] if j % 4 == 0 else 0,
                cref=kfs[10 + j % 3]["mnId"] if j % 4 == 0 else 0) for j in range(24)]
    order = list(g.permutation(K))
    return kfs, mps, order


def write_scene(path, kfs, mps, order):
    """The map lists the key frames in `order`; indices in the file are positions in that list."""
    at = {k: n for n, k in enumerate(order)}
    with open(path, "wb") as fh:
        fh.write(struct.pack("<4i", len(kfs), len(mps), at[LOOP], at[CUR]))
        for k in order:
            kf = kfs[k]
            fh.write(struct.pack("<3i", kf["mnId"], int(kf["bad"]), at[kf["parent"]] if kf["parent"] >= 0 else -1) + kf["R"].tobytes() + kf["t"].tobytes())
            fh.write(struct.pack("<i", len(kf["loop"])) + struct.pack("<%di" % len(kf["loop"]), *[at[l] for l in kf["loop"]]))
            fh.write(struct.pack("<i", len(kf["cov"])) + b"".join(struct.pack("<2i", at[c], w) for c, w in kf["cov"]))
            fh.write(struct.pack("<i", len(kf["child"])) + struct.pack("<%di" % len(kf["child"]), *[at[c] for c in kf["child"]]))
            for s in (kf["corrected"], kf["noncorrected"]):
                fh.write(struct.pack("<i", int(s is not None)) + (b"" if s is None else np.asarray(s, "<f8").tobytes()))
            fh.write(struct.pack("<i", len(kf["conn"])) + struct.pack("<%di" % len(kf["conn"]), *[at[c] for c in kf["conn"]]))
        for mp in mps:
            fh.write(struct.pack("<2i", int(mp["bad"]), at[mp["ref"]]) + mp["pos"].tobytes() + struct.pack("<2i", mp["by"], mp["cref"]))


def read_out(path, kfs, mps, order):
    buf = open(path, "rb").read()
    off = [0]

    def take(dtype, n):
        a = np.frombuffer(buf, dtype, n, off[0])
        off[0] += a.nbytes
        return a
    o = {}
    o["ret"], Kv, E, P, o["iterations"], o["trials"], o["blocks"] = [int(v) for v in take("<i4", 7)]
    o["Scw"], o["Scwn"] = take("<f8", 8 * Kv).reshape(Kv, 8), take("<f8", 8 * Kv).reshape(Kv, 8)
    o["edge_i"], o["edge_j"], o["conn"], o["ref"] = take("<i4", E), take("<i4", E), take("u1", E), take("<i4", P)
    o["kf"] = {}
    for k in order:
        n = int(take("<i4", 1)[0])
        o["kf"][k] = (n, take("<f4", 16).reshape(4, 4))
    o["mp"] = []
    for _ in mps:
        n = take("<i4", 2)
        o["mp"].append((int(n[0]), int(n[1]), take("<f4", 3)))
    assert off[0] == len(buf)
    return o


def gather(kfs, mps, order):
    """src/Optimizer.cc:2437-2598 and :2627-2647 on the graph, with the adaptor's departures -> the scene dict, the vertices (key-frame
    numbers in ascending mnId), the points that are mapped and those that keep their place."""
    vertices = sorted((k for k in range(K) if not kfs[k]["bad"]), key=lambda k: kfs[k]["mnId"])
    index = {k: n for n, k in enumerate(vertices)}

    def from_pose(kf):
        return em._from_floats(kf["R"], kf["t"])
    Scw = np.array([kfs[k]["corrected"] if kfs[k]["corrected"] is not None else from_pose(kfs[k]) for k in vertices])
    Scwn = np.array([kfs[k]["noncorrected"] if kfs[k]["noncorrected"] is not None else Scw[index[k]] for k in vertices])
    edges, inserted = [], set()

    def add(i, j, c):
        if i in index and j in index:
            edges.append((index[i], index[j], c))
            return True
        return False

    def weight(k, other):
        return dict(kfs[k]["cov"]).get(other, 0)
    at = {k: n for n, k in enumerate(order)}
    # LoopConnections: a std::map and std::set over pointers into one vector: the map's listing order
    for k in sorted((k for k in range(K) if kfs[k]["conn"]), key=lambda k: at[k]):
        for l in sorted(kfs[k]["conn"], key=lambda l: at[l]):
            if (k != CUR or l != LOOP) and weight(k, l) < 100:
                continue
            if add(k, l, 1):
                inserted.add((min(kfs[k]["mnId"], kfs[l]["mnId"]), max(kfs[k]["mnId"], kfs[l]["mnId"])))
    for k in order:
        kf = kfs[k]
        if kf["bad"]:
            continue
        if kf["parent"] >= 0:
            add(k, kf["parent"], 0)
        for l in sorted(kf["loop"], key=lambda l: at[l]):
            if kfs[l]["mnId"] < kf["mnId"]:
                add(k, l, 0)
        for n, w in kf["cov"]:
            if w < 100 or n == kf["parent"] or n in kf["child"] or n in kf["loop"]:
                continue
            if not kfs[n]["bad"] and kfs[n]["mnId"] < kf["mnId"]:
                if (min(kf["mnId"], kfs[n]["mnId"]), max(kf["mnId"], kfs[n]["mnId"])) in inserted:
                    continue
                add(k, n, 0)
    by_id = {kfs[k]["mnId"]: k for k in range(K)}
    mapped, kept, ref = [], [], []
    for j, mp in enumerate(mps):
        if mp["bad"]:
            continue
        r = by_id[mp["cref"]] if mp["by"] == kfs[CUR]["mnId"] else mp["ref"]
        if r in index:
            mapped.append(j), ref.append(index[r])
        else:
            kept.append(j)
    sc = dict(Scw=Scw, Scwn=Scwn, edge_i=np.array([e[0] for e in edges], np.int32), edge_j=np.array([e[1] for e in edges], np.int32),
              conn=np.array([e[2] for e in edges], np.uint8), points=np.array([mps[j]["pos"] for j in mapped], np.float32).reshape(-1, 3),
              ref=np.array(ref, np.int32), fixed=index.get(LOOP, -1), n_iterations=20)
    return sc, vertices, mapped, kept


def run(tmp_path, kfs, mps, order):
    scene, out = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    write_scene(scene, kfs, mps, order)
    r = subprocess.run([build_driver(), scene, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return read_out(out, kfs, mps, order)


def test_cpp_optimize_essential_graph(uvo, tmp_path):
    kfs, mps, order = graph()
    got = run(tmp_path, kfs, mps, order)
    sc, vertices, mapped, kept = gather(kfs, mps, order)
    assert got["ret"] == 0
    # the gathering: vertices, similarities, the edge list in the reference's order of insertion, nIDr
    assert np.array_equal(got["Scw"], sc["Scw"]) and np.array_equal(got["Scwn"], sc["Scwn"])
    assert list(zip(got["edge_i"], got["edge_j"], got["conn"])) == list(zip(sc["edge_i"], sc["edge_j"], sc["conn"]))
    assert np.array_equal(got["ref"], sc["ref"])
    # what the walk was built to refuse and to take
    pairs = {(vertices[i], vertices[j], c) for i, j, c in zip(sc["edge_i"], sc["edge_j"], sc["conn"])}
    assert (12, 1, 1) in pairs and (12, 2, 1) in pairs and (11, 2, 1) in pairs and (11, 1, 1) not in pairs and (1, 12, 1) not in pairs
    assert (9, 3, 0) in pairs and (3, 9, 0) not in pairs and (12, 9, 0) in pairs and (12, 2, 0) not in pairs and (11, 8, 0) in pairs and (12, 8, 0) not in pairs
    assert (7, 5, 0) in pairs and (7, 4, 0) in pairs and (9, 5, 0) in pairs
    assert not any(BAD in (i, j) for i, j, c in pairs) and (7, 5, 0) in pairs      # 7's parent 6 is bad: no parent edge, and 6 is no covisible
    # the write-back equals the Python binding's answer for the gathered problem
    m = uvo.ORBmatcher(0.8)
    h = uvo.EssentialGraph(m, 64, 512, 2048, 256)
    want = h.optimize(sc)
    h.close()
    assert (got["iterations"], got["trials"], got["blocks"]) == (want.iterations, want.n_trials, want.envelope_blocks) and want.iterations > 0
    for n, k in enumerate(vertices):
        assert got["kf"][k][0] == 1 and np.array_equal(got["kf"][k][1], want.kf_Tcw[n]), k
    assert got["kf"][BAD][0] == 0 and np.array_equal(got["kf"][BAD][1][:3, :3], kfs[BAD]["R"])
    for n, j in enumerate(mapped):
        assert got["mp"][j][:2] == (1, 1) and np.array_equal(got["mp"][j][2], want.points[n]), j
    for j in kept:
        assert got["mp"][j][:2] == (1, 1) and np.array_equal(got["mp"][j][2], mps[j]["pos"])
    assert got["mp"][5][:2] == (0, 0) and sorted(kept) == [7]
    moved = np.abs(want.kf_Tcw[:, :3, 3] - np.array([kfs[k]["t"] for k in vertices])).max()
    assert moved > 1e-3


def test_cpp_bad_loop_key_frame_touches_nothing(uvo, tmp_path):
    kfs, mps, order = graph(bad_loop=True)
    got = run(tmp_path, kfs, mps, order)
    assert got["ret"] == -1
    assert all(got["kf"][k][0] == 0 for k in range(K)) and all(mp[:2] == (0, 0) for mp in got["mp"])
