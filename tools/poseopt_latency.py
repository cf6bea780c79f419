#!/usr/bin/env python3
"""Optimizer::PoseOptimization as one library call (uvo_pose_optimize: one upload, one launch of one workgroup per problem, one
download), host clock around the C call (it ends in a stream synchronise), beside the host build of the same source
(tests/emu/poseopt_emu.cpp, one core, the problems in turn) answering the same problems on the same box in the same run.  The
reference's g2o cannot be built here, so the host build stands in for it.  N = 100, 300, 1000, 2000 correspondences, a quarter of them
shifted by 5..8 px, for 1 and 8 problems a call.  Median of repeated calls after warm-up.  Prints one JSON line and writes it to
profiles/poseopt_latency.json.

  python tools/poseopt_latency.py [calls=200] [warmup=20]
"""
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(times):
    times = sorted(times)
    return {"median_ms": round(times[len(times) // 2], 4), "p10_ms": round(times[len(times) // 10], 4), "p90_ms": round(times[len(times) * 9 // 10], 4)}


def main():
    import torch  # noqa: F401  (torch's HIP runtime first, as bench.py does)
    import poseopt_checks as pc
    import poseopt_model as pm
    uvo = importlib.import_module("u-vip-slam_amd")
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    emu = pc.Emu(uvo)
    klt = uvo.KLT(64, 64, max_points=16)
    out = {"calls": calls, "warmup": warmup, "device": uvo.device_info(0), "shapes": {}}
    for P in (1, 8):
        for n in (100, 300, 1000, 2000):
            scenes = [pm.scene(seed=7000 + 13 * j + n, n=n, shifted=n // 4, off=(0.05, 0.1)) for j in range(P)]
            opt = uvo.PoseOptimizer(klt, P, n)
            # the C call alone: problems and results prepared once
            cp, cr = (uvo.PoseProblemC * P)(), (uvo.PoseResultC * P)()
            keep = []
            for j, (p3d, p2d, w, K, Tcw) in enumerate(scenes):
                m = np.zeros(n, np.uint8)
                keep.append((p3d, p2d, w, m))
                cp[j].p3d, cp[j].p2d, cp[j].inv_sigma2, cp[j].n = p3d.ctypes.data, p2d.ctypes.data, w.ctypes.data, n
                cp[j].fx, cp[j].fy, cp[j].cx, cp[j].cy = [float(v) for v in K]
                cp[j].Tcw = (ctypes.c_float * 16)(*np.asarray(Tcw, np.float32).reshape(16).tolist())
                cr[j].outlier, cr[j].outlier_cap = m.ctypes.data, n
            dev_t = []
            for k in range(warmup + calls):
                t0 = time.perf_counter()
                rc = uvo.lib.uvo_pose_optimize(opt._h, cp, P, cr)
                t1 = time.perf_counter()
                assert rc == 0
                if k >= warmup:
                    dev_t.append((t1 - t0) * 1e3)
            dev_T = [np.array(cr[j].Tcw, np.float32).tobytes() for j in range(P)]
            dev_inl = [int(cr[j].n_inliers) for j in range(P)]
            trials = [len(opt.trace(j).trial) for j in range(P)]
            opt.close()
            # the host build, one core, the problems in turn
            edges = [pc.Emu.edges(p3d, p2d, w) for (p3d, p2d, w, K, Tcw) in scenes]
            Ks = [np.asarray(sc[3], np.float32) for sc in scenes]
            Ts = [np.ascontiguousarray(sc[4], np.float32) for sc in scenes]
            To, ni, nr, mask = np.zeros(16, np.float32), ctypes.c_int32(), ctypes.c_int32(), np.zeros(n + 1, np.uint8)
            host_t, host_T, host_inl = [], [], []
            for k in range(warmup + calls):
                host_T, host_inl = [], []
                t0 = time.perf_counter()
                for j in range(P):
                    emu.L.emu_pose_optimize(edges[j].ctypes.data, n, Ks[j].ctypes.data, Ts[j].ctypes.data, To.ctypes.data, ctypes.byref(ni), ctypes.byref(nr),
                                            mask.ctypes.data, None)
                    host_T.append(To.tobytes())
                    host_inl.append(ni.value)
                t1 = time.perf_counter()
                if k >= warmup:
                    host_t.append((t1 - t0) * 1e3)
            out["shapes"]["%dx%d" % (P, n)] = {"device_one_call": stats(dev_t), "host_build_one_core": stats(host_t), "same_result": dev_T == host_T and dev_inl == host_inl,
                                               "inliers": dev_inl, "levenberg_trials": trials}
    klt.close()
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, "profiles", "poseopt_latency.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
