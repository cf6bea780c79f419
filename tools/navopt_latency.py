#!/usr/bin/env python3
"""The two IMU overloads of Optimizer::PoseOptimization as one library call (uvo_nav_optimize: one upload, one launch of one workgroup
per problem, one download), host clock around the C call (it ends in a stream synchronise), beside the host build of the same source
(tests/emu/navopt_emu.cpp, one core, the problems in turn) answering the same problems on the same box in the same run.  The
reference's g2o and Cholmod cannot be built here, so the host build stands in for them.  Both forms, N = 100, 300, 1000, 2000
correspondences a frame, a quarter of them shifted by 5..8 px, the depth edge and the marginals on, for 1 and 8 problems a call.
Median of repeated calls after warm-up.  Prints one JSON line and writes it to profiles/navopt_latency.json.

  python tools/navopt_latency.py [calls=30] [warmup=3]
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
    import navopt_checks as nc
    import navopt_model as nm
    uvo = importlib.import_module("u-vip-slam_amd")
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    emu = nc.Emu(uvo)
    klt = uvo.KLT(64, 64, max_points=16)
    out = {"calls": calls, "warmup": warmup, "device": uvo.device_info(0), "shapes": {}}
    for form, tag in ((nm.KEYFRAME, "keyframe"), (nm.FRAME, "frame")):
        for P in (1, 8):
            for n in (100, 300, 1000, 2000):
                scenes = [nm.scene(seed=7000 + 13 * j + n, form=form, n=n, shifted=n // 4, has_depth=True, marg=True) for j in range(P)]
                opt = uvo.NavOptimizer(klt, P, n)
                # the C call alone: problems and results prepared once
                cp, cr = (uvo.NavProblemC * P)(), (uvo.NavResultC * P)()
                keep = []
                for j, sc in enumerate(scenes):
                    cp[j] = uvo.NavOptimizer.problem(sc, keep)
                dev_t = []
                for k in range(warmup + calls):
                    t0 = time.perf_counter()
                    rc = uvo.lib.uvo_nav_optimize(opt._h, cp, P, cr)
                    t1 = time.perf_counter()
                    assert rc == 0
                    if k >= warmup:
                        dev_t.append((t1 - t0) * 1e3)
                dev_ns = [bytes(cr[j].ns) for j in range(P)]
                dev_inl = [int(cr[j].n_inliers) for j in range(P)]
                trials = [len(opt.trace(j).trial) for j in range(P)]
                opt.close()
                # the host build, one core, the problems in turn
                recs, edges = [nm.record(sc) for sc in scenes], [nm.all_edges(sc) for sc in scenes]
                res, mask = np.zeros(1, nc.OUT_DTYPE), np.zeros(2 * n + 1, np.uint8)
                host_t, host_ns, host_inl = [], [], []
                for k in range(warmup + calls):
                    host_ns, host_inl = [], []
                    t0 = time.perf_counter()
                    for j in range(P):
                        emu.L.emu_nav_optimize(recs[j].ctypes.data, edges[j].ctypes.data, res.ctypes.data, mask.ctypes.data, None)
                        host_ns.append(res["ns"][0].tobytes())
                        host_inl.append(int(res["n_inliers"][0]))
                    t1 = time.perf_counter()
                    if k >= warmup:
                        host_t.append((t1 - t0) * 1e3)
                out["shapes"]["%s_%dx%d" % (tag, P, n)] = {"device_one_call": stats(dev_t), "host_build_one_core": stats(host_t),
                                                          "same_result": dev_ns == host_ns and dev_inl == host_inl, "inliers": dev_inl, "levenberg_trials": trials}
    klt.close()
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, "profiles", "navopt_latency.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
