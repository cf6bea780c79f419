#!/usr/bin/env python3
"""Optimizer::OptimizeSim3 as one library call (uvo_sim3_optimize: the host gather of Rcw X + tcw, one upload, one launch of one
workgroup per problem, one download), host clock around the C call (it ends in a stream synchronise), beside the host build of the same
source (tests/emu/sim3opt_emu.cpp, one core, the problems in turn, the pairs gathered beforehand) answering the same problems on the
same box in the same run.  The reference's g2o cannot be built here, so the host build stands in for it.  1, 4 and 16 problems of 30,
100 and 300 pairs, a fifth of the pairs shifted in the second image so that the second round runs 10 iterations.  Median of repeated
calls after warm-up.  Prints one JSON line and writes it to profiles/sim3opt_latency.json.

  python tools/sim3opt_latency.py [calls=200] [warmup=20]
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
    import sim3opt_checks as pc
    import sim3opt_model as sm
    uvo = importlib.import_module("u-vip-slam_amd")
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    emu = pc.Emu(uvo)
    matcher = uvo.ORBmatcher(0.8)
    out = {"calls": calls, "warmup": warmup, "device": uvo.device_info(0), "shapes": {}}
    for P in (1, 4, 16):
        for n in (30, 100, 300):
            scenes = [sm.scene(seed=7000 + 13 * j + n, n=n, shifted2=n // 5) for j in range(P)]
            opt = uvo.Sim3Optimizer(matcher, P, n)
            # the C call alone: problems and results prepared once
            cp, cr = (uvo.Sim3OptProblemC * P)(), (uvo.Sim3OptResultC * P)()
            keep = []
            for j, sc in enumerate(scenes):
                m = np.zeros(n, np.uint8)
                keep.append(m)
                c = cp[j]
                c.x1w, c.x2w, c.obs1, c.obs2, c.info1, c.info2 = [sc[k].ctypes.data for k in ("x1w", "x2w", "obs1", "obs2", "info1", "info2")]
                c.n, c.th2 = n, float(sc["th2"])
                c.kf1, c.kf2 = uvo.Sim3KeyFrame.make(*sc["kf1"]), uvo.Sim3KeyFrame.make(*sc["kf2"])
                c.R12 = (ctypes.c_float * 9)(*sc["R12"].reshape(9).tolist())
                c.t12 = (ctypes.c_float * 3)(*sc["t12"].tolist())
                c.s12 = float(sc["s12"])
                cr[j].removed, cr[j].removed_cap = m.ctypes.data, n
            dev_t = []
            for k in range(warmup + calls):
                t0 = time.perf_counter()
                rc = uvo.lib.uvo_sim3_optimize(opt._h, cp, P, cr)
                t1 = time.perf_counter()
                assert rc == 0
                if k >= warmup:
                    dev_t.append((t1 - t0) * 1e3)
            dev_est = [np.array(list(cr[j].q) + list(cr[j].t) + [cr[j].s]).tobytes() for j in range(P)]
            dev_cnt = [(int(cr[j].n_inliers), int(cr[j].n_bad), int(cr[j].more_iterations)) for j in range(P)]
            trials = [len(opt.trace(j).trial) for j in range(P)]
            opt.close()
            # the host build, one core, the problems in turn
            pairs = [np.ascontiguousarray(emu.pairs(sc)) for sc in scenes]
            K1 = [pc.Emu._k(sc["kf1"][2]) for sc in scenes]
            K2 = [pc.Emu._k(sc["kf2"][2]) for sc in scenes]
            R = [np.ascontiguousarray(sc["R12"], np.float32).reshape(9) for sc in scenes]
            t = [np.ascontiguousarray(sc["t12"], np.float32) for sc in scenes]
            est, estf, cnt, mask = np.zeros(8), np.zeros(13, np.float32), np.zeros(4, np.int32), np.zeros(n + 1, np.uint8)
            host_t, host_est, host_cnt = [], [], []
            for k in range(warmup + calls):
                host_est, host_cnt = [], []
                t0 = time.perf_counter()
                for j in range(P):
                    emu.L.emu_sim3opt_optimize(pairs[j].ctypes.data, n, K1[j].ctypes.data, K2[j].ctypes.data, R[j].ctypes.data, t[j].ctypes.data, float(scenes[j]["s12"]),
                                               float(scenes[j]["th2"]), est.ctypes.data, estf.ctypes.data, cnt.ctypes.data, mask.ctypes.data, None)
                    host_est.append(est.tobytes())
                    host_cnt.append((int(cnt[0]), int(cnt[2]), int(cnt[3])))
                t1 = time.perf_counter()
                if k >= warmup:
                    host_t.append((t1 - t0) * 1e3)
            out["shapes"]["%dx%d" % (P, n)] = {"device_one_call": stats(dev_t), "host_build_one_core": stats(host_t),
                                               "same_result": dev_est == host_est and dev_cnt == host_cnt, "inliers_bad_more": dev_cnt, "levenberg_trials": trials}
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, "profiles", "sim3opt_latency.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
