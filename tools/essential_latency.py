#!/usr/bin/env python3
"""Optimizer::OptimizeEssentialGraph as one library call (uvo_essential_graph_optimize: the host's structure building, the upload, every
phase a launch, one status read per Levenberg trial, the download), host clock around the C call, beside the host build of the same
source (tests/emu/essential_emu.cpp, one core) answering the same graph on the same box in the same run.  The reference's g2o cannot be
built here, so the host build stands in for it: parity with g2o is unpinned.  Graphs of 100 / 500 / 2000 key frames (a drifting
trajectory, the parent edge and about two covisibility edges a key frame, two map points a key frame) closed by one loop and by three
loops.  Median of repeated calls after warm-up; the envelope's block count, the trials and status reads per call; and, from one more
profiled call, the per-phase kernel table of the matcher's profile tap with k_essential_solve's share of the kernel time.  Prints one
JSON line and writes it to profiles/essential_latency.json.

  python tools/essential_latency.py [calls=20] [warmup=3]
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

SIZES = (100, 500, 2000)


def stats(times):
    times = sorted(times)
    return {"median_ms": round(times[len(times) // 2], 4), "p10_ms": round(times[len(times) // 10], 4), "p90_ms": round(times[len(times) * 9 // 10], 4)}


def loops_of(K, n):
    return [(K - 1, 3)] if n == 1 else [(K - 1, 3), (2 * K // 3, K // 4), (K // 2, K // 10)]


def blocks_of(sc):
    import essential_model as em
    K = len(sc["Scw"])
    free = em.free_index(K, sc["fixed"])
    first = np.arange(K - 1)
    a, c = free[sc["edge_i"]], free[sc["edge_j"]]
    ok = (a >= 0) & (c >= 0)
    np.minimum.at(first, np.maximum(a, c)[ok], np.minimum(a, c)[ok])
    return int((np.arange(K - 1) - first + 1).sum())


def main():
    import torch  # noqa: F401  (torch's HIP runtime first, as bench.py does)
    import essential_checks as pc
    import essential_model as em
    uvo = importlib.import_module("u-vip-slam_amd")
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    emu = pc.Emu(uvo)
    matcher = uvo.ORBmatcher(0.8)
    out = {"calls": calls, "warmup": warmup, "device": uvo.device_info(0), "shapes": {}}
    for K in SIZES:
        for n_loops in (1, 3):
            sc = em._scene(np.random.default_rng(7000 + K + n_loops), K, loops_of(K, n_loops), extra=2, P=2 * K, correction=(0.03, 0.3, 1.1), n_corrected=5,
                           drift=(0.4 / K, 2.0 / K))
            E, blocks = len(sc["edge_i"]), blocks_of(sc)
            h = uvo.EssentialGraph(matcher, K, E, blocks, 2 * K)
            c, r, arrays, keep = uvo.essential_marshal(sc)
            dev_t = []
            for k in range(warmup + calls):
                t0 = time.perf_counter()
                rc = uvo.lib.uvo_essential_graph_optimize(h._h, ctypes.byref(c), ctypes.byref(r))
                t1 = time.perf_counter()
                assert rc == 0, uvo.last_error()
                if k >= warmup:
                    dev_t.append((t1 - t0) * 1e3)
            dev = [a.tobytes() for a in arrays], (r.iterations, r.n_trials, r.envelope_blocks)
            syncs = r.n_syncs
            matcher.profile(True)
            assert uvo.lib.uvo_essential_graph_optimize(h._h, ctypes.byref(c), ctypes.byref(r)) == 0
            table = {k: [round(float(v[0]), 4), int(v[1])] for k, v in matcher.kernel_times().items() if k.startswith("k_essential_")}
            matcher.profile(False)
            h.close()
            c2, r2, arrays2, keep2 = uvo.essential_marshal(sc)
            host_t = []
            for k in range(1 + max(calls // 4, 3)):
                t0 = time.perf_counter()
                rc = emu.L.emu_essential_optimize(ctypes.addressof(c2), 1 << 22, ctypes.addressof(r2), None)
                t1 = time.perf_counter()
                assert rc == 0
                if k >= 1:
                    host_t.append((t1 - t0) * 1e3)
            host = [a.tobytes() for a in arrays2], (r2.iterations, r2.n_trials, r2.envelope_blocks)
            total = sum(v[0] for v in table.values())
            out["shapes"]["%d_kf_%d_loop%s" % (K, n_loops, "" if n_loops == 1 else "s")] = {
                "edges": E, "points": 2 * K, "envelope_blocks": blocks, "device_one_call": stats(dev_t), "host_build_one_core": stats(host_t), "same_result": dev == host,
                "iterations_trials": [int(dev[1][0]), int(dev[1][1])], "synchronisations": syncs,
                "solve_share_of_kernel_time": round(table.get("k_essential_solve", [0.0])[0] / total, 4) if total else None, "kernels_ms_launches": table}
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, "profiles", "essential_latency.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
