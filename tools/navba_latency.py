#!/usr/bin/env python3
"""Optimizer::LocalBundleAdjustmentNavState as one library call (uvo_nav_bundle_adjust: the host's list building, the upload, every phase
a launch, one status read per Levenberg trial, the download), host clock around the C call, beside the host build of the same source
(tests/emu/navba_emu.cpp, one core) answering the same problem on the same box in the same run.  The reference's g2o cannot be built
here, so the host build stands in for it.  Windows of 5, 10 and 20 free key frames + the previous one + as many covisible fixed ones,
with 300, 1000 and 3000 points seen by 4, 5 and 6 key frames on average; a tenth of the observations shifted by 5..8 px; a forward and a
backward depth entry.  Median of repeated calls after warm-up; the number of trials and of status reads per call; and, from one more
profiled call, the per-phase kernel table of the matcher's profile tap.  Prints one JSON line and writes it to
profiles/navba_latency.json.

  python tools/navba_latency.py [calls=20] [warmup=3]
"""
import ctypes
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((5, 5, 300, 4), (10, 10, 1000, 5), (20, 20, 3000, 6))


def stats(times):
    times = sorted(times)
    return {"median_ms": round(times[len(times) // 2], 4), "p10_ms": round(times[len(times) // 10], 4), "p90_ms": round(times[len(times) * 9 // 10], 4)}


def main():
    import torch  # noqa: F401  (torch's HIP runtime first, as bench.py does)
    import navba_checks as pc
    import navba_model as vm
    uvo = importlib.import_module("u-vip-slam_amd")
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    emu = pc.Emu(uvo)
    matcher = uvo.ORBmatcher(0.8)
    out = {"calls": calls, "warmup": warmup, "device": uvo.device_info(0), "shapes": {}}
    for free, fixed, P, mean in SIZES:
        sc = vm.scene(9000 + P, free, fixed, P, vm.sees_random(mean, P), shifted=0.1, depth=(("fwd", free - 1), ("bwd", free // 2)))
        E = len(sc["edge_kf"])
        adj = uvo.NavBundleAdjuster(matcher, free, fixed + 1, P, E, 2)
        c, r, arrays, keep = uvo.navba_marshal(sc)
        dev_t = []
        for k in range(warmup + calls):
            t0 = time.perf_counter()
            rc = uvo.lib.uvo_nav_bundle_adjust(adj._h, ctypes.byref(c), ctypes.byref(r))
            t1 = time.perf_counter()
            assert rc == 0
            if k >= warmup:
                dev_t.append((t1 - t0) * 1e3)
        dev = [a.tobytes() for a in arrays], (r.n_excluded, r.n_erased, r.iterations[0], r.iterations[1], r.n_trials)
        syncs = r.n_syncs
        matcher.profile(True)
        assert uvo.lib.uvo_nav_bundle_adjust(adj._h, ctypes.byref(c), ctypes.byref(r)) == 0
        table = {k: [round(float(v[0]), 4), int(v[1])] for k, v in matcher.kernel_times().items() if k.startswith("k_navba_")}
        matcher.profile(False)
        adj.close()
        c2, r2, arrays2, keep2 = uvo.navba_marshal(sc)
        host_t = []
        for k in range(max(warmup // 2, 1) + max(calls // 4, 3)):
            t0 = time.perf_counter()
            rc = emu.L.emu_navba_adjust(ctypes.byref(c2), ctypes.byref(r2), None)
            t1 = time.perf_counter()
            assert rc == 0
            if k >= max(warmup // 2, 1):
                host_t.append((t1 - t0) * 1e3)
        host = [a.tobytes() for a in arrays2], (r2.n_excluded, r2.n_erased, r2.iterations[0], r2.iterations[1], r2.n_trials)
        out["shapes"]["%d+1+%d_%d_%d" % (free, fixed, P, mean)] = {
            "edges": E, "unknowns": 15 * free, "device_one_call": stats(dev_t), "host_build_one_core": stats(host_t), "same_result": dev == host,
            "excluded_erased_iterations_trials": list(dev[1]), "synchronisations": syncs, "kernels_ms_launches": table}
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, "profiles", "navba_latency.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
