#!/usr/bin/env python3
"""One Initializer::Initialize call (200 iterations) as one library call (uvo_initializer_initialize), host clock around the call (it
ends in a stream synchronise), beside the host build of the same source (tests/emu/initializer_emu.cpp, one core, which walks
FindFundamental and the four CheckRT as the reference writes them) answering the same call on the same box in the same run.
N = 200, 400 and 1000 matches, outlier share 0.2; the reference frame is set outside the timed region and the generator reseeded, so
every timed call does the same work.  Prints
one JSON line.

  python tools/initializer_latency.py [calls=100] [warmup=10]
"""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(uvo, obj, k2, m12, calls, warmup):
    times, res = [], None
    for k in range(warmup + calls):
        rng = uvo.GlibcRand(1)
        t0 = time.perf_counter()
        res = obj.initialize(k2, m12, rng)
        t1 = time.perf_counter()
        if k >= warmup:
            times.append((t1 - t0) * 1e3)
    times.sort()
    return {"median_ms": round(times[len(times) // 2], 4), "p10_ms": round(times[len(times) // 10], 4), "p90_ms": round(times[len(times) * 9 // 10], 4),
            "initialized": bool(res.initialized), "n_inliers": int(res.n_inliers), "n_good": [int(v) for v in res.n_good],
            "bits": (res.R21.tobytes() + res.t21.tobytes() + res.F21.tobytes() + res.p3d.tobytes()).hex()}


def main():
    import torch  # noqa: F401  (torch's HIP runtime first, as bench.py does)
    import initializer_checks as ic
    uvo = importlib.import_module("u-vip-slam_amd")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    calls = int(args[0]) if len(args) > 0 else 100
    warmup = int(args[1]) if len(args) > 1 else 10
    emu = ic.Emu()
    klt = uvo.KLT(64, 64, max_points=256)
    out = {"calls": calls, "warmup": warmup, "iterations": 200, "device": uvo.device_info(0), "shapes": {}}
    for n in (200, 400, 1000):
        k1, k2, m12, _ = ic.scene(100 + n, n, 0.2)
        dev, host = uvo.Initializer(klt, n + ic.EXTRA_REFERENCE_KEYS), emu.make(uvo, n + ic.EXTRA_REFERENCE_KEYS)
        for obj in (dev, host):
            obj.set_reference(k1, ic.CAM, 1.0, 200)
        d, h = measure(uvo, dev, k2, m12, calls, warmup), measure(uvo, host, k2, m12, calls, warmup)
        dev.close()
        host.close()
        same = d["bits"] == h["bits"] and d["n_good"] == h["n_good"]
        for r in (d, h):
            del r["bits"]
        out["shapes"]["N=%d" % n] = {"device_one_call": d, "host_build_one_core": h, "same_result": same}
    klt.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
