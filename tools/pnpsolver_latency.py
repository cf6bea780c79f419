#!/usr/bin/env python3
"""Relocalisation's first round -- iterate(5) over all candidate PnPsolvers, none of which has iterated yet -- as one library call
(uvo_pnpsolver_iterate), host clock around the call (it ends in a stream synchronise), beside the host build of the same source
(tests/emu/pnpsolver_emu.cpp, one core, which walks the solvers in turn and stops at the first pose) answering the same call on the
same box in the same run.  Candidates x points: 8 x 100 and 16 x 300, inlier ratio 0.5.  Every timed call starts from the same state:
the set is cleared and refilled and the generator reseeded outside the timed region.  Prints one JSON line.

  python tools/pnpsolver_latency.py [calls=200] [warmup=20]
"""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(uvo, pset, cands, calls, warmup):
    ids = list(range(len(cands)))
    times, res = [], None
    for k in range(warmup + calls):
        pset.clear()
        for c in cands:
            pset.add(*c[:6])
        rng = uvo.GlibcRand(1)
        t0 = time.perf_counter()
        res = pset.iterate(ids, 5, rng)
        t1 = time.perf_counter()
        if k >= warmup:
            times.append((t1 - t0) * 1e3)
    times.sort()
    return {"median_ms": round(times[len(times) // 2], 4), "p10_ms": round(times[len(times) // 10], 4), "p90_ms": round(times[len(times) * 9 // 10], 4),
            "returned": int(res.returned), "n_inliers": int(res.n_inliers), "draws": int(res.draws), "Tcw": res.Tcw.tobytes().hex()}


def main():
    import torch  # noqa: F401  (torch's HIP runtime first, as bench.py does)
    import pnpsolver_checks as pc
    import pnpsolver_model as psm
    uvo = importlib.import_module("u-vip-slam_amd")
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    emu = pc.Emu()
    klt = uvo.KLT(64, 64, max_points=16)
    out = {"calls": calls, "warmup": warmup, "device": uvo.device_info(0), "shapes": {}}
    for C, n in ((8, 100), (16, 300)):
        cands = [psm.candidate(9000 + 17 * j + n, n, 0.5) for j in range(C)]
        dev, host = uvo.PnPsolverSet(klt, C, n), emu.make_set(uvo, C, n)
        d, h = measure(uvo, dev, cands, calls, warmup), measure(uvo, host, cands, calls, warmup)
        dev.close()
        host.close()
        same = all(d[k] == h[k] for k in ("returned", "n_inliers", "draws", "Tcw"))
        for r in (d, h):
            del r["Tcw"]
        # what the one call evaluates: every listed solver's max(mRansacMaxIts, 5) hypotheses, whichever solver returns
        hyp = sum(max(psm.derive_params(n, **{k: v for k, v in psm.CALL_SITE.items() if k != "th2"})[1], 5) for _ in range(C))
        out["shapes"]["%dx%d" % (C, n)] = {"device_one_call": d, "host_build_one_core": h, "same_result": same, "hypotheses_evaluated_on_device": hyp}
    klt.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
