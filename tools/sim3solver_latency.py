#!/usr/bin/env python3
"""ComputeSim3's first round -- iterate(5) over all candidate Sim3Solvers, none of which has iterated yet -- as one library call
(uvo_sim3solver_iterate), host clock around the call (it ends in a stream synchronise), beside the host build of the same source
(tests/emu/sim3solver_emu.cpp, one core, which walks the solvers in turn and stops at the first transform) answering the same call on
the same box in the same run.  Candidates x points: 4 and 16 of 30 and 300, inlier ratio 0.5, the call site's SetRansacParameters
(0.99, 2, 300).  Every timed call starts from the same state: the set is cleared and refilled and the generator reseeded outside the
timed region.  Prints one JSON line.

  python tools/sim3solver_latency.py [calls=200] [warmup=20]
"""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(uvo, sc, sset, cands, calls, warmup):
    ids = list(range(len(cands)))
    times, res = [], None
    for k in range(warmup + calls):
        sset.clear()
        for c in cands:
            sc.add_candidate(sset, c, uvo.Sim3SolverParams())
        rng = uvo.GlibcRand(1)
        t0 = time.perf_counter()
        res = sset.iterate(ids, 5, rng)
        t1 = time.perf_counter()
        if k >= warmup:
            times.append((t1 - t0) * 1e3)
    times.sort()
    return {"median_ms": round(times[len(times) // 2], 4), "p10_ms": round(times[len(times) // 10], 4), "p90_ms": round(times[len(times) * 9 // 10], 4),
            "returned": int(res.returned), "n_inliers": int(res.n_inliers), "draws": int(res.draws), "T12": res.T12.tobytes().hex()}


def main():
    import torch  # noqa: F401  (torch's HIP runtime first, as bench.py does)
    import sim3_checks as sc
    import sim3_model as sm
    uvo = importlib.import_module("u-vip-slam_amd")
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    emu = sc.Emu()
    matcher = uvo.ORBmatcher(0.8)
    out = {"calls": calls, "warmup": warmup, "device": uvo.device_info(0), "shapes": {}}
    for C in (4, 16):
        for n in (30, 300):
            cands = [sm.candidate(9000 + 17 * j + n, n, 0.5) for j in range(C)]
            dev, host = uvo.Sim3SolverSet(matcher, C, n), emu.make_set(uvo, C, n)
            d, h = measure(uvo, sc, dev, cands, calls, warmup), measure(uvo, sc, host, cands, calls, warmup)
            dev.close()
            host.close()
            same = all(d[k] == h[k] for k in ("returned", "n_inliers", "draws", "T12"))
            for r in (d, h):
                del r["T12"]
            # what the one call evaluates: every listed solver's min(mRansacMaxIts, 5) hypotheses, whichever solver returns; the host
            # build evaluates draws / 3
            hyp = C * min(sm.derive_params(n, **sm.CALL_SITE), 5)
            out["shapes"]["%dx%d" % (C, n)] = {"device_one_call": d, "host_build_one_core": h, "same_result": same, "hypotheses_evaluated_on_device": hyp,
                                               "hypotheses_evaluated_on_host": h["draws"] // 3}
    matcher.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
