#!/usr/bin/env python3
"""The three keyframe-database queries host to host -- uvo_kfdb_detect_reloc, _detect_loop, _detect_loop_haloc, the host clock around
each call (every one ends in a stream synchronise) -- at (keyframes, words) = (256, 300), (2048, 300), (4096, 1000), beside the host
build of the same rules (tests/emu/kfdb_emu.cpp, a serial loop over the slots on one core) answering the same queries on the same box
in the same run.  Words come from a pool of 20 x `words` ids in 0..10^6, so a query shares a few dozen words with a keyframe and lists
nearly all of them; every keyframe has ten covisibles and a 64-float hash.  Each device call uses a fresh query id, so every call
lists every sharing keyframe again; the host build restores the stored fields in front of each repetition, which is the same work.
Writes profiles/kfdb_latency.json and prints it as one JSON line.

  python tools/kfdb_latency.py [calls=100] [warmup=10]
"""
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ((256, 300), (2048, 300), (4096, 1000))
HASH_LEN = 64


def make_case(kc, nkf, words, seed):
    rng = np.random.default_rng(seed)
    pool = rng.choice(10 ** 6, size=20 * words, replace=False)
    ops = [("add", int(i) + 1, *kc.rand_bow(rng, words, pool), rng.standard_normal(HASH_LEN).astype(np.float32)) for i in rng.permutation(nkf)]
    ops += [("cov", k, [int(x) for x in rng.integers(0, nkf, size=10)]) for k in range(nkf)]
    q = kc.rand_bow(rng, words, pool)
    conn = [int(x) for x in rng.choice(nkf, size=20, replace=False)]
    queries = [("reloc", 10 ** 6, *q), ("loop", 10 ** 6, *q, conn, np.float32(0.01)),
               ("haloc", 10 ** 6, rng.standard_normal(HASH_LEN).astype(np.float32), [int(x) + 1 for x in conn], np.float32(80.0))]
    return (nkf, words, HASH_LEN, ops), queries


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "p10_ms": round(ms[len(ms) // 10], 4), "p90_ms": round(ms[len(ms) * 9 // 10], 4)}


def main():
    import kfdb_cases as kc
    import test_kfdb_emu as te
    uvo = importlib.import_module("u-vip-slam_amd")
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    emu = te.build_emu(os.path.join(ROOT, "tests", "emu", "kfdb_emu"))
    out = {"calls": calls, "warmup": warmup, "device": uvo.device_info(0), "hash_len": HASH_LEN, "shapes": {}}
    for nkf, words in SHAPES:
        case, queries = make_case(kc, nkf, words, 7 * nkf + words)
        db = uvo.KeyFrameDatabase(nkf, words, HASH_LEN)
        for op in case[3]:
            if op[0] == "add":
                db.add(op[1], (op[2], op[3]), op[4])
            else:
                db.set_covisibles(op[1], op[2])
        rec = {}
        for q in queries:
            ms, n_cand = [], 0
            for k in range(warmup + calls):
                qid = q[1] + k
                t0 = time.perf_counter()
                if q[0] == "reloc":
                    cand = db.detect_reloc(qid, (q[2], q[3]))
                elif q[0] == "loop":
                    cand = db.detect_loop(qid, (q[2], q[3]), q[4], q[5])
                else:
                    cand = db.detect_loop_haloc(qid, q[2], q[3], q[4])
                t1 = time.perf_counter()
                n_cand = len(cand)
                if k >= warmup:
                    ms.append((t1 - t0) * 1e3)
            rec[q[0]] = {"device": stats(ms), "candidates": n_cand}
            if q[0] != "haloc":
                rec[q[0]]["listed"] = len(db.last_query()[0])
        db.close()
        with tempfile.TemporaryDirectory() as tmp:
            script = os.path.join(tmp, "case.txt")
            with open(script, "w") as fh:
                fh.write(kc.to_script((case[0], case[1], case[2], case[3] + queries)))
            host = json.loads(subprocess.run([emu, "--time", str(max(3, calls // 10)), script], capture_output=True, text=True, check=True).stdout)
        for name in ("reloc", "loop", "haloc"):
            rec[name]["host_one_core_ms"] = round(host[name + "_s"] * 1e3, 4)
        out["shapes"]["%dx%d" % (nkf, words)] = rec
        with open(os.path.join(ROOT, "profiles", "kfdb_latency.json"), "w") as fh:      # after every shape: a long run leaves what it has
            fh.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
