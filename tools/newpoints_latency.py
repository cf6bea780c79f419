#!/usr/bin/env python3
"""LocalMapping::CreateNewMapPoints' loop (src/LocalMapping.cc:1058-1199) over 20 neighbour key frames of ~1000 key points each, two ways on
one box in one run (host clock around the calls, C++ caller: tests/cpp/compat_newpoints.cpp):
  begin_next_host_svd_ms : SearchForTriangulationBegin + 20 x (SearchForTriangulationNext, fp32 Jacobi triangulation on the host, AddMapPoint)
  one_call_ms            : CreateNewMapPoints (uvo_create_new_map_points) + the caller's AddMapPoint loop over its output
and the device's per-kernel times of the one call (uvo_matcher_profile).  Prints one JSON line.
"""
import importlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch  # noqa: F401  (torch's HIP runtime first, as bench.py does)
    import triangulation_model as tm
    import test_gpu_cpp_newpoints as drv
    uvo = importlib.import_module("u-vip-slam_amd")
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    sc = tm.make_scene(seed=4242, n_pairs=20, n_points=900, clutter=100)
    out = {"shape": {"pairs": 20, "n1": len(sc["kp1"]), "n2_mean": sum(len(P["kp"]) for P in sc["pairs"]) / 20.0}}
    with tempfile.TemporaryDirectory() as d:
        scene_p, out_p = os.path.join(d, "scene.bin"), os.path.join(d, "out.bin")
        tm.write_scene_file(scene_p, sc, True)
        r = subprocess.run([drv.build_driver(), scene_p, out_p, str(reps)], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit(r.stdout + r.stderr)
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    m = uvo.ORBmatcher(0.6, True)
    args = (uvo.FeatureVector(sc["groups1"]), sc["kp1"], sc["desc1"], sc["has_mp1"],
            [(uvo.FeatureVector(P["groups"]), P["kp"], P["desc"], P["has_mp"], P["F12"], P["sigma2"]) for P in sc["pairs"]],
            uvo.TriangulationCamera(*[getattr(sc["cam1"], k) for k in ("rcw", "tcw", "ow", "fx", "fy", "cx", "cy", "sf", "sigma2")]),
            [uvo.TriangulationCamera(*[getattr(c, k) for k in ("rcw", "tcw", "ow", "fx", "fy", "cx", "cy", "sf", "sigma2")]) for c in sc["cams2"]],
            sc["ratio_factor"])
    m.CreateNewMapPoints(*args)
    m.profile(True)
    for _ in range(20):
        dev, _ = m.CreateNewMapPoints(*args)
    out["kernel_ms_per_call"] = {k: round(v[0] / 20.0, 4) for k, v in m.kernel_times().items()}
    out["matches_per_pair"] = [len(x["idx1"]) for x in dev]
    m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
