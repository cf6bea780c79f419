#!/usr/bin/env python3
"""The per-frame front-end as Tracking::GrabImage runs it with the harbor settings (Settings_VI_Aqualoc_harbor.yaml: Enhance 1,
fastTh 20, Px_distance 20): CLAHE -> optical-flow pyramid -> Lucas-Kanade tracking of the previous frame's points -> top-up ORB
extraction (tracked points pass through, the occupancy grid keeps new detections away from them).  Every stage on the GPU through
the C ABI; per-stage wall-clock (host buffers in/out) and a check of the final keypoints / descriptors against the oracle fed with
the same tracked points.  The RANSAC stage of perform_matching (src/Tracking.cc:1062) is timed through the fused call
(uvo_klt_track_filtered: tracker + undistortion + findFundamentalMat) on the same points, beside the chain: "track_filtered" is its
wall-clock, "total_with_ransac" the frame with it in place of the plain tracker call.  The pose step that follows it in
Tracking::TrackWithPnP (cv::solvePnPRansac, src/Tracking.cc:1864) is timed after the fused call on a synthetic scene with as many
map points as the RANSAC kept ("solve_pnp_ransac"), and alone at 200 / 1000 / max_points points and inlier ratios 0.9 / 0.5
("pnp_ms": median host-to-host time of 200 calls after 20 of warm-up).  Prints one JSON object."""
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    torch.zeros(1, device="cuda")
    uvo = importlib.import_module("u-vip-slam_amd")
    synth = importlib.import_module("u-vip-slam_amd.synth")
    import oracle_lib
    import pnp_model as pm
    o = oracle_lib.Oracle()
    W, H, NF, MINPX = 640, 512, 1000, 20
    frames = [synth.make_frame(4242, W, H)]
    for i in range(20):
        frames.append(synth.warp_frame(frames[-1], 5000 + i))
    frames = [(f.astype(np.float32) * 0.45 + 25).astype(np.uint8) for f in frames]      # dim, low contrast
    ex = uvo.ORBextractor(NF, 1.2, 8, 0, 20, max_width=W, max_height=H, max_input_keypoints=4096)
    oe = o.extractor(NF, 1.2, 8, 20)
    klt = uvo.KLT(W, H, (21, 21), 5, max_points=4096, slots=2)
    cam = uvo.CameraModel.make(0.9 * W, 0.9 * W, W / 2, H / 2, [])
    res = {}
    if os.environ.get("UVO_FF_PROFILE"):
        ex.profile(True)
    exact = True
    ntracked = []
    # pass 0: the stages back to back (a busy GPU); pass 1: the oracle's ~25 ms of CPU work between frames, so every stage
    # starts on a GPU that has gone idle, as it does at a 20 Hz camera rate
    for check in (False, True, "chain"):
        # "chain": the enhanced frame stays in HBM between the three calls (clahe without download, pyramid and extraction from it)
        chain = check == "chain"
        t = {"clahe": [], "pyramid": [], "track": [], "extract": []}
        tf, nin, tp = [], [], []
        prev_pts = None
        for i, raw in enumerate(frames):
            t0 = time.perf_counter()
            img = ex.clahe(raw, 4.0, (12, 12), download=not chain)
            t1 = time.perf_counter()
            if chain:
                klt.build_pyramid_from(i & 1, ex)
            else:
                klt.build_pyramid(i & 1, img)
            t2 = time.perf_counter()
            kin = np.zeros(0, uvo.KEYPOINT_DTYPE)
            if prev_pts is not None and len(prev_pts):
                nxt, st, err = klt.track((i - 1) & 1, i & 1, prev_pts)
                inside = (st > 0) & (nxt[:, 0] >= 20) & (nxt[:, 0] < W - 20) & (nxt[:, 1] >= 20) & (nxt[:, 1] < H - 20)
                good = nxt[inside]
                kin = np.zeros(len(good), uvo.KEYPOINT_DTYPE)
                kin["x"], kin["y"], kin["size"], kin["angle"], kin["class_id"] = good[:, 0], good[:, 1], 31, -1, np.arange(len(good))
                if check:
                    ntracked.append(len(good))
            t3 = time.perf_counter()
            grid = np.zeros((H // MINPX + 2, W // MINPX + 2), np.int32, order="F")
            np.add.at(grid, ((kin["y"] / MINPX).astype(np.int64), (kin["x"] / MINPX).astype(np.int64)), 1)
            need = max(NF - len(kin), 1)
            g_gpu, g_orc = grid.copy(order="F"), grid.copy(order="F")
            kin_gpu = kin.copy()
            t4 = time.perf_counter()
            kp, de = ex(img, kin_gpu, g_gpu, MINPX, i == 0, need)
            t5 = time.perf_counter()
            if prev_pts is not None and len(prev_pts) >= 10:     # the fused call on the same points, outside the chain
                t6 = time.perf_counter()
                f = klt.track_filtered((i - 1) & 1, i & 1, prev_pts, cam)
                tf.append(time.perf_counter() - t6)
                nin.append(int(f[5].sum()))
                if nin[-1] >= 5:      # the pose from the surviving points' map points
                    _, obj, pts, _, _, _ = pm.scene(i, nin[-1], 0.9, 0.5, pm.PLAIN)
                    t7 = time.perf_counter()
                    klt.solve_pnp_ransac(obj, pts, cam)
                    tp.append(time.perf_counter() - t7)
            if i >= 3:
                t["clahe"].append(t1 - t0), t["pyramid"].append(t2 - t1), t["track"].append(t3 - t2), t["extract"].append(t5 - t4)
            if check:   # both the idle-GPU pass and the chained pass are checked against the oracle
                kp_o, de_o = oe(o.clahe(raw, 4.0, (12, 12)), kin.copy(), g_orc, MINPX, i == 0, need)
                exact = exact and kp.tobytes() == kp_o.tobytes() and np.array_equal(de, de_o) and np.array_equal(g_gpu, g_orc)
            prev_pts = np.stack([kp["x"], kp["y"]], 1).astype(np.float32)
        key = "hbm_chained_idle_gpu_between_frames" if chain else ("idle_gpu_between_frames" if check else "back_to_back")
        res[key] = {k: round(float(np.median(v)) * 1e3, 3) for k, v in t.items()}
        res[key]["total"] = round(float(sum(np.median(v) for v in t.values())) * 1e3, 3)
        res[key]["track_filtered"] = round(float(np.median(tf[2:])) * 1e3, 3)
        res[key]["total_with_ransac"] = round(res[key]["total"] + res[key]["track_filtered"] - res[key]["track"], 3)
        res[key]["mean_ransac_inliers"] = round(float(np.mean(nin)), 1)
        res[key]["solve_pnp_ransac"] = round(float(np.median(tp[2:])) * 1e3, 3) if len(tp) > 2 else None
    pnp = {}
    for n in (200, 1000, 4096):
        for ratio in (0.9, 0.5):
            _, obj, pts, _, _, _ = pm.scene(n, n, ratio, 0.5, pm.PLAIN)
            ts = []
            for r in range(220):
                t0 = time.perf_counter()
                info = klt.solve_pnp_ransac(obj, pts, cam)[4]
                ts.append(time.perf_counter() - t0)
            pnp["n%d_ratio%.1f" % (n, ratio)] = {"ms": round(float(np.median(ts[20:])) * 1e3, 3), "iterations": info.iterations, "inliers": info.inliers}
    out = {"workload": "640x512 sequence of 21 frames, CLAHE(4, 12x12) + KLT(21x21, 5 levels) + top-up ORB (1000 feats, fastTh 20, Px_distance 20)",
           "ms_per_frame": res,
           "pnp_ms": pnp,
           "mean_tracked_points": round(float(np.mean(ntracked)), 1),
           "extraction_bit_exact_vs_oracle_given_the_same_tracked_points": bool(exact)}
    if os.environ.get("UVO_FF_PROFILE"):
        out["kernel_us"] = {k: round(v[0] / v[1] * 1e3, 1) for k, v in ex.kernel_times().items()}
    print(json.dumps(out, indent=1))
    return 0 if exact else 1


if __name__ == "__main__":
    sys.exit(main())
