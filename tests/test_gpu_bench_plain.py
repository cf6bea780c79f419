"""bench.py without --full: the result line of the headline figure alone, `--steps` timed steps, and --dump-outputs -- the results of the
last timed step as float32 .npy files, the same on a second run with the same arguments and the same as the CPU oracle computes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, STEPS = 8, 5
NAMES = {"frame_index", "n_keypoints", "keypoints", "descriptors", "knn_idx0", "knn_dist0", "knn_idx1", "knn_dist1"}


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", str(B), "--steps", str(STEPS), "--warmup", "1", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "bench.py failed:\n%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path, oracle, synth):
    d, a = _plain_run(tmp_path / "a")
    assert d["steps"] == STEPS and d["warmup"] == 1 and d["n_gpus"] == 1 and d["config"]["batch_per_gpu"] == B
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "u8" and d["metric"].startswith("frames/sec")
    assert d["value"] > 0 and abs(d["value"] - B * STEPS / (d["ms_per_step"] * STEPS * 1e-3)) < 1e-3 * d["value"]
    assert not set(d) & {"roofline", "verification", "sub_records", "cpu_baseline", "host_to_host", "step_spread"}
    assert set(a) == NAMES and all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) < 64e6
    n = a["n_keypoints"].astype(np.int64)
    assert (a["frame_index"] == np.arange(B + 1)).all() and (n > 100).all()
    assert a["keypoints"].shape == (n.sum(), 7) and a["descriptors"].shape == (n.sum(), 32)
    assert all(a[k].shape == (n[:B].sum(),) for k in ("knn_idx0", "knn_dist0", "knn_idx1", "knn_dist1"))
    # the same inputs on a second run: the same outputs
    _, b = _plain_run(tmp_path / "b")
    for k in NAMES:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # and they are what the path computes: frame 0 equals the oracle's extraction of one of the four input batches in rotation
    # (the sequence and its mirror images); which one the last step read depends on the step count only
    f0 = synth.make_sequence(0, 1, 640, 512, n_shapes=400)[0]
    oe = oracle.extractor(1000, 1.2, 8, 20)
    hits = 0
    for img in (f0, f0[:, ::-1], f0[::-1, :], f0[::-1, ::-1]):
        kp, de = oe(np.ascontiguousarray(img))
        if len(kp) != n[0]:
            continue
        fields = np.stack([kp[f].astype(np.float32) for f in ("x", "y", "size", "angle", "response", "octave", "class_id")], 1)
        hits += np.array_equal(fields, a["keypoints"][:n[0]]) and np.array_equal(de.astype(np.float32), a["descriptors"][:n[0]])
    assert hits == 1
