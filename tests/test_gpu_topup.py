"""k_assemble<TOPUP> held to the reference's sequential occupancy filter (src/ORBextractor.cc:872-909) where its closed form and its HBM
walk can go wrong: the level cap and the global cap on the same point, a KP_counter carried across levels and beyond the next cap, levels
past the eighth, grids and survivor lists on both sides of the staging limits, cells that are taken, free and below zero.  Every case is
compared with the oracle's call and with tests/topup_model.py on the GPU's OWN survivor lists (a FullDetect call on the same handle), grid
included.  tests/test_topup_model.py shows without a GPU that the inputs (tests/topup_cases.py) reach what they aim at.  Exact throughout."""
import numpy as np
import pytest

import topup_cases as tc
import topup_model as tm
from test_gpu_describe import raw_batch
from test_gpu_parity import _assert_same_features

pytestmark = pytest.mark.gpu


class Scene:
    def __init__(self, uvo, oracle, synth, name, max_batch=1, in_cap=0):
        nf, sf, nl, th = tc.CFGS[name]
        self.name, self.img = name, tc.images(synth)[name]
        self.ex = uvo.ORBextractor(nf, sf, nl, 0, th, max_width=tc.W, max_height=tc.H, max_batch=max_batch, max_input_keypoints=in_cap)
        self.oe = oracle.extractor(nf, sf, nl, th)
        self.scales = self.ex.mvScaleFactor
        kp, de = self.ex(self.img)
        _assert_same_features(kp, de, *self.oe(self.img), "%s FullDetect" % name)
        self.levels = tm.survivors_from_full_detect(kp, self.scales)       # the GPU's own survivors, in list order

    def check(self, label, grid, d, need):
        label = "%s %s" % (self.name, label)
        g_gpu, g_orc = grid.copy(order="F"), grid.copy(order="F")
        kp, de = self.ex(self.img, None, g_gpu, d, False, need)
        _assert_same_features(kp, de, *self.oe(self.img, None, g_orc, d, False, need), label)
        np.testing.assert_array_equal(g_gpu, g_orc, err_msg=label)
        accepted, g_model, trace = tm.topup(self.levels, self.scales, grid, d, need)
        want = tm.output_positions(self.levels, self.scales, accepted)
        got = np.stack([kp["x"], kp["y"], kp["octave"].astype(np.float32)], 1) if len(kp) else np.zeros((0, 3), np.float32)
        assert got.tobytes() == want.tobytes(), "%s: differs from the sequential model on the GPU's survivors (%d / %d points)" % (label, len(got), len(want))
        np.testing.assert_array_equal(g_gpu, g_model, err_msg=label)
        return tm.takes_staged_walk(self.levels, grid), {t[3] for t in trace}


@pytest.mark.parametrize("name", ["noise", "synth", "noise10", "synth10", "rich"])
def test_scene(uvo, oracle, synth, name):
    s = Scene(uvo, oracle, synth, name)
    left = {True: set(), False: set()}
    for label, grid, d, need in tc.scene_cases(name, s.levels, s.scales):
        staged, how = s.check(label, grid, d, need)
        left[staged] |= how
    s.ex.close()
    # which walk the cases took (from the survivor counts and the grids), and that each was left at the level cap and at the global cap
    print(name, {k: sorted(v) for k, v in left.items()})
    if name in ("noise", "synth"):
        assert {"cap", "need", "end"} <= left[True] and {"cap", "need", "end"} <= left[False]
    if name == "rich":
        assert not left[True] and {"cap", "need", "end"} <= left[False] and sum(len(p) for p in s.levels) > tm.STAGED_POINTS


def test_negative_need_is_the_reference(uvo, oracle, synth):
    """uvo.h: num_feats_needed <= 0 is not refused -- no counter ever equals a cap, free cells alone limit the call."""
    s = Scene(uvo, oracle, synth, "noise")
    n = [len(s.ex(s.img, None, tc.empty_grid(5), 5, False, need)[0]) for need in (-30, -1, 0, 100000)]
    s.ex.close()
    assert len(set(n)) == 1 and n[0] > 300, n


def test_batch_of_three(uvo, oracle, synth):
    """Three frames with their own need, grid and caller keypoints in one call; one of them has no survivors at all."""
    s = Scene(uvo, oracle, synth, "synth", max_batch=3, in_cap=4)
    d, frames = tc.batch_of_three(tc.images(synth), s.levels, s.scales)
    rc, n_out, out_kp, out_desc, grids = raw_batch(uvo, s.ex, [f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], d, [f[3] for f in frames])
    assert rc == uvo.UVO_OK, rc
    for b, (img, kin, grid, need) in enumerate(frames):
        g_orc = grid.copy(order="F")
        kp_o, de_o = s.oe(img, kin.copy(), g_orc, d, False, need)
        _assert_same_features(out_kp[b, :n_out[b]], out_desc[b, :n_out[b]], kp_o, de_o, "batch of three, frame %d" % b)
        np.testing.assert_array_equal(grids[b], g_orc, err_msg="grid of frame %d" % b)
    assert n_out[2] == 3 and (grids[2] == 0).all()
    s.ex.close()
