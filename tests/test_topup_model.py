"""tests/topup_model.py held to the oracle on the very inputs of tests/test_gpu_topup.py (tests/topup_cases.py), and the coverage
conditions of those inputs shown from the oracle alone: no GPU."""
import numpy as np
import pytest

import topup_cases as tc
import topup_model as tm


def oracle_scene(oracle, synth, scene):
    cfg = tc.CFGS[scene]
    oe = oracle.extractor(*cfg)
    oe(tc.images(synth)[scene])
    return oe, [np.stack([k["x"], k["y"]], 1) for k in (oe.level_keypoints(l) for l in range(cfg[2]))]


def check_case(oe, img, levels, grid, d, need, label):
    """The oracle's top-up call against the model on the oracle's survivor lists: positions, octaves, order, count and grid."""
    g = grid.copy(order="F")
    kp, _ = oe(img, None, g, d, False, need)
    accepted, g_model, trace = tm.topup(levels, oe.scale, grid, d, need)
    want = tm.output_positions(levels, oe.scale, accepted)
    assert len(kp) == len(want), "%s: oracle %d, model %d" % (label, len(kp), len(want))
    got = np.stack([kp["x"], kp["y"], kp["octave"].astype(np.float32)], 1) if len(kp) else np.zeros((0, 3), np.float32)
    assert got.tobytes() == want.tobytes(), label
    np.testing.assert_array_equal(g, g_model, err_msg=label)
    return kp, g, trace


def test_c_division():
    assert [tm.c_div(a, 30) for a in (-31, -30, -29, -1, 0, 1, 29, 30, 59)] == [-1, -1, 0, 0, 0, 0, 0, 1, 1]


@pytest.mark.parametrize("scene", ["noise", "synth"])
def test_eight_levels(oracle, synth, scene):
    oe, levels = oracle_scene(oracle, synth, scene)
    img = tc.images(synth)[scene]
    assert all(len(p) > 0 for p in levels) and tm.survivors_from_full_detect(oe(img)[0], oe.scale)[3].tobytes() == levels[3].astype(np.float32).tobytes()
    counts, left = {}, {True: set(), False: set()}
    for label, grid, d, need in tc.scene_cases(scene, levels, oe.scale):
        kp, g, trace = check_case(oe, img, levels, grid, d, need, "%s %s" % (scene, label))
        counts[label] = (len(kp), np.bincount(kp["octave"], minlength=8).tolist())
        left[tm.takes_staged_walk(levels, grid)] |= {t[3] for t in trace}
        if label.startswith("carry"):
            k = int(label[-1])
            entry, cap, taken, how = trace[2]
            assert trace[0][3] == "end" and trace[1][2] == k and entry == trace[0][2] + k, (label, trace)
            # the carry is beyond level 2's cap on entry, so the cap can never fire: the level takes every free cell it has
            free = tm.topup(levels, oe.scale, grid, d, 0)[2][2][2]       # what level 2 takes on this grid when nothing is capped
            assert entry > cap > 0 and how == "end" and counts[label][1][2] == taken == free, (label, trace)
            assert all(t[0] > t[1] and t[3] == "end" for t in trace[2:]), (label, trace)      # ... and overshoots every later cap for good
        if label.startswith("contents"):
            g0, top = tc.contents_grid(levels, oe.scale, 20)
            assert [int(g0[c]) for c in top] == [-5, -1, 2, 7] and g[top[2]] == 2 and g[top[3]] == 7
            if need == 1000:
                # a cell below zero takes points until it counts 1 (`> 0` and `++`): more than one here, which one point per cell would miss
                assert g[top[0]] > -4 and g[top[1]] == 1, (label, [int(g[c]) for c in top])
        if label == "occupied":
            assert len(kp) == 0 and (g == 3).all()
    print(scene, counts)
    # the sweep: 30 wanted give 36 (every level stops at its cap, the global cap is never looked at), 31 stop at 31, free cells alone limit 100000
    n = {need: counts["sweep need=%d" % need] for need in tc.NEEDS}
    assert n[30] == (36, [8, 7, 6, 5, 4, 3, 2, 1]) and n[37][0] == 40 and n[31][0] == 31 and n[29][0] == 29 and n[1][0] == 1
    assert n[100000][0] < 1000 and n[100000] == n[0] == n[-1] == n[-30]            # nothing ever equals a cap at or below zero
    # both walks leave levels at the level cap and at the global cap
    print("levels left by", left)
    assert {"cap", "need", "end"} <= left[True] and {"cap", "need", "end"} <= left[False]
    staged = {d: tm.takes_staged_walk(levels, tc.empty_grid(d)) for d in (1, 3, 5, 20, 64)}
    assert staged == {1: False, 3: False, 5: True, 20: True, 64: True}
    assert not tm.takes_staged_walk(levels, tc.contents_grid(levels, oe.scale, 20)[0])


@pytest.mark.parametrize("scene", ["noise10", "synth10"])
def test_ten_levels(oracle, synth, scene):
    """numofpoint is 0 on level 8 and negative on level 9: no cap there."""
    oe, levels = oracle_scene(oracle, synth, scene)
    on_last = 0
    for label, grid, d, need in tc.scene_cases(scene, levels, oe.scale):
        kp, g, trace = check_case(oe, tc.images(synth)[scene], levels, grid, d, need, "%s %s" % (scene, label))
        assert [t[1] for t in trace[8:]] == [0, tm.c_div(-need, 30)][:len(trace) - 8]
        on_last += int((kp["octave"] >= 8).sum())
        print(scene, label, len(kp), np.bincount(kp["octave"], minlength=10).tolist())
    assert on_last > 0


def test_many_survivors(oracle, synth):
    oe, levels = oracle_scene(oracle, synth, "rich")
    assert sum(len(p) for p in levels) > tm.STAGED_POINTS
    left = set()
    for label, grid, d, need in tc.scene_cases("rich", levels, oe.scale):
        assert not tm.takes_staged_walk(levels, grid) and grid.size <= tm.STAGED_CELLS
        kp, g, trace = check_case(oe, tc.images(synth)["rich"], levels, grid, d, need, label)
        left |= {t[3] for t in trace}
        print(label, len(kp), np.bincount(kp["octave"], minlength=8).tolist())
    assert {"cap", "need", "end"} <= left


def test_batch_frames(oracle, synth):
    oe, levels = oracle_scene(oracle, synth, "synth")
    d, frames = tc.batch_of_three(tc.images(synth), levels, oe.scale)
    n = []
    for img, kin, grid, need in frames:
        kp, _ = oe(img, kin.copy(), grid.copy(order="F"), d, False, need)
        n.append((len(kin), len(kp)))
    print("batch of three (n_in, n_out):", n)
    assert n[2][1] == n[2][0] == 3 and n[0][1] == 2 + 36 and n[1][0] == 0 and n[1][1] > 50
    assert all(len(oe.level_keypoints(l)) == 0 for l in range(8))          # the constant image: no survivors on any level
