"""The sequence scenarios against the oracle alone (no GPU): every scenario must be able to catch a carry-over from one call into the
next, and the sizes it uses must be what the handle's own rules say they are.  Conditions on the inputs, not tolerances."""
import importlib

import numpy as np
import pytest

import extractor_sequence_cases as sc


@pytest.fixture(scope="module")
def scenarios(synth):
    return sc.all_scenarios(synth)


@pytest.fixture(scope="module")
def results(oracle, scenarios):
    """every step of every scenario through the oracle, once"""
    return {name: [sc.expected(oracle, cfg, st) for st in steps] for name, (cfg, steps) in scenarios.items()}


def _flat(res):
    """the per-frame results of a scenario's extraction steps, in call order"""
    out = []
    for r in res:
        out.extend(r if isinstance(r, list) else ([r] if r.levels is not None else []))
    return out


def test_every_step_can_show_a_carry_over(scenarios, results):
    """Every extraction step returns keypoints on at least two levels and at least 30 in all, and no two consecutive extraction steps
    (for batches: consecutive frames) expect the same bytes -- a result left over from the call before can never pass for this call's."""
    for name, (cfg, steps) in scenarios.items():
        flat = _flat(results[name])
        assert flat, name
        counts = [len(r.kp) // 28 for r in flat]
        populated = [sum(1 for n in r.levels if n > 0) for r in flat]
        print("%-28s steps %2d  frames %3d  smallest keypoint count %4d  fewest levels populated %d" % (name, len(steps), len(flat), min(counts), min(populated)))
        for i, r in enumerate(flat):
            assert populated[i] >= 2, (name, i, r.levels)
            assert counts[i] >= 30, (name, i, counts[i])
            if i:
                assert r.kp != flat[i - 1].kp, (name, i)
                assert r.cands != flat[i - 1].cands, (name, i)


def test_repeated_first_image_expects_the_first_bytes(scenarios, results):
    """the walks come back to their first image: the expected bytes of that step are those of the first"""
    for name in [n for n in scenarios if n.startswith("size walk")]:
        first, again = results[name][0], results[name][6]
        assert first.kp == again.kp and np.array_equal(first.desc, again.desc), name
        cfg, steps = scenarios[name]
        assert [st.img.shape[1] for st in steps[6:]] == [sc.MAX_W] * 3 and steps[7].img.shape[0] < sc.MAX_H       # only the height changes
    for name in ("mode walk 320 x 256", "mode walk 253 x 190"):
        assert results[name][0].kp == results[name][7].kp, name


def test_the_topup_steps_mutate_their_grids(scenarios, results):
    for name in ("mode walk 320 x 256", "mode walk 253 x 190"):
        cfg, steps = scenarios[name]
        grids = {st.name[:2].strip(): r.grid for st, r in zip(steps, results[name]) if st.op in ("topup", "tracked")}
        h, w = steps[0].img.shape
        assert grids["2"].shape == (h // 20 + 2, w // 20 + 2) and grids["3"].shape == (h // 5 + 2, w // 5 + 2)
        assert grids["3"].size > 10 * grids["2"].size          # the grid -- and the staging behind it -- grows between the two calls
        kin = steps[1].kin
        for key in ("2", "3", "4a"):
            start = sc.occupancy_grid(kin, 20, w, h) if key != "3" else np.zeros_like(grids["3"])
            assert (grids[key] != start).sum() >= 20, (name, key)
        # a negative budget is no empty call in the reference (its caps compare against a negative number and never bite): new points are
        # accepted behind the caller's and mark their cells
        assert len(results[name][8].kp) // 28 > len(kin) and (grids["8"] != sc.occupancy_grid(kin, 20, w, h)).sum() >= 20, name


def test_fallback_claims(oracle, scenarios):
    """A step that claims the literal-7 fall-back has, on some level, a cell that holds a candidate at fastTh and another whose candidates
    all score between 7 and fastTh; the adaptive walk's frames lie clear of the 14 % / 22 % hysteresis band of decide_fast_pass
    (csrc/describe.hip), so that the per-level pass threshold depends on the last two calls alone."""
    claimed = 0
    for name, (cfg, steps) in scenarios.items():
        for st in steps:
            if not st.claims_fallback:
                continue
            img = oracle.clahe(st.img, 4.0, (12, 12)) if st.op == "clahe_full" else st.img
            per_level = sc.fallback_cells(oracle, cfg, img)
            assert any(hi and lo for hi, lo, _ in per_level), (name, st.name)
            claimed += 1
    assert claimed >= 3
    cfg, steps = scenarios["adaptive walk"]
    share = {}
    for st in steps:
        per_level = sc.fallback_cells(oracle, cfg, st.img)
        share[st.name] = [1.0 - len(hi) / cells for hi, _, cells in per_level]      # cells without a candidate at fastTh
        print("adaptive walk %-14s share of cells without a corner at fastTh per level: %s" % (st.name, " ".join("%.2f" % s for s in share[st.name])))
    assert max(share["normal"]) < 0.10 and max(share["normal again"]) < 0.10
    assert min(share["low contrast"]) > 0.30


def test_sizes_follow_the_handles_own_rule(oracle, synth):
    """The smallest accepted square comes from cvRound(size * invScale^l) over the extractor's own table, the side below it has a level
    under 56 px, every size of a walk is accepted by a 320 x 256 handle, and at 1.35 the walk changes `resize_fast` between steps."""
    uvo_synth = importlib.import_module("u-vip-slam_amd.synth")
    assert uvo_synth is synth
    for scale, nlevels in sc.WALK_PYRAMIDS:
        cfg = sc.walk_cfg(scale, nlevels)
        inv = oracle.extractor(cfg.nfeatures, scale, nlevels, cfg.fast_th).inv_scale
        side = sc.smallest_side(inv)
        assert side == sc.SMALLEST_SQUARE[(scale, nlevels)] and (side, side) in sc.WALK_SIZES[(scale, nlevels)]
        assert sc.level_side(side, inv, nlevels - 1) == 56 and sc.level_side(side - 1, inv, nlevels - 1) == 55
        assert sc.geom_probe(cfg, side, side)[0] == sc.GEOM_OK and sc.geom_probe(cfg, side - 1, side - 1)[0] == sc.GEOM_UNSUPPORTED
        fast = []
        for w, h in sc.WALK_SIZES[(scale, nlevels)]:
            verdict, dims, ok = sc.geom_probe(cfg, w, h)
            assert verdict == sc.GEOM_OK, (scale, w, h, verdict)
            assert dims == [(sc.level_side(w, inv, l), sc.level_side(h, inv, l)) for l in range(nlevels)]
            assert min(min(d) for d in dims) >= 56
            fast.append(tuple(ok))
        print("scale %.2f / %d  resize_fast per step: %s" % (scale, nlevels, fast))
        if scale == 1.35:
            assert any(a != b for a, b in zip(fast, fast[1:])) and (1, 1, 1) in fast and len(set(fast)) >= 3
        else:
            assert set(fast) == {(1,) * nlevels}
    # no width up to the handle's loses the 12-byte window at 1.33 (the module's docstring): 1.35 is where the walk has to go for it
    cfg = sc.walk_cfg(1.33, 3)
    for w in range(99, sc.MAX_W + 1):
        verdict, _, ok = sc.geom_probe(cfg, w, max(99, w * 4 // 5))
        assert verdict == sc.GEOM_OK and ok == [1, 1, 1], (w, verdict, ok)


def test_default_tile_plans_of_the_walk_sizes_stay_inside_their_planes(oracle, scenarios):
    """The fused pyramid launch walks a plan compiled per size: for every size of the walks the default plan, run on the host, stores
    every byte of a level's image and ring exactly once, keeps every tap window inside its LDS tile, and gives the oracle's planes --
    or does not exist because a level is outside the 12-byte window, which is exactly where `resize_fast` says so."""
    for scale, nlevels in sc.WALK_PYRAMIDS:
        cfg, steps = scenarios["size walk %.2f / %d" % (scale, nlevels)]
        for st in steps[:6]:
            h, w = st.img.shape
            fast = sc.geom_probe(cfg, w, h)[2]
            rc, same = sc.default_tile_plan_on_host(oracle, cfg, st.img)
            assert rc == (0 if all(fast) else 2) and same == all(fast), (scale, w, h, rc, same, fast)


def test_which_check_refuses_the_shapes_of_the_refusal_test():
    """Shapes of at most the handle's area that extract_batch_device (no check of the sides) hands to set_geometry(): the transposed
    shape exceeds the first capacity check at 1.2 / 4 but passes the first THREE at 1.35 / 3 and fails the row-table check; a strip of the
    same area fails the column-table check.  At 1.35 / 3 both also have another `resize_fast` than the handle's own size."""
    assert sc.geom_probe(sc.walk_cfg(1.2, 4), 256, 320)[0] == sc.GEOM_CAP_BLOCKS
    cfg = sc.walk_cfg(1.35, 3)
    own = sc.geom_probe(cfg, sc.MAX_W, sc.MAX_H)
    transposed, strip = sc.geom_probe(cfg, 256, 320), sc.geom_probe(cfg, 640, 110)
    assert own[0] == sc.GEOM_OK and transposed[0] == sc.GEOM_CAP_YTAB and strip[0] == sc.GEOM_CAP_XTAB
    assert transposed[2] != own[2]
    assert sc.geom_probe(cfg, 150, 256)[0] == sc.GEOM_UNSUPPORTED      # a level's detection window less than half as wide as high


def test_lds_of_the_two_handles(oracle):
    """the host formula: 1600 features on 2 levels need more than 64 KiB of dynamic LDS for the quad-tree, 300 on 4 levels far less"""
    lds = {}
    for cfg in (sc.BIG_CFG, sc.SMALL_CFG):
        oe = oracle.extractor(cfg.nfeatures, cfg.scale, cfg.nlevels, cfg.fast_th)
        sizes = [(sc.level_side(sc.MAX_W, oe.inv_scale, l), sc.level_side(sc.MAX_H, oe.inv_scale, l)) for l in range(cfg.nlevels)]
        lds[cfg] = sc.octree_lds(oe.quota, sizes)
    print("quad-tree LDS: %d and %d bytes" % (lds[sc.BIG_CFG], lds[sc.SMALL_CFG]))
    assert lds[sc.BIG_CFG] > 64 * 1024 and lds[sc.SMALL_CFG] < 16 * 1024
