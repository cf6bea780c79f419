"""k_octree<256> and k_octree<1024> (csrc/octree.hip, octree_core.hpp, octree_pyramid.hpp) on candidate lists of the test's choosing:
the batches of tests/octree_cases.py go through uvo_extractor_octree_tap -- the lists written where k_fast_score leaves them, then
launch_octree unchanged -- in both workgroup sizes and two orders of the device arrays each.  Everything is integer code and every
comparison is exact: each problem's selected list in the kernel's order against the std::list restatement of DistributeOctTree, the
gathered candidate count and the fall-back cell count against the numpy statement of the gather, and no cursor word or cell flag left
non-zero.  tests/test_octree_cases.py proves on the CPU which of run_pyramid, run<8> and run<0> each problem takes in each form; the
path is printed next to the form that was launched.

A mismatch here with the host emulation passing points at what only the device build has: the shuffle scan (block_scan_excl), the rank
sort (block_sort), oct_bcast, PointRegs in registers, the LDS carve under the handle's Mmax, the ready-made path tables, pstate in HBM."""
import numpy as np
import pytest

import octree_cases as oc

pytestmark = pytest.mark.gpu

FORMS = {256: 0, 1024: 1 << 20}      # threads per workgroup -> UVO_TUNE_OCT_WIDE_MAX (the batches have at most 12 problems)


@pytest.fixture(scope="module")
def handles(uvo, synth):
    """one extractor per handle of the cases, each behind a completed extract call (the tap needs the geometry and the lane)"""
    made = {}

    def get(name):
        if name not in made:
            w, h, nfeatures = oc.HANDLES[name]
            ex = uvo.ORBextractor(nfeatures, oc.SCALE, oc.NLEVELS, 0, 20, max_width=w, max_height=h, max_batch=3)
            ex(synth.make_frame(700, w, h, n_shapes=60))
            made[name] = ex
        return made[name]
    yield get
    for ex in made.values():
        ex.close()


def _run(uvo, ex, oracle, b, nt, variant):
    want = oc.expected(oracle, b)
    problems, flags = oc.device_lists(b, variant)
    ex.tune(uvo.UVO_TUNE_OCT_WIDE_MAX, FORMS[nt])
    got = ex.octree_tap(problems, flags)
    lv = oc.levels(b.handle)
    assert got.threads == nt, (b.name, got.threads)
    for (f, l), (sel, cand_count, fcount, cand) in sorted(want.items()):
        if variant == 0:
            print("%-28s %4d threads  frame %d level %d  P %5d  N %3d  %s" % (b.name, got.threads, f, l, cand_count, lv[l].quota, oc.path(nt, lv[l], cand, lv[l].quota)))
        where = "%s, %d threads, order %d, frame %d level %d" % (b.name, nt, variant, f, l)
        assert got.cand_count[f, l] == cand_count, where
        assert got.fcount[f, l] == fcount, where
        assert got.sel_count[f, l] == len(sel), where
        if got.selected[f][l] != sel:
            first = next(i for i, (a, c) in enumerate(zip(got.selected[f][l], sel)) if a != c)
            pytest.fail("%s: %d selected as the reference, entry %d is %s, the reference has %s" % (where, len(sel), first, got.selected[f][l][first], sel[first]))
    assert got.residue == (0, 0), (b.name, nt, got.residue)


@pytest.mark.parametrize("nt", [256, 1024])
@pytest.mark.parametrize("name", oc.names())
def test_case_equals_the_reference(uvo, oracle, handles, name, nt):
    b = oc.by_name(name)
    ex = handles(b.handle)
    for variant in oc.VARIANTS:
        _run(uvo, ex, oracle, b, nt, variant)


@pytest.mark.parametrize("name", ["main", "big"])
def test_extract_after_taps_equals_the_oracle(uvo, oracle, synth, handles, name):
    """the tap leaves the lane as an extract call expects it: cursors, flags and the fall-back list zero, nothing of the injected lists
    in the next frames' keypoints -- a batch of three and a single frame, after tap calls in both forms"""
    w, h, nfeatures = oc.HANDLES[name]
    ex = handles(name)
    b = oc.by_name("mixed batch" if name == "main" else "big: random 6000")
    for nt in (256, 1024):
        _run(uvo, ex, oracle, b, nt, 1)
        ex.tune(uvo.UVO_TUNE_OCT_WIDE_MAX, FORMS[nt])
        frames = np.stack([synth.make_frame(810 + i, w, h, n_shapes=120) for i in range(3)])
        oe = oracle.extractor(nfeatures, oc.SCALE, oc.NLEVELS, 20)
        outs = ex.extract_batch(frames) + [ex(frames[1])]
        for (kp, de), img in zip(outs, list(frames) + [frames[1]]):
            kp_o, de_o = oe(img)
            assert len(kp) == len(kp_o) > 100, (len(kp), len(kp_o))
            assert kp.tobytes() == kp_o.tobytes() and (de == de_o).all()


def test_refusals(uvo, oracle, handles):
    """every refusal is UVO_E_BADARG and is followed by a good call on the same handle"""
    w, h, nfeatures = oc.HANDLES["main"]
    fresh = uvo.ORBextractor(nfeatures, oc.SCALE, oc.NLEVELS, 0, 20, max_width=w, max_height=h, max_batch=3)
    ex = handles("main")
    lv = oc.levels("main")
    good = oc.by_name("two adjacent")
    nfl = oc.flags_per_frame("main")
    empty = np.zeros((0, 3), np.int64)

    def frame(level, hi, lo=empty):
        return [(np.asarray(hi, np.int64).reshape(-1, 3), np.asarray(lo, np.int64).reshape(-1, 3)) if l == level else (empty, empty) for l in range(oc.NLEVELS)]

    def refused(handle, problems, flags=None):
        with pytest.raises(uvo.UvoError) as ei:
            handle.octree_tap(problems, np.zeros((max(len(problems), 1), nfl), np.uint8) if flags is None else flags)
        assert ei.value.code == uvo.UVO_E_BADARG, ei.value
        if handle is ex:
            _run(uvo, ex, oracle, good, 256, 0)

    try:
        refused(fresh, [frame(0, [[100, 100, 50]])])                                     # no geometry yet
    finally:
        fresh.close()
    refused(ex, [])                                                                      # batch 0
    refused(ex, [frame(0, [[100, 100, 50]])] * 4)                                        # batch above max_batch
    L = lv[0]
    for x, y in ((2, 100), (L.bw - 3, 100), (100, 2), (100, L.bh - 3)):                  # one outside the window's interior, each side
        refused(ex, [frame(0, [[x, y, 50]])])
        refused(ex, [frame(0, [[50, 50, 50]], [[x, y, 50]])])
    refused(ex, [frame(1, [[lv[1].bw - 3, 10, 50]])])                                    # inside level 0's window, outside level 1's
    refused(ex, [frame(0, [[100, 100, 256]])])                                           # scores
    refused(ex, [frame(0, [], [[100, 100, 256]])])
    refused(ex, [frame(0, [[100, 100, -1]])])
    L3 = lv[3]
    rng = np.random.default_rng(3)
    over = np.concatenate([oc._uniform(L3, L3.cand_cap + 1, rng), np.full((L3.cand_cap + 1, 1), 9)], 1)
    refused(ex, [frame(3, over[:2000], over[2000:])])                                    # cand_cap + 1 in both lists together
    full = oc.Problem(over[:2000], over[2000:-1], np.zeros((L3.nRows, L3.nCols), np.uint8), False)   # cand_cap itself is taken, and right
    _run(uvo, ex, oracle, oc.Batch("level 3 filled to cand_cap", "main", [[oc._free(lv[0]), oc._free(lv[1]), oc._free(lv[2]), full]], {}, ""), 256, 0)
    refused(ex, [frame(0, [[100, 100, 50], [100, 100, 60]])])                            # the same (x, y) twice: in one list
    refused(ex, [frame(0, [[100, 100, 50]], [[7, 7, 9], [100, 100, 60]])])               # across the two lists
    refused(ex, [frame(0, [[100, 100, 50]])], np.zeros((1, nfl + 1), np.uint8))          # not the handle's flag grid
    refused(ex, [frame(0, [[100, 100, 50]])], np.zeros((1, nfl - 1), np.uint8))
