"""What tests/octree_cases.py claims about its batches, proved without a GPU: the geometry the references use is the handle's, every
problem takes the path of octree_body it aims at for each workgroup size (tests/emu/octree_emu.cpp run with phases of 256 and of 1024
threads: emu_octree_algo(algo = 1) returns -2 exactly when the closed form gives up), the pass-per-generation form and the kernel's
combination equal the std::list reference on it, the tie cases contain ties that the candidate order decides, every refusal-free list
fits its level, and each handle's LDS request lies on the side of 64 KiB it was built for."""
import numpy as np
import pytest

import octree_cases as oc


def test_geometry_is_the_handles(oracle):
    for name, (w, h, nfeatures) in oc.HANDLES.items():
        e = oracle.extractor(nfeatures, oc.SCALE, oc.NLEVELS, 20)
        lv = oc.levels(name)
        assert (lv[0].w, lv[0].h) == (w, h)
        for l, L in enumerate(lv):
            assert L.quota == int(e.quota[l]), (name, l)
            assert (L.bw, L.bh) == (L.w - 26, L.h - 26)
            assert L.nIni == int(np.floor(np.float32(L.bw) / np.float32(L.bh) + np.float32(0.5)))
            assert (L.nCols, L.nRows) == (L.bw // 30, L.bh // 30) and (L.wCell, L.hCell) == (-(-L.bw // L.nCols), -(-L.bh // L.nRows))
            assert L.n_cells == int(L.is_cell.sum()) == L.nRows * L.nCols          # no grid position without a cell at these sizes
    assert oc.levels("main")[0][2:4] == (294, 230) and oc.levels("main")[0].quota == 161       # where the path-taking sets were probed
    assert oc.levels("three")[0].quota == 3
    assert oc.levels("wide")[0][2:4] == (374, 74) and oc.levels("wide")[0].nIni == 5


def test_names_are_the_batches():
    assert list(oc.NAMES) == [b.name for b in oc.batches()] and len(set(oc.NAMES)) == len(oc.NAMES)


def test_collecting_the_modules_loads_no_hip_library():
    """importing the cases and collecting both test modules must not bring a HIP runtime into the process (see NAMES)"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); import octree_cases as oc; oc.names(); import test_gpu_octree, test_octree_cases; "
            "maps = open('/proc/self/maps').read(); assert 'geom_emu' not in maps and 'amdhip' not in maps, 'a HIP library was loaded'" % here)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_lds_request_sides():
    """only the `big` handle makes prepare_octree() raise the kernel's dynamic-LDS limit"""
    got = {name: oc.lds_bytes(name) for name in oc.HANDLES}
    assert got["big"] > 65536, got
    assert all(v <= 65536 for k, v in got.items() if k != "big"), got
    assert got["big"] <= 160 * 1024                                                # what a workgroup of gfx950 can have


def test_lists_pass_the_taps_checks():
    """coordinates inside [3, bw - 3) x [3, bh - 3), scores 0 .. 255, both lists within cand_cap, no coordinate twice"""
    for b in oc.batches():
        for variant in oc.VARIANTS:
            problems, flags = oc.device_lists(b, variant)
            assert flags.shape == (len(b.problems), oc.flags_per_frame(b.handle)) and len(problems) <= 3
            for frame in problems:
                for L, (hi, lo) in zip(oc.levels(b.handle), frame):
                    both = np.concatenate([hi, lo])
                    assert len(both) <= L.cand_cap and len(both) <= 9000, (b.name, len(both))      # (the control group's longest list)
                    if len(both):
                        assert both[:, 0].min() >= 3 and both[:, 0].max() < L.bw - 3 and both[:, 1].min() >= 3 and both[:, 1].max() < L.bh - 3, b.name
                        assert both[:, 2].min() >= 0 and both[:, 2].max() <= 255
                        assert len(np.unique(both[:, :2], axis=0)) == len(both), b.name


def test_two_variants_differ_and_name_the_same_problem():
    for b in oc.batches():
        (p0, f0), (p1, f1) = (oc.device_lists(b, v) for v in oc.VARIANTS)
        assert (f0 == f1).all()
        for fr0, fr1 in zip(p0, p1):
            for (h0, l0), (h1, l1) in zip(fr0, fr1):
                a, c = np.concatenate([h0, l0]), np.concatenate([h1, l1])
                assert sorted(map(tuple, a.tolist())) == sorted(map(tuple, c.tolist()))
                if len(a) > 3:
                    assert a.tolist() != c.tolist(), b.name


@pytest.mark.parametrize("name", oc.names())
def test_case_takes_its_path_and_the_emulation_equals_the_reference(oracle, name):
    b = oc.by_name(name)
    want = oc.expected(oracle, b)
    lv = oc.levels(b.handle)
    rng = np.random.default_rng(5)
    for (f, l), (sel, cand_count, fcount, cand) in sorted(want.items()):
        L = lv[l]
        dev = cand[rng.permutation(len(cand))]                   # the device array is in arbitrary order
        for nt in (256, 1024):
            path = oc.path(nt, L, dev, L.quota)
            print("%-28s frame %d level %d P %5d N %3d  %4d threads: %s" % (name, f, l, len(cand), L.quota, nt, path))
            aim = b.aim.get((f, l), {}).get(nt)
            if aim is not None:
                assert path == aim, (name, f, l, nt, len(cand))
            if path == oc.EMPTY:
                assert sel == []
                continue
            k = 8 if len(cand) <= 8 * nt else 0
            for algo in (0, 2):                                     # passes only / as the kernel
                m, got = oc.emulate(nt, L, dev, L.quota, k, algo)
                assert m == len(sel) and got == sel, (name, f, l, nt, algo)
            # ... and in the device's shape: the handle's node capacity on every level, one carved block, ready-made path tables
            m, got = oc.emulate(nt, L, dev, L.quota, k, 2, handle=b.handle)
            assert m == len(sel) and got == sel, (name, f, l, nt, "device shape")
            if path == oc.PYRAMID:
                assert oc.emulate(nt, L, dev, L.quota, 0, 1)[1] == sel
        assert len(sel) <= L.sel_cap


def test_paths_cover_both_fallbacks_and_the_closed_form_in_both_sizes(oracle):
    seen = {256: set(), 1024: set()}
    for b in oc.batches():
        want = oc.expected(oracle, b)
        for (f, l), (sel, n, fc, cand) in want.items():
            for nt in (256, 1024):
                if b.aim.get((f, l), {}).get(nt):
                    seen[nt].add(b.aim[(f, l)][nt])
    for nt in (256, 1024):
        assert {oc.PYRAMID, oc.RUN8, oc.RUN0, oc.EMPTY} <= seen[nt], seen


@pytest.mark.parametrize("name", ["row, every score 50", "random 3000, scores 1 .. 3"])
def test_tie_cases_contain_ties_the_order_decides(oracle, name):
    """the same set handed to the reference in the reverse candidate order selects other pixels: some node's best score is shared"""
    b = oc.by_name(name)
    sel, n, fc, cand = oc.expected(oracle, b)[(0, 0)]
    L = oc.levels(b.handle)[0]
    e = oracle.extractor(oc.HANDLES[b.handle][2], oc.SCALE, oc.NLEVELS, 20)
    other = [tuple(s) for s in e.octree(cand[::-1], L.bw, L.bh, L.quota).tolist()]
    assert len(other) == len(sel) and other != sel
    assert [s[2] for s in other] == [s[2] for s in sel]          # the same scores, other pixels


def test_named_results(oracle):
    """the answers the issue's table names"""
    n_sel = lambda name: len(oc.expected(oracle, oc.by_name(name))[(0, 0)][0])
    assert n_sel("block 20 x 20") == 1 and n_sel("two adjacent") == 1 and n_sel("one pixel") == 1 and n_sel("empty") == 0
    assert n_sel("quota 3") == 4                                 # the first pass splits unconditionally
    assert n_sel("big: row") == 288                              # P < N: every node ends as a single point
    assert oc.expected(oracle, oc.by_name("band of 8 rows"))[(0, 0)][1] == 2304 and oc.expected(oracle, oc.by_name("band of 29 rows"))[(0, 0)][1] == 8352


def test_gather_cases_reach_their_edges(oracle):
    b = oc.by_name("gather: cell boundaries")
    for f, frame in enumerate(b.problems):
        for L, p in zip(oc.levels(b.handle), frame):
            x, y = p.lo[:, 0] - 3, p.lo[:, 1] - 3
            for k in range(1, L.nCols):
                assert (x == k * L.wCell - 1).any() and (x == k * L.wCell).any()
            for k in range(1, L.nRows):
                assert (y == k * L.hCell - 1).any() and (y == k * L.hCell).any()
            ci, cj = oc.cell_of(L, p.lo[:, 0], p.lo[:, 1])
            for s in (6, 7, 255):                                   # every score on a flagged and on an unflagged cell
                assert {0, 1} <= set(p.flags[ci, cj][p.lo[:, 2] == s].tolist()), (f, s)
            cand, fcount = oc.gather(L, p)
            assert 0 < fcount < L.n_cells and len(p.hi) < len(cand) < len(p.hi) + len(p.lo)
    for name, n in (("1", 1), ("8 x 256", 2048), ("8 x 256 + 1", 2049), ("8 x 1024", 8192), ("8 x 1024 + 1", 8193)):
        p = oc.by_name("gather: n_lo = " + name).problems[0][0]
        assert len(p.hi) == 0 and len(p.lo) == n
    small = oc.by_name("gather: 160 x 120")
    assert all(len(p.lo) == 0 and len(p.hi) > 0 and p.flags.all() for p in small.problems[1])
    assert all(oc.expected(oracle, small)[(1, l)][2] == 0 for l in range(4))
