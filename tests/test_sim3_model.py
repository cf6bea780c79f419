"""What tests/sim3_model.py believes about USLAM::Sim3Solver, pinned: the SetRansacParameters tables, the repeating triples of the subset
draw, iterate()'s AND against the PnPsolver's OR, the truncated thresholds, the four mutation switches the host build's seeded faults
correspond to, and the Horn tolerance -- measured here between the model's own two forms of computeT, the code under test taking no
part in it."""
import numpy as np

import pnpsolver_model as psm
import sim3_model as sm


def test_tables():
    for n, want in sm.CALL_SITE_TABLE.items():
        assert sm.derive_params(n, **sm.CALL_SITE) == want, n
    for n, want in sm.HEADER_TABLE.items():
        assert sm.derive_params(n, **sm.HEADER_DEFAULT) == want, n
    assert [sm.derive_params(n, **sm.CALL_SITE) for n in (3, 4, 5, 6, 7, 8)] == [14, 35, 70, 123, 196, 293]
    assert all(sm.derive_params(n, **sm.CALL_SITE) == 300 for n in range(9, 2000, 37))
    # minInliers == N is one iteration; fewer points than minInliers never iterate, and the derived value is 1 whatever log() makes of it
    assert sm.derive_params(2, 0.99, 2, 300) == 1 and sm.derive_params(6, 0.99, 6, 300) == 1 and sm.derive_params(5, 0.99, 6, 300) == 1
    assert sm.derive_params(50, 0.99, 0, 300) == 1          # epsilon 0: the ratio is -inf
    assert sm.derive_params(1000, 0.99, 2, 300) == 300      # the ratio is far beyond int: maxIterations


def test_repeated_triple_counts():
    for n, want in sm.REPEATS_OF_3000.items():
        g, gi = sm.GlibcRand(1), sm.GlibcRand(1)
        got = [sm.draw_subset(g, n, 3) for _ in range(3000)]
        meant = [sm.draw_subset_intended(gi, n, 3) for _ in range(3000)]
        repeats = [len(set(t)) < 3 for t in got]
        assert sum(repeats) == want, (n, sum(repeats))
        assert all(len(set(t)) == 3 for t in meant)
        assert [a != b for a, b in zip(got, meant)] == repeats      # the draw as written differs from the draw as meant where it repeats


def test_loop_condition_is_an_and():
    counts = [0] * 400
    m = sm.replay(0, 0, counts, 5, 14, 2)
    assert (m["performed"], m["no_more"], m["iterations"]) == (5, 0, 5)
    o = sm.replay(0, 0, counts, 5, 14, 2, loop_or=True)
    assert (o["performed"], o["no_more"]) == (14, 1)
    # the third call of five reaches mRansacMaxIts = 14 after four iterations
    m = sm.replay(10, 0, counts, 5, 14, 2)
    assert (m["performed"], m["no_more"], m["iterations"]) == (4, 1, 14)
    assert sm.replay(10, 0, counts, 5, 14, 2, loop_or=True)["performed"] == 5
    # exhausted: nothing runs, bNoMore
    m = sm.replay(14, 0, counts, 5, 14, 2)
    assert (m["performed"], m["no_more"]) == (0, 1)
    assert sm.iterations_ahead(10, 14, 5) == 4 and sm.iterations_ahead(0, 14, 5) == 5 and sm.iterations_ahead(14, 14, 5) == 0
    assert sm.iterations_ahead(10, 14, 5, loop_or=True) == 5 == psm.iterations_ahead(10, 14, 5)


def test_best_update_and_return():
    # >=: a later tie wins; a count of 0 replaces the initial best of 0
    m = sm.replay(0, 0, [0, 2, 2, 1, 0], 5, 14, 2)
    assert (m["best"], m["best_from"], m["returned"]) == (2, 2, -1)
    assert sm.replay(0, 0, [0, 2, 2, 1, 0], 5, 14, 2, strict_best=True)["best_from"] == 1
    assert sm.replay(0, 0, [0] * 5, 5, 14, 2)["best_from"] == 4 and sm.replay(0, 0, [0] * 5, 5, 14, 2, strict_best=True)["best_from"] == -1
    # the return is strict: count == minInliers does not return
    assert sm.replay(0, 0, [2] * 5, 5, 14, 2)["returned"] == -1
    m = sm.replay(0, 0, [2, 3, 9], 5, 14, 2)
    assert (m["returned"], m["performed"], m["inliers"], m["no_more"]) == (1, 2, 3, 0)
    # a return at the last iteration leaves bNoMore false
    m = sm.replay(13, 0, [5], 5, 14, 2)
    assert (m["returned"], m["iterations"], m["no_more"]) == (0, 14, 0)
    # a count below the best is no return, however large
    assert sm.replay(0, 9, [8, 8, 8, 8, 8], 5, 14, 2)["returned"] == -1
    # re-entry after a return: the first hypothesis that ties the best returns again; under > it does not
    assert sm.replay(1, 8, [8], 5, 293, 2)["returned"] == 0 and sm.replay(1, 8, [8, 8, 8, 8, 8], 5, 293, 2, strict_best=True)["returned"] == -1


def test_thresholds_are_truncated():
    sigma2 = (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
    got = sm.thresholds(sigma2)
    assert got[0] == 9 and sm.thresholds([1.44])[0] == 13
    assert (got == np.floor(9.210 * sigma2.astype(np.float64))).all() and got.dtype == np.float32
    loose = sm.thresholds(sigma2, truncate=False)
    assert (loose > got).all()                                      # the mutation is visible at every octave


def test_compute_t_recovers_a_true_similarity():
    c = sm.candidate(7, 12, 1.0, noise=0.0)
    x1c, x2c = sm.prepare(c[6], c[0])[0], sm.prepare(c[7], c[1])[0]
    s, R, t = c[8]
    g = sm.GlibcRand(1)
    seen = 0
    for _ in range(40):
        idx = sm.draw_subset(g, 12, 3)
        P1, P2 = x1c[idx].T, x2c[idx].T
        if not sm.well_conditioned(P1, P2, idx):
            continue
        m = sm.compute_t(P1, P2)
        assert m["finite"] and sm.sim3_deviation(m["s"], m["R"], m["t"], s, R, t) < 2e-3
        s64, R64, t64 = sm.horn64(P1, P2)
        assert sm.sim3_deviation(s64, R64, t64, s, R, t) < 2e-3
        _, _, inl, _ = sm.check_inliers(m["T12"], m["T21"], x1c, x2c, sm.to_image(x1c, c[6][2]), sm.to_image(x2c, c[7][2]), c[6][2], c[7][2],
                                        sm.thresholds(c[2]), sm.thresholds(c[3]))
        assert inl.all()
        seen += 1
    assert seen >= 20


def test_degenerate_triples_are_not_finite_or_harmless():
    c = sm.candidate(7, 12, 1.0, noise=0.0)
    x1c, x2c = sm.prepare(c[6], c[0])[0], sm.prepare(c[7], c[1])[0]
    same = sm.compute_t(x1c[[0, 0, 0]].T, x2c[[0, 0, 0]].T)
    assert not same["finite"]                                       # 0/0 in vec / norm(vec) and nom / den


def test_horn_tolerance():
    worst, at = 0.0, None
    for seed, n in sm.HORN_SCENES:
        x1c, x2c, triples = sm.horn_triples(seed, n)
        plain = [t for t in triples if len(set(t)) == 3]
        kept = [t for t in plain if sm.well_conditioned(x1c[t].T, x2c[t].T, t)]
        assert len(plain) - len(kept) <= sm.COND_MAX_LEFT_OUT * len(plain), (seed, n, len(plain), len(kept))
        for t in kept:
            m = sm.compute_t(x1c[t].T, x2c[t].T)
            s64, R64, t64 = sm.horn64(x1c[t].T, x2c[t].T)
            d = sm.sim3_deviation(m["s"], m["R"], m["t"], s64, R64, t64)
            if d > worst:
                worst, at = d, (seed, n, t)
    print("largest deviation between compute_t and horn64: %.6e at %s; HORN_TOL = %.6e" % (worst, at, sm.HORN_TOL))
    assert abs(worst / sm.HORN_MEASURED - 1) < 1e-3, (worst, sm.HORN_MEASURED)
    assert sm.HORN_TOL == 4 * sm.HORN_MEASURED
