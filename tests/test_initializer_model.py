"""The numpy model of the two-view initialisation (tests/initializer_model.py) against an independent double-precision computation:
numpy.linalg.svd for the null vector, the rank-2 projection and the essential decomposition, a DLT triangulation.  The worst
distances over the scene set are the project's yardsticks; the product is held to four times them (TOL_* of the model).  Nothing here
touches the product: these tests pass with or without it."""
import numpy as np
import pytest

import initializer_checks as ic
import initializer_model as im


@pytest.fixture(scope="module")
def measured():
    """Worst distances between the model and the independent computation over ic.model_scenes()."""
    out = {"null": 0.0, "F": 0.0, "R": 0.0, "t": 0.0, "point": 0.0, "accepted": 0}
    for spec in ic.model_scenes():
        k1, k2, m12, _ = ic.scene(*spec)
        r = ic.model_run(spec)
        T1, T2 = im.normalize(k1), im.normalize(k2)
        pn1, pn2 = im.normalized(T1, k1), im.normalized(T2, k2)
        for h in range(len(r.sets)):
            F, null = im.independent_f21(pn1[m12[r.sets[h]]], pn2[r.sets[h]], T1, T2)
            out["null"] = max(out["null"], im.sign_free_distance(r.null_row[h], null))
            out["F"] = max(out["F"], im.sign_free_distance(r.F[h], F))
        if r.initialized:
            R, t, pts = im.independent_pose(r.F21, ic.CAM, k1, k2, m12, r.inliers)
            out["accepted"] += 1
            out["R"] = max(out["R"], ic.rotation_distance(r.R21, R))
            out["t"] = max(out["t"], im.sign_free_distance(r.t21, t))
            out["point"] = max(out["point"], ic.point_distance(r.p3d, pts, r.triangulated))
    print("measured model-to-independent distances:", out)
    return out


def test_measured_distances_are_the_recorded_yardsticks(measured):
    assert measured["accepted"] >= 4
    for key, rec in (("null", im.MEASURED_NULL_ROW), ("F", im.MEASURED_F), ("R", im.MEASURED_R), ("t", im.MEASURED_T), ("point", im.MEASURED_POINT)):
        assert measured[key] <= rec * 1.0000001, "%s: measured %.4g, recorded %.4g" % (key, measured[key], rec)
        assert measured[key] >= rec * 0.5, "%s: the recorded yardstick %.4g is stale (measured %.4g)" % (key, rec, measured[key])


def test_completion_row_is_the_null_vector_of_the_eight_equations():
    spec = ic.model_scenes()[0]
    k1, k2, m12, _ = ic.scene(*spec)
    r = ic.model_run(spec)
    T1, T2 = im.normalize(k1), im.normalize(k2)
    A = im.design_rows(im.normalized(T1, k1)[m12[r.sets]], im.normalized(T2, k2)[r.sets]).astype(np.float64)
    resid = np.abs(np.einsum("hij,hj->hi", A, r.null_row.astype(np.float64))).max(1) / np.linalg.norm(A, axis=(1, 2))
    assert resid.max() < 1e-5 and np.allclose(np.linalg.norm(r.null_row.astype(np.float64), axis=1), 1, atol=1e-6)


def test_jacobi_singular_values_and_vectors_against_numpy():
    rng = np.random.RandomState(5)
    M = rng.normal(size=(50, 3, 3)).astype(np.float32)
    u, w, vt = im.svd33(M)
    assert np.allclose(w, np.linalg.svd(M.astype(np.float64), compute_uv=False), rtol=2e-5, atol=2e-6)
    assert np.abs(np.einsum("bij,bj,bjk->bik", u.astype(np.float64), w.astype(np.float64), vt.astype(np.float64)) - M).max() < 1e-5


def test_glibc_stream_and_sets():
    g = im.GlibcRand(1)
    assert [g.next() for _ in range(3)] == [1804289383, 846930886, 1681692777]      # rand() after srand(1)
    sets = im.draw_sets(im.GlibcRand(1), 8, 5)
    assert all(sorted(s) == list(range(8)) for s in sets.tolist())                  # N = 8: every set is a permutation


def test_both_verdicts_occur_and_the_scenes_are_conditioned():
    specs = ic.model_scenes()
    kept = [s for s in specs if ic.conditioned(s)]
    assert len(kept) * 4 >= len(specs) * 3                                          # at most a quarter dropped by the condition
    verdicts = {s: ic.model_run(s).initialized for s in specs}
    assert any(verdicts.values()) and not verdicts[(0, 64, 0.1, "rotation")]
    r = ic.model_run((0, 64, 0.1, "general"))
    R, t = ic.scene(0, 64, 0.1)[3]
    assert ic.rotation_distance(r.R21, R) < 0.02 and im.sign_free_distance(r.t21, t) < 0.2


def test_n_below_eight_has_no_result():
    k1, k2, m12, _ = ic.scene(0, 7, 0.0)
    g = im.GlibcRand(1)
    assert im.initialize(k1, k2, m12, ic.CAM, 1.0, 200, g) is None and g.n == 310
