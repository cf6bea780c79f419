"""Holds tests/projection_model.py: the numpy restatement of the six projection prologues against the oracle (bit for bit), against
verdicts derived by hand on the exact scene, and against the real-valued evaluator on the generic scenes.  No GPU.

The oracle takes the MapPoint members mfMinDistance / mfMaxDistance and forms the invariance bounds itself (0.8f x, 1.2f x), where the C
ABI and the model take the bounds.  A scene row whose bounds are not such products of one pair of members (`linked` false: PredictScale
at ratio 1/2, whose members would fail the distance test) cannot be put to the oracle and is left out of that comparison only.  The
oracle exposes no projection-only form of PIXEL_BOUNDED and PIXEL (it projects inside orc_search_by_projection_last / _frames and
returns matches): those two modes are held by the hand table and the evaluator alone.  NaN results compare as NaN (x86 produces the
negative quiet NaN, the device the positive one).

Forward-error constant.  On the generic scenes (GENERIC_POSES poses x GENERIC_N points per mode, this CPU) the model's worst distance
from the evaluator, in units of 2^-24 x the forward-error form of projection_model.evaluate, was
    u 1.95   v 1.93   Z 2.49   dist 1.58   cosine 2.28   ratio 1.22   log quotient 0.68        (worst of all: 2.49)
and C = 5.0 is that worst value with the factor of 2 for the tail of other seeds, rounded up.  A point is `too close` when one of its
margins is within C x 2^-24 x form of zero; at most 1 % of a scene may be.
"""
import numpy as np
import pytest

import projection_model as pm
from projection_model import f32, f64, LD, FRUSTUM, KF_RELOC, FUSE, PIXEL_BOUNDED, PIXEL, SIM3

C = 5.0
MEASURED_WORST = 2.49
MODES = list(zip(pm.ALL_MODES, pm.MODE_IDS))
mode_param = pytest.mark.parametrize("mode", pm.ALL_MODES, ids=pm.MODE_IDS)


def bits(a):
    a = np.asarray(a)
    if a.dtype != np.float32:
        return a
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def oracle_run(oracle, s, mode, sf, scale_factor, cos_limit=0.5, usable=None):
    """The oracle on the linked rows of a scene -> (rows, its outputs); None for a mode it has no projection-only form of"""
    m, rows = min(mode, SIM3), np.nonzero(s["linked"])[0]
    us = None if usable is None else usable[rows]
    if m in (PIXEL_BOUNDED, PIXEL):
        return None
    if m == SIM3:
        return rows, oracle.project_sim3(*s["chain"], s["cam"].array(), s["xyz"][rows], s["mf_min"][rows], s["mf_max"][rows], us, sf)
    return rows, oracle.project_points(m, s["cam"].array(), s["xyz"][rows], s["normal"][rows], s["mf_min"][rows], s["mf_max"][rows], us, sf, scale_factor, cos_limit)


def all_scenes(mode):
    yield "exact sf 2", pm.exact_scene(mode, 2.0), pm.T8, 2.0
    yield "exact sf 1.2f", pm.exact_scene(mode, f32(1.2)), pm.T8, f32(1.2)
    yield "exact repeated table", pm.exact_scene(mode, 2.0), pm.T8_REPEATED, 2.0
    yield "exact one level", pm.exact_scene(mode, 2.0), pm.T1, 2.0
    yield "depth", pm.depth_scene(mode), pm.T8, 2.0
    yield "degenerate", pm.degenerate_scene(mode), pm.T8, 2.0
    yield "degenerate sf 1.2f", pm.degenerate_scene(mode), pm.SF12, f32(1.2)
    for p in range(pm.GENERIC_POSES):
        yield "generic %d" % p, pm.generic_scene(mode, p), pm.SF12, f32(1.2)


@mode_param
def test_model_equals_oracle(oracle, mode):
    if min(mode, SIM3) in (PIXEL_BOUNDED, PIXEL):
        assert not hasattr(oracle.L, "orc_project_pixel")          # no projection-only form: see the module docstring
        return
    for name, s, sf, sfac in all_scenes(mode):
        for usable in (None, pm.usable_mask(len(s["xyz"]))):
            rows, ref = oracle_run(oracle, s, mode, sf, float(sfac), usable=usable)
            got = pm.run_model(s, min(mode, SIM3), sf, sfac, usable=usable)
            assert len(rows) >= len(s["xyz"]) - 1, name
            for g, r, what in zip(got, ref, ("valid", "u", "v", "level", "view_cos")):
                assert g.dtype == r.dtype
                np.testing.assert_array_equal(bits(g[rows]), bits(r), err_msg="%s: %s" % (name, what))


_MARGIN_OF = {"u_max": ("u_max", "u_max_open"), "u_min": ("u_min",), "v_max": ("v_max", "v_max_open"), "v_min": ("v_min",), "dist_min": ("dist_min",),
              "dist_max": ("dist_max",), "cos_frustum": ("cos",), "cos_fuse": ("cos",)}
# the boundaries every mode must hold: tag -> the modes that have the test (ratio_* stands for all seven ratio_<entry> rows)
_HAS = {"u_max": (0, 1, 2, 3, 5), "u_min": (0, 1, 2, 3, 5), "v_max": (0, 1, 2, 3, 5), "v_min": (0, 1, 2, 3, 5), "dist_min": (0, 2, 5), "dist_max": (0, 2, 5),
        "cos_frustum": (0,), "cos_fuse": (2,), "ratio_": (1, 2, 5)}


def _margin(E, s, tag):
    if tag.startswith("ratio_"):
        return E["ratio"] - LD(float(tag[6:]))
    for k in _MARGIN_OF[tag]:
        if k in E["margins"]:
            return E["margins"][k]
    raise KeyError(tag)


@mode_param
@pytest.mark.parametrize("sfac", [2.0, f32(1.2)], ids=["sf2", "sf1.2f"])
def test_exact_scene_against_the_hand_table(mode, sfac):
    m = min(mode, SIM3)
    s = pm.exact_scene(mode, sfac)
    valid, u, v, level, vc, inter = pm.run_model(s, m, pm.T8, sfac, full=True)
    want = pm.expected_valid(s, mode)
    assert (want >= 0).all()
    np.testing.assert_array_equal(valid, want, err_msg=str(s["tag"]))
    E = pm.run_evaluator(s, m, pm.T8, sfac)
    side, row = s["side"], s["row"]
    on = side == 0
    # rows on a boundary and plain rows: every intermediate is exact, the model equals the evaluator
    plain = on & (row >= 0)
    np.testing.assert_array_equal(valid[plain] != 0, E["valid"][plain])
    for i in np.nonzero(plain)[0]:
        r = pm.EXACT_ROWS[row[i]]
        if r[0] in ("u_max", "u_min", "v_max", "v_min") or not valid[i]:
            pass
        elif m in (KF_RELOC, FUSE, SIM3):
            assert level[i] == r[12] == E["level"][i], r[0]
        elif m == FRUSTUM and float(sfac) == 2.0 and r[13] is not None:
            assert level[i] == r[13] == E["level"][i], r[0]
        if valid[i]:
            assert LD(u[i]) == E["u"][i] and LD(v[i]) == E["v"][i], r[0]
            if r[0] not in ("u_max", "u_min", "v_max", "v_min") and "dist" in inter:
                assert LD(inter["dist"][i]) == E["dist"][i], r[0]
            if m == FRUSTUM and r[0].startswith("cos"):               # 1.5 / 3: the one cosine here that fp32 holds exactly
                assert LD(vc[i]) == E["cos"][i] == 0.5, r[0]
    # neighbours: the verdict the evaluator gives, a margin of 0 on the boundary and opposite signs on its two sides
    nb = side != 0
    np.testing.assert_array_equal(valid[nb] != 0, E["valid"][nb])
    seen = set()
    for i in np.nonzero(nb & (side < 0))[0]:
        tag, j = s["tag"][i], [k for k in np.nonzero(nb & (side > 0))[0] if row[k] == row[i]][0]
        mg = _margin(E, s, tag)
        assert mg[row[i]] == 0 and mg[i] * mg[j] < 0, (tag, mg[row[i]], mg[i], mg[j])
        seen.add("ratio_" if tag.startswith("ratio_") else tag)
        if tag.startswith("ratio_"):                                  # on the entry and below it -> its index, above it -> the next (clamped)
            k = int(np.argmax(pm.T8 == f32(float(tag[6:]))))
            assert level[row[i]] == k and level[i] == k and level[j] == min(k + 1, 7), tag
    assert seen == {t for t, ms in _HAS.items() if m in ms}
    if m in (KF_RELOC, FUSE, SIM3):
        assert sum(t.startswith("ratio_") and sd == 1 for t, sd in zip(s["tag"], side)) == 7
    # PredictScale at ratio = sf^k: in view, and with scale factor 2 and k a power of two (exact logs) the level of real arithmetic
    ps = [i for i, k in enumerate(s["ps_k"]) if k is not None]
    if m == FRUSTUM:
        assert [s["ps_k"][i] for i in ps] == pm.PS_K and valid[ps].all()
        for i in ps:
            if float(sfac) == 2.0 and s["ps_k"][i] in (0, 1, 2, 4, 8):
                assert level[i] == pm.PS_LEVEL_REAL[pm.PS_K.index(s["ps_k"][i])]
            assert abs(int(level[i]) - pm.PS_LEVEL_REAL[pm.PS_K.index(s["ps_k"][i])]) <= 1
    # controls
    i_b = s["tag"].index("behind")
    assert bool(valid[i_b]) == (m in (KF_RELOC, PIXEL_BOUNDED, PIXEL))
    masked = pm.run_model(s, m, pm.T8, sfac, usable=pm.usable_mask(len(valid)))
    assert valid[0] == 1 and masked[0][0] == 0 and masked[1][0] == 0 and masked[3][0] == 0
    assert (pm.run_model(s, m, pm.T1, sfac)[3] == 0).all()
    if m in (KF_RELOC, FUSE, SIM3):
        rep = pm.run_model(s, m, pm.T8_REPEATED, sfac)
        Er = pm.run_evaluator(s, m, pm.T8_REPEATED, sfac)
        ok = plain & (rep[0] != 0)
        np.testing.assert_array_equal(rep[3][ok], Er["level"][ok])
        assert rep[3][s["tag"].index("ratio_1.5")] == 2 and rep[3][s["tag"].index("ratio_2")] == 4
    if m == KF_RELOC:                                                 # cam->ow is not read
        t = dict(s, cam=s["cam"].with_ow(np.full(3, np.nan)))
        for a, b in zip(pm.run_model(t, m, pm.T8, sfac), (valid, u, v, level, vc)):
            np.testing.assert_array_equal(bits(a), bits(b))


@mode_param
def test_depth_boundary(mode):
    m = min(mode, SIM3)
    s = pm.depth_scene(mode)
    valid, u, v, level, vc = pm.run_model(s, m, pm.T8, 2.0)
    assert valid.tolist() == [int(w[m]) for w in pm.DEPTH_VALID]
    Z = pm.run_evaluator(s, m, pm.T8, 2.0)["Z"]
    assert Z[0] == 0 and Z[1] == 0 and np.signbit(s["xyz"][1, 2]) and Z[2] < 0 < Z[3] and Z[3] == -Z[2] == LD(2.0) ** -149
    if m == FRUSTUM:                                                  # +inf -> (int) -> INT_MIN -> level 0, what the x86-64 build does
        assert np.isnan(u[[0, 1, 3]]).all() and (level == 0).all()


def _forms_and_errors(s, m, sf, sfac):
    out = pm.run_model(s, m, sf, sfac, full=True)
    inter, E = out[5], pm.run_evaluator(s, m, sf, sfac)
    F, err = E["forms"], {}
    with np.errstate(all="ignore"):
        for k in ("u", "v", "Z", "dist"):
            if k in inter and k in E:
                err[k] = np.abs(inter[k].astype(LD) - E[k]) / (pm.EPS * F[k])
        if m == FRUSTUM:
            err["cos"] = np.abs(inter["vc"].astype(LD) - E["cos"]) / (pm.EPS * F["cos"])
            q = pm.logf(inter["ratio"]) / pm.logf(f32(sfac))
            err["q"] = np.abs(q.astype(LD) - E["q"]) / (pm.EPS * F["q"])
        elif m == FUSE:
            err["cos"] = np.abs((inter["dot"] - 0.5 * inter["dist"].astype(f64)).astype(LD) - E["cos"]) / (pm.EPS * F["cos"])
        if m in (KF_RELOC, FUSE, SIM3):
            err["ratio"] = np.abs(inter["ratio"].astype(LD) - E["ratio"]) / (pm.EPS * F["ratio"])
    return out, E, err


_FORM_OF = {"depth": "Z", "u_min": "u", "u_max": "u", "u_max_open": "u", "v_min": "v", "v_max": "v", "v_max_open": "v", "dist_min": "dist", "dist_max": "dist", "cos": "cos"}


@mode_param
def test_generic_scene_against_the_evaluator(mode):
    m = min(mode, SIM3)
    worst = {}
    for p in range(pm.GENERIC_POSES):
        s = pm.generic_scene(mode, p)
        (valid, u, v, level, vc, inter), E, err = _forms_and_errors(s, m, pm.SF12, f32(1.2))
        for k, e in err.items():
            worst[k] = max(worst.get(k, 0.0), float(np.nanmax(np.where(np.isfinite(e), e, 0))))
            assert worst[k] <= C, (k, worst[k])
        close = np.zeros(len(valid), bool)
        for k, mg in E["margins"].items():
            form = E["forms"]["q" if m == FRUSTUM else "ratio"] if k == "level" else E["forms"][_FORM_OF[k]]
            near = np.abs(mg) <= C * pm.EPS * form
            close |= near if k != "level" else (near & E["valid"])
        assert close.mean() <= 0.01, close.mean()
        np.testing.assert_array_equal(valid[~close] != 0, E["valid"][~close])
        both = ~close & E["valid"]
        np.testing.assert_array_equal(level[both], E["level"][both])
        if m not in (PIXEL_BOUNDED, PIXEL):
            # FUSE and SIM3 admit dist >= min_inv only, so ratio >= 1 = sf[0] and level 0 needs dist == min_inv exactly: the exact
            # scene's dist_min row holds it; a drawn point cannot
            lowest = 1 if m in (FUSE, SIM3) else 0
            assert set(level[valid != 0].tolist()) == set(range(lowest, 8)), sorted(set(level[valid != 0].tolist()))
        assert valid.sum() > 300
    print("%s: worst model error in units of 2^-24 x form: %s" % (pm.MODE_IDS[mode], {k: round(x, 2) for k, x in worst.items()}))
    assert max(worst.values()) <= C


def test_the_unpinned_gemm_assumption_is_reported(capsys):
    """Reported, not asserted: how far u and v move, in units of C x 2^-24 x form, when R P + t accumulates in double (the general gemm
    path) instead of the fp32 row sum the model assumes."""
    worst = 0.0
    for p in range(pm.GENERIC_POSES):
        s = pm.generic_scene(FRUSTUM, p)
        cam = s["cam"]
        _, _, _, _, _, inter = pm.run_model(s, PIXEL, pm.SF12, f32(1.2), full=True)
        E = pm.run_evaluator(s, PIXEL, pm.SF12, f32(1.2))
        P = s["xyz"].astype(f64)
        R, t = cam.rcw.astype(f64).reshape(3, 3), cam.tcw.astype(f64)
        X, Y, Z = [(R[i, 0] * P[:, 0] + R[i, 1] * P[:, 1] + R[i, 2] * P[:, 2] + t[i]).astype(f32) for i in range(3)]
        with np.errstate(all="ignore"):
            invz = (1.0 / Z.astype(f64)).astype(f32)
            u2, v2 = cam.fx * X * invz + cam.cx, cam.fy * Y * invz + cam.cy
            d = np.maximum(np.abs(u2.astype(LD) - inter["u"].astype(LD)) / E["forms"]["u"], np.abs(v2.astype(LD) - inter["v"].astype(LD)) / E["forms"]["v"])
        worst = max(worst, float(np.nanmax(d)) / (C * pm.EPS))
    with capsys.disabled():
        print("\ndouble-accumulating R P + t moves u / v by at most %.3f x the forward-error bound (C = %g)" % (worst, C))
