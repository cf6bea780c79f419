"""The checks that hold an implementation of the visual-inertial pose optimisation to tests/navopt_model.py, layer by layer, and the
driver of the host build (tests/emu/navopt_emu.cpp).  tests/test_navopt_emu.py runs them on the host build and on its seeded mutations,
tests/test_gpu_navopt.py on the device (layers 2, 4, 5 and 6: what the trace tap and the result show).

The bounds of layers 1 to 3 and 6 are DERIVED, first order in u = 2^-53: (operations on the path) x u x (the model's sum of absolute
terms), x cond for a solve or an inverse; none is fitted to an observed difference.  T and M of layer 5 cannot be derived and are
MEASURED ON THE MODEL (measure_spread below), never on the code under test; DESIGN.md section 4 records the measurement."""
import ctypes
import math
import os

import numpy as np

import host_build
import navopt_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
MUTATIONS = {"NO_RESET": 1, "BREAK_ACTIVE": 2, "IMU_NO_KERNEL": 3, "DEPTH_SWAP": 4, "DEPTH_HALF": 5, "MARG_FRESH": 6, "MARG_SWAP": 7, "ORDER": 8, "HUBER_B": 9,
             "JRINV": 10}

# Layer 5, measured on the model over every scene of nm.SCENES under 4 random edge orders (measure_spread): the
# largest spread of any word of the final NavState was 6.2e-9, the largest change of any edge's chi2 at a classification 2.4e-6, and
# no mask changed in the 156 runs.
STATE_SPREAD, CHI2_SPREAD = 6.2e-9, 2.4e-6
T_STATE, M_CHI2 = 4 * STATE_SPREAD, 4 * CHI2_SPREAD


class Run:
    """What one call gave: ns (dict), Tcw float32[4, 4], n_inliers, rounds, outlier (a list of uint8 arrays, one per frame), marg_cov,
    marg_cov_inv, marg_ok and the trace (uvo.NavTrace)."""

    def __init__(self, ns, Tcw, n_inliers, rounds, outlier, marg_cov, marg_cov_inv, marg_ok, trace):
        self.ns, self.Tcw, self.n_inliers, self.rounds, self.outlier = ns, Tcw, n_inliers, rounds, outlier
        self.marg_cov, self.marg_cov_inv, self.marg_ok, self.trace = marg_cov, marg_cov_inv, marg_ok, trace


OUT_DTYPE = np.dtype([("ns", "<f8", 22), ("Tcw", "<f4", 16), ("n_inliers", "<i4"), ("rounds", "<i4"), ("marg_ok", "<i4"), ("pad_", "<i4"), ("marg_cov", "<f8", 225),
                      ("marg_cov_inv", "<f8", 225)])


def states(est):
    return np.ascontiguousarray(np.stack([nm.state_vec(est[0]), nm.state_vec(est[1])]))


def full_of_tri(tri, nd):
    """The packed upper triangle of a trace record -> the symmetric nd x nd matrix."""
    H = np.zeros((nd, nd))
    H[np.triu_indices(nd)] = np.asarray(tri)[:nd * (nd + 1) // 2]
    return H + np.triu(H, 1).T


class Emu:
    """tests/emu/navopt_emu.cpp, built on first use with the library's contract: no FMA contraction.  `mutation`: a key of MUTATIONS,
    compiled into a library of its own."""
    _libs = {}

    def __init__(self, uvo, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.uvo = uvo
        if mutation not in Emu._libs:
            variant = (["-DNAVOPT_MUT=%d" % MUTATIONS[mutation]], "_" + mutation.lower()) if mutation else ()
            L = ctypes.CDLL(host_build.build("navopt_emu", *variant))
            vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
            L.emu_nav_so3.argtypes = [ci, vp, vp]
            L.emu_nav_so3.restype = None
            L.emu_nav_reproj.argtypes = [vp, vp, vp, ci, vp]
            L.emu_nav_single.argtypes = [vp, vp, vp, vp, vp, vp]
            L.emu_nav_linearise.argtypes = [vp, vp, vp, vp, ci, vp, vp]
            L.emu_nav_linearise.restype = cd
            L.emu_nav_trial.argtypes = [vp, vp, vp, vp, ci, vp, vp, cd, vp, vp, vp]
            L.emu_nav_marginals.argtypes = [vp, vp, vp]
            L.emu_nav_optimize.argtypes = [vp, vp, vp, vp, vp]
            L.emu_nav_optimize.restype = None
            assert L.emu_nav_mutation() == (MUTATIONS[mutation] if mutation else 0)
            assert (L.emu_nav_sizes(0), L.emu_nav_sizes(1)) == (nm.PROBLEM_DTYPE.itemsize, OUT_DTYPE.itemsize)
            Emu._libs[mutation] = L
        self.L = Emu._libs[mutation]

    def so3(self, what, v, n_out):
        v, out = np.ascontiguousarray(v, np.float64), np.zeros(n_out)
        self.L.emu_nav_so3(what, v.ctypes.data, out.ctypes.data)
        return out

    def reproj(self, sc, s, edge, robust=True):
        r, sv, e, out = nm.record(sc), np.ascontiguousarray(nm.state_vec(s)), np.ascontiguousarray(edge, np.float32), np.zeros(17)
        self.L.emu_nav_reproj(r.ctypes.data, sv.ctypes.data, e.ctypes.data, int(robust), out.ctypes.data)
        return out

    def single(self, sc, est):
        r, sv = nm.record(sc), states(est)
        e, J, sing, oimu = np.zeros(31), np.zeros((31, 30)), np.zeros((3, 4)), np.zeros((9, 9))
        self.L.emu_nav_single(r.ctypes.data, sv.ctypes.data, e.ctypes.data, J.ctypes.data, sing.ctypes.data, oimu.ctypes.data)
        return e, J, sing, oimu

    @staticmethod
    def level_bytes(sc, active):
        return np.ascontiguousarray(np.concatenate([(~np.asarray(a, bool)).astype(np.uint8) for a in active] + [np.zeros(1, np.uint8)]))

    def linearise(self, sc, est, active, robust):
        r, sv, e, st = nm.record(sc), states(est), nm.all_edges(sc), self.level_bytes(sc, active)
        H, b = np.zeros((30, 30)), np.zeros(30)
        chi = self.L.emu_nav_linearise(r.ctypes.data, sv.ctypes.data, e.ctypes.data, st.ctypes.data, int(robust), H.ctypes.data, b.ctypes.data)
        nd = nm.nd_of(sc)
        H = np.triu(H[:nd, :nd])
        return H + np.triu(H, 1).T, b[:nd].copy(), chi

    def trial(self, sc, est, active, robust, H, b, lam, dx_prev=None):
        nd = nm.nd_of(sc)
        r, sv, e, st = nm.record(sc), states(est), nm.all_edges(sc), self.level_bytes(sc, active)
        Hf, bf, dx = np.zeros((30, 30)), np.zeros(30), np.zeros(30)
        Hf[:nd, :nd], bf[:nd] = H, b
        if dx_prev is not None:
            dx[:nd] = dx_prev
        so, out = np.zeros((2, 22)), np.zeros(2)
        ok = self.L.emu_nav_trial(r.ctypes.data, sv.ctypes.data, e.ctypes.data, st.ctypes.data, int(robust), Hf.ctypes.data, bf.ctypes.data, lam, dx.ctypes.data,
                                  so.ctypes.data, out.ctypes.data)
        return bool(ok), dx[:nd].copy(), [nm.state_of_vec(so[0]), nm.state_of_vec(so[1])], out

    def marginals(self, sc, H):
        nd = nm.nd_of(sc)
        r, Hf, out = nm.record(sc), np.zeros((30, 30)), np.zeros(1, OUT_DTYPE)
        Hf[:nd, :nd] = H
        ok = self.L.emu_nav_marginals(r.ctypes.data, Hf.ctypes.data, out.ctypes.data)
        return bool(ok), out["marg_cov"][0].reshape(15, 15).copy(), out["marg_cov_inv"][0].reshape(15, 15).copy()

    def optimize(self, sc):
        r, e = nm.record(sc), nm.all_edges(sc)
        n, nl = int(r["n"][0]), int(r["n_last"][0])
        out, mask, tr = np.zeros(1, OUT_DTYPE), np.zeros(n + nl + 1, np.uint8), self.uvo.NavTraceC()
        self.L.emu_nav_optimize(r.ctypes.data, e.ctypes.data, out.ctypes.data, mask.ctypes.data, ctypes.byref(tr))
        o = out[0]
        masks = [mask[:n].copy()] + ([mask[n:n + nl].copy()] if sc["form"] == nm.FRAME else [])
        return Run(nm.state_of_vec(o["ns"]), o["Tcw"].reshape(4, 4).copy(), int(o["n_inliers"]), int(o["rounds"]), masks, o["marg_cov"].reshape(15, 15).copy(),
                   o["marg_cov_inv"].reshape(15, 15).copy(), int(o["marg_ok"]), self.uvo.NavTrace(tr))


_MODEL = {}


def model(name):
    """The model's run of a named scene: computed once, shared, never changed."""
    if name not in _MODEL:
        sc = nm.make(name)
        _MODEL[name] = (sc, nm.optimize(sc))
    return _MODEL[name]


def start_of(sc):
    """The estimates every round starts from: the input states, their quaternions normalised."""
    return [dict(sc["cur"], q=nm.qnorm(sc["cur"]["q"])), dict(sc["last"], q=nm.qnorm(sc["last"]["q"]))]


# ---- layer 1: one edge ----------------------------------------------------------------------------------------------------------------
ROWS = dict(prior=0, imu=15, bias=24, depth=30)


def magnitude(sc, est):
    """The sum of the absolute values (inf-norms) of everything a single edge's residual adds up: the scale its roundings are relative to."""
    a = lambda v: float(np.abs(np.asarray(v, np.float64)).max())
    dT = float(sc["dT"])
    m = 0.0
    for s in list(est) + [sc["prior"]]:
        m += a(s["P"]) + a(s["V"]) * (1 + dT) + a(s["bg"]) + a(s["ba"]) + a(s["dbg"]) + a(s["dba"])
    db = max(a(est[1]["dbg"]), a(est[1]["dba"]))
    m += a(sc["gw"]) * (dT + dT * dT) + 9.81 * dT * dT + a(sc["dP"]) + a(sc["dV"]) + (a(sc["JPg"]) + a(sc["JPa"]) + a(sc["JVg"]) + a(sc["JVa"]) + a(sc["JRg"])) * 3 * db
    m += abs(float(sc["depth_meas"])) * (1 + abs(float(sc["shi"]))) + dT
    return m


def single_bounds(sc, est):
    """de (per row) and dJ (one number) of the single edges against the model at equal estimates.
    Derivation.  A position, velocity, bias or depth row is a chain of at most 64 additions and products of quantities whose absolute
    values sum to at most magnitude(); rotating by a unit quaternion or a rotation matrix multiplies that sum by at most 4 (three
    products of factors <= 1 and the doubling in q * v): 256 u (1 + magnitude).  A rotation row is the log of a product of four unit
    quaternions: 4 x 28 operations on values <= 1, four normalisations, exp's sin and cos (4 u absolute each) and the atan (4 u),
    multiplied by 2 atan(n / w) / n <= pi: 1024 u.  A Jacobian entry is at most a product of four 3 x 3 matrices whose entries are
    bounded by 1 + magnitude (rotations, JacobianR, JacobianRInv <= 1 + theta, hat of a residual term, the preintegration's Jacobians):
    4 x 5 operations a product, the inputs good to 256 u: 1024 u (1 + magnitude)."""
    m = magnitude(sc, est)
    de = np.full(31, 256 * U * (1 + m))
    de[6:9] = de[21:24] = 1024 * U
    return de, 1024 * U * (1 + m)


def reproj_bounds(sc, s, edges):
    """As tests/poseopt_checks.py's edge_bounds, for Pc = (Rcb Rwb^T) (Pw - Pwb) - Rcb Pbc: the matrix product's entries are good to 8 u,
    the difference to u |d|, the three products and two sums of a row add 5 u each on 3 |d|: dp = 64 u (|Pw| + |Pwb| + |Pbc|) per
    coordinate.  A Jacobian entry is (f / z) (1, x / z or y / z) times an entry of Rcb or of hat(Paux) Rcb (|.| <= 2 |Paux|): relative
    16 u + 8 dp / |z| on the scale S = (f / |z|) (1 + |x / z| + |y / z|) (1 + 2 |Paux|), plus S dp / |z| for what passes through zero."""
    ev = nm.reproj(s, sc, edges)
    fx, fy, cx, cy = [float(v) for v in sc["K"]]
    e = np.asarray(edges, np.float64).reshape(-1, 6)
    x, y, z = ev["x"], ev["y"], ev["z"]
    with np.errstate(all="ignore"):
        dp = 64 * U * (np.abs(e[:, :3]).max(1) + float(np.abs(s["P"]).max()) + float(np.abs(np.asarray(sc["Pbc"])).max()))
        de0 = fx * (dp / np.abs(z)) * (1 + np.abs(x / z)) + 5 * U * (np.abs(e[:, 3]) + fx * np.abs(x / z) + abs(cx))
        de1 = fy * (dp / np.abs(z)) * (1 + np.abs(y / z)) + 5 * U * (np.abs(e[:, 4]) + fy * np.abs(y / z) + abs(cy))
        c2 = ev["chi2"]
        dchi = 2 * ev["w"] * (np.abs(ev["e0"]) * de0 + np.abs(ev["e1"]) * de1) + 5 * U * c2
        S = (max(fx, fy) / np.abs(z)) * (1 + np.abs(x / z) + np.abs(y / z)) * (1 + 2 * np.abs(ev["aux"]).max(1))
        dJ = (16 * U + 9 * dp / np.abs(z)) * S
    return dict(ev=ev, de0=de0, de1=de1, dchi=dchi, dJ=dJ)


def rho_bounds(c2, dchi, delta, robust=True):
    rho0, rho1 = nm.huber(c2, delta, robust)
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        drho0 = dchi + 4 * U * (np.abs(rho0) + dsqr)
        drho1 = np.where((c2 + dchi > dsqr) & robust, rho1 * (dchi / (2 * np.maximum(c2, dsqr - dchi)) + 3 * U), 0.0)
    return rho0, rho1, drho0, drho1


def check_edges(emu, name, count=24):
    """Every single edge's error and Jacobian, and e, chi2, rho and the 2 x 6 Jacobian of reprojection edges, at the scene's start."""
    sc, _ = model(name)
    est = start_of(sc)
    e, J, sing, oimu = emu.single(sc, est)
    de, dJ = single_bounds(sc, est)
    seen = np.zeros((31, 30), bool)
    for nme, em, info, Jm, delta in nm.single_edges(est, sc):
        r0 = ROWS[nme]
        assert (np.abs(e[r0:r0 + len(em)] - em) <= de[r0:r0 + len(em)]).all(), (name, nme, "error", e[r0:r0 + len(em)] - em)
        for c, blk in Jm.items():
            assert (np.abs(J[r0:r0 + len(em), c:c + blk.shape[1]] - blk) <= dJ).all(), (name, nme, "Jacobian at column", c)
            seen[r0:r0 + len(em), c:c + blk.shape[1]] = True
    assert (J[~seen] == 0).all(), (name, "a Jacobian entry outside the edges' vertices")
    for f, edges in nm.frames_of(sc):
        B = reproj_bounds(sc, est[f], edges)
        ev = B["ev"]
        rho0, rho1, drho0, drho1 = rho_bounds(ev["chi2"], B["dchi"], nm.D_MONO)
        for i in range(min(count, len(edges))):
            if not np.isfinite([ev["x"][i] / ev["z"][i], ev["y"][i] / ev["z"][i]]).all():
                continue
            got = emu.reproj(sc, est[f], edges[i])
            assert abs(got[0] - ev["e0"][i]) <= B["de0"][i] and abs(got[1] - ev["e1"][i]) <= B["de1"][i], (name, f, i)
            assert abs(got[2] - ev["chi2"][i]) <= B["dchi"][i] and abs(got[3] - rho0[i]) <= drho0[i] and abs(got[4] - rho1[i]) <= drho1[i], (name, f, i)
            Jg = got[5:].reshape(2, 6)
            assert (np.abs(Jg - ev["J"][i][:, [0, 1, 2, 6, 7, 8]]) <= B["dJ"][i]).all(), (name, f, i, Jg - ev["J"][i][:, [0, 1, 2, 6, 7, 8]])


# ---- layer 2: one linearisation -------------------------------------------------------------------------------------------------------
def solver_factor(n):
    """Both sides' solvers are backward stable, |dA| <= 3 n u g |A|: g = 1 for the LDL^T of a positive definite matrix; for LAPACK's
    partial pivoting g is taken as n (the worst case 2^(n - 1) is reached by no matrix of this kind).  The forward errors add."""
    return (3 * n + 3 * n * n) * U


def lin_bounds(sc, est, active, robust):
    """Bounds on H, b and the robust chi2 of one linearisation against the model's at the same estimates over the same edges.
    Both sides add the same terms in different orders: 2 (N - 1) u sum |t| (N: the terms of the longest sum).  The terms differ by what
    layer 1 allows their factors: for a single edge with W = rho1 Omega
        dH = dJ^T |W| |J| + |J|^T |W| dJ + |J|^T dW |J|,   db = dJ^T |W| |e| + |J|^T dW |e| + |J|^T |W| de,
        dW = |W| (dOmega / Omega + drho1 / rho1);  dOmega / Omega = cond(CovPVPhi) solver_factor(9) for the IMU edge (two different
        inverses), 4 u else;  dchi2 = 2 |e|^T |Omega| de + |e|^T |Omega| |e| (dOmega / Omega + (m + 2) u), rho by rho_bounds;
    for a reprojection edge as tests/poseopt_checks.py's lin_bounds."""
    nd = nm.nd_of(sc)
    L = nm.linearise(est, sc, active, robust)
    de, dJs = single_bounds(sc, est)
    n_terms = 31 + max(int(a.sum()) for a in active)
    c = (2 * n_terms + 64) * U
    bH, bb, bc = c * L["absH"], c * L["absb"], c * L["abschi2"]
    with np.errstate(all="ignore"):
        for nme, e, info, J, delta in L["singles"]:
            m = len(e)
            Jf = np.zeros((m, nd))
            dJ = np.zeros((m, nd))
            for col, blk in J.items():
                Jf[:, col:col + blk.shape[1]] = np.abs(blk)
                dJ[:, col:col + blk.shape[1]] = dJs
            rel_om = float(np.linalg.cond(np.asarray(sc["cov"]).reshape(9, 9))) * solver_factor(9) if nme == "imu" else 4 * U
            ae, ai = np.abs(e), np.abs(info)
            dee = de[ROWS[nme]:ROWS[nme] + m]
            c2 = float(e @ (info @ e))
            dchi = float(2 * ae @ (ai @ dee) + ae @ (ai @ ae) * (rel_om + (m + 2) * U))
            rho0, rho1, drho0, drho1 = [float(v) for v in rho_bounds(c2, dchi, delta)]
            W = rho1 * ai
            dW = W * rel_om + ai * drho1
            bH += dJ.T @ W @ Jf + Jf.T @ W @ dJ + Jf.T @ dW @ Jf
            bb += dJ.T @ (W @ ae) + Jf.T @ (dW @ ae) + Jf.T @ (W @ dee)
            bc += drho0
        for f, edges in nm.frames_of(sc):
            idx = np.flatnonzero(active[f])
            B = reproj_bounds(sc, est[f], edges)
            ev = B["ev"]
            rho0, rho1, drho0, drho1 = rho_bounds(ev["chi2"][idx], B["dchi"][idx], nm.D_MONO, robust)
            J, dJ = np.abs(ev["J"][idx]), B["dJ"][idx][:, None, None] * (ev["J"][idx] != 0)
            wd = ev["w"][idx]
            wo = (rho1 * wd)[:, None, None, None]
            eH = (dJ[:, :, :, None] * wo * J[:, :, None, :] + J[:, :, :, None] * wo * dJ[:, :, None, :] +
                  J[:, :, :, None] * J[:, :, None, :] * (wd * drho1)[:, None, None, None]).sum(1)
            ee = np.abs(np.stack([ev["e0"][idx], ev["e1"][idx]], 1))
            dee = np.stack([B["de0"][idx], B["de1"][idx]], 1)
            r = wd[:, None] * ee * rho1[:, None]
            dr = wd[:, None] * (dee * rho1[:, None] + ee * drho1[:, None]) + 2 * U * r
            eb = (dJ * r[:, :, None] + J * dr[:, :, None]).sum(1)
            c0 = 15 * f
            bH[c0:c0 + 9, c0:c0 + 9] += eH.sum(0)
            bb[c0:c0 + 9] += eb.sum(0)
            bc += float(drho0.sum())
    return L, bH, bb, float(bc)


def check_linearisation(name, H, b, chi, lin=0):
    """H [nd, nd], b, chi2 of the implementation's linearisation `lin` of the model's run (default the first: the start, every edge active)."""
    sc, res = model(name)
    R = res.lin[lin]
    L, bH, bb, bc = lin_bounds(sc, R["est"], R["active"], R["robust"])
    dH, db, dc = np.abs(H - R["H"]), np.abs(b - R["b"]), abs(chi - R["chi2"])
    assert same_class(H, R["H"]) and same_class(b, R["b"]) and same_class(chi, R["chi2"]), (name, "class")
    f = np.isfinite(R["H"])
    assert (dH[f] <= bH[f]).all(), (name, "H", np.nanmax(dH / bH))
    f = np.isfinite(R["b"])
    assert (db[f] <= bb[f]).all(), (name, "b", np.nanmax(db / bb))
    assert not math.isfinite(R["chi2"]) or dc <= bc, (name, "chi2", dc, bc)


# ---- layer 3: one trial ---------------------------------------------------------------------------------------------------------------
def check_trial(emu, name, trial=0):
    """The step against numpy.linalg.solve, the tried estimates, tmp and scale, on the model's own H, b, lambda and estimates of a trial.
    |ddx| <= cond(H + lambda I) solver_factor(nd) |x| in norm.  The estimates: P += R dP (|R| = 1), V, the biases take ddx directly; the
    quaternion takes half of it; exp, the product and the normalisations are 128 operations on values <= 1 + |x|, sin and cos 4 u
    each: dstate <= ddx + 256 u (1 + |state| + |x|).  scale as tests/poseopt_checks.py.  tmp: the layer-2 bound on the robust chi2 at
    the tried estimates plus what their error moves it, the gradient of the robust chi2 being -2 b' (b' of a linearisation there) and
    a state error a tangent error of at most twice as much: |dtmp| <= layer 2 + 4 |b'|_1 dstate."""
    sc, res = model(name)
    tr = res.trials[trial]
    R = res.lin[tr["lin"]]
    nd = nm.nd_of(sc)
    ok, dx, est1, (tmp, scale) = emu.trial(sc, tr["est0"], R["active"], R["robust"], R["H"], R["b"], tr["lam"])
    assert ok == tr["ok"] and ok
    ddx = tr["cond"] * solver_factor(nd) * float(np.linalg.norm(tr["dx"]))
    assert float(np.linalg.norm(dx - tr["dx"])) <= ddx, (name, np.linalg.norm(dx - tr["dx"]), ddx)
    dstate = 0.0
    for f in range(2):
        want, got = nm.state_vec(tr["est"][f]), nm.state_vec(est1[f])
        ds = ddx + 256 * U * (1 + float(np.abs(want).max()) + float(np.abs(tr["dx"]).max()))
        assert np.abs(got - want).max() <= ds, (name, f, np.abs(got - want).max(), ds)
        dstate = max(dstate, ds)
    x, b, lam = np.abs(tr["dx"]), np.abs(R["b"]), tr["lam"]
    dscale = float((ddx * (2 * lam * x + b)).sum() + (nd + 14) * U * (x * (lam * x + b)).sum()) + 2 * U
    assert abs(scale - tr["scale"]) <= dscale, (name, scale - tr["scale"], dscale)
    L1, _, _, bc = lin_bounds(sc, tr["est"], R["active"], R["robust"])
    dtmp = bc + 4 * float(np.abs(L1["b"]).sum()) * dstate
    assert abs(tmp - tr["tmp"]) <= dtmp, (name, tmp - tr["tmp"], dtmp)
    return ddx, dtmp


# ---- layer 4: the Levenberg trajectory ------------------------------------------------------------------------------------------------
_PREFIX = {}


def compared_prefix(name):
    """The number of leading trials whose model margin |cur - tmp| exceeds the layer-2 bound on the two robust chi2 it is the difference
    of: that at the linearisation's estimates plus that at the tried ones.  The prefix ends at the first trial that does not."""
    if name not in _PREFIX:
        sc, res = model(name)
        k = 0
        for tr in res.trials:
            R = res.lin[tr["lin"]]
            if not (tr["ok"] and math.isfinite(tr["margin"])):
                break
            bound = lin_bounds(sc, R["est"], R["active"], R["robust"])[3] + lin_bounds(sc, tr["est"], R["active"], R["robust"])[3]
            if not tr["margin"] > bound:
                break
            k += 1
        _PREFIX[name] = k
    return _PREFIX[name]


def first_iteration_trials(res):
    return sum(1 for tr in res.trials if tr["lin"] == 0)


LAMBDA_RTOL = 1e-6     # as tests/poseopt_checks.py: lambda moves by exact factors or by 1 - (2 rho - 1)^3, derivative <= 6 in rho


def not_finite(res):
    return len(res.lin) > 0 and not math.isfinite(res.lin[0]["chi2"])


def same_class(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.isnan(a) == np.isnan(b)).all() and (np.isposinf(a) == np.isposinf(b)).all() and (np.isneginf(a) == np.isneginf(b)).all())


def check_trajectory(name, run):
    sc, res = model(name)
    k = compared_prefix(name)
    tr = run.trace.trial
    if not_finite(res):
        assert len(tr) == len(res.trials) and len(run.trace.lin) == len(res.lin), (name, len(tr), len(res.trials))
        for i, m in enumerate(res.trials):
            assert (int(tr["lin"][i]), bool(tr["ok"][i]), bool(tr["accepted"][i])) == (m["lin"], m["ok"], m["accepted"]), (name, i)
            assert same_class(tr["lambda"][i], m["lam"]) and same_class(tr["cur"][i], m["cur"]) and same_class(tr["tmp"][i], m["tmp"]), (name, i)
        return len(tr)
    assert len(tr) >= min(k, len(res.trials)), (name, len(tr), k)
    for i in range(k):
        m = res.trials[i]
        assert int(tr["lin"][i]) == m["lin"], (name, i, "linearisation index")
        assert bool(tr["ok"][i]) == m["ok"] and bool(tr["accepted"][i]) == m["accepted"], (name, i, "decision", tr[i], m["rho"])
        assert abs(tr["lambda"][i] - m["lam"]) <= LAMBDA_RTOL * m["lam"], (name, i, "lambda", tr["lambda"][i], m["lam"])
    if len(tr) and len(res.trials):
        first = [i for i in range(len(tr)) if i == 0 or tr["lin"][i] != tr["lin"][i - 1]]
        assert all(tr["cur"][i] == run.trace.lin["chi2"][tr["lin"][i]] for i in first), (name, "cur")
    # the driver replayed on the trace: rounds and iterations of the linearisations, and every round's first linearisation stands at the
    # start again -- the estimates are reset -- so its H, b and chi2 are those of the model's first linearisation of that round within
    # layer 2 whenever the same edges are active (round 0 always)
    li = run.trace.lin
    if k:
        last = res.trials[k - 1]["lin"]
        for j in range(last + 1):
            assert (int(li["round"][j]), int(li["iteration"][j])) == (res.lin[j]["round"], res.lin[j]["iteration"]), (name, j)
    nd = nm.nd_of(sc)
    if len(li):
        check_linearisation(name, full_of_tri(li["H"][0], nd), li["b"][0][:nd], float(li["chi2"][0]), 0)
    if not thin(name):
        for rnd in range(1, run.rounds):
            mine = [j for j in range(len(li)) if li["round"][j] == rnd]
            theirs = [j for j, R in enumerate(res.lin) if R["round"] == rnd]
            assert bool(mine) == bool(theirs), (name, rnd)
            if mine:
                check_linearisation(name, full_of_tri(li["H"][mine[0]], nd), li["b"][mine[0]][:nd], float(li["chi2"][mine[0]]), theirs[0])
    return k


# ---- layer 5: results -----------------------------------------------------------------------------------------------------------------
def thin(name):
    """Whether the scene's smallest model margin |chi2 - th| is within M: its masks are then not compared."""
    _, res = model(name)
    return not nm.min_class_margin(res) > M_CHI2


def check_result(name, run):
    sc, res = model(name)
    assert run.rounds == res.rounds, (name, run.rounds, res.rounds)
    if not thin(name):
        for f in range(len(res.outlier)):
            assert run.outlier[f].tobytes() == res.outlier[f].tobytes(), (name, f, np.flatnonzero(run.outlier[f] != res.outlier[f]))
        assert run.n_inliers == res.n_inliers, (name, run.n_inliers, res.n_inliers)
    got, want = nm.state_vec(run.ns), nm.state_vec(res.ns)
    assert same_class(got, want), name
    f = np.isfinite(want)
    assert not f.any() or np.abs(got[f] - want[f]).max() <= T_STATE, (name, np.abs(got[f] - want[f]).max())
    Tm = res.Tcw.astype(np.float64)
    assert same_class(run.Tcw, Tm)
    fin = np.isfinite(Tm)
    # UpdatePoseFromNS in float: three roundings to float on values <= 1 + |P| each side, and the state's spread
    tol = 4 * np.spacing(np.float32(1 + np.abs(Tm[fin]).max())).astype(np.float64) + 4 * T_STATE * (1 + np.abs(Tm[fin]).max()) if fin.any() else 0.0
    assert (np.abs(run.Tcw.astype(np.float64) - Tm)[fin] <= tol).all(), (name, np.abs(run.Tcw.astype(np.float64) - Tm)[fin].max(), tol)


# ---- layer 6: marginals ---------------------------------------------------------------------------------------------------------------
def check_marginals(name, run):
    """marg_cov and marg_cov_inv against numpy's inverses of the H the run's own trace shows for its LAST linearisation -- computeMarginals
    inverts _Hpp as the last buildSystem left it, not a new linearisation at the final estimate.
    |d inv(A)| <= cond(A) solver_factor(n) |inv(A)| for each inverse; marg_cov_inv takes the errors of both."""
    sc, res = model(name)
    if not sc["compute_marg"] or not run.rounds:
        assert run.marg_ok == 0 and not run.marg_cov.any() and not run.marg_cov_inv.any(), name
        return
    nd = nm.nd_of(sc)
    H = full_of_tri(run.trace.lin["H"][-1], nd)
    cov, inv, ok = nm.marginals(H, sc)
    assert bool(run.marg_ok) == ok == res.marg_ok, (name, run.marg_ok, ok, res.marg_ok)
    if not ok:
        return
    c1 = float(np.linalg.cond(H)) * solver_factor(nd)
    assert np.abs(run.marg_cov - cov).max() <= c1 * np.abs(cov).max(), (name, "marg_cov", np.abs(run.marg_cov - cov).max(), c1 * np.abs(cov).max())
    c2 = (float(np.linalg.cond(cov)) + float(np.linalg.cond(cov[:9, :9])) + float(np.linalg.cond(cov[9:, 9:]))) * (solver_factor(15) + c1)
    assert np.abs(run.marg_cov_inv - inv).max() <= c2 * np.abs(inv).max(), (name, "marg_cov_inv", np.abs(run.marg_cov_inv - inv).max(), c2 * np.abs(inv).max())
    if sc["form"] == nm.KEYFRAME:
        assert not run.marg_cov_inv[:9, 9:].any() and not run.marg_cov_inv[9:, :9].any(), (name, "the key-frame form stores the two diagonal blocks only")
    else:
        assert run.marg_cov_inv[:9, 9:].any(), (name, "the frame form stores the inverse of the whole block")
    # and the last linearisation is the model's last wherever the whole trajectory was compared
    if compared_prefix(name) == len(res.trials) and len(run.trace.lin) == len(res.lin):
        assert (int(run.trace.lin["round"][-1]), int(run.trace.lin["iteration"][-1])) == (res.lin[-1]["round"], res.lin[-1]["iteration"]), name


def check_all(name, run):
    """Layers 2 (on the trace), 4, 5 and 6 on one run of a named scene."""
    k = check_trajectory(name, run)
    check_result(name, run)
    check_marginals(name, run)
    return k


# ---- measuring T and M on the model ---------------------------------------------------------------------------------------------------
def measure_spread(names, orders=4, seed=2024):
    """The model on each scene under `orders` random permutations of each frame's edge order -> (largest spread of any word of the final
    NavState, largest change of any edge's chi2 at a classification, mask changes)."""
    g = np.random.default_rng(seed)
    st, chi, flips = 0.0, 0.0, 0
    for name in names:
        sc, base = model(name)
        for _ in range(orders):
            r = nm.optimize(sc, order=[g.permutation(len(e)) for _, e in nm.frames_of(sc)])
            a, b = nm.state_vec(r.ns), nm.state_vec(base.ns)
            f = np.isfinite(b)
            if f.any():
                st = max(st, float(np.abs(a[f] - b[f]).max()))
            for ca, cb in zip(r.class_chi2, base.class_chi2):
                for xa, xb in zip(ca, cb):
                    f = np.isfinite(xa) & np.isfinite(xb)
                    if f.any():
                        chi = max(chi, float(np.abs(xa[f] - xb[f]).max()))
            flips += sum(int((x != y).sum()) for x, y in zip(r.outlier, base.outlier))
    return st, chi, flips
