"""The parts of the Radau IIA step (pfc_radau_table, pfc_radau_{seed,jacobian,factor,unpack,newton,finish}_device) without a device:
the scalar statements of the kernels' arithmetic (csrc/pfc_radau.h, stated in include/pfc.h) that tests/test_gpu_radau.py compares
bytes with, and what pins them without leaning on those statements.

`radau_tables`, `lu_scalar` / `solve_scalar`, `factor_scalar`, `newton_scalar`, `finish_scalar` and `radau_step_scalar(de, de_dual, ..)`
are the statements in Python floats (no fma, the written order; a "wave sum" is the six-round butterfly of pfc.h).

What pins them:
* the tables: the generator (scripts/radau_tables.py, mpmath at 50 digits) against the reference's table files (a data fixture,
  tests/golden/radau_tables_ref.npz) to 4 ulp, T up to a complex scale per column, and the defining relations at rounding level;
  the compiled constants are the generator's floats;
* `lu_scalar` + `solve_scalar` against a 50-digit solve: forward error <= kappa_inf n 2^-52 |x|_inf, kappa_inf computed per case;
* a body in free fall and a pendulum, `de` and its partials from the statements of tests/test_dynamics_abi.py and
  tests/test_dynamics_dual_abi.py: the analytic step, implicit Euler's step, the collocation equations with the 50-digit table;
* synthetic `de`: flags, iteration counts, h, rule and cooldown against `reference_step`, a NumPy restatement of the reference's
  own sequence (explicit inverses of all three matrices, real part of the sum, pow) on the reference's own table values.
"""
import ctypes as C
import importlib.util
import math
import os
import re
import subprocess

import numpy as np
import pytest

import test_dynamics_abi as D
import test_dynamics_dual_abi as DD
import test_kinematics_abi as K

ROOT = K.ROOT
EPS = K.EPS
INF = float("inf")
MAX_NX = 64
NAMES = (("pfc_radau_table", 8), ("pfc_radau_seed_device", 14), ("pfc_radau_jacobian_device", 21), ("pfc_radau_factor_device", 12),
         ("pfc_radau_unpack_device", 16), ("pfc_radau_newton_device", 26), ("pfc_radau_finish_device", 29),
         ("pfc_radau_configure", 9), ("pfc_radau_sizes", 4), ("pfc_radau_set_state", 3), ("pfc_radau_get_state", 3),
         ("pfc_radau_set_rule_state", 4),
         ("pfc_radau_set_tau", 2), ("pfc_radau_step", 5), ("pfc_radau_rule_state", 2))
# words of a scene's records (csrc/pfc_radau.h)
ITER, KITER, FLAG, PHASE, ATTEMPTS, EXIT, EXITITER = range(7)
THETA, THETA_PREV, PSI, RES1, RES2, RES, HTAKEN = range(7)
DEFAULTS = dict(h0=1e-4, tol_a=1e-4, tol_r=1e-4, tol_newton=1e-16, h_max=0.01, h_min=1e-8, k_iter_max=15, max_rule=2, n_chunk=6,
                cooldown=10)


def _generator():
    spec = importlib.util.spec_from_file_location("radau_tables", os.path.join(ROOT, "scripts", "radau_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_TABLES = {}


def radau_tables(rule):
    """The constants of a rule as the generator rounds them: c, A, lam, T, Tinv (complex as Python complex), bhat0, bhat."""
    if rule not in _TABLES:
        _TABLES[rule] = _generator().tables(rule)
    return _TABLES[rule]


# ---- the statements ---------------------------------------------------------------------------------------------------------------
def wave_sum(vals):
    v = [float(x) for x in vals] + [0.0] * (64 - len(vals))
    for off in (32, 16, 8, 4, 2, 1):
        v = [v[i] + v[i ^ off] for i in range(64)]
    return v[0]


def _cmul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def _cdiv(a, b):
    den = b[0] * b[0] + b[1] * b[1]
    return ((a[0] * b[0] + a[1] * b[1]) / den, (a[1] * b[0] - a[0] * b[1]) / den)


def _csub(a, b):
    return (a[0] - b[0], a[1] - b[1])


class _Real:
    mul = staticmethod(lambda a, b: a * b)
    div = staticmethod(lambda a, b: a / b)
    sub = staticmethod(lambda a, b: a - b)
    mag = staticmethod(abs)
    is_zero = staticmethod(lambda a: a == 0.0)


class _Cplx:
    mul, div, sub = staticmethod(_cmul), staticmethod(_cdiv), staticmethod(_csub)
    mag = staticmethod(lambda a: abs(a[0]) + abs(a[1]))
    is_zero = staticmethod(lambda a: a[0] == 0.0 and a[1] == 0.0)


def lu_scalar(M, cplx=False):
    """P A = L U as pfc_radau_factor_device states it.  M: n rows of n numbers ((re, im) pairs if cplx).  Returns (LU rows, perm, info)."""
    N = _Cplx if cplx else _Real
    n = len(M)
    A = [list(row) for row in M]
    perm = list(range(n))
    for k in range(n):
        best, p = -1.0, k
        for i in range(k, n):
            m = N.mag(A[i][k])
            if m != m:
                m = INF
            if m > best:
                best, p = m, i
        piv = A[p][k]
        if N.is_zero(piv):
            return A, perm, k + 1
        if p != k:
            A[k], A[p] = A[p], A[k]
            perm[k], perm[p] = perm[p], perm[k]
        for i in range(k + 1, n):
            l = N.div(A[i][k], piv)
            A[i][k] = l
            for j in range(k + 1, n):
                A[i][j] = N.sub(A[i][j], N.mul(l, A[k][j]))
    return A, perm, 0


def solve_scalar(LU, perm, b, cplx=False):
    N = _Cplx if cplx else _Real
    n = len(b)
    acc = [b[perm[i]] for i in range(n)]
    for k in range(n):
        yk = acc[k]
        for i in range(k + 1, n):
            acc[i] = N.sub(acc[i], N.mul(LU[i][k], yk))
    for k in range(n - 1, -1, -1):
        xk = N.div(acc[k], LU[k][k])
        acc[k] = xk
        for i in range(k):
            acc[i] = N.sub(acc[i], N.mul(LU[i][k], xk))
    return acc


def factor_scalar(neg_J, h, rule):
    """(lu0, perm0, info0, lu1, perm1, info1) of a scene; neg_J[i][j] = -J(i, j).  Rule 1: lu1 and perm1 are None, info1 = 0."""
    n = len(neg_J)
    hinv = 1.0 / float(h)
    t = radau_tables(2 if rule == 2 else 1)
    s0 = hinv * t["lam"][0].real
    A0 = [[float(neg_J[i][j]) + s0 if i == j else float(neg_J[i][j]) for j in range(n)] for i in range(n)]
    lu0, p0, i0 = lu_scalar(A0)
    if rule != 2:
        return lu0, p0, i0, None, None, 0
    sr, si = hinv * t["lam"][1].real, hinv * t["lam"][1].imag
    A1 = [[(float(neg_J[i][j]) + sr, si) if i == j else (float(neg_J[i][j]), 0.0) for j in range(n)] for i in range(n)]
    lu1, p1, i1 = lu_scalar(A1, True)
    return lu0, p0, i0, lu1, p1, i1


def new_records(h0=DEFAULTS["h0"], cooldown=DEFAULTS["cooldown"]):
    """A scene's records as pfc_radau_set_state's reset leaves them: the reference's RadauStep / RadauRule constructors."""
    return dict(h=float(h0), rule=1, cool=int(cooldown), enorm=[-9999.0, -9999.0],
                nstate=[-9999.0, -9999.0, 9999.0, INF, INF, 0.0, 0.0, 0.0], istate=[0, 0, -1, 0, 0, -9999, 0, 0])


def arm(st):
    if st["istate"][EXIT] != 5:
        st["istate"][ITER], st["istate"][KITER], st["istate"][FLAG], st["istate"][PHASE], st["istate"][ATTEMPTS] = 1, 0, -1, 1, 1
        st["nstate"][RES1] = st["nstate"][RES2] = INF


def newton_scalar(st, fac, x0, X, F, tol_newton=DEFAULTS["tol_newton"], k_iter_max=DEFAULTS["k_iter_max"]):
    """One iteration of an iterating scene as pfc_radau_newton_device states it.  st: the records (h, rule, nstate, istate), updated;
    fac: factor_scalar's tuple; X: the NS stage states (lists, updated in place); F: their derivatives."""
    is_, ns_ = st["istate"], st["nstate"]
    if is_[ITER] != 1:
        return
    rule = 2 if st["rule"] == 2 else 1
    NS = 2 * rule - 1
    t = radau_tables(rule)
    n = len(x0)
    lu0, p0, i0, lu1, p1, i1 = fac
    k_iter = is_[KITER] + 1
    is_[KITER] = k_iter
    if i0 != 0 or (NS == 3 and i1 != 0):
        is_[ITER], is_[FLAG] = 0, 4
        return
    h = st["h"]
    hinv, mh = 1.0 / h, -h
    residual = 0.0
    e0 = [0.0] * n
    e1 = [(0.0, 0.0)] * n
    l1 = (hinv * t["lam"][1].real, hinv * t["lam"][1].imag) if NS == 3 else None
    for s in range(NS):
        r = []
        for i in range(n):
            v = X[s][i] - x0[i]
            for j in range(NS):
                v = v + (mh * t["A"][s][j]) * F[j][i]
            r.append(v)
        residual = residual + wave_sum([v * v for v in r])
        c0 = (hinv * t["lam"][0].real) * t["Tinv"][0][s].real
        e0 = [e0[i] + c0 * r[i] for i in range(n)]
        if NS == 3:
            cf = _cmul(l1, (t["Tinv"][1][s].real, t["Tinv"][1][s].imag))
            e1 = [(e1[i][0] + cf[0] * r[i], e1[i][1] + cf[1] * r[i]) for i in range(n)]
    w0 = solve_scalar(lu0, p0, e0)
    w1 = solve_scalar(lu1, p1, e1, True) if NS == 3 else None
    dz = []
    for s in range(NS):
        row = []
        for i in range(n):
            v = t["T"][s][0].real * w0[i]
            if NS == 3:
                v = v + 2.0 * (t["T"][s][1].real * w1[i][0] - t["T"][s][1].imag * w1[i][1])
            row.append(v)
        dz.append(row)
    finite = math.isfinite(residual) and all(math.isfinite(v) for row in dz for v in row)
    flag = -1
    if not finite:
        flag = 3
    else:
        for s in range(NS):
            if 10.0 < max(abs(v) for v in dz[s]):
                flag = 3
                break
            X[s][:] = [X[s][i] - dz[s][i] for i in range(n)]
    if flag < 0:
        if residual < tol_newton:
            flag = 0
        else:
            if k_iter != 1:
                ns_[THETA_PREV] = ns_[THETA]
                ns_[THETA] = math.sqrt(residual)
                ns_[PSI] = math.sqrt(ns_[THETA_PREV] * ns_[THETA])
            else:
                ns_[THETA] = math.sqrt(residual)
                ns_[PSI] = ns_[THETA]
            res3 = ns_[RES2]
            ns_[RES2] = ns_[RES1]
            ns_[RES1] = residual
            if res3 < ns_[RES2] < ns_[RES1]:
                flag = 3
            elif k_iter >= k_iter_max:
                flag = 1
    ns_[RES] = float("nan") if residual != residual else residual      # one NaN, whatever its sign
    is_[ITER], is_[FLAG] = (1 if flag < 0 else 0), flag


def finish_scalar(st, fac, x, t, X, F, xdot0, mrp_off=(), tol_a=DEFAULTS["tol_a"], tol_r=DEFAULTS["tol_r"], h_max=DEFAULTS["h_max"],
                  h_min=DEFAULTS["h_min"], k_iter_max=DEFAULTS["k_iter_max"], max_rule=DEFAULTS["max_rule"], cooldown=DEFAULTS["cooldown"]):
    """The end of an attempt as pfc_radau_finish_device states it; returns the new (x, t).  The records are updated."""
    is_, ns_ = st["istate"], st["nstate"]
    if is_[PHASE] != 1 or is_[ITER] != 0:
        return x, t
    flag, k_iter = is_[FLAG], is_[KITER]
    rule = 2 if st["rule"] == 2 else 1
    NS = 2 * rule - 1
    tb = radau_tables(rule)
    n = len(x)
    h = st["h"]
    if flag == 0:
        d = [0.0 + (tb["bhat0"] * h) * xdot0[i] for i in range(n)]
        for k in range(NS):
            cf = (tb["bhat"][k] - tb["A"][NS - 1][k]) * h
            d = [d[i] + cf * F[k][i] for i in range(n)]
        e = solve_scalar(fac[0], fac[1], d)
        xf = X[NS - 1]
        q = []
        for i in range(n):
            ax, a0 = abs(xf[i]), abs(x[i])
            sc = tol_a + (a0 if ax < a0 else ax) * tol_r
            qk = e[i] / sc
            q.append(qk * qk)
        err = math.sqrt(wave_sum(q) / float(n))
        k2 = 2 * k_iter_max
        fac_h = (0.9 * float(k2 + 1)) / float(k2 + k_iter)
        inv = 1.0 / err if err != 0.0 else INF
        root = math.sqrt(math.sqrt(inv)) if NS == 3 else math.sqrt(inv)
        est = (fac_h * h) * root
    else:
        est = h * 0.1
    h_new = h_max
    if 2.0 * h < h_new:
        h_new = 2.0 * h
    if est < h_new:
        h_new = est
    is_[EXITITER] = k_iter
    st["h"] = h_new
    if flag == 0:
        st["cool"] -= 1
        if st["cool"] < 1 and ns_[PSI] < 0.1:
            st["rule"] = min(rule + 1, max_rule)
        xi = list(xf)
        for o in mrp_off:
            nn = (xf[o] * xf[o] + xf[o + 1] * xf[o + 1]) + xf[o + 2] * xf[o + 2]
            if nn > 1.0:
                for r in range(3):
                    xi[o + r] = -(xf[o + r] / nn)
        st["enorm"] = [st["enorm"][1], err]
        ns_[HTAKEN] = h
        is_[EXIT], is_[PHASE] = 0, 0
        return xi, t + h
    st["cool"] = cooldown
    st["rule"] = max(rule - 1, 1)
    if h_new < h_min:
        is_[EXIT], is_[PHASE] = 5, 0
    else:
        is_[EXIT] = flag
        is_[ITER], is_[KITER], is_[FLAG], is_[ATTEMPTS] = 1, 0, -1, is_[ATTEMPTS] + 1
        ns_[RES1] = ns_[RES2] = INF
    return x, t


def jacobian_scalar(de_dual, x, n_chunk=DEFAULTS["n_chunk"]):
    """calcJacobian!: (neg_J rows, xdot0) from de_dual(x, seeds) -> (xdot, [dxdot per seed]), a chunk of unit seeds at a time."""
    n = len(x)
    neg_J = [[0.0] * n for _ in range(n)]
    xdot0 = None
    for j0 in range(0, n, n_chunk):
        seeds = [[1.0 if i == j else 0.0 for i in range(n)] for j in range(j0, min(j0 + n_chunk, n))]
        xd, dxd = de_dual(x, seeds)
        if j0 == 0:
            xdot0 = [float(e) for e in xd]
        for d, col in enumerate(dxd):
            for i in range(n):
                neg_J[i][j0 + d] = -float(col[i])
    return neg_J, xdot0


def radau_step_scalar(de, de_dual, x, t, st, mrp_off=(), log=None, **par):
    """One step of one scene (solveRadau): the Jacobian, then attempts until one succeeds or h falls below h_min.  de(x) -> xdot;
    de_dual as jacobian_scalar.  Returns (x, t); st is updated; st["istate"][EXIT] is 0 or 5.  log, a list, receives per attempt
    (rule, h, flag, k_iter, X)."""
    p = dict(DEFAULTS, **par)
    x = [float(e) for e in x]
    neg_J, xdot0 = jacobian_scalar(de_dual, x, p["n_chunk"])
    arm(st)
    while st["istate"][PHASE] == 1:
        fac = factor_scalar(neg_J, st["h"], st["rule"])
        NS = 3 if st["rule"] == 2 else 1
        X = [list(x) for _ in range(NS)]
        rule, h = st["rule"], st["h"]
        while st["istate"][ITER] == 1:
            F = [[float(e) for e in de(X[s])] for s in range(NS)]
            newton_scalar(st, fac, x, X, F, p["tol_newton"], p["k_iter_max"])
        if log is not None:
            log.append((rule, h, st["istate"][FLAG], st["istate"][KITER], [list(r) for r in X]))
        x, t = finish_scalar(st, fac, x, t, X, F, xdot0, mrp_off, p["tol_a"], p["tol_r"], p["h_max"], p["h_min"], p["k_iter_max"],
                             p["max_rule"], p["cooldown"])
    return x, t


def radau_step_batch(de_batch, de_dual_batch, xs, ts, recs, mrp_off=(), **par):
    """One step of a batch of scenes in the evaluation shapes of pfc_radau_step, for a `de` whose bytes depend on what it is evaluated
    with: de_batch(rows) takes the 3 n_scene stage-scene states (stage n_scene + scene; a scene that is not iterating, or starts an
    attempt, at x0; the unused stages of a rule-1 scene at its stage 0) and returns their derivatives; de_dual_batch(xs, seeds) takes
    the n_scene states and a chunk of seeds and returns (xdot rows, per scene the list of partial columns).  F of an iteration is
    kept per scene for the finish, as the newton part keeps it.  Returns (xs, ts); the records are updated."""
    p = dict(DEFAULTS, **par)
    ns, n = len(xs), len(xs[0])
    xs = [[float(e) for e in x] for x in xs]
    ts = list(ts)
    neg_J = [[[0.0] * n for _ in range(n)] for _ in range(ns)]
    xdot0 = None
    for j0 in range(0, n, p["n_chunk"]):
        seeds = [[1.0 if i == j else 0.0 for i in range(n)] for j in range(j0, min(j0 + p["n_chunk"], n))]
        xd, dxd = de_dual_batch(xs, seeds)
        if j0 == 0:
            xdot0 = [[float(e) for e in row] for row in xd]
        for s in range(ns):
            for d, col in enumerate(dxd[s]):
                for i in range(n):
                    neg_J[s][i][j0 + d] = -float(col[i])
    for st in recs:
        arm(st)
    X = [[list(xs[s]) for s in range(ns)] for _ in range(3)]
    F_keep = [[None] * ns for _ in range(3)]
    facs = [None] * ns
    iterating = lambda s: recs[s]["istate"][ITER] == 1
    while any(st["istate"][PHASE] == 1 for st in recs):
        for s in range(ns):
            if iterating(s):
                facs[s] = factor_scalar(neg_J[s], recs[s]["h"], recs[s]["rule"])
        while any(iterating(s) for s in range(ns)):
            rows = []
            for k in range(3):
                for s in range(ns):
                    start = recs[s]["istate"][KITER] == 0
                    if iterating(s) and start:
                        X[k][s] = list(xs[s])
                    rows.append(list(xs[s]) if (not iterating(s) or start) else list(X[k if recs[s]["rule"] == 2 else 0][s]))
            F = de_batch(rows)
            for s in range(ns):
                if iterating(s):
                    NS = 3 if recs[s]["rule"] == 2 else 1
                    for k in range(NS):
                        F_keep[k][s] = [float(e) for e in F[k * ns + s]]
                    newton_scalar(recs[s], facs[s], xs[s], [X[k][s] for k in range(NS)], [F_keep[k][s] for k in range(NS)],
                                  p["tol_newton"], p["k_iter_max"])
        for s in range(ns):
            st = recs[s]
            if st["istate"][PHASE] == 1 and st["istate"][ITER] == 0:
                NS = 3 if st["rule"] == 2 else 1
                xs[s], ts[s] = finish_scalar(st, facs[s], xs[s], ts[s], [X[k][s] for k in range(NS)], [F_keep[k][s] for k in range(NS)],
                                             xdot0[s], mrp_off, p["tol_a"], p["tol_r"], p["h_max"], p["h_min"], p["k_iter_max"],
                                             p["max_rule"], p["cooldown"])
    return xs, ts


# ---- 1. the tables ----------------------------------------------------------------------------------------------------------------
def _fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "radau_tables_ref.npz"))


def _ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("rule", [1, 2])
def test_generated_tables_agree_with_the_reference_files(rule):
    fx, t = _fixture(), radau_tables(rule)
    s = 2 * rule - 1
    assert _ulps(t["A"], fx["A%d" % rule]).max() <= 4
    assert _ulps(t["c"], fx["c%d" % rule]).max() <= 4
    lam = np.array(t["lam"])
    assert _ulps(lam.real, fx["lam%d" % rule].real).max() <= 4 and _ulps(lam.imag[lam.imag != 0], fx["lam%d" % rule].imag[lam.imag != 0]).max(initial=0) <= 4
    assert _ulps([t["bhat0"]] + list(t["bhat"]), fx["bhat%d" % rule]).max() <= 4
    T, Tr = np.array(t["T"]), fx["T%d" % rule]
    for col in range(s):      # an eigenvector is fixed up to a complex scale
        k = int(np.argmax(np.abs(Tr[:, col])))
        scale = T[k, col] / Tr[k, col]
        assert abs(abs(scale) - 1.0) <= 8 * EPS                   # both have unit norm
        assert np.abs(T[:, col] - scale * Tr[:, col]).max() <= 8 * EPS
    # the defining relations at rounding level: entries are below 5, sums have s terms
    A, Ti = np.array(t["A"]), np.array(t["Tinv"])
    assert np.abs(Ti @ T - np.eye(s)).max() <= 16 * s * EPS * np.abs(Ti).max()
    assert np.abs(np.linalg.inv(A) @ T - T @ np.diag(lam)).max() <= 64 * s * EPS * np.abs(lam).max()
    assert lam[0].imag == 0.0 and (s == 1 or (lam[2] == np.conj(lam[1]) and (T[:, 2] == np.conj(T[:, 1])).all()))


def test_bhat_satisfies_its_three_relations_at_fifty_digits():
    import mpmath as mp
    t = _generator().tables_mp(2)
    tiny = mp.mpf(10) ** -45
    assert abs(t["bhat0"] + sum(t["bhat"]) - 1) < tiny
    assert abs(sum(b * c for b, c in zip(t["bhat"], t["c"])) - mp.mpf(1) / 2) < tiny
    assert abs(sum(b * c * c for b, c in zip(t["bhat"], t["c"])) - mp.mpf(1) / 3) < tiny
    assert abs(t["bhat0"] * mp.re(t["lam"][0]) - 1) < tiny
    r1 = radau_tables(1)
    assert r1["A"] == [[1.0]] and r1["c"] == [1.0] and r1["lam"] == [1.0] and r1["T"] == [[1.0]] and r1["bhat0"] == 1.0 and r1["bhat"] == [0.0]


def test_compiled_tables_are_the_generators(pfc):
    gen = _generator()
    assert open(gen.HEADER).read() == gen.header_text(), "csrc/pfc_radau_tables.h is stale: run scripts/radau_tables.py"
    for rule in (1, 2):
        got, t = pfc.scenario.radau_table(rule), radau_tables(rule)
        for key in ("c", "A", "lam", "T", "Tinv", "bhat"):
            assert np.array_equal(got[key], np.array(t[key])), (rule, key)
        assert got["bhat0"] == t["bhat0"]
    with pytest.raises(pfc._lib.PFCError):
        pfc.scenario.radau_table(3)
    with pytest.raises(ValueError):
        gen.tables(3)


# ---- 2. the factorisation and the substitutions against fifty digits -----------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n", [1, 2, 7, 18, 64])
def test_lu_scalar_against_a_fifty_digit_solve(n, cplx):
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(100 * n + cplx)
    A = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if cplx else 0.0)
    if n > 1:
        A[0, 0] = 0.0                                   # forces a row exchange in the first column
    b = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)
    num = (lambda z: (float(z.real), float(z.imag))) if cplx else float
    LU, perm, info = lu_scalar([[num(A[i, j]) for j in range(n)] for i in range(n)], cplx)
    assert info == 0 and sorted(perm) == list(range(n)) and (n == 1 or perm[0] != 0)
    x = solve_scalar(LU, perm, [num(e) for e in b], cplx)
    Am = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            Am[i, j] = mp.mpc(A[i, j])
    Ai = Am ** -1
    xm = Ai * mp.matrix([mp.mpc(e) for e in b])
    norm = lambda M: max(sum(abs(M[i, j]) for j in range(M.cols)) for i in range(M.rows))
    kappa = norm(Am) * norm(Ai)
    xs = [mp.mpc(*e) if cplx else mp.mpf(e) for e in x]
    err = max(abs(xs[i] - xm[i]) for i in range(n))
    bound = kappa * n * mp.mpf(2) ** -52 * max(abs(xm[i]) for i in range(n))
    print("n", n, "complex", cplx, "kappa", float(kappa), "err", float(err), "bound", float(bound))
    assert err <= bound


def test_lu_scalar_flags_a_zero_pivot_and_takes_the_first_of_equal_magnitudes():
    LU, perm, info = lu_scalar([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [1.0, 1.0, 1.0]])
    assert info == 3 and perm[0] == 1
    LU, perm, info = lu_scalar([[0.0, 0.0], [0.0, 1.0]])
    assert info == 1 and perm == [0, 1] and LU == [[0.0, 0.0], [0.0, 1.0]]
    LU, perm, info = lu_scalar([[(1.0, -1.0), (1.0, 0.0)], [(-2.0, 0.0), (0.0, 1.0)], ], True)      # |re| + |im| = 2 twice: row 0
    assert info == 0 and perm == [0, 1]


# ---- 3. mechanisms: free fall and a pendulum ----------------------------------------------------------------------------------------
def _mech_de(mech, rec, g):
    nq = nv = mech["nv"]
    zero = [0.0] * nv

    def de(x):
        qd, H, c = D.dyn_scalar(mech, rec, g, x[:nq], x[nq:])
        vd, info = D.chol_scalar(H, c, zero)
        assert info == 0
        return [float(e) for e in qd] + [float(e) for e in vd]

    def de_dual(x, seeds):
        _, H, c = D.dyn_scalar(mech, rec, g, x[:nq], x[nq:])
        cols, vd = [], None
        for sd in seeds:
            dqd, dH, dc = DD.dyn_dual_scalar(mech, rec, g, x[:nq], x[nq:], sd[:nq], sd[nq:])
            vd, dvd, info = DD.chol_dual_scalar(H, c, zero, [dH], [dc], [zero])
            assert info == 0
            cols.append([float(e) for e in dqd] + [float(e) for e in dvd[0]])
        return de(x), cols

    return de, de_dual


def _free_fall():
    mech = K.make_mech([-1], [K.PRISMATIC], [K.WORLD_X], [[0.0, 0.0, 1.0]])
    rec = D.make_inertia(0.7, [0.0, 0.0, 0.0], np.zeros((3, 3))).reshape(1, 13)
    return _mech_de(mech, rec, (0.0, 0.0, -9.81))


@pytest.mark.parametrize("h", [1e-4, 3e-3, 0.01])
def test_free_fall_steps_are_the_analytic_values(h):
    """qdot = v, vdot = -g: a rule-2 step (order 5) is exact, q0 + v0 h - g h^2 / 2 and v0 - g h; a rule-1 step is implicit Euler's
    q0 + h (v0 - g h).  A few ulps of the terms: the iteration stops at a residual below 1e-16, i.e. |r| < 1e-8, but for a linear
    problem with the exact Jacobian the second iteration's update lands within rounding of the fixed point."""
    de, de_dual = _free_fall()
    g, q0, v0 = 9.81, 0.3, 1.7
    for rule in (1, 2):
        st = new_records(h0=h)
        st["rule"] = rule
        x, t = radau_step_scalar(de, de_dual, [q0, v0], 0.25, st)
        assert st["istate"][EXIT] == 0 and st["istate"][ATTEMPTS] == 1 and t == 0.25 + h and st["nstate"][HTAKEN] == h
        q_ref = q0 + v0 * h - g * h * h / 2 if rule == 2 else q0 + h * (v0 - g * h)
        terms_q, terms_v = abs(q0) + abs(v0 * h) + g * h * h, abs(v0) + g * h
        assert abs(x[0] - q_ref) <= 8 * EPS * terms_q, (rule, x[0] - q_ref)
        assert abs(x[1] - (v0 - g * h)) <= 8 * EPS * terms_v, (rule, x[1] - (v0 - g * h))


def test_the_batch_statement_is_the_scene_statement_for_a_scene_independent_de():
    """Three pendulum scenes that need different numbers of iterations and (the third, from h = h_max at a large swing) attempts:
    radau_step_batch, whose finish runs after the slowest scene's last pass, returns what radau_step_scalar returns scene by scene."""
    m, l, g = 0.7, 0.4, 9.81
    mech = K.make_mech([-1], [K.REVOLUTE], [K.WORLD_X], [[0.0, 1.0, 0.0]])
    rec = D.make_inertia(m, [0.0, 0.0, -l], np.zeros((3, 3))).reshape(1, 13)
    de, de_dual = _mech_de(mech, rec, (0.0, 0.0, -g))
    x0 = [[0.9, -0.4], [0.0, 0.0], [2.5, 30.0]]
    h0 = [1e-4, 2e-3, 0.01]
    a, b = [new_records(h0=h) for h in h0], [new_records(h0=h) for h in h0]
    for r in a + b:
        r["rule"] = 2
    xs, ts = [list(x) for x in x0], [0.0, 0.0, 0.0]
    ys, us = [list(x) for x in x0], [0.0, 0.0, 0.0]

    def dual_batch(rows, seeds):
        out = [de_dual(r, seeds) for r in rows]
        return [o[0] for o in out], [o[1] for o in out]

    for step in range(3):
        xs, ts = radau_step_batch(lambda rows: [de(r) for r in rows], dual_batch, xs, ts, a)
        for s in range(3):
            ys[s], us[s] = radau_step_scalar(de, de_dual, ys[s], us[s], b[s])
        assert xs == ys and ts == us and a == b, step
    assert len({r["istate"][EXITITER] for r in a}) > 1


def test_pendulum_stages_satisfy_the_collocation_equations():
    """X_i = x0 + h sum_j A[i,j] de(X_j) with the 50-digit A, to the Newton tolerance: the loop ends when the squared residual of the
    iterate BEFORE the last update is below tol_newton = 1e-16 and the last update contracts it further, so each component of the
    final residual is below sqrt(1e-16) = 1e-8 (in fact far below: the contraction is ~h |J - J0|)."""
    import mpmath as mp
    m, l, g = 0.7, 0.4, 9.81
    mech = K.make_mech([-1], [K.REVOLUTE], [K.WORLD_X], [[0.0, 1.0, 0.0]])
    rec = D.make_inertia(m, [0.0, 0.0, -l], np.zeros((3, 3))).reshape(1, 13)
    de, de_dual = _mech_de(mech, rec, (0.0, 0.0, -g))
    st = new_records(h0=2e-3)
    st["rule"] = 2
    log = []
    x0 = [0.9, -0.4]
    x, t = radau_step_scalar(de, de_dual, x0, 0.0, st, log=log)
    rule, h, flag, k_iter, X = log[-1]
    assert flag == 0 and rule == 2 and x == X[2]
    A = _generator().tables_mp(2)["A"]
    F = [de(X[j]) for j in range(3)]
    for i in range(3):
        for c in range(2):
            r = mp.mpf(X[i][c]) - mp.mpf(x0[c]) - mp.mpf(h) * sum(A[i, j] * mp.mpf(F[j][c]) for j in range(3))
            assert abs(r) < 1e-8
    # and against the closed form of the first integral: the energy error of an order-5 step of 2 ms is far below 1e-9
    E = lambda y: 0.5 * m * l * l * y[1] ** 2 - m * g * l * math.cos(y[0])
    assert abs(E(x) - E(x0)) < 1e-9 * abs(E(x0))


# ---- 4. synthetic de against a restatement of the reference --------------------------------------------------------------------
def reference_step(de, jac, x0, st, **par):
    """solveRadau as the reference runs it (radau_solve.jl, radau_functions.jl, adaptive.jl) in NumPy, on the reference's own table
    values: the explicit inverses of all NS matrices, the real part of the sum of the three products, pow.  st: dict(h, rule, cool,
    theta, theta_prev, psi, enorm0, enorm1), updated.  Returns (x, h_taken, attempts: list of (flag, k_iter)); x is None where the
    reference throws "time step is too small"."""
    p = dict(DEFAULTS, **par)
    fx = _fixture()
    x0 = np.array(x0, dtype=np.float64)
    n = x0.size
    neg_J, xx0 = -np.array(jac(x0), dtype=np.float64).reshape(n, n), np.array(de(x0), dtype=np.float64)
    attempts = []
    while True:
        s = st["rule"]
        A, lam, T, Ti, bh = fx["A%d" % s], fx["lam%d" % s], fx["T%d" % s], fx["Tinv%d" % s], fx["bhat%d" % s]
        NS, h = 2 * s - 1, st["h"]
        invC = [np.linalg.inv(neg_J.astype(complex) + (1.0 / h) * lam[i] * np.eye(n)) for i in range(NS)]
        X = [x0.copy() for _ in range(NS)]
        res_vec, flag, k_iter = [INF, INF, INF], 1, 0
        for k_iter in range(1, p["k_iter_max"] + 1):
            F = [np.array(de(X[i]), dtype=np.float64) for i in range(NS)]
            Ew, dZ, residual = np.zeros((NS, n), complex), np.zeros((NS, n), complex), 0.0
            for i in range(NS):
                r = X[i] - x0
                for j in range(NS):
                    r = r + (-h * A[i, j]) * F[j]
                residual += float(r @ r)
                for j in range(NS):
                    Ew[j] += ((1.0 / h) * lam[j] * Ti[j, i]) * r
            for i in range(NS):
                w = invC[i] @ Ew[i]
                for j in range(NS):
                    dZ[j] += T[j, i] * w
            diverged = False
            for i in range(NS):
                u = dZ[i].real
                if 10.0 < np.abs(u).max():
                    diverged = True
                    break
                X[i] = X[i] - u
            if diverged:
                flag = 3
                break
            if residual < p["tol_newton"]:
                flag = 0
                break
            if k_iter != 1:
                st["theta_prev"] = st["theta"]; st["theta"] = math.sqrt(residual); st["psi"] = math.sqrt(st["theta_prev"] * st["theta"])
            else:
                st["theta"] = math.sqrt(residual); st["psi"] = st["theta"]
            res_vec = [residual, res_vec[0], res_vec[1]]
            if res_vec[2] < res_vec[1] < res_vec[0]:
                flag = 3
                break
        attempts.append((flag, k_iter))
        if flag == 0:
            d = (bh[0] * h) * xx0
            for k in range(NS):
                d = d + ((bh[1 + k] - A[NS - 1, k]) * h) * F[k]
            e = (invC[0] @ d).real
            sc = p["tol_a"] + np.maximum(np.abs(X[NS - 1]), np.abs(x0)) * p["tol_r"]
            st["enorm0"], st["enorm1"] = st["enorm1"], math.sqrt(float(((e / sc) ** 2).sum()) / n)
            fac = 0.9 * (2 * p["k_iter_max"] + 1) / (2 * p["k_iter_max"] + k_iter)
            with np.errstate(divide="ignore"):
                h_new = fac * h * float(np.float64(1.0) / np.float64(st["enorm1"])) ** (1 / (1 + NS))
        else:
            h_new = h * 0.1
        h_new = min(p["h_max"], 2 * h, h_new)
        st["h"] = h_new
        if flag == 0:
            st["cool"] -= 1
            if st["cool"] < 1 and st["psi"] < 0.1:
                st["rule"] = min(st["rule"] + 1, p["max_rule"])
            return X[NS - 1], h, attempts
        st["cool"] = 10
        st["rule"] = max(st["rule"] - 1, 1)
        if st["h"] < p["h_min"]:
            return None, None, attempts


def _ref_records(h0=DEFAULTS["h0"], rule=1, cool=10):
    return dict(h=h0, rule=rule, cool=cool, theta=-9999.0, theta_prev=-9999.0, psi=9999.0, enorm0=-9999.0, enorm1=-9999.0)


def _synthetic(de, jac):
    """(de, de_dual) for radau_step_scalar from de and the Jacobian it is to be GIVEN (which need not be de's)."""
    def de_dual(x, seeds):
        J = np.array(jac(np.array(x)), dtype=np.float64).reshape(len(x), len(x))
        return de(np.array(x)), [list(J @ np.array(sd)) for sd in seeds]
    return (lambda x: [float(e) for e in de(np.array(x))]), de_dual


def _both(de, jac, x0, h0, rule=1, cool=10, steps=1, **par):
    """Run `steps` steps by the statement and by the reference restatement; flags, counts, rule and cooldown must be equal, h and x
    agree to rounding (1e-10 relative: the two differ in the conjugate factor, the solves and the pow, a few hundred roundings on
    well-conditioned 2 x 2 problems).  Returns the statement's records and per-step attempt lists."""
    f, f_dual = _synthetic(de, jac)
    st, rs = new_records(h0=h0), _ref_records(h0, rule, cool)
    st["rule"], st["cool"] = rule, cool
    x, xr, t, history = list(map(float, x0)), np.array(x0, dtype=np.float64), 0.0, []
    for _ in range(steps):
        log = []
        x, t = radau_step_scalar(f, f_dual, x, t, st, log=log, **par)
        xr_new, h_taken, attempts = reference_step(de, jac, xr, rs, **par)
        assert [(a[2], a[3]) for a in log] == attempts, (log, attempts)
        assert st["rule"] == rs["rule"] and st["cool"] == rs["cool"]
        assert abs(st["h"] - rs["h"]) <= 1e-10 * rs["h"]
        if xr_new is None:
            assert st["istate"][EXIT] == 5
            history.append(attempts)
            break
        assert st["istate"][EXIT] == 0 and st["nstate"][HTAKEN] == h_taken
        assert np.abs(np.array(x) - xr_new).max() <= 1e-10 * max(1.0, np.abs(xr_new).max())
        assert abs(st["nstate"][PSI] - rs["psi"]) <= 1e-6 * abs(rs["psi"]) and abs(st["enorm"][1] - rs["enorm1"]) <= 1e-6 * abs(rs["enorm1"]) + 1e-12      # eps |terms <= 1| / sc >= 1e-4
        xr = xr_new
        history.append(attempts)
    return st, history, x, t


M_STIFF = np.array([[-1000.0, 3.0], [2.0, -1.0]])


@pytest.mark.parametrize("rule", [1, 2])
def test_linear_stiff_matches_the_reference(rule):
    st, hist, x, t = _both(lambda x: M_STIFF @ x, lambda x: M_STIFF, [1.0, -2.0], 1e-4, rule=rule, steps=3)
    assert all(a[-1][0] == 0 and len(a) == 1 for a in hist) and all(a[0][1] == 2 for a in hist)      # exact Jacobian: two iterations


def test_an_update_above_ten_is_divergence_and_the_step_is_retried():
    # xdot = 1e10 with the Jacobian 0: the first update is h 1e10 > 10 at every h >= h_min: each attempt diverges in its first
    # iteration (flag 3) until h falls below h_min, where the reference throws and the statement retires the scene (flag 5)
    st, hist, x, t = _both(lambda x: np.array([1e10, 0.0]), lambda x: np.zeros((2, 2)), [0.0, 0.0], 1e-4)
    assert all(a == (3, 1) for a in hist[0]) and len(hist[0]) == 5 and st["istate"][EXIT] == 5 and x == [0.0, 0.0] and t == 0.0


def test_residuals_rising_twice_is_divergence():
    # xdot = a x with the Jacobian GIVEN as 0 (rule 1): X <- x0 + h a X, the residual doubles per iteration for h a = 2
    a = 2e4
    st, hist, x, t = _both(lambda x: a * x, lambda x: np.zeros((2, 2)), [1e-3, 2e-3], 1e-4)
    assert hist[0][0] == (3, 3)
    assert hist[0][-1][0] == 0                       # h = 1e-5: h a = 0.2 contracts


def test_fifteen_slow_iterations_hit_the_limit():
    a = 9e3                                         # h a = 0.9: contracts too slowly for 1e-16 in 15 iterations
    st, hist, x, t = _both(lambda x: a * x, lambda x: np.zeros((2, 2)), [1e-3, 2e-3], 1e-4)
    assert hist[0][0] == (1, 15)


def test_zero_error_norm_doubles_h_and_h_max_clamps():
    zero = lambda x: np.zeros(2)
    st, hist, x, t = _both(zero, lambda x: np.zeros((2, 2)), [1.0, 2.0], 1e-4)
    assert st["enorm"][1] == 0.0 and st["h"] == 2e-4 and hist[0] == [(0, 1)] and x == [1.0, 2.0] and t == 1e-4
    st, hist, x, t = _both(zero, lambda x: np.zeros((2, 2)), [1.0, 2.0], 0.008)
    assert st["h"] == 0.01
    st, hist, x, t = _both(lambda x: -x, lambda x: -np.eye(2), [1.0, 2.0], 0.009, rule=2)      # a finite estimate above h_max
    assert st["h"] == 0.01


def test_cooldown_expiry_with_small_psi_raises_the_rule():
    st, hist, x, t = _both(lambda x: -x, lambda x: -np.eye(2), [1.0, 2.0], 1e-4, steps=11)
    assert st["rule"] == 2 and st["cool"] == -1 and st["nstate"][PSI] < 0.1
    st, hist, x, t = _both(lambda x: -x, lambda x: -np.eye(2), [1.0, 2.0], 1e-4, steps=9)
    assert st["rule"] == 1 and st["cool"] == 1
    st, hist, x, t = _both(lambda x: -x, lambda x: -np.eye(2), [1.0, 2.0], 1e-4, steps=3, max_rule=1, cool=1)
    assert st["rule"] == 1


def test_deviations_nonfinite_is_flag_3_singular_is_flag_4_and_h_min_is_flag_5():
    nan_de = lambda x: [float("nan"), 0.0]
    f, f_dual = _synthetic(lambda x: np.array(nan_de(x)), lambda x: np.zeros((2, 2)))
    st = new_records()
    log = []
    x, t = radau_step_scalar(f, f_dual, [1.0, 2.0], 0.5, st, log=log)
    assert all(a[2] == 3 and a[3] == 1 for a in log) and st["istate"][EXIT] == 5 and x == [1.0, 2.0] and t == 0.5
    assert st["h"] < DEFAULTS["h_min"] and st["istate"][ATTEMPTS] == len(log) == 5 and log[0][4] == [[1.0, 2.0]]      # nothing was updated
    # a singular factor: -J + (1 / h) I = 0 for J = (1 / h) I
    st = new_records()
    f, f_dual = _synthetic(lambda x: x * 0.0, lambda x: np.eye(2) * (1.0 / 1e-4))
    log = []
    radau_step_scalar(f, f_dual, [1.0, 2.0], 0.0, st, log=log)
    assert log[0][2] == 4 and log[0][3] == 1 and st["istate"][EXIT] == 0 and log[-1][2] == 0
    # a retired scene is not armed again
    st = new_records()
    st["istate"][EXIT] = 5
    arm(st)
    assert st["istate"][ITER] == 0 and st["istate"][PHASE] == 0


def test_principal_value_flips_an_mrp_outside_the_unit_ball():
    st = new_records()
    st["istate"][:5] = [0, 2, 0, 1, 1]
    X = [[0.9, 0.8, 0.1, 5.0, 0.3, 0.2, 0.1, 7.0]]
    fac = factor_scalar([[0.0] * 8 for _ in range(8)], st["h"], 1)
    x, t = finish_scalar(st, fac, [0.0] * 8, 0.0, X, [[0.0] * 8], [0.0] * 8, mrp_off=(0, 4))
    nn = (0.9 * 0.9 + 0.8 * 0.8) + 0.1 * 0.1
    assert x == [-(0.9 / nn), -(0.8 / nn), -(0.1 / nn), 5.0, 0.3, 0.2, 0.1, 7.0]


# ---- 5. exports -------------------------------------------------------------------------------------------------------------------
def test_radau_symbols_are_declared_exported_and_bound(pfc):
    hdr = open(os.path.join(ROOT, "include", "pfc.h")).read()
    assert int(re.search(r"#define\s+PFC_MAX_NX_RADAU\s+(\d+)", hdr).group(1)) == MAX_NX
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in NAMES:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        res, args = pfc._lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, name
    out = subprocess.run(["nm", "-D", "--defined-only", pfc._lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pfc_[a-z_0-9]+)", out))
    assert {name for name, _ in NAMES} <= exported
    M = pfc.scenario.MechanismScenario
    for meth in ("radau_seed_device", "radau_jacobian_device", "radau_factor_device", "radau_unpack_device", "radau_newton_device",
                 "radau_finish_device", "radau_configure", "radau_sizes", "radau_set_state", "radau_get_state", "radau_set_rule_state", "radau_set_tau",
                 "radau_step", "radau_rule_state", "integrate_radau"):
        assert callable(getattr(M, meth)), meth
    assert callable(pfc.scenario.radau_table)


def test_radau_kernels_are_built_from_their_header():
    srcs = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "_lib.py")).read()
    assert '"pfc_radau.h"' in srcs and '"pfc_radau_tables.h"' in srcs      # a change of the kernels or the tables rebuilds the library
    src = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc", "pfc_hip.hip")).read()
    assert '#include "pfc_radau.h"' in src and '#include "pfc_radau_tables.h"' in src
    rad = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc", "pfc_radau.h")).read()
    for k in ("k_radau_seed", "k_radau_jac", "k_radau_factor", "k_radau_unpack", "k_radau_newton", "k_radau_finish"):
        assert "__global__ void __launch_bounds__" in rad and k + "(" in rad, k
    assert "fma(" not in rad
