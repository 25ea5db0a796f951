"""pfc_set_inertia, pfc_dynamics[_device], pfc_accelerations[_device], pfc_state_derivative[_device]: the C ABI, the scalar statement
of the kernels' arithmetic (csrc/pfc_dyn.h, stated in include/pfc.h) that tests/test_gpu_dynamics.py compares bytes with, and what
pins qdot, H, c and vdot without leaning on that statement -- without a device.

`dyn_scalar` and `chol_scalar` are the statement in Python floats (no fma, the written order), fed by test_kinematics_abi.kin_scalar.

The bound of `test_scalar_statement_agrees_with_joint_dynamics` (derived, not tuned).  scenario.joint_dynamics is the NumPy matrix
formulation on scenario.joint_kinematics' outputs.  Let D be the exact function (x_w_b, twist_w_b, columns) -> (H, c).
* B1 bounds |dyn_scalar - D(joint_kinematics' outputs)|: the statement is run a second time on `Err` numbers, (value, bound) pairs
  whose + - * carry  e(a + b) = e_a + e_b + u' |a + b|,  e(a b) = |a| e_b + |b| e_a + e_a e_b + u' |a b|  (u' = 0.51 eps, the .01
  covering the rounding of the bound's own arithmetic) -- the standard running error analysis -- with the kinematic inputs starting
  at test_kinematics_abi.kin_bound, the bound on |kin_scalar - joint_kinematics| that file derives and asserts.  The exact D of
  any input within those bounds, joint_kinematics' among them, then lies within the final bounds.
* B2 bounds |joint_dynamics - D(its own inputs)| by magnitudes, gamma_k = 1.01 k eps / 2.  The 6x6 world inertia is formed in at
  most 12 nested roundings from terms whose magnitudes are Iabs = [ |R||M||R|' + m |T||T| + |T||C| + |C||T|, hat(|R||cp| + m|t|) ;
  ., m I ] (T = hat t, C = hat(|R||cp|)); J' I J nests two products of inner dimension 6 (12 roundings, with or without fma) and the
  sum over bodies n_body more:  B2_H = gamma_(24 + n_body) sum_b |J_b|' Iabs_b |J_b|.  For c the chain is tw x_m S (6), Jdot v
  (nv), - g (1), I (12 + 6), tw x* (6), J' (6), the sum over bodies:  B2_c = gamma_(40 + nv + n_body) sum_b |J_b|' (Iabs_b
  (|Jdot_b||v| + |g|) + |crm(tw_b)|' Iabs_b |tw_b|).
* qdot: both sides spend at most 8 roundings on pdot's terms, whose magnitudes sum to 1/4 ((1 + p.p)|w| + 2 |p| x |w| + 2 (|p|.|w|)|p|),
  and tdot = R_j u carries the joint rotation's 33 eps + 38 eps (test_kinematics_abi.JOINT_ERR, Frobenius) times |u|_2 plus
  gamma_3 twice on |R||u|.
The test asserts |difference| <= B1 + B2 elementwise and that the bound stays a rounding bound: below 1e-8, which is the kinematic
bound's 1e-12 on a pose times the sensitivity of H and c to a pose, of order m |t| n_body (1 + |v|^2 + |g|) <~ 1e4 for |t| <= 10 per
joint at depth 4, |v| <= 1 and inertias of order one (|H| and |c| themselves reach 1e3)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

import test_kinematics_abi as K
from test_kinematics_abi import EPS, FIXED, FLOATING, NDOF, PRISMATIC, REVOLUTE, WORLD_X, make_mech, mech_a, mech_b, mech_c, random_state

ROOT = K.ROOT
NAMES = (("pfc_set_inertia", 4), ("pfc_dynamics_device", 10), ("pfc_dynamics", 9), ("pfc_accelerations_device", 9),
         ("pfc_accelerations", 8), ("pfc_state_derivative_device", 27), ("pfc_state_derivative", 26))
MAX_NV_SOLVE = 64
GRAVITY = (0.0, 0.0, -9.81)


# ---- inertias ------------------------------------------------------------------------------------------------------------------
def make_inertia(m, com, Ic):
    """The 13-double record from the mass, the centre of mass and the moment about it (3x3), all in the body frame."""
    com = np.asarray(com, dtype=np.float64)
    Kc = np.array([[0.0, -com[2], com[1]], [com[2], 0.0, -com[0]], [-com[1], com[0], 0.0]])
    M = np.asarray(Ic, dtype=np.float64) + m * (Kc @ Kc.T)
    M = 0.5 * (M + M.T)
    return np.concatenate([M.reshape(-1, order="F"), m * com, [m]])


def random_inertia(mech, rng, massless=()):
    """One record per body: mass in (0.5, 2), a centre of mass within 0.3 of the frame origin, principal moments in (0.05, 0.3) about
    random axes; bodies in `massless` get zeros."""
    out = np.zeros((mech["n_body"], 13))
    for b in range(mech["n_body"]):
        if b in massless:
            continue
        Q = K._random_rotation(rng)
        out[b] = make_inertia(rng.uniform(0.5, 2.0), rng.uniform(-0.3, 0.3, 3), Q @ np.diag(rng.uniform(0.05, 0.3, 3)) @ Q.T)
    return out


# ---- the scalar statement ------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _inertia_to_world(rec, x):
    m, t = rec[12], x[9:12]
    hc = [(x[r] * rec[9] + x[3 + r] * rec[10]) + x[6 + r] * rec[11] for r in range(3)]
    mt = [m * t[r] for r in range(3)]
    h = [hc[r] + mt[r] for r in range(3)]
    B = [None] * 9
    for c in range(3):
        for r in range(3):
            B[3 * c + r] = (x[r] * rec[3 * c] + x[3 + r] * rec[3 * c + 1]) + x[6 + r] * rec[3 * c + 2]
    s1 = (t[0] * hc[0] + t[1] * hc[1]) + t[2] * hc[2]
    s2 = (t[0] * mt[0] + t[1] * mt[1]) + t[2] * mt[2]
    d = 2.0 * s1 + s2
    J = []
    for r in range(3):
        for c in range(r, 3):
            A = (B[r] * x[c] + B[3 + r] * x[3 + c]) + B[6 + r] * x[6 + c]
            e = (A - (hc[r] * t[c] + t[r] * hc[c])) - mt[r] * t[c]
            J.append(e + d if r == c else e)
    return J + h + [m]


def _mul(I, m):
    h = I[6:9]
    return [((I[0] * m[0] + I[1] * m[1]) + I[2] * m[2]) + (h[1] * m[5] - h[2] * m[4]),
            ((I[1] * m[0] + I[3] * m[1]) + I[4] * m[2]) + (h[2] * m[3] - h[0] * m[5]),
            ((I[2] * m[0] + I[4] * m[1]) + I[5] * m[2]) + (h[0] * m[4] - h[1] * m[3]),
            I[9] * m[3] - (h[1] * m[2] - h[2] * m[1]),
            I[9] * m[4] - (h[2] * m[0] - h[0] * m[2]),
            I[9] * m[5] - (h[0] * m[1] - h[1] * m[0])]


def _crossm(a, b):
    p, q = _cross(a[:3], b[3:]), _cross(a[3:], b[:3])
    return _cross(a[:3], b[:3]) + [p[r] + q[r] for r in range(3)]


def _crossf(a, f):
    p, q = _cross(a[:3], f[:3]), _cross(a[3:], f[3:])
    return [p[r] + q[r] for r in range(3)] + _cross(a[:3], f[3:])


def _dot6(a, b):
    return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5]


def subtree(mech, b):
    return [d for d in range(b, mech["n_body"]) if b in K.ancestors(mech, d)]


def dyn_core(mech, inertia, g, v, xs, tws, cols, zero=0.0):
    """H (nv lists of nv) and c (nv) from the kinematic quantities, on whatever numbers they are made of (floats, Err)."""
    nb, nv = mech["n_body"], mech["nv"]
    I = [_inertia_to_world(list(inertia[b]), xs[b]) for b in range(nb)]
    jt = []
    for b in range(nb):
        o, n = int(mech["off"][b]), NDOF[int(mech["joint_type"][b])]
        t = [zero] * 6
        for k in range(n):
            t = [cols[o + k][e] * v[o + k] if k == 0 else t[e] + cols[o + k][e] * v[o + k] for e in range(6)]
        jt.append(t)
    w = []
    for b in range(nb):
        a = [zero, zero, zero, -g[0], -g[1], -g[2]]
        for p in reversed(K.ancestors(mech, b)):
            o = _crossm(tws[p], jt[p])
            a = [a[e] + o[e] for e in range(6)]
        w1, w3 = _mul(I[b], a), _crossf(tws[b], _mul(I[b], tws[b]))
        w.append([w1[e] + w3[e] for e in range(6)])
    Ic, W = [], []
    for b in range(nb):
        i, ww = I[b], w[b]
        for d in subtree(mech, b)[1:]:
            i = [i[e] + I[d][e] for e in range(10)]
            ww = [ww[e] + w[d][e] for e in range(6)]
        Ic.append(i); W.append(ww)
    owner = [b for b in range(nb) for _ in range(NDOF[int(mech["joint_type"][b])])]
    H = [[zero] * nv for _ in range(nv)]
    c = [None] * nv
    for i in range(nv):
        b = owner[i]
        F = _mul(Ic[b], cols[i])
        c[i] = _dot6(cols[i], W[b])
        anc = K.ancestors(mech, b)
        for j in range(i + 1):
            H[i][j] = _dot6(cols[j], F) if owner[j] in anc else zero
            H[j][i] = H[i][j]
    return H, c


def qdot_scalar(mech, q, v):
    qd = [float(e) for e in v]
    for b, t in enumerate(mech["joint_type"]):
        if t == FLOATING:
            o = int(mech["off"][b])
            p, w, u = [float(e) for e in q[o:o + 3]], [float(e) for e in v[o:o + 3]], [float(e) for e in v[o + 3:o + 6]]
            p2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
            pw = (p[0] * w[0] + p[1] * w[1]) + p[2] * w[2]
            a, bb, cr = 1.0 - p2, 2.0 * pw, _cross(p, w)
            xj, _ = K._joint(FLOATING, [0.0] * 3, [float(e) for e in q[o:o + 6]], [0.0] * 6, None)
            for r in range(3):
                qd[o + r] = 0.25 * ((a * w[r] + 2.0 * cr[r]) + bb * p[r])
                qd[o + 3 + r] = (xj[r] * u[0] + xj[3 + r] * u[1]) + xj[6 + r] * u[2]
    return qd


def dyn_scalar(mech, inertia, g, q, v, trig=None):
    """One scene in Python floats, expression for expression as include/pfc.h states pfc_dynamics_device.  Returns qdot (nv,),
    H (nv,nv), c (nv,) as arrays."""
    xs, tws, cols = K.kin_scalar(mech, q, v, trig)
    vf = [float(e) for e in v]
    H, c = dyn_core(mech, [[float(e) for e in row] for row in np.asarray(inertia).reshape(-1, 13)], [float(e) for e in g], vf, xs, tws, cols)
    nv = mech["nv"]
    return np.array(qdot_scalar(mech, q, v)).reshape(nv), np.array(H, dtype=np.float64).reshape(nv, nv), np.array(c, dtype=np.float64).reshape(nv)


def chol_scalar(H, c, f, tau=None):
    """vdot = H^-1 ((f - c) + tau) in the order include/pfc.h states for pfc_accelerations_device.  Returns (vdot (nv,), info)."""
    n = len(c)
    A = [[float(H[i][j]) for j in range(n)] for i in range(n)]
    rhs = [(float(f[i]) - float(c[i])) + (float(tau[i]) if tau is not None else 0.0) for i in range(n)]
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        col = []
        for i in range(j, n):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            col.append(s)
        if not col[0] > 0.0:
            return np.full(n, np.nan), j + 1
        L[j][j] = math.sqrt(col[0])
        for i in range(j + 1, n):
            L[i][j] = col[i - j] / L[j][j]
    y = [0.0] * n
    for i in range(n):
        s = rhs[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(n - 1, i, -1):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    return np.array(x), 0


def dyn_reference(mech, inertia, g, q, v, trig=None):
    """(qdot (n_scene,nv), H (n_scene,nv,nv), c (n_scene,nv)) by dyn_scalar."""
    q, v = np.atleast_2d(q), np.atleast_2d(v)
    out = [dyn_scalar(mech, inertia, g, q[s], v[s], trig) for s in range(q.shape[0])]
    return tuple(np.array([o[k] for o in out]) for k in range(3))


# ---- running error numbers ----------------------------------------------------------------------------------------------------
U1 = 0.51 * EPS


class Err:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = float(v), float(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def __add__(self, o):
        o = Err.of(o); z = self.v + o.v
        return Err(z, self.e + o.e + U1 * abs(z))

    __radd__ = __add__

    def __sub__(self, o):
        o = Err.of(o); z = self.v - o.v
        return Err(z, self.e + o.e + U1 * abs(z))

    def __rsub__(self, o):
        return Err.of(o) - self

    def __neg__(self):
        return Err(-self.v, self.e)

    def __mul__(self, o):
        o = Err.of(o); z = self.v * o.v
        return Err(z, abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e + U1 * abs(z))

    __rmul__ = __mul__


def _hat(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def _crm(t):
    M = np.zeros((6, 6))
    M[:3, :3] = _hat(t[:3]); M[3:, 3:] = _hat(t[:3]); M[3:, :3] = _hat(t[3:])
    return M


def spatial_inertia_world(rec, x):
    """The 6x6 inertia of a body in world about the world origin, NumPy: through the centre of mass (not the statement's form)."""
    R, t = np.asarray(x[:9]).reshape(3, 3, order="F"), np.asarray(x[9:])
    M, cp, m = np.asarray(rec[:9]).reshape(3, 3, order="F"), np.asarray(rec[9:12]), float(rec[12])
    I6 = np.zeros((6, 6))
    if m == 0.0:
        return I6
    com = R @ (cp / m) + t
    Jc = R @ (M - m * (_hat(cp / m) @ _hat(cp / m).T)) @ R.T
    I6[:3, :3] = Jc + m * (_hat(com) @ _hat(com).T); I6[:3, 3:] = m * _hat(com); I6[3:, :3] = -m * _hat(com); I6[3:, 3:] = m * np.eye(3)
    return I6


def _inertia_abs(rec, x):
    R, t = np.abs(np.asarray(x[:9]).reshape(3, 3, order="F")), np.abs(np.asarray(x[9:]))
    M, cp, m = np.abs(np.asarray(rec[:9]).reshape(3, 3, order="F")), np.abs(np.asarray(rec[9:12])), float(rec[12])
    T, Cm = np.abs(_hat(t)), np.abs(_hat(R @ cp))
    A = np.zeros((6, 6))
    A[:3, :3] = R @ M @ R.T + m * (T @ T) + T @ Cm + Cm @ T
    A[:3, 3:] = np.abs(_hat(R @ cp + m * t)); A[3:, :3] = A[:3, 3:]; A[3:, 3:] = m * np.eye(3)
    return A


def dyn_bound(pfc, mech, inertia, g, q, v):
    """(bound on qdot, on H, on c), elementwise, between dyn_scalar and scenario.joint_dynamics; the module docstring derives it."""
    nb, nv = mech["n_body"], mech["nv"]
    xs, tws, cols = K.kin_scalar(mech, q, v)
    bx, btw, bj = K.kin_bound(mech, q, v)
    owner = [b for b in range(nb) for _ in range(NDOF[int(mech["joint_type"][b])])]
    ex = [[Err(xs[b][e], bx[b, e]) for e in range(12)] for b in range(nb)]
    etw = [[Err(tws[b][e], btw[b, e]) for e in range(6)] for b in range(nb)]
    ecol = [[Err(cols[i][e], bj[owner[i], i, e]) for e in range(6)] for i in range(nv)]
    He, ce = dyn_core(mech, [[Err(e) for e in row] for row in inertia], [Err(e) for e in g], [Err(e) for e in v], ex, etw, ecol, zero=Err(0.0))
    B1H = np.array([[He[i][j].e for j in range(nv)] for i in range(nv)]); B1c = np.array([ce[i].e for i in range(nv)])
    xn, twn, Jn = pfc.scenario.joint_kinematics(mech["parent"], mech["joint_type"], mech["x_p_j"], mech["axis"], q, v)
    gam = lambda k: 1.01 * k * EPS / 2
    B2H, B2c = np.zeros((nv, nv)), np.zeros(nv)
    g6 = np.abs(np.concatenate([np.zeros(3), g]))
    for b in range(nb):
        Ja, Ia = np.abs(Jn[b].T), _inertia_abs(inertia[b], xn[b])
        Jd = np.zeros((6, nv))
        for k in range(nv):
            Jd[:, k] = np.abs(_crm(twn[owner[k]])) @ Ja[:, k]
        B2H += Ja.T @ Ia @ Ja
        B2c += Ja.T @ (Ia @ (Jd @ np.abs(v) + g6) + np.abs(_crm(twn[b])).T @ (Ia @ np.abs(twn[b])))
    Bq = np.zeros(nv)
    for b, t in enumerate(mech["joint_type"]):
        if t == FLOATING:
            o = int(mech["off"][b])
            p, w, u = np.abs(q[o:o + 3]), np.abs(v[o:o + 3]), np.abs(v[o + 3:o + 6])
            Bq[o:o + 3] = 16 * EPS * 0.25 * ((1 + p @ p) * w + 2 * K._acx(p, w) + 2 * (p @ w) * p)
            xj, _ = K._joint(FLOATING, [0.0] * 3, [float(e) for e in q[o:o + 6]], [0.0] * 6, None)
            Bq[o + 3:o + 6] = 71 * EPS * np.linalg.norm(u) + 3 * EPS * (np.abs(K._R(xj)) @ u)
    return Bq, B1H + gam(24 + nb) * B2H, B1c + gam(40 + nv + nb) * B2c


# ---- 1. ABI --------------------------------------------------------------------------------------------------------------------
def test_dynamics_symbols_are_declared_exported_and_bound(pfc):
    hdr = open(os.path.join(ROOT, "include", "pfc.h")).read()
    assert re.search(r"#define\s+PFC_MAX_NV_SOLVE\s+(\d+)", hdr) and int(re.search(r"#define\s+PFC_MAX_NV_SOLVE\s+(\d+)", hdr).group(1)) >= 64
    assert int(re.search(r"#define\s+PFC_MAX_NV_SOLVE\s+(\d+)", hdr).group(1)) == MAX_NV_SOLVE
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
    for meth in ("set_inertia", "dynamics", "dynamics_device", "accelerations", "accelerations_device", "state_derivative",
                 "state_derivative_device"):
        assert callable(getattr(M, meth)), meth
    assert callable(pfc.scenario.joint_dynamics) and callable(pfc.geometry.mesh_inertia)


def test_dynamics_kernels_are_built_from_their_header(pfc):
    srcs = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "_lib.py")).read()
    assert '"pfc_dyn.h"' in srcs      # a change of the kernels rebuilds the library
    src = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc", "pfc_hip.hip")).read()
    assert '#include "pfc_dyn.h"' in src
    dyn = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc", "pfc_dyn.h")).read()
    assert "kin_column<double>" in dyn and "atomic" not in dyn.replace("no atomics", "")


# ---- 2. the statement against scenario.joint_dynamics ---------------------------------------------------------------------------
def _numpy_dynamics(pfc, mech, inertia, g, q, v):
    return pfc.scenario.joint_dynamics(mech["parent"], mech["joint_type"], mech["x_p_j"], mech["axis"], inertia, g, q, v)


def test_scalar_statement_agrees_with_joint_dynamics(pfc):
    rng = np.random.default_rng(20261019)
    worst, largest = 0.0, 0.0
    for k in range(48):
        mech = (mech_a(), mech_b(), mech_c(), mech_a(seed=6))[k % 4]
        q, v = random_state(mech, rng, k // 4)
        inertia = random_inertia(mech, rng)
        g = np.array(GRAVITY) if k % 3 else rng.uniform(-10, 10, 3)
        got = dyn_scalar(mech, inertia, g, q, v)
        ref = _numpy_dynamics(pfc, mech, inertia, g, q, v)
        bnd = dyn_bound(pfc, mech, inertia, g, q, v)
        for name, a, r, b in zip(("qdot", "H", "c"), got, ref, bnd):
            d = np.abs(a - r)
            assert (d <= b).all(), (k, name, np.argwhere(d > b)[:4], d.max(), b.max())
            worst = max(worst, float((d / np.maximum(b, 1e-300)).max()))
            largest = max(largest, float(b.max()))
    print(f"largest difference / bound over 48 states: {worst:.3f}; largest bound {largest:.2e}")
    assert largest < 1e-8      # a rounding bound, not a loose one


# ---- 3. properties of H --------------------------------------------------------------------------------------------------------
def test_mass_matrix_is_symmetric_to_the_bit_positive_definite_and_zero_across_branches():
    rng = np.random.default_rng(7)
    for k in range(12):
        mech = (mech_a(), mech_b(), mech_c())[k % 3]
        q, v = random_state(mech, rng, k)
        _, H, _ = dyn_scalar(mech, random_inertia(mech, rng), GRAVITY, q, v)
        assert H.tobytes() == np.ascontiguousarray(H.T).tobytes()
        assert np.linalg.eigvalsh(H).min() > 0
    mech = mech_a()
    q, v = random_state(mech, rng)
    _, H, _ = dyn_scalar(mech, random_inertia(mech, rng), GRAVITY, q, v)
    # coordinates 0..5 b0, 6 b1, 7 b2, 8 b4 (a branch off b0), 9 b5 (a second root)
    related = {6: range(0, 8), 7: range(0, 8), 8: list(range(0, 6)) + [8], 9: [9]}
    for i, rel in related.items():
        for j in range(10):
            if j in rel:
                assert H[i, j] != 0
            else:
                assert H[i, j].tobytes() == np.float64(0.0).tobytes() and H[j, i].tobytes() == np.float64(0.0).tobytes()   # +0.0


# ---- 4. c from derivatives of the pinned Jacobians -----------------------------------------------------------------------------
def _c_from_jacobian_differences(pfc, mech, inertia, g, q, v, h):
    args = (mech["parent"], mech["joint_type"], mech["x_p_j"], mech["axis"])
    qd = K.state_rate(mech, q, v)
    x, tw, J = pfc.scenario.joint_kinematics(*args, q, v)
    _, _, Jp = pfc.scenario.joint_kinematics(*args, q + h * qd, v)
    _, _, Jm = pfc.scenario.joint_kinematics(*args, q - h * qd, v)
    g6 = np.concatenate([np.zeros(3), g])
    c, scale = np.zeros(mech["nv"]), np.zeros(mech["nv"])
    for b in range(mech["n_body"]):
        I6 = spatial_inertia_world(inertia[b], x[b])
        Jdv = ((Jp[b] - Jm[b]) / (2 * h)).T @ v
        c += J[b] @ (I6 @ (Jdv - g6) - _crm(tw[b]).T @ (I6 @ tw[b]))
        scale += np.abs(J[b]) @ (np.abs(I6) @ (np.abs(Jdv) + np.abs(g6)) + np.abs(_crm(tw[b])).T @ (np.abs(I6) @ np.abs(tw[b])))
    return c, scale


def test_bias_is_the_sum_formula_with_differenced_jacobians(pfc):
    """c = sum_b J_b' (I_b (Jdot_b v - [0; g]) + tw_b x* I_b tw_b) with Jdot_b v from central differences of joint_kinematics'
    Jacobians along state_rate -- quantities test_kinematics_abi pins -- in Float64 at two steps, h = 2e-3 and 1e-3.  The error must
    fall as h^2 (a ratio of 4; asserted within [3.5, 4.5] where the finer error is a thousand times above the rounding floor
    eps |J| / h) and the finer one must lie below h^2 times the magnitude sum of the formula's terms: truncation is
    h^2 / 6 |d3 J / dt3 v|, and the third derivative of a column along a motion with |v| <= 1 is below 6 times the magnitudes
    (each derivative multiplies by a twist of norm <= sqrt(3) (1 + |t|) / (1 + |t|), the lever arm already being in |J|)."""
    rng = np.random.default_rng(11)
    seen = 0
    for k in range(9):
        mech = (mech_a(), mech_b(), mech_c())[k % 3]
        q, v = random_state(mech, rng, 2 * k)       # |p| < 1
        inertia = random_inertia(mech, rng)
        g = np.array(GRAVITY)
        _, _, c = dyn_scalar(mech, inertia, g, q, v)
        c1, scale = _c_from_jacobian_differences(pfc, mech, inertia, g, q, v, 2e-3)
        c2, _ = _c_from_jacobian_differences(pfc, mech, inertia, g, q, v, 1e-3)
        e1, e2 = np.abs(c1 - c), np.abs(c2 - c)
        assert (e2 <= 1e-6 * scale + 1e-9).all(), (k, e2, scale)
        for i in range(mech["nv"]):
            if e2[i] > 1e3 * EPS * scale[i] / 1e-3:
                seen += 1
                assert 3.5 <= e1[i] / e2[i] <= 4.5, (k, i, e1[i], e2[i])
    assert seen >= 10


def test_power_balance(pfc):
    """With tau = f = 0, H vdot = -c, and energy is conserved: d/dt (1/2 v'Hv + V) = 0 gives v'c = 1/2 v' Hdot v + dV/dt, V = -sum m
    g . com.  Hdot and dV/dt by central differences of dyn_scalar's H and of V along qdot, at h and h / 2 as above: O(h^2), the
    finer error below h^2 times the magnitudes."""
    rng = np.random.default_rng(12)
    for k in range(6):
        mech = (mech_a(), mech_c(), mech_b())[k % 3]
        q, v = random_state(mech, rng, 2 * k)
        inertia = random_inertia(mech, rng)
        g = np.array(GRAVITY)
        qd, H, c = dyn_scalar(mech, inertia, g, q, v)

        def energy_rate(h):
            def V(qq):
                xs, _, _ = K.kin_scalar(mech, qq, v)
                return -sum(float(g @ (K._R(xs[b]) @ inertia[b, 9:12] + inertia[b, 12] * np.asarray(xs[b][9:]))) for b in range(mech["n_body"]))
            Hp, Hm = dyn_scalar(mech, inertia, g, q + h * qd, v)[1], dyn_scalar(mech, inertia, g, q - h * qd, v)[1]
            return 0.5 * v @ ((Hp - Hm) / (2 * h)) @ v + (V(q + h * qd) - V(q - h * qd)) / (2 * h)
        lhs = float(v @ c)
        scale = float(np.abs(v) @ np.abs(H) @ np.abs(v)) * 10 + float(np.abs(v) @ np.abs(c))
        e1, e2 = abs(energy_rate(2e-3) - lhs), abs(energy_rate(1e-3) - lhs)
        assert e2 <= 1e-6 * scale + 1e-9, (k, e1, e2, scale)
        assert e2 <= e1 / 3 or e2 <= 1e3 * EPS * scale / 1e-3, (k, e1, e2)


# ---- 5. qdot -------------------------------------------------------------------------------------------------------------------
def test_pose_differentiated_along_qdot_reproduces_the_twist():
    """test_kinematics_abi.test_twist_is_the_time_derivative_of_the_pose with the new qdot output in place of state_rate: the same
    step, the same tolerance."""
    rng = np.random.default_rng(5)
    h = 1e-6
    for k in range(30):
        mech = (mech_a(), mech_b(), mech_c())[k % 3]
        q, v = random_state(mech, rng, k)
        qd, _, _ = dyn_scalar(mech, random_inertia(mech, rng), GRAVITY, q, v)
        xs, tws, _ = K.kin_scalar(mech, q, v)
        xp, _, _ = K.kin_scalar(mech, q + h * qd, v)
        xm, _, _ = K.kin_scalar(mech, q - h * qd, v)
        for b in range(mech["n_body"]):
            x = np.asarray(xs[b]); dx = (np.asarray(xp[b]) - np.asarray(xm[b])) / (2 * h)
            W = K._R(dx) @ K._R(x).T
            omega = np.array([W[2, 1], W[0, 2], W[1, 0]])
            lin = dx[9:] - np.cross(omega, x[9:])
            tol = 1e-7 * (1 + np.abs(x).max())
            assert np.abs(np.concatenate([omega, lin]) - tws[b]).max() <= tol, (k, b)


# ---- 6. closed forms -----------------------------------------------------------------------------------------------------------
def test_free_body_is_newton_euler_in_the_body_frame():
    """One floating body: H is the body-frame spatial inertia [[M, cp^], [-cp^, m]] and, with a = -R'g, n = M w + cp x u,
    f = m u - cp x w:  c = [cp x a + w x n + u x f;  m a + w x f].  The statement works in world coordinates, where the terms reach
    m (1 + |t|)^2 (1 + |v|^2 + |g|) =: scale; about 60 roundings lie between the two: tolerance 64 eps scale."""
    rng = np.random.default_rng(13)
    mech = make_mech([-1], [FLOATING], [np.concatenate([K._random_rotation(rng).reshape(-1, order="F"), rng.uniform(-1, 1, 3)])], [[0, 0, 0]])
    for k in range(20):
        q, v = random_state(mech, rng, k)
        rec = random_inertia(mech, rng)
        g = rng.uniform(-10, 10, 3)
        _, H, c = dyn_scalar(mech, rec, g, q, v)
        xs, _, _ = K.kin_scalar(mech, q, v)
        R, t = K._R(xs[0]), np.asarray(xs[0][9:])
        M, cp, m = rec[0, :9].reshape(3, 3, order="F"), rec[0, 9:12], rec[0, 12]
        w, u, a = v[:3], v[3:], -R.T @ g
        n, f = M @ w + np.cross(cp, u), m * u - np.cross(cp, w)
        ref = np.concatenate([np.cross(cp, a) + np.cross(w, n) + np.cross(u, f), m * a + np.cross(w, f)])
        Href = np.block([[M, _hat(cp)], [-_hat(cp), m * np.eye(3)]])
        scale = m * (1 + np.linalg.norm(t)) ** 2 * (1 + v @ v + np.linalg.norm(g))
        assert np.abs(c - ref).max() <= 64 * EPS * scale, (k, np.abs(c - ref).max(), scale)
        assert np.abs(H - Href).max() <= 64 * EPS * scale


def test_point_mass_pendulum():
    """A point mass m at (0, 0, -l) of a body revolute about y on the world: H = m l^2, c = m g l sin(theta), vdot = -(g / l) sin(theta)
    (f = tau = 0): a handful of roundings, 16 eps relative."""
    m, l, g = 0.7, 0.4, 9.81
    mech = make_mech([-1], [REVOLUTE], [WORLD_X], [[0.0, 1.0, 0.0]])
    rec = make_inertia(m, [0.0, 0.0, -l], np.zeros((3, 3))).reshape(1, 13)
    for th in (-2.5, -0.3, 0.0, 0.9, 3.0):
        _, H, c = dyn_scalar(mech, rec, (0.0, 0.0, -g), [th], [1.3])
        assert abs(H[0, 0] - m * l * l) <= 16 * EPS * m * l * l
        assert abs(c[0] - m * g * l * math.sin(th)) <= 16 * EPS * m * g * l
        vdot, info = chol_scalar(H, c, [0.0])
        assert info == 0 and abs(vdot[0] + (g / l) * math.sin(th)) <= 32 * EPS * g / l


def test_prismatic_mass_on_a_revolute_arm():
    """A massless arm revolute about z, a point mass sliding along its x: position r (cos th, sin th), gravity -g e_y.
    H = diag(m r^2, m), c = [2 m r rdot thdot + m g r cos th,  -m r thdot^2 + m g sin th]: the Coriolis and the centrifugal term."""
    m, g = 1.3, 9.81
    mech = make_mech([-1, 0], [REVOLUTE, PRISMATIC], [WORLD_X, WORLD_X], [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    rec = np.zeros((2, 13)); rec[1, 12] = m
    rng = np.random.default_rng(14)
    for _ in range(10):
        th, r, thd, rd = rng.uniform(-3, 3), rng.uniform(0.2, 2), rng.uniform(-1, 1), rng.uniform(-1, 1)
        _, H, c = dyn_scalar(mech, rec, (0.0, -g, 0.0), [th, r], [thd, rd])
        scale = m * (1 + r) ** 2 * (1 + g)
        ref = [2 * m * r * rd * thd + m * g * r * math.cos(th), -m * r * thd * thd + m * g * math.sin(th)]
        assert np.abs(H - np.diag([m * r * r, m])).max() <= 32 * EPS * scale
        assert np.abs(c - ref).max() <= 32 * EPS * scale


# ---- 7. the solve --------------------------------------------------------------------------------------------------------------
def test_cholesky_solve_against_fifty_digits():
    """chol_scalar against mpmath's solve of the same H and the same rounded right-hand side at 50 digits.  Higham, Accuracy and
    Stability of Numerical Algorithms, Theorem 10.4: the computed x solves (H + dH) x = b with |dH| <= gamma_(3n+1) |L'||L|, and
    (10.7) | |L'||L| |_2 <= n (1 - n gamma_(n+1))^-1 |H|_2; so |x - x*|_2 / |x*|_2 <= k / (1 - k) with k = n gamma_(3n+1) kappa_2(H)
    (1 - n gamma_(n+1))^-1, asserted as 2 k with k < 1/2; gamma_m = m u / (1 - m u), u = 2^-53, kappa_2 from mpmath's eigenvalues."""
    import mpmath
    mpmath.mp.dps = 50
    rng = np.random.default_rng(15)
    worst = 0.0
    for k in range(6):
        mech = (mech_a(), mech_b(), mech_c())[k % 3]
        q, v = random_state(mech, rng, k)
        _, H, c = dyn_scalar(mech, random_inertia(mech, rng), GRAVITY, q, v)
        n = mech["nv"]
        f, tau = rng.standard_normal(n), rng.standard_normal(n)
        x, info = chol_scalar(H, c, f, tau)
        assert info == 0
        rhs = [(float(f[i]) - float(c[i])) + float(tau[i]) for i in range(n)]
        Hm = mpmath.matrix(H.tolist())
        ref = mpmath.lu_solve(Hm, mpmath.matrix(rhs))
        ev = mpmath.eigsy(Hm, eigvals_only=True)
        kappa = max(ev) / min(ev)
        u = mpmath.mpf(2) ** -53
        gam = lambda m: m * u / (1 - m * u)
        kk = n * gam(3 * n + 1) * kappa / (1 - n * gam(n + 1))
        assert kk < 0.5
        err = mpmath.norm(mpmath.matrix(x.tolist()) - ref) / mpmath.norm(ref)
        assert err <= 2 * kk, (k, float(err), float(kk))
        worst = max(worst, float(err / (2 * kk)))
    print(f"Cholesky solve: largest error / bound {worst:.2e}")


def test_massless_moving_body_flags_its_pivot():
    mech = mech_c()      # coordinates 0 (b0), 1 (b1), 2 (b2), 3 (b3): b3 massless makes pivot 4 zero
    rng = np.random.default_rng(16)
    q, v = random_state(mech, rng)
    _, H, c = dyn_scalar(mech, random_inertia(mech, rng, massless=(3,)), GRAVITY, q, v)
    assert H[3, 3] == 0.0
    vdot, info = chol_scalar(H, c, np.zeros(4))
    assert info == 4 and np.isnan(vdot).all()
    H[1, 1] = np.nan
    vdot, info = chol_scalar(H, c, np.zeros(4))
    assert info == 2 and np.isnan(vdot).all()


# ---- 8. geometry.mesh_inertia --------------------------------------------------------------------------------------------------
def test_mesh_inertia_of_a_box_shell_and_a_solid_box(pfc):
    """A box of half-widths r = (a, b, c) centred at t.  Solid, density rho: m = 8 rho a b c, I_xx = m (b^2 + c^2) / 3 about the
    centre.  Shell of thickness d: the faces normal to x weigh rho d 4 b c each and have I_xx = m_f (b^2 + c^2) / 3, those normal to
    y have m_f (a^2 / 3 + c^2) about the box's x axis (offset b... by the axis theorem) and so on.  The rules are exact for the
    quadratic integrand (the reference's getTriQuadRule(3) / getTetQuadRule(4) are as well), so what is left is the rounding of
    sums of n_elem x n_quad terms: bound n_terms eps times the sum of the terms' magnitudes, which is below m (|t| + |r|)^2 for
    every entry of the moment about the frame origin."""
    G = pfc.geometry
    r, t, rho, d = np.array([0.05, 0.08, 0.03]), np.array([0.3, -0.2, 0.1]), 400.0, 0.09
    solid = G.emesh_box_div(r, 2, t)
    shell = G.as_tri_emesh(G.emesh_box_div(r, 2, t))
    a, b, c = r
    for mesh, dd, m, Ic in (
            (solid, None, 8 * rho * a * b * c, 8 * rho * a * b * c / 3 * np.array([b * b + c * c, a * a + c * c, a * a + b * b])),
            (shell, d, rho * d * 8 * (a * b + b * c + a * c), None)):
        if Ic is None:
            mx, my, mz = (rho * d * 4 * s for s in (b * c, a * c, a * b))      # one face normal to x, y, z
            Ic = np.array([2 * mx * (b * b + c * c) / 3 + 2 * my * (b * b + c * c / 3) + 2 * mz * (c * c + b * b / 3),
                           2 * my * (a * a + c * c) / 3 + 2 * mx * (a * a + c * c / 3) + 2 * mz * (c * c + a * a / 3),
                           2 * mz * (a * a + b * b) / 3 + 2 * mx * (a * a + b * b / 3) + 2 * my * (b * b + a * a / 3)])
        rec = G.mesh_inertia(mesh, rho, dd)
        ref = make_inertia(m, t, np.diag(Ic))
        n_terms = (mesh.n_tet if dd is None else mesh.n_tri) * 4 + 16
        tol = n_terms * EPS * m * (np.linalg.norm(t) + np.linalg.norm(r)) ** 2
        assert abs(rec[12] - m) <= n_terms * EPS * m
        assert np.abs(rec[9:12] - m * t).max() <= n_terms * EPS * m * (np.linalg.norm(t) + np.linalg.norm(r))
        assert np.abs(rec[:9] - ref[:9]).max() <= tol, (np.abs(rec[:9] - ref[:9]).max(), tol)
        M = rec[:9].reshape(3, 3)
        assert np.array_equal(M, M.T)
