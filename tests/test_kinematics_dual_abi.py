"""pfc_kinematics_dual[_device], pfc_eval_dual_state_device[_more]: the C ABI, the scalar statement of the Dual kinematics kernels'
arithmetic (the second half of csrc/pfc_kin.h, stated in include/pfc.h) that tests/test_gpu_kinematics_dual.py compares bytes with,
an independent check of its partials, and the conventions pinned against RigidBodyDynamics' definitions -- without a device.

The statement, `kin_dual_scalar`, is kin_scalar's statements (tests/test_kinematics_abi.py, duplicated here over the number type) run on
a (value, partial) number with ForwardDiff's rules: sum and difference componentwise, unary minus on both parts, the product
{a.v b.v, a.d b.v + a.v b.d}, a literal or mechanism constant {x, 0.0}, the quotient {a.v / b.v, a.d (1 / b.v) + b.d (-(a.v / (b.v b.v)))}
and sin th = {sin th.v, cos th.v th.d}, cos th = {cos th.v, -(sin th.v th.d)}; no fma, nothing restated, no zero-seed shortcut.

The independent check is the same statement on the same number type over 50-digit mpmath values: the exact directional derivative
of the exact kinematics (its own rounding is 1e-50).  Both the statement and scenario.joint_kinematics_partials (NumPy: the matrix
form of the derivative, in the other association) are held to it.  The bound, `kin_dual_bound`, is carried level by level as
kin_bound is -- a rotation's error and its partial's as Frobenius norms, a vector's as 2-norms -- and applied elementwise; u = eps / 2,
gamma_k = k u / (1 - k u), products of two errors are O(eps^2) and lie in the slack of the rounded-up constants.  |dq|, |dv| <= 1
per coordinate.  The errors of the VALUES (eR, et of a pose, e_ang, e_lin of a motion vector) are kin_bound's, which bounds the sum of
both evaluations' errors and so either one's.

* Joint partials (`_joint_partial_err`, per side: statement, NumPy).
  Revolute.  cos, sin are within 1 ulp <= eps of exact, so s.d = cos th dth and c1.d = sin th dth (0 - c.d is exact) are within
  1.5 eps |dth|.  A diagonal entry (c1 a_r) a_r + c has the partial fl(fl(c1.d a_r) a_r) + c.d -- the products with the constants'
  zero partials add exact zeros -- within (1.5 + 1 + 1.5 + 0.5) eps |dth| = 4.5 eps |dth|, an off-diagonal one within
  (2.5 |a_r a_c| + 2 |a_k| + 0.75) eps |dth| < 4.5 eps |dth|: 13.5 eps |dth| in the Frobenius norm (statement).  NumPy forms
  dth (cos th K + sin th K K): K K is gamma_2 on terms below 1, then two scalings, one sum and the scaling by dth, below 5 eps |dth|
  an entry, 15 eps |dth|; and K K = a a' - |a|^2 I sees an axis that misses unit length in full, sin th | |a|^2 - 1 | |dth| on the
  diagonal.
  Prismatic.  dt_j = a ddq is one rounded product on either side: u |a| |ddq|.
  Floating, statement.  With S1 = 2 |p| |dp| >= |da2|: da2 is three doubled products summed, within 1.5 eps S1; den.d = da2 and
  (1 - a2).d = -da2 exactly; den has relative error 2 eps.  dw = -da2 (1 / den) + da2 (-((1 - a2) / den^2)): the first term is within
  (1.5 + 2.5 + 0.5) eps S1 / den, the second -- (1 - a2) / den^2 is within (1.5 a2 + 0.5 |1 - a2|) eps / den^2 + 5 eps |1 - a2| / den^2
  <= 7 eps / den -- within (7 + 1.5 + 0.5) eps S1 / den, their sum adds eps S1 / den: 14.5 eps S1 / den.  dx_i = 2 dp_i (1 / den) +
  da2 (-(2 p_i / den^2)): 3 eps 2 |dp_i| / den, (5 + 1.5 + 0.5) eps S1 2 |p_i| / den^2 with 2 |p_i| <= den, and 0.5 eps of the sum:
  (7 |dp_i| + 7.5 S1) eps / den.  So every one of dw, dx, dy, dz is within e1 = (7 |dp|_inf + 14.5 S1) eps / den and below
  m1 = (2 |dp|_inf + 2 S1) / den in magnitude; w, x, y, z are below 1 and within 4 eps (kin_bound's derivation).  An entry of R is four
  products of two of them, summed (and doubled, exactly): its partial is eight products, each within e1 + 4.5 eps m1, paired
  exactly or by one addition, then three additions on partial sums below 8 m1: 8 e1 + 48 eps m1 an entry, three times that in the
  Frobenius norm.  dt_j is copied.
  Floating, NumPy.  dR = dN / den^2 - (2 dp2 / den^3) N, N = 4 (1 - p2) P + 8 P P, dN = 4 (1 - p2) dP - 4 dp2 P + 8 (dP P + P dP).
  The longest chain of roundings from a product of inputs to an entry is 17 (dp2: 3; den^3: 6; the quotient: 1; N: 5; the product and
  the difference: 2), so an entry is within gamma_18 < 9.5 eps of its value times the sum of the magnitudes of its terms, 1 - p2
  entering with 1 + p2 = den (its absolute error is relative to that): Mag = (4 den |dP| + 4 |dp2| |P| + 8 (|dP| |P| + |P| |dP|)) /
  den^2 + 2 |dp2| (4 den |P| + 8 |P| |P|) / den^3.
* Composition (`G_D`).  dR_X = dR_P R_A + R_P dR_A, dt_X = dR_P t_A + R_P dt_A + dt_P with A = X_pj o X_j.  From a product to an
  entry the statement rounds at most 10 times over the two levels (Dual product and sum 2, dot product 2, translation 1, each level)
  and NumPy's (dH_P X_pj) X_j + (H_P X_pj) dX_j at most 9 (4-term rows twice, one sum): gamma_12 < 6.5 eps times the magnitude sum
  |dR_P| |R_pj| |R_j| + |R_P| |R_pj| |dR_j| (for t: |dR_P| (|R_pj| |t_j| + |t_pj|) + |R_P| |R_pj| |dt_j| + |dt_P|), which bounds the
  magnitude sums of both associations.  The operands' errors pass through to first order:
  e_dR_X = G_D |..|_F + e_dR_P |R_A|_2 + |dR_P|_2 eR_A + eR_P |dR_A|_2 + |R_P|_2 e_dR_A, and likewise for dt with e_dt_P added.
* Motion vectors (`G_MD`): o_ang = R m_ang, o_lin = R m_lin + t x o_ang, and their partials do_ang = dR m_ang + R dm_ang,
  do_lin = dR m_lin + R dm_lin + dt x o_ang + t x do_ang.  The statement rounds at most 9 times from a product to an entry (m = a qdot 1,
  Dual product 2, dot 2, cross product and sum 4), NumPy's dAd S v + dv (Ad S)' at most 19 (hat products 3, S 6, v 6, the transpose
  product's operand 3, the sum 1): gamma_20 < 10.5 eps times the magnitude sums, plus the operands' errors to first order
  (`_motion_partial_err`); the twist adds eps |dtw| per level for the sums.
Nothing in the bound is fitted to an observed difference.  Largest observed difference / bound over the states below: printed by
test_partials_agree_with_a_50_digit_evaluation and recorded in DESIGN section 4, "Dual kinematics from joint states"."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

import test_kinematics_abi as K
from test_kinematics_abi import EPS, FLOATING, NDOF, PRISMATIC, REVOLUTE, WORLD_X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = (("pfc_kinematics_dual_device", 11), ("pfc_kinematics_dual", 10), ("pfc_eval_dual_state_device", 34),
         ("pfc_eval_dual_state_device_more", 28))
G_D, G_MD = 6.5 * EPS, 10.5 * EPS


# ---- the (value, partial) number and the statement over the number type ---------------------------------------------------------
class D:
    """One partial of a ForwardDiff.Dual: value v and partial d (tests/test_dual_seeds_from_bodies_abi.py's D, duplicated, plus the
    quotient).  v and d are Python floats, or mpmath numbers for the exact evaluation: the rules are the same."""
    __slots__ = ("v", "d")

    def __init__(self, v, d):
        self.v, self.d = v, d

    def __add__(self, o): return D(self.v + o.v, self.d + o.d)
    def __sub__(self, o): return D(self.v - o.v, self.d - o.d)
    def __neg__(self): return D(-self.v, -self.d)
    def __mul__(self, o): return D(self.v * o.v, self.d * o.v + self.v * o.d)
    def __truediv__(self, o): return D(self.v / o.v, self.d * (1.0 / o.v) + o.d * (-(self.v / (o.v * o.v))))


class _Float:
    """The number type of the kernels: Float64, the trigonometry from `trig` ({theta: (cos, sin)}) or math."""
    def __init__(self, trig=None):
        self.trig = trig

    def num(self, x): return float(x)

    def cos_sin(self, th):
        return self.trig[th] if self.trig is not None else (math.cos(th), math.sin(th))


class _Exact:
    """50-digit mpmath numbers."""
    def __init__(self):
        import mpmath
        self.mp = mpmath
        mpmath.mp.dps = 50

    def num(self, x): return self.mp.mpf(float(x))

    def cos_sin(self, th): return self.mp.cos(th), self.mp.sin(th)


def _lit(N, x):
    return D(N.num(x), N.num(0.0))


def _sincos(N, th):
    cv, sv = N.cos_sin(th.v)
    return D(cv, -(sv * th.d)), D(sv, cv * th.d)      # c, s


def _compose(a, b):
    x = [None] * 12
    for c in range(3):
        for r in range(3):
            x[3 * c + r] = (a[r] * b[3 * c] + a[3 + r] * b[3 * c + 1]) + a[6 + r] * b[3 * c + 2]
    for r in range(3):
        x[9 + r] = ((a[r] * b[9] + a[3 + r] * b[10]) + a[6 + r] * b[11]) + a[9 + r]
    return x


def _to_world(x, m):
    o = [(x[r] * m[0] + x[3 + r] * m[1]) + x[6 + r] * m[2] for r in range(3)]
    o.append(((x[0] * m[3] + x[3] * m[4]) + x[6] * m[5]) + (x[10] * o[2] - x[11] * o[1]))
    o.append(((x[1] * m[3] + x[4] * m[4]) + x[7] * m[5]) + (x[11] * o[0] - x[9] * o[2]))
    o.append(((x[2] * m[3] + x[5] * m[4]) + x[8] * m[5]) + (x[9] * o[1] - x[10] * o[0]))
    return o


def _joint(N, t, a, q, v):
    zero, one, two = _lit(N, 0.0), _lit(N, 1.0), _lit(N, 2.0)
    xj, tj = [one if e in (0, 4, 8) else zero for e in range(12)], [zero] * 6
    if t == PRISMATIC:
        for r in range(3):
            xj[9 + r] = a[r] * q[0]; tj[3 + r] = a[r] * v[0]
    elif t == REVOLUTE:
        c, s = _sincos(N, q[0])
        c1 = one - c
        xj[0] = (c1 * a[0]) * a[0] + c; xj[4] = (c1 * a[1]) * a[1] + c; xj[8] = (c1 * a[2]) * a[2] + c
        xj[1] = (c1 * a[0]) * a[1] + s * a[2]; xj[3] = (c1 * a[0]) * a[1] - s * a[2]
        xj[2] = (c1 * a[0]) * a[2] - s * a[1]; xj[6] = (c1 * a[0]) * a[2] + s * a[1]
        xj[5] = (c1 * a[1]) * a[2] + s * a[0]; xj[7] = (c1 * a[1]) * a[2] - s * a[0]
        for r in range(3):
            tj[r] = a[r] * v[0]
    elif t == FLOATING:
        a2 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]
        den = a2 + one
        w, x, y, z = (one - a2) / den, (two * q[0]) / den, (two * q[1]) / den, (two * q[2]) / den
        xj[0] = ((w * w + x * x) - y * y) - z * z; xj[1] = two * (x * y + z * w); xj[2] = two * (x * z - y * w)
        xj[3] = two * (x * y - z * w); xj[4] = ((w * w - x * x) + y * y) - z * z; xj[5] = two * (y * z + x * w)
        xj[6] = two * (x * z + y * w); xj[7] = two * (y * z - x * w); xj[8] = ((w * w - x * x) - y * y) + z * z
        xj[9:12] = q[3:6]
        tj = list(v[0:6])
    return xj, tj


def _column(N, t, k, a, x):
    zero = _lit(N, 0.0)
    if t == FLOATING:
        c = k if k < 3 else k - 3
        d = [x[3 * c + r] for r in range(3)]
    else:
        d = [(x[r] * a[0] + x[3 + r] * a[1]) + x[6 + r] * a[2] for r in range(3)]
    if t == REVOLUTE or (t == FLOATING and k < 3):
        return d + [x[10] * d[2] - x[11] * d[1], x[11] * d[0] - x[9] * d[2], x[9] * d[1] - x[10] * d[0]]
    return [zero, zero, zero] + d


def kin_dual_scalar(mech, q, v, dq, dv, trig=None, N=None):
    """One scene and one seed direction on D numbers, expression for expression as include/pfc.h states pfc_kinematics_dual_device:
    kin_scalar's statements with every literal and mechanism constant lifted to {x, 0.0}.  q, v (nv,): values; dq, dv (nv,): their
    partials.  trig as kin_scalar.  Returns (x (n_body lists of 12 D), tw (n_body lists of 6 D), cols (nv lists of 6 D))."""
    N = N or _Float(trig)
    qd = [D(N.num(a), N.num(b)) for a, b in zip(q, dq)]
    vd = [D(N.num(a), N.num(b)) for a, b in zip(v, dv)]
    world, zero6 = [_lit(N, e) for e in WORLD_X], [_lit(N, 0.0)] * 6
    xs, tws, cols = [], [], [None] * mech["nv"]
    for b in range(mech["n_body"]):
        t, o, p = int(mech["joint_type"][b]), int(mech["off"][b]), int(mech["parent"][b])
        a = [_lit(N, e) for e in mech["axis"][b]]
        xj, tj = _joint(N, t, a, qd[o:o + 6], vd[o:o + 6])
        xa = _compose([_lit(N, e) for e in mech["x_p_j"][b]], xj)
        x = _compose(xs[p] if p >= 0 else world, xa)
        ow = _to_world(x, tj)
        twp = tws[p] if p >= 0 else zero6
        xs.append(x); tws.append([twp[e] + ow[e] for e in range(6)])
        for k in range(NDOF[t]):
            cols[o + k] = _column(N, t, k, a, x)
    return xs, tws, cols


def _partials_one(mech, q, v, dq, dv, trig=None, N=None, part="d"):
    """(x (n_body,12), tw (n_body,6), jac (n_body,nv,6)) of one scene and direction: the partial parts (or, part = "v", the values)
    of kin_dual_scalar, the Jacobian assembled over each body's ancestors (+0.0 elsewhere).  With the exact number type the arrays
    hold the mpmath numbers themselves, so that a difference with them is not rounded to Float64 first."""
    nb, nv = mech["n_body"], mech["nv"]
    xs, tws, cols = kin_dual_scalar(mech, q, v, dq, dv, trig, N)
    dt = object if isinstance(N, _Exact) else np.float64
    get = lambda row: np.array([getattr(e, part) for e in row], dtype=dt)
    jac = np.zeros((nb, nv, 6), dtype=dt)
    for b in range(nb):
        for a in K.ancestors(mech, b):
            for c in range(mech["off"][a], mech["off"][a + 1]):
                jac[b, c] = get(cols[c])
    return np.array([get(r) for r in xs]).reshape(nb, 12), np.array([get(r) for r in tws]).reshape(nb, 6), jac


def kin_dual_reference(mech, q, v, dq, dv, trig=None):
    """The three outputs of pfc_kinematics_dual by kin_dual_scalar, in the ABI's layouts: q (n_scene,nq), v (n_scene,nv), dq, dv
    (n_scene,n_dir,nv) or None (zeros; not both) -> d_x_w_b (n_scene,n_body,n_dir,12), d_twist_w_b (n_scene,n_body,n_dir,6), d_jac
    (n_scene n_body,n_dir,nv,6)."""
    q, v = np.atleast_2d(q), np.atleast_2d(v)
    ns, nb, nv = q.shape[0], mech["n_body"], mech["nv"]
    n_dir = np.shape(dq if dq is not None else dv)[-2]
    dq = np.zeros((ns, n_dir, nv)) if dq is None else np.asarray(dq, dtype=np.float64).reshape(ns, n_dir, nv)
    dv = np.zeros((ns, n_dir, nv)) if dv is None else np.asarray(dv, dtype=np.float64).reshape(ns, n_dir, nv)
    dx, dtw, djac = np.zeros((ns, nb, n_dir, 12)), np.zeros((ns, nb, n_dir, 6)), np.zeros((ns * nb, n_dir, nv, 6))
    for s in range(ns):
        for k in range(n_dir):
            x1, tw1, j1 = _partials_one(mech, q[s], v[s], dq[s, k], dv[s, k], trig)
            dx[s, :, k], dtw[s, :, k], djac[s * nb:(s + 1) * nb, k] = x1, tw1, j1
    return dx, dtw, djac


# ---- the rounding bound --------------------------------------------------------------------------------------------------------
_n2 = lambda M: float(np.linalg.norm(M, 2))
_nf = lambda M: float(np.linalg.norm(M))
_hat_abs = lambda a: np.abs(np.array([[0.0, a[2], a[1]], [a[2], 0.0, a[0]], [a[1], a[0], 0.0]]))


def _joint_partial_err(t, axis, q, dq, side):
    """(e_dR_j in the Frobenius norm, e_dt_j in the 2-norm) of one joint's partial: side 0 the statement, 1 NumPy."""
    if t == REVOLUTE:
        unit = abs(float(np.dot(axis, axis)) - 1.0)
        return ((13.5 * EPS, 15 * EPS + 3 * unit)[side] * abs(dq[0]), 0.0)
    if t == PRISMATIC:
        return 0.0, 0.5 * EPS * _nf(axis) * abs(dq[0])
    if t == FLOATING:
        p, dp = np.asarray(q[:3]), np.asarray(dq[:3])
        den = 1.0 + float(p @ p)
        S1 = 2.0 * _nf(p) * _nf(dp)
        if side == 0:
            e1 = (7 * np.abs(dp).max() + 14.5 * S1) * EPS / den
            m1 = (2 * np.abs(dp).max() + 2 * S1) / den
            return 3 * (8 * e1 + 48 * EPS * m1), 0.0
        P, dP = _hat_abs(p), _hat_abs(dp)
        mag = (4 * den * dP + 4 * S1 * P + 8 * (dP @ P + P @ dP)) / den ** 2 + 2 * S1 * (4 * den * P + 8 * (P @ P)) / den ** 3
        return 9.5 * EPS * _nf(mag), 0.0
    return 0.0, 0.0


def _motion_partial_err(R, t, dR, dt, eR, et, e_dR, e_dt, m, dm, e_ang):
    """(ang, lin) 2-norm bounds on the error of [dR m_a + R dm_a; dR m_l + R dm_l + dt x o_a + t x do_a]: pose (R, t) and its partial
    (dR, dt) carrying the errors (eR, et), (e_dR, e_dt); m, dm the motion vector of the body frame and its partial; e_ang the error
    of o_a = R m_a."""
    aR, adR, am, adm = np.abs(R), np.abs(dR), np.abs(m), np.abs(dm)
    M, dM = aR @ am[:3], adR @ am[:3] + aR @ adm[:3]
    e_dang = G_MD * _nf(dM) + e_dR * _nf(m[:3]) + eR * _nf(dm[:3])
    e_dlin = (G_MD * (_nf(adR @ am[3:] + aR @ adm[3:]) + _nf(K._acx(np.abs(dt), M)) + _nf(K._acx(np.abs(t), dM)))
              + e_dR * _nf(m[3:]) + eR * _nf(dm[3:]) + e_dt * _nf(M) + _nf(dt) * e_ang + et * _nf(dM) + _nf(t) * e_dang)
    return e_dang, e_dlin


def kin_dual_bound(mech, q, v, dq, dv, side):
    """Elementwise bound on |evaluation - exact partial| for one scene and direction: (dx (n_body,12), dtw (n_body,6), djac
    (n_body,nv,6)); side 0: kin_dual_scalar, side 1: scenario.joint_kinematics_partials.  The module docstring derives it."""
    nb, nv = mech["n_body"], mech["nv"]
    q, v, dq, dv = (np.asarray(a, dtype=np.float64) for a in (q, v, dq, dv))
    bx, btw, _ = K.kin_bound(mech, q, v)      # the values' errors (both evaluations' summed: an upper bound for either)
    xv, twv, _ = _partials_one(mech, q, v, dq, dv, part="v")
    xd, twd, _ = _partials_one(mech, q, v, dq, dv)
    ex, etw, ej = np.zeros((nb, 12)), np.zeros((nb, 6)), np.zeros((nb, nv, 6))
    Z = (0.0, 0.0)
    ed = [None] * nb      # (e_dR, e_dt) of the pose partial
    N = _Float()
    for b in range(nb):
        t, o, p = int(mech["joint_type"][b]), int(mech["off"][b]), int(mech["parent"][b])
        axis = np.asarray(mech["axis"][b], dtype=np.float64)
        qb, vb, dqb, dvb = (np.concatenate([a[o:o + NDOF[t]], np.zeros(6)])[:6] for a in (q, v, dq, dv))
        xj, tj = _joint(N, t, [_lit(N, e) for e in axis], [D(float(a), float(c)) for a, c in zip(qb, dqb)],
                        [D(float(a), float(c)) for a, c in zip(vb, dvb)])
        J, dJ = K._split([e.v for e in xj]), K._split([e.d for e in xj])
        Pj = K._split(mech["x_p_j"][b])
        if p >= 0:
            Pw, dPw, ePw, edPw = K._split(xv[p]), K._split(xd[p]), (bx[p, 0], bx[p, 9]), ed[p]
        else:
            Pw, dPw, ePw, edPw = K._split(WORLD_X), K._split(np.zeros(12)), Z, Z
        # values' errors of A = X_pj o X_j (this side's joint error), partial errors of the joint
        unit = abs(float(axis @ axis) - 1.0) if t == REVOLUTE else 0.0
        et_j = 0.5 * EPS * _nf(J[1]) if t == PRISMATIC else 0.0
        eA = K._compose_err(Pj, Z, J, (K.JOINT_ERR[t][side] + (6 * unit if side else 0.0), et_j))
        e_dRj, e_dtj = _joint_partial_err(t, axis, qb, dqb, side)
        A = (Pj[0] @ J[0], Pj[0] @ J[1] + Pj[1])
        dA = (Pj[0] @ dJ[0], Pj[0] @ dJ[1])
        e_dA = (_n2(Pj[0]) * e_dRj, _n2(Pj[0]) * e_dtj)      # (the rounding of this product is in G_D's count)
        aP, adP, aPj = np.abs(Pw[0]), np.abs(dPw[0]), np.abs(Pj[0])
        e_dR = (G_D * _nf(adP @ aPj @ np.abs(J[0]) + aP @ aPj @ np.abs(dJ[0])) + edPw[0] * _n2(A[0]) + _n2(dPw[0]) * eA[0]
                + ePw[0] * _n2(dA[0]) + _n2(Pw[0]) * e_dA[0])
        e_dt = (G_D * _nf(adP @ (aPj @ np.abs(J[1]) + np.abs(Pj[1])) + aP @ aPj @ np.abs(dJ[1]) + np.abs(dPw[1]))
                + edPw[0] * _nf(A[1]) + _n2(dPw[0]) * eA[1] + ePw[0] * _nf(dA[1]) + _n2(Pw[0]) * e_dA[1] + edPw[1])
        ed[b] = (e_dR, e_dt)
        ex[b, :9], ex[b, 9:] = e_dR, e_dt
        X, dX = K._split(xv[b]), K._split(xd[b])
        eR, et = bx[b, 0], bx[b, 9]
        m, dm = np.array([e.v for e in tj]), np.array([e.d for e in tj])
        e_ang, _ = K._motion_err(X[0], X[1], eR, et, m)
        e_dang, e_dlin = _motion_partial_err(X[0], X[1], dX[0], dX[1], eR, et, e_dR, e_dt, m, dm, e_ang)
        etw[b] = etw[p] if p >= 0 else 0.0
        etw[b, :3] += e_dang + EPS * _nf(twd[b, :3]); etw[b, 3:] += e_dlin + EPS * _nf(twd[b, 3:])
        if p >= 0:
            ej[b] = ej[p]
        for k in range(NDOF[t]):
            m = np.zeros(6)
            if t == FLOATING:
                m[k] = 1.0
            else:
                m[0 if t == REVOLUTE else 3:3 if t == REVOLUTE else 6] = axis
            e_ang, _ = K._motion_err(X[0], X[1], eR, et, m)
            ej[b, o + k, :3], ej[b, o + k, 3:] = _motion_partial_err(X[0], X[1], dX[0], dX[1], eR, et, e_dR, e_dt, m, np.zeros(6), e_ang)
    return ex, etw, ej


# ---- a. ABI --------------------------------------------------------------------------------------------------------------------
def test_dual_kinematics_symbols_are_declared_exported_and_bound(pfc):
    hdr = open(os.path.join(ROOT, "include", "pfc.h")).read()
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
    L = pfc._lib.lib()
    for name, _ in NAMES[:2]:
        a = getattr(L, name).argtypes
        assert a[1] is C.c_int and a[2] is C.c_int, name                                    # n_scene, n_dir
    for name, _ in NAMES[2:]:
        a = getattr(L, name).argtypes
        assert a[1] is C.c_int and a[2] is C.c_int and a[5] is C.c_int, name                # n_items, n_dir, n_scene
    M = pfc.scenario.MechanismScenario
    for meth in ("kinematics_dual", "kinematics_dual_device", "eval_dual_state_device", "eval_dual_state_device_more",
                 "force_all_elastic_intersections_dual_state"):
        assert callable(getattr(M, meth)), meth
    assert callable(pfc.scenario.joint_kinematics_partials)


def test_dual_kinematics_kernels_are_built_from_a_listed_header(pfc):
    csrc = os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc")
    srcs = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "_lib.py")).read()
    for kernel in ("k_kinematics_dual", "k_kin_jacobian_dual"):
        holders = [f for f in sorted(os.listdir(csrc)) if f.endswith(".h")
                   and re.search(r"__global__ void (__launch_bounds__\(\w+\) )?" + kernel + r"\(", open(os.path.join(csrc, f)).read())]
        assert holders == ["pfc_kin.h"], (kernel, holders)
    assert '"pfc_kin.h"' in srcs      # a change of the kernels rebuilds the library
    assert '#include "pfc_kin.h"' in open(os.path.join(csrc, "pfc_hip.hip")).read()
    # one definition of the (value, partial) type, of its product rule and of its quotient
    text = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip")))
    assert len(re.findall(r"struct ScatDual\s*\{", text)) == 1
    assert len(re.findall(r"operator\*\(ScatDual", text)) == 1 and len(re.findall(r"operator/\(ScatDual", text)) == 1


# ---- b. the scalar statement ---------------------------------------------------------------------------------------------------
def _seeds(mech, rng, n_dir):
    return rng.uniform(-1, 1, (n_dir, mech["nv"])), rng.uniform(-1, 1, (n_dir, mech["nv"]))


def test_value_parts_are_the_bytes_of_kin_scalar():
    rng = np.random.default_rng(20261101)
    for k in range(40):
        mech = (K.mech_a(), K.mech_b(), K.mech_c(), K.mech_a(seed=6))[k % 4]
        q, v = K.random_state(mech, rng, k // 4)
        dq, dv = _seeds(mech, rng, 1)
        trig = None
        if k % 2:      # a table of other values, as the device's are fed: the statement takes them as kin_scalar does
            trig = {float(q[mech["off"][b]]): (0.25 + 0.01 * b, -0.5) for b, t in enumerate(mech["joint_type"]) if t == REVOLUTE}
        xs, tws, cols = kin_dual_scalar(mech, q, v, dq[0], dv[0], trig)
        xr, twr, cr = K.kin_scalar(mech, q, v, trig)
        val = lambda rows: np.array([[e.v for e in r] for r in rows]).tobytes()
        assert val(xs) == np.array(xr).tobytes() and val(tws) == np.array(twr).tobytes() and val(cols) == np.array(cr).tobytes(), k


# ---- c. the partials against a 50-digit evaluation -----------------------------------------------------------------------------
def _numpy_partials(pfc, mech, q, v, dq, dv):
    return pfc.scenario.joint_kinematics_partials(mech["parent"], mech["joint_type"], mech["x_p_j"], mech["axis"], q, v, dq, dv)


def test_partials_agree_with_a_50_digit_evaluation(pfc):
    rng = np.random.default_rng(20261102)
    exact = _Exact()
    n_dir = 2
    worst, largest, n_lt, n_gt = [0.0, 0.0], 0.0, 0, 0
    for k in range(24):
        mech = (K.mech_a(), K.mech_c(), K.mech_a(seed=6))[k % 3]
        q, v = K.random_state(mech, rng, k // 3)
        for b, t in enumerate(mech["joint_type"]):
            if t == FLOATING:
                p = np.linalg.norm(q[mech["off"][b]:mech["off"][b] + 3])
                n_lt += p < 1; n_gt += 1 < p < 3
        dq, dv = _seeds(mech, rng, n_dir)
        npx, nptw, npj = _numpy_partials(pfc, mech, q, v, dq, dv)
        for d in range(n_dir):
            ref = _partials_one(mech, q, v, dq[d], dv[d], N=exact)
            sides = (_partials_one(mech, q, v, dq[d], dv[d]), (npx[:, d], nptw[:, d], npj[:, d]))
            for side, got in enumerate(sides):
                bnd = kin_dual_bound(mech, q, v, dq[d], dv[d], side)
                for name, g, r, bd in zip(("dx", "dtw", "djac"), got, ref, bnd):
                    diff = np.abs(g - r).astype(np.float64)      # the difference is formed in 50 digits
                    assert (diff <= bd).all(), (k, d, side, name, np.argwhere(diff > bd)[:4], diff.max(), bd.max())
                    worst[side] = max(worst[side], float((diff / np.maximum(bd, 1e-300)).max()))
                    largest = max(largest, float(bd.max()))
                assert all(np.abs(r.astype(np.float64)).max() > 0 for r in ref)
    print(f"largest difference / bound over 24 states x {n_dir} directions: statement {worst[0]:.3f}, joint_kinematics_partials "
          f"{worst[1]:.3f}; largest bound {largest:.2e}; MRP |p| < 1: {n_lt}, in (1, 3): {n_gt}")
    assert n_lt >= 4 and n_gt >= 4
    assert largest < 1e-11      # a rounding bound, not a loose one


# ---- d. conventions, on the statement ------------------------------------------------------------------------------------------
def test_twist_partial_along_a_velocity_is_the_jacobian_column():
    """The twist is linear in v: with dq = 0, dv = e_c its partial is column c of the body's Jacobian, exactly -- every other term of
    the Dual statement is a product with an exact zero (np.array_equal: up to the sign of zeros)."""
    mech = K.mech_a()
    rng = np.random.default_rng(41)
    for k in range(2):
        q, v = K.random_state(mech, rng, k)
        _, _, jac = K.kin_reference(mech, q, v)
        for c in range(mech["nv"]):
            dv = np.zeros(mech["nv"]); dv[c] = 1.0
            _, dtw, _ = _partials_one(mech, q, v, np.zeros(mech["nv"]), dv)
            for b in range(mech["n_body"]):
                assert np.array_equal(dtw[b], jac[b, c]), (k, b, c, dtw[b], jac[b, c])
        assert np.abs(jac).max() > 0


def _state_rate_err(mech, q, v):
    """Bound on the rounding of K.state_rate, per coordinate.  mrp_rate: 0.25 ((1 - p'p) I + 2 P + 2 p p') omega rounds at most 10
    times from a product to an entry (p'p 3, the difference 1, 2 p p' 1, the sums 2, the matrix-vector product 3): gamma_10 < 5.5 eps
    times 0.25 ((1 + p'p) I + 2 |P| + 2 |p| |p|') |omega|.  R_j v: an entry of R_j is within 11 eps (kin_bound's derivation), the
    product adds gamma_3 = 1.5 eps: 12.5 eps sum |v_k|.  Revolute and prismatic rates are copied."""
    e = np.zeros(mech["nv"])
    for b, t in enumerate(mech["joint_type"]):
        if t == FLOATING:
            o = mech["off"][b]
            p, w = q[o:o + 3], v[o:o + 3]
            e[o:o + 3] = 5.5 * EPS * 0.25 * (((1.0 + p @ p) * np.eye(3) + 2.0 * _hat_abs(p) + 2.0 * np.outer(np.abs(p), np.abs(p))) @ np.abs(w))
            e[o + 3:o + 6] = 12.5 * EPS * np.abs(v[o + 3:o + 6]).sum()
    return e


def test_pose_partial_along_the_motion_is_the_pose_velocity(pfc):
    """With dq = state_rate(q, v), dv = 0 the pose's partial is its time derivative as the value twist implies it (RigidBodyDynamics'
    twist_wrt_world): dR = hat(ang) R, dt = lin + ang x t.  Bound: kin_dual_bound for the partial; the rounding of state_rate passed
    through the partial's linear dependence on dq, sum_i |dx / dq_i| e_i (the columns from joint_kinematics_partials with dq = I,
    their own error being of second order); and the product: hat(ang) R is gamma_2 = eps on |hat(ang)| |R| (one entry of a row of
    hat is zero), lin + ang x t gamma_3 = 1.5 eps on |lin| + |hat(ang)| |t|, with the values' errors (kin_bound's, entrywise below
    their norms) to first order: |hat(e_ang)| |R| + |hat(ang)| eR and e_lin + |hat(e_ang)| |t| + |hat(ang)| et."""
    rng = np.random.default_rng(43)
    worst = 0.0
    for k in range(12):
        mech = (K.mech_a(), K.mech_c(), K.mech_b())[k % 3]
        nv = mech["nv"]
        q, v = K.random_state(mech, rng, k // 3)
        qd = K.state_rate(mech, q, v)
        dx, _, _ = _partials_one(mech, q, v, qd, np.zeros(nv))
        ex, _, _ = kin_dual_bound(mech, q, v, qd, np.zeros(nv), 0)
        cols, _, _ = _numpy_partials(pfc, mech, q, v, np.eye(nv), None)      # (n_body, nv, 12)
        e_rate = np.einsum("bic,i->bc", np.abs(cols), _state_rate_err(mech, q, v))
        xs, tws, _ = K.kin_scalar(mech, q, v)
        bx, btw, _ = K.kin_bound(mech, q, v)
        for b in range(mech["n_body"]):
            R, t = K._split(xs[b])
            ang, lin = np.asarray(tws[b][:3]), np.asarray(tws[b][3:])
            dR, dt = pfc.scenario._hat(ang) @ R, lin + np.cross(ang, t)
            e_ang, e_lin = np.full(3, btw[b, 0]), np.full(3, btw[b, 3])
            bR = EPS * (_hat_abs(ang) @ np.abs(R)) + _hat_abs(e_ang) @ np.abs(R) + _hat_abs(ang) @ np.full((3, 3), bx[b, 0])
            bt = 1.5 * EPS * (np.abs(lin) + _hat_abs(ang) @ np.abs(t)) + e_lin + _hat_abs(e_ang) @ np.abs(t) + _hat_abs(ang) @ np.full(3, bx[b, 9])
            bound = ex[b] + e_rate[b] + np.concatenate([bR.reshape(-1, order="F"), bt])
            diff = np.abs(dx[b] - np.concatenate([dR.reshape(-1, order="F"), dt]))
            assert (diff <= bound).all(), (k, b, diff, bound)
            worst = max(worst, float((diff / np.maximum(bound, 1e-300)).max()))
            assert bound.max() < 1e-11
        assert np.abs(dx).max() > 0
    print(f"pose partial along the motion against the pose velocity: largest difference / bound {worst:.3f}")


def test_partial_jacobian_columns_of_non_ancestors_are_positive_zero():
    mech = K.mech_a()
    rng = np.random.default_rng(44)
    q, v = K.random_state(mech, rng)
    dq, dv = _seeds(mech, rng, 1)
    _, _, djac = kin_dual_reference(mech, q, v, dq[None], dv[None])
    own = {0: range(0, 6), 1: range(0, 7), 2: range(0, 8), 3: range(0, 8), 4: list(range(0, 6)) + [8], 5: [9]}
    for b in range(6):
        for c in range(10):
            if c not in own[b]:
                assert djac[b, 0, c].tobytes() == np.zeros(6).tobytes()      # +0.0, not -0.0
    assert all(np.abs(djac[b, 0, c]).max() > 0 for b in (1, 2, 3) for c in range(6))


# ---- e. the layout function ----------------------------------------------------------------------------------------------------
def test_reference_layout_and_null_seeds():
    mech = K.mech_a()
    rng = np.random.default_rng(45)
    n_scene, n_dir, nb, nv = 2, 3, mech["n_body"], mech["nv"]
    qs, vs = zip(*(K.random_state(mech, rng, k) for k in range(n_scene)))
    q, v = np.array(qs), np.array(vs)
    dq, dv = rng.uniform(-1, 1, (n_scene, n_dir, nv)), rng.uniform(-1, 1, (n_scene, n_dir, nv))
    dx, dtw, djac = kin_dual_reference(mech, q, v, dq, dv)
    assert dx.shape == (n_scene, nb, n_dir, 12) and dtw.shape == (n_scene, nb, n_dir, 6) and djac.shape == (n_scene * nb, n_dir, nv, 6)
    x1, tw1, j1 = _partials_one(mech, q[1], v[1], dq[1, 2], dv[1, 2])
    assert np.array_equal(dx[1, :, 2], x1) and np.array_equal(dtw[1, :, 2], tw1) and np.array_equal(djac[nb:, 2], j1)
    for a, b in ((dq, None), (None, dv)):
        got = kin_dual_reference(mech, q, v, a, b)
        ref = kin_dual_reference(mech, q, v, a if a is not None else np.zeros_like(dq), b if b is not None else np.zeros_like(dv))
        assert all(g.tobytes() == r.tobytes() for g, r in zip(got, ref))
        assert np.abs(got[0]).max() > 0 or a is None
    assert not kin_dual_reference(mech, q, v, None, dv)[0].any()      # the poses do not depend on v
