"""pfc_set_mechanism, pfc_mechanism_sizes, pfc_kinematics[_device], pfc_eval_state[_device]: the C ABI, the scalar statement of the
kernels' arithmetic (csrc/pfc_kin.h, stated in include/pfc.h) that tests/test_gpu_kinematics.py compares bytes with, and the
conventions of "twist" and "Jacobian" pinned against RigidBodyDynamics' definitions -- without a device.

The statement is checked here against scenario.joint_kinematics (NumPy: 4x4 homogeneous products in the other association,
(H_parent X_pj) X_j, 6x6 adjoints, Rodrigues' formula).  Bound, carried level by level (`kin_bound`) and applied elementwise; the
error of a rotation is carried as a Frobenius norm and that of a vector as a 2-norm, because a product with a rotation leaves these
as they are, where an entrywise bound would grow by up to sqrt(3) at each of the eight products of a depth-4 chain.  u = eps / 2.

* A dot product of 3 products is within gamma_3 = 1.5 eps (G_R) of the exact sum times sum |a_k| |b_k|, with the translation added
  gamma_4 = 2 eps (G_T), whatever the order and whether or not BLAS contracts a product into an fma (NumPy's fourth product of a 4x4
  row is with an exact 0 or 1).
* The joint rotation (JOINT_ERR: statement, NumPy).  MRP, statement: a2 has relative error gamma_3 and den = a2 + 1 below 2 eps, so
  x, y, z = (2 p) / den -- one division each, 2 p exact -- below 2.5 eps; 1 - a2 has absolute error below 1.5 eps a2 +
  0.5 eps |1 - a2|, so w = (1 - a2) / den -- the second division -- below 1.5 eps + 2.5 eps |w| <= 4 eps.  A diagonal entry
  ((ww + xx) - yy) - zz then errs by at most 8 eps |w| + 5.5 eps (1 - w^2) + 2 eps < 11 eps and so does an off-diagonal one
  (|xy| + |zw| <= 1/2, doubled): 11 eps an entry, 33 eps in the Frobenius norm.  NumPy: I + (4 (1 - p2) P + 8 P P) / (1 + p2)^2;
  (1 + p2)^2 has relative error below 4.5 eps, 8 P P below 1 eps, 4 (1 - p2) P an absolute error below 6 eps |p| (1 + p2), the terms
  are below 2 and 1.3 for every p: 12.5 eps an entry, 38 eps.  Revolute: c and s are within 1 ulp on either side (math / NumPy
  libm), c1 = 1 - c <= 2, then three roundings on terms below 2 (statement: 6 eps an entry, 18 eps) or K K, two scalings and two
  additions (NumPy: 8 eps, 24 eps); an axis may miss unit length by 1e-12 in |a|^2, which NumPy's K K = a a' - |a|^2 I sees in full
  on the diagonal, c1 | |a|^2 - 1 | <= 2 | |a|^2 - 1 | an entry (6 in the norm).  Prismatic: t_j = a d is one rounded product on
  either side, u |a d|.  Floating: t_j is copied.
* Composition: the statement forms A = X_pj o X_j and then X = X_parent o A, NumPy (X_parent X_pj) X_j.  Each side's error against
  the exact product is carried with its own operands: for X = P o A with errors (eR, et) on the operands,
  eR_X = G_R | |R_P| |R_A| |_F + eR_P |R_A|_2 + |R_P|_2 eR_A and et_X = G_T | |R_P| |t_A| + |t_P| |_2 + eR_P |t_A|_2 +
  |R_P|_2 et_A + et_P; the bound on the difference is the sum of the two sides' errors, each entry being below the norm.
* Twist and Jacobian columns are [R m_ang; R m_lin + t x (R m_ang)] of a motion vector m of the body frame (joint twist; unit
  vector or axis).  The statement spends gamma_3 on R m and gamma_4 on the cross product and the sum; NumPy nests hat(t) R
  (gamma_2), S (gamma_3) and v (gamma_6): together below 8 eps (G_M) times the magnitudes.  With M = |R| |m_ang|:
  e_ang = G_M |M| + bR |m_ang| + eps |m_ang| (m = a qdot is itself one product) and e_lin = G_M (| |R| |m_lin| | + | |t| x M |) +
  bR |m_lin| + eps |m_lin| + bt |M| + |t| e_ang, `x` on magnitudes being the cross product with every sign positive; the twist
  adds eps |tw| per level for the sums.
For translations of length <= 10, |theta| <= 2 pi, |p| < 3, |v| <= 1 and the depth-4 mechanism below the bound stays under 1e-12
(asserted): it is a rounding bound, not a loose one."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = (("pfc_set_mechanism", 6), ("pfc_mechanism_sizes", 4), ("pfc_kinematics_device", 8), ("pfc_kinematics", 7),
         ("pfc_eval_state_device", 21), ("pfc_eval_state", 20))
EPS = float(np.finfo(np.float64).eps)
FIXED, REVOLUTE, PRISMATIC, FLOATING = 0, 1, 2, 3
NDOF = {FIXED: 0, REVOLUTE: 1, PRISMATIC: 1, FLOATING: 6}
WORLD_X = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


# ---- the test mechanisms -----------------------------------------------------------------------------------------------------
def make_mech(parent, joint_type, x_p_j, axis):
    parent = np.asarray(parent, dtype=np.int32); joint_type = np.asarray(joint_type, dtype=np.int32)
    n = parent.size
    off = np.concatenate([[0], np.cumsum([NDOF[int(t)] for t in joint_type])]).astype(int)
    return dict(parent=parent, joint_type=joint_type, x_p_j=np.asarray(x_p_j, dtype=np.float64).reshape(n, 12),
                axis=np.asarray(axis, dtype=np.float64).reshape(n, 3), off=off, n_body=n, nv=int(off[-1]))


def _random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def _unit(rng):
    a = rng.standard_normal(3)
    return a / np.linalg.norm(a)


def mech_a(seed=5):
    """(A) b0 floating on the world, b1 revolute on b0, b2 prismatic on b1, b3 fixed on b2, b4 revolute on b0 (a branch), b5 prismatic
    on the world: every joint type, depth 4, a branch and two roots; nq = nv = 10."""
    rng = np.random.default_rng(seed)
    x = [np.concatenate([_random_rotation(rng).reshape(-1, order="F"), rng.uniform(-1, 1, 3)]) for _ in range(6)]
    return make_mech([-1, 0, 1, 2, 0, -1], [FLOATING, REVOLUTE, PRISMATIC, FIXED, REVOLUTE, PRISMATIC], x, [_unit(rng) for _ in range(6)])


def mech_b(rot=None):
    """(B) C1's five bodies: the plane fixed on the world and four floating boxes, nv = 24.  rot (5,9): the rotations of the
    joint_poses, column-major (default: box b turned by 0.1 b about z, as configs.c1_boxes() turns it)."""
    x = np.zeros((5, 12))
    for b in range(5):
        c, s = math.cos(0.1 * b), math.sin(0.1 * b)
        x[b, :9] = [c, s, 0.0, -s, c, 0.0, 0.0, 0.0, 1.0] if rot is None else rot[b]
    return make_mech([-1] * 5, [FIXED] + [FLOATING] * 4, x, np.zeros((5, 3)))


def mech_c():
    """(C) the pencil's chain: prismatic z on the world, revolute y on it, two prismatic fingers on that."""
    x = np.tile(np.array(WORLD_X), (4, 1))
    x[1, 9:] = [0.0, 0.0, 0.1]; x[2, 9:] = [0.02, 0.0, 0.05]; x[3, 9:] = [-0.02, 0.0, 0.05]
    return make_mech([-1, 0, 1, 1], [PRISMATIC, REVOLUTE, PRISMATIC, PRISMATIC], x, [[0, 0, 1], [0, 1, 0], [1, 0, 0], [-1, 0, 0]])


def random_state(mech, rng, k=0):
    """Translations of length <= 10 (|d| <= 10 for a prismatic joint), |theta| <= 2 pi, |v| <= 1; MRP vectors with |p| < 1 (k even) or |p| in (1, 3) (k odd)."""
    q, v = np.zeros(mech["nv"]), rng.uniform(-1, 1, mech["nv"])
    for b, t in enumerate(mech["joint_type"]):
        o = mech["off"][b]
        if t == REVOLUTE:
            q[o] = rng.uniform(-2 * math.pi, 2 * math.pi)
        elif t == PRISMATIC:
            q[o] = rng.uniform(-10, 10)
        elif t == FLOATING:
            q[o:o + 3] = _unit(rng) * (rng.uniform(0, 1) if k % 2 == 0 else rng.uniform(1, 3))
            q[o + 3:o + 6] = _unit(rng) * rng.uniform(0, 10)
    return q, v


# ---- the scalar statement ------------------------------------------------------------------------------------------------------
def _compose(a, b):
    x = [0.0] * 12
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


def _joint(t, a, q, v, trig):
    xj, tj = list(WORLD_X), [0.0] * 6
    if t == PRISMATIC:
        for r in range(3):
            xj[9 + r] = a[r] * q[0]; tj[3 + r] = a[r] * v[0]
    elif t == REVOLUTE:
        c, s = trig[q[0]] if trig is not None else (math.cos(q[0]), math.sin(q[0]))
        c1 = 1.0 - c
        xj[0] = (c1 * a[0]) * a[0] + c; xj[4] = (c1 * a[1]) * a[1] + c; xj[8] = (c1 * a[2]) * a[2] + c
        xj[1] = (c1 * a[0]) * a[1] + s * a[2]; xj[3] = (c1 * a[0]) * a[1] - s * a[2]
        xj[2] = (c1 * a[0]) * a[2] - s * a[1]; xj[6] = (c1 * a[0]) * a[2] + s * a[1]
        xj[5] = (c1 * a[1]) * a[2] + s * a[0]; xj[7] = (c1 * a[1]) * a[2] - s * a[0]
        for r in range(3):
            tj[r] = a[r] * v[0]
    elif t == FLOATING:
        a2 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]
        den = a2 + 1.0
        w, x, y, z = (1.0 - a2) / den, (2.0 * q[0]) / den, (2.0 * q[1]) / den, (2.0 * q[2]) / den
        xj[0] = ((w * w + x * x) - y * y) - z * z; xj[1] = 2.0 * (x * y + z * w); xj[2] = 2.0 * (x * z - y * w)
        xj[3] = 2.0 * (x * y - z * w); xj[4] = ((w * w - x * x) + y * y) - z * z; xj[5] = 2.0 * (y * z + x * w)
        xj[6] = 2.0 * (x * z + y * w); xj[7] = 2.0 * (y * z - x * w); xj[8] = ((w * w - x * x) - y * y) + z * z
        xj[9:12] = q[3:6]
        tj = list(v[0:6])
    return xj, tj


def _column(t, k, a, x):
    if t == FLOATING:
        c = k if k < 3 else k - 3
        d = [x[3 * c + r] for r in range(3)]
    else:
        d = [(x[r] * a[0] + x[3 + r] * a[1]) + x[6 + r] * a[2] for r in range(3)]
    if t == REVOLUTE or (t == FLOATING and k < 3):
        return d + [x[10] * d[2] - x[11] * d[1], x[11] * d[0] - x[9] * d[2], x[9] * d[1] - x[10] * d[0]]
    return [0.0, 0.0, 0.0] + d


def kin_scalar(mech, q, v, trig=None):
    """One scene in Python floats, expression for expression as include/pfc.h states pfc_kinematics_device: every dot product summed
    left to right, no fma, the world going through the same expressions.  A body's pose and twist come from its parent's stored
    result.  trig: {theta: (cos theta, sin theta)} for the revolute joints' angles, else math's.  Returns (x (n_body lists of 12),
    tw (n_body lists of 6), cols (nv lists of 6))."""
    q, v = [float(e) for e in q], [float(e) for e in v]
    xs, tws, cols = [], [], [None] * mech["nv"]
    for b in range(mech["n_body"]):
        t, o, p = int(mech["joint_type"][b]), int(mech["off"][b]), int(mech["parent"][b])
        a = [float(e) for e in mech["axis"][b]]
        xj, tj = _joint(t, a, q[o:o + 6], v[o:o + 6], trig)
        xa = _compose([float(e) for e in mech["x_p_j"][b]], xj)
        x = _compose(xs[p] if p >= 0 else list(WORLD_X), xa)
        ow = _to_world(x, tj)
        twp = tws[p] if p >= 0 else [0.0] * 6
        xs.append(x); tws.append([twp[e] + ow[e] for e in range(6)])
        for k in range(NDOF[t]):
            cols[o + k] = _column(t, k, a, x)
    return xs, tws, cols


def ancestors(mech, b):
    out = []
    while b >= 0:
        out.append(b); b = int(mech["parent"][b])
    return out


def kin_reference(mech, q, v, trig=None):
    """The three outputs of pfc_kinematics by kin_scalar: q (n_scene,nq), v (n_scene,nv) -> x_w_b (n_scene,n_body,12), twist_w_b
    (n_scene,n_body,6), jac (n_scene n_body,nv,6)."""
    q, v = np.atleast_2d(q), np.atleast_2d(v)
    ns, nb, nv = q.shape[0], mech["n_body"], mech["nv"]
    x, tw, jac = np.zeros((ns, nb, 12)), np.zeros((ns, nb, 6)), np.zeros((ns * nb, nv, 6))
    for s in range(ns):
        xs, tws, cols = kin_scalar(mech, q[s], v[s], trig)
        x[s], tw[s] = xs, tws
        for b in range(nb):
            for a in ancestors(mech, b):
                for c in range(mech["off"][a], mech["off"][a + 1]):
                    jac[s * nb + b, c] = cols[c]
    return x, tw, jac


# ---- the rounding bound --------------------------------------------------------------------------------------------------------
def _acx(a, b):
    return np.array([a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]])


def _split(x):
    x = np.asarray(x, dtype=np.float64)
    return x[:9].reshape(3, 3, order="F"), x[9:]


def _compose_err(P, eP, A, eA):
    """Error (Frobenius norm of the rotation's, 2-norm of the translation's) of the computed P o A against the exact product of the
    exact operands, the computed operands P, A = (R, t) carrying the errors eP, eA."""
    n2 = lambda M: float(np.linalg.norm(M, 2))
    eR = G_R * float(np.linalg.norm(np.abs(P[0]) @ np.abs(A[0]))) + eP[0] * n2(A[0]) + n2(P[0]) * eA[0]
    et = G_T * float(np.linalg.norm(np.abs(P[0]) @ np.abs(A[1]) + np.abs(P[1]))) + eP[0] * float(np.linalg.norm(A[1])) + n2(P[0]) * eA[1] + eP[1]
    return eR, et


def _motion_err(R, t, bR, bt, m):
    """(ang, lin) 2-norm bounds on [R m_ang; R m_lin + t x (R m_ang)] between the two evaluations: pose (R, t) with bounds bR, bt."""
    nrm = lambda a: float(np.linalg.norm(a))
    M = np.abs(R) @ np.abs(m[:3])
    e_ang = G_M * nrm(M) + bR * nrm(m[:3]) + EPS * nrm(m[:3])
    e_lin = (G_M * (nrm(np.abs(R) @ np.abs(m[3:])) + nrm(_acx(np.abs(t), M))) + bR * nrm(m[3:]) + EPS * nrm(m[3:]) + bt * nrm(M)
             + nrm(t) * e_ang)
    return e_ang, e_lin


G_R, G_T, G_M = 1.5 * EPS, 2 * EPS, 8 * EPS      # gamma_3, gamma_4, and both sides' nested products of the motion vectors
JOINT_ERR = {FLOATING: (33 * EPS, 38 * EPS), REVOLUTE: (18 * EPS, 24 * EPS), PRISMATIC: (0.0, 0.0), FIXED: (0.0, 0.0)}


def kin_bound(mech, q, v):
    """Elementwise bound on |kin_scalar - joint_kinematics| for one scene: (x (n_body,12), tw (n_body,6), jac (n_body,nv,6)); the
    module docstring derives it."""
    nb, nv = mech["n_body"], mech["nv"]
    q, v = np.asarray(q, dtype=np.float64), np.asarray(v, dtype=np.float64)
    bx, btw, bj = np.zeros((nb, 12)), np.zeros((nb, 6)), np.zeros((nb, nv, 6))
    W, Z = _split(WORLD_X), (0.0, 0.0)
    es, en = [None] * nb, [None] * nb      # (eR, et) of x_w_b: the statement's, NumPy's
    xs, tws, cols = kin_scalar(mech, q, v)
    for b in range(nb):
        t, o, p = int(mech["joint_type"][b]), int(mech["off"][b]), int(mech["parent"][b])
        axis = [float(e) for e in mech["axis"][b]]
        xj, tj = _joint(t, axis, [float(e) for e in q[o:o + 6]], [float(e) for e in v[o:o + 6]], None)
        J, Pj, X = _split(xj), _split(mech["x_p_j"][b]), _split(xs[b])
        et_j = 0.5 * EPS * float(np.linalg.norm(J[1])) if t == PRISMATIC else 0.0
        unit = abs(float(mech["axis"][b] @ mech["axis"][b]) - 1.0) if t == REVOLUTE else 0.0
        eJs, eJn = (JOINT_ERR[t][0], et_j), (JOINT_ERR[t][1] + 6 * unit, et_j)
        Pw, ePs, ePn = (_split(xs[p]), es[p], en[p]) if p >= 0 else (W, Z, Z)
        # statement: A = X_pj o X_j, X = X_parent o A
        A = _split(_compose([float(e) for e in mech["x_p_j"][b]], xj))
        es[b] = _compose_err(Pw, ePs, A, _compose_err(Pj, Z, J, eJs))
        # NumPy: B = X_parent X_pj, X = B X_j
        B = _split(_compose(xs[p] if p >= 0 else list(WORLD_X), [float(e) for e in mech["x_p_j"][b]]))
        en[b] = _compose_err(B, _compose_err(Pw, ePn, Pj, Z), J, eJn)
        bR, bt = es[b][0] + en[b][0], es[b][1] + en[b][1]
        bx[b, :9], bx[b, 9:] = bR, bt
        e_ang, e_lin = _motion_err(X[0], X[1], bR, bt, np.asarray(tj))
        tw = np.asarray(tws[b])
        btw[b] = btw[p] if p >= 0 else 0.0
        btw[b, :3] += e_ang + EPS * float(np.linalg.norm(tw[:3])); btw[b, 3:] += e_lin + EPS * float(np.linalg.norm(tw[3:]))
        if p >= 0:
            bj[b] = bj[p]
        for k in range(NDOF[t]):
            m = np.zeros(6)
            if t == FLOATING:
                m[k] = 1.0
            else:
                m[0 if t == REVOLUTE else 3:3 if t == REVOLUTE else 6] = axis
            bj[b, o + k, :3], bj[b, o + k, 3:] = _motion_err(X[0], X[1], bR, bt, m)
    return bx, btw, bj


# ---- 1. ABI --------------------------------------------------------------------------------------------------------------------
def test_kinematics_symbols_are_declared_exported_and_bound(pfc):
    hdr = open(os.path.join(ROOT, "include", "pfc.h")).read()
    for k, name in enumerate(("PFC_JOINT_FIXED", "PFC_JOINT_REVOLUTE", "PFC_JOINT_PRISMATIC", "PFC_JOINT_FLOATING_MRP")):
        assert re.search(r"\b" + name + r"\s*=?\s*" + str(k) + r"\b", hdr), name
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
    L = pfc._lib
    assert (L.JOINT_FIXED, L.JOINT_REVOLUTE, L.JOINT_PRISMATIC, L.JOINT_FLOATING_MRP) == (FIXED, REVOLUTE, PRISMATIC, FLOATING)
    M = pfc.scenario.MechanismScenario
    for meth in ("set_mechanism", "mechanism_sizes", "kinematics", "kinematics_device", "force_all_elastic_intersections_state",
                 "eval_state_device"):
        assert callable(getattr(M, meth)), meth
    assert callable(pfc.scenario.joint_kinematics)


def test_kinematics_kernels_are_built_from_their_header(pfc):
    srcs = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "_lib.py")).read()
    assert '"pfc_kin.h"' in srcs      # a change of the kernels rebuilds the library
    src = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc", "pfc_hip.hip")).read()
    assert '#include "pfc_kin.h"' in src


# ---- 3. the statement against scenario.joint_kinematics ------------------------------------------------------------------------
def _numpy_kinematics(pfc, mech, q, v):
    return pfc.scenario.joint_kinematics(mech["parent"], mech["joint_type"], mech["x_p_j"], mech["axis"], q, v)


def test_scalar_statement_agrees_with_joint_kinematics(pfc):
    rng = np.random.default_rng(20260214)
    worst, largest, n_lt, n_gt = 0.0, 0.0, 0, 0
    for k in range(200):
        mech = (mech_a(), mech_b(), mech_c(), mech_a(seed=6))[k % 4]
        q, v = random_state(mech, rng, k // 4)
        for b, t in enumerate(mech["joint_type"]):
            if t == FLOATING:
                p = np.linalg.norm(q[mech["off"][b]:mech["off"][b] + 3])
                n_lt += p < 1; n_gt += 1 < p < 3
        x, tw, jac = kin_reference(mech, q, v)
        xn, twn, jn = _numpy_kinematics(pfc, mech, q, v)
        bx, btw, bj = kin_bound(mech, q, v)
        for name, got, ref, bnd in (("x", x[0], xn, bx), ("tw", tw[0], twn, btw), ("jac", jac, jn, bj)):
            d = np.abs(got - ref)
            assert (d <= bnd).all(), (k, name, np.argwhere(d > bnd)[:4], d.max(), bnd.max())
            worst = max(worst, float((d / np.maximum(bnd, 1e-300)).max()))
        largest = max(largest, float(bx.max()), float(btw.max()), float(bj.max()))
    print(f"largest difference / bound over 200 states: {worst:.3f}; largest bound {largest:.2e}; MRP |p| < 1: {n_lt}, in (1, 3): {n_gt}")
    assert n_lt > 50 and n_gt > 50
    assert largest < 1e-12      # a rounding bound, not a loose one


# ---- 4. conventions, on the statement ------------------------------------------------------------------------------------------
def _R(x):
    return np.asarray(x[:9]).reshape(3, 3, order="F")


def test_rotations_are_orthonormal_and_zero_mrp_is_the_identity():
    rng = np.random.default_rng(3)
    for k in range(40):
        mech = (mech_a(), mech_c())[k % 2]
        xs, _, _ = kin_scalar(mech, *random_state(mech, rng, k))
        for x in xs:
            assert np.abs(_R(x).T @ _R(x) - np.eye(3)).max() <= 16 * EPS
    xj, _ = _joint(FLOATING, [0.0] * 3, [0.0, 0.0, 0.0, 1.0, 2.0, 3.0], [0.0] * 6, None)
    assert xj == WORLD_X[:9] + [1.0, 2.0, 3.0]


def test_jacobian_times_v_is_the_twist():
    rng = np.random.default_rng(4)
    for k in range(60):
        mech = (mech_a(), mech_b(), mech_c())[k % 3]
        q, v = random_state(mech, rng, k)
        _, tw, jac = kin_reference(mech, q, v)
        _, btw, bj = kin_bound(mech, q, v)
        for b in range(mech["n_body"]):
            jv = jac[b].T @ v
            bound = btw[b] + np.abs(bj[b]).T @ np.abs(v) + (mech["nv"] + 2) * EPS * (np.abs(jac[b]).T @ np.abs(v))
            assert (np.abs(jv - tw[0, b]) <= bound).all(), (k, b, np.abs(jv - tw[0, b]), bound)


def mrp_rate(p, omega_body):
    """The MRP kinematic equation: pdot = 1/4 [(1 - p'p) I + 2 [p]x + 2 p p'] omega_body."""
    P = np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])
    return 0.25 * (((1.0 - p @ p) * np.eye(3) + 2.0 * P + 2.0 * np.outer(p, p)) @ omega_body)


def state_rate(mech, q, v):
    """qdot of the state's motion: v for revolute and prismatic joints; (mrp_rate(p, omega_body), R_j(p) v_body) for a floating one."""
    qd = np.array(v, dtype=np.float64)
    for b, t in enumerate(mech["joint_type"]):
        if t == FLOATING:
            o = mech["off"][b]
            xj, _ = _joint(FLOATING, [0.0] * 3, [float(e) for e in q[o:o + 6]], [0.0] * 6, None)
            qd[o:o + 3] = mrp_rate(q[o:o + 3], v[o:o + 3]); qd[o + 3:o + 6] = _R(xj) @ v[o + 3:o + 6]
    return qd


def test_twist_is_the_time_derivative_of_the_pose():
    """RigidBodyDynamics' twist_wrt_world: omega^ = Rdot R', lin = tdot - omega x t (about the world origin), by central differences
    of the pose along the state's motion, h = 1e-6.  Tolerance 1e-7 (1 + max |x|): truncation is about h^2 |x'''| / 6 <~ 1e-11 and
    rounding about eps |x| / h ~ 2e-9 at |x| <= 10, a margin of about 50."""
    rng = np.random.default_rng(5)
    h = 1e-6
    for k in range(30):
        mech = (mech_a(), mech_b(), mech_c())[k % 3]
        q, v = random_state(mech, rng, k)
        qd = state_rate(mech, q, v)
        xs, tws, _ = kin_scalar(mech, q, v)
        xp, _, _ = kin_scalar(mech, q + h * qd, v)
        xm, _, _ = kin_scalar(mech, q - h * qd, v)
        for b in range(mech["n_body"]):
            x = np.asarray(xs[b]); dx = (np.asarray(xp[b]) - np.asarray(xm[b])) / (2 * h)
            W = _R(dx) @ _R(x).T
            omega = np.array([W[2, 1], W[0, 2], W[1, 0]])
            lin = dx[9:] - np.cross(omega, x[9:])
            tol = 1e-7 * (1 + np.abs(x).max())
            assert np.abs(W + W.T).max() <= tol
            assert np.abs(np.concatenate([omega, lin]) - tws[b]).max() <= tol, (k, b, omega, lin, tws[b])


def test_jacobian_columns_of_non_ancestors_are_positive_zero():
    mech = mech_a()
    q, v = random_state(mech, np.random.default_rng(6))
    _, _, jac = kin_reference(mech, q, v)
    own = {0: range(0, 6), 1: range(0, 7), 2: range(0, 8), 3: range(0, 8), 4: list(range(0, 6)) + [8], 5: [9]}
    for b in range(6):
        for c in range(10):
            if c in own[b]:
                assert np.abs(jac[b, c]).max() > 0
            else:
                assert jac[b, c].tobytes() == np.zeros(6).tobytes()      # +0.0, not -0.0
    fixed = make_mech([-1, 0, -1], [FIXED, FIXED, PRISMATIC], np.tile(np.array(WORLD_X), (3, 1)), [[0, 0, 1]] * 3)
    _, _, jac = kin_reference(fixed, [0.5], [1.0])
    assert jac[0].tobytes() == np.zeros((1, 6)).tobytes() and jac[1].tobytes() == np.zeros((1, 6)).tobytes() and jac[2].any()
