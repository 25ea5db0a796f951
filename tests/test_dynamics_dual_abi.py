"""pfc_dynamics_dual[_device], pfc_accelerations_dual[_device], pfc_state_derivative_dual_device[_more]: the C ABI, the scalar
statements of the two Dual kernels' arithmetic (csrc/pfc_dyn.h, stated in include/pfc.h) that tests/test_gpu_dynamics_dual.py compares
bytes with, and what pins the partials of qdot, H, c and vdot without leaning on those statements -- without a device.

`dyn_dual_scalar` is test_dynamics_abi.dyn_core and the qdot statement on test_kinematics_dual_abi.D numbers, fed by
kin_dual_scalar: gravity, the inertia records, the axes and the literals are {x, 0.0}.  `chol_dual_scalar` is chol_scalar's factor
and vdot, then per direction  t_i = ((dH_i0 vdot_0 + dH_i1 vdot_1) + ...),  r_i = ((df_i - dc_i) + dtau_i) - t_i  and the same two
substitutions on r.

The bounds of `test_partials_agree_with_a_50_digit_evaluation` (derived, nothing fitted).
* dqdot, dH, dc.  The whole statement -- kinematics and dynamics, value and partial parts -- is run a second time on D numbers whose
  parts are `E` numbers, (value, bound) pairs carrying the standard running error:  e(a + b) = e_a + e_b + u' |a + b|,
  e(a b) = |a| e_b + |b| e_a + e_a e_b + u' |a b|,  e(a / b) = (e_a + |a / b| e_b) / (|b| - e_b) + u' |a / b|  (u' = 0.51 eps, the .01
  covering the rounding of the bound's own arithmetic), and cos, sin within eps of exact (1 ulp, as test_kinematics_dual_abi takes
  them) plus the angle's own error.  The E numbers' values go through the very operations of the Float64 statement, so they are its
  bytes (asserted), and the inputs q, v, dq, dv, the records and gravity are exact: the bound of the partial part is a bound on
  |statement - exact directional derivative|.  This is dyn_bound's B1 with the kinematic inputs' bounds produced by the same
  mechanism instead of taken from kin_bound, extended to the partial part by the product rule the D number applies.
* dvdot, against the exact dvdot* = H^-1 (((df - dc) + dtau) - dH H^-1 ((f - c) + tau)) of the solve's own Float64 inputs, in the
  2-norm.  Higham, Theorem 10.4 and (10.7) as test_cholesky_solve_against_fifty_digits: a computed solve x^ of H x = b has
  |x^ - H^-1 b| <= 2 k |H^-1 b|, k = n gamma_(3n+1) kappa_2(H) / (1 - n gamma_(n+1)) < 1/2.  With lmin the smallest eigenvalue:
    rhs^ = fl((f - c) + tau):      |rhs^ - rhs| <= gamma_2 (|f| + |c| + |tau|) =: e_rhs  (elementwise, then the 2-norm)
    vdot^:                         |vdot^ - vdot*| <= 2 k (|vdot*| + e_rhs / lmin) + e_rhs / lmin =: e_v
    t^, r^ (n + 1 and 3 roundings): |r^ - r*| <= gamma_3 (|df| + |dc| + |dtau|) + gamma_(n+1) |dH| |vdot^| + |dH|_2 e_v =: e_r
    dvdot^:                        |dvdot^ - dvdot*| <= 2 k (|dvdot*| + e_r / lmin) + e_r / lmin.
* The residual  H dvdot^ + dH vdot^ - ((df - dc) + dtau)  at 50 digits:  H (dvdot^ - H^-1 r^) + (r^ - ((df - dc) + dtau - dH vdot^)),
  below |H|_2 2 k (|dvdot*| + e_r / lmin) + gamma_3 (|df| + |dc| + |dtau|) + gamma_(n+1) |dH| |vdot^| in the 2-norm.
Largest observed error / bound: printed by the tests and recorded in DESIGN section 4, "Dual forward dynamics from joint states"."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

import test_dynamics_abi as DY
import test_kinematics_abi as K
import test_kinematics_dual_abi as KD
from test_dynamics_abi import GRAVITY, _cross, chol_scalar, dyn_core, dyn_scalar, make_inertia, random_inertia
from test_kinematics_abi import EPS, FLOATING, NDOF, PRISMATIC, REVOLUTE, WORLD_X, make_mech, mech_a, mech_b, mech_c, random_state
from test_kinematics_dual_abi import D, _Exact, _Float

ROOT = K.ROOT
NAMES = (("pfc_dynamics_dual_device", 15), ("pfc_dynamics_dual", 14), ("pfc_accelerations_dual_device", 15),
         ("pfc_accelerations_dual", 14), ("pfc_state_derivative_dual_device", 45), ("pfc_state_derivative_dual_device_more", 37))
U1 = 0.51 * EPS


def _literal_times(self, x):
    """x * D for a Python float x -- dyn_core's `2.0 * s1` -- is the product with the literal {x, 0.0} of the D's own part type."""
    t = type(self.v)
    return D(t(x), t(0.0)) * self


D.__rmul__ = _literal_times      # the only operator dyn_core needs that D lacks; it changes nothing D already does


# ---- the scalar statements -----------------------------------------------------------------------------------------------------
def qdot_dual(N, mech, qd, vd):
    """The qdot statement of include/pfc.h on D numbers: qd, vd lists of D."""
    out = list(vd)
    one, two, quarter = KD._lit(N, 1.0), KD._lit(N, 2.0), KD._lit(N, 0.25)
    zero3 = [KD._lit(N, 0.0)] * 3
    for b, t in enumerate(mech["joint_type"]):
        if t == FLOATING:
            o = int(mech["off"][b])
            p, w, u = qd[o:o + 3], vd[o:o + 3], vd[o + 3:o + 6]
            p2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
            pw = (p[0] * w[0] + p[1] * w[1]) + p[2] * w[2]
            a, bb, cr = one - p2, two * pw, _cross(p, w)
            xj, _ = KD._joint(N, FLOATING, zero3, qd[o:o + 6], [KD._lit(N, 0.0)] * 6)
            for r in range(3):
                out[o + r] = quarter * ((a * w[r] + two * cr[r]) + bb * p[r])
                out[o + 3 + r] = (xj[r] * u[0] + xj[3 + r] * u[1]) + xj[6 + r] * u[2]
    return out


def dyn_dual_numbers(mech, inertia, g, q, v, dq, dv, trig=None, N=None):
    """(qdot (nv D), H (nv lists of nv D), c (nv D)) of one scene and one direction on the number type N."""
    N = N or _Float(trig)
    xs, tws, cols = KD.kin_dual_scalar(mech, q, v, dq, dv, trig, N)
    lit = lambda x: KD._lit(N, x)
    vd = [D(N.num(a), N.num(b)) for a, b in zip(v, dv)]
    qd = [D(N.num(a), N.num(b)) for a, b in zip(q, dq)]
    H, c = dyn_core(mech, [[lit(e) for e in row] for row in np.asarray(inertia).reshape(-1, 13)], [lit(e) for e in g], vd, xs, tws, cols,
                    zero=lit(0.0))
    return qdot_dual(N, mech, qd, vd), H, c


def dyn_dual_scalar(mech, inertia, g, q, v, dq, dv, trig=None, part="d"):
    """One scene and one direction in Python floats, expression for expression as include/pfc.h states pfc_dynamics_dual_device.
    Returns the partial parts (part = "v": the value parts) dqdot (nv,), dH (nv,nv), dc (nv,)."""
    qd, H, c = dyn_dual_numbers(mech, inertia, g, q, v, dq, dv, trig)
    nv = mech["nv"]
    get = lambda e: getattr(e, part)
    return (np.array([get(e) for e in qd]).reshape(nv), np.array([[get(e) for e in row] for row in H], dtype=np.float64).reshape(nv, nv),
            np.array([get(e) for e in c], dtype=np.float64).reshape(nv))


def dyn_dual_reference(mech, inertia, g, q, v, dq, dv, trig=None):
    """pfc_dynamics_dual's three outputs: q, v (n_scene,nv); dq, dv (n_scene,n_dir,nv) or None (zeros; not both) ->
    dqdot (n_scene,n_dir,nv), dH (n_scene,n_dir,nv,nv), dc (n_scene,n_dir,nv)."""
    q, v = np.atleast_2d(q), np.atleast_2d(v)
    ns, nv = q.shape[0], mech["nv"]
    n_dir = np.shape(dq if dq is not None else dv)[-2]
    dq = np.zeros((ns, n_dir, nv)) if dq is None else np.asarray(dq, dtype=np.float64).reshape(ns, n_dir, nv)
    dv = np.zeros((ns, n_dir, nv)) if dv is None else np.asarray(dv, dtype=np.float64).reshape(ns, n_dir, nv)
    dqd, dH, dc = np.zeros((ns, n_dir, nv)), np.zeros((ns, n_dir, nv, nv)), np.zeros((ns, n_dir, nv))
    for s in range(ns):
        for k in range(n_dir):
            dqd[s, k], dH[s, k], dc[s, k] = dyn_dual_scalar(mech, inertia, g, q[s], v[s], dq[s, k], dv[s, k], trig)
    return dqd, dH, dc


def chol_dual_scalar(H, c, f, dH, dc, df, tau=None, dtau=None):
    """vdot and dvdot (n_dir,nv) in the order include/pfc.h states for pfc_accelerations_dual_device.  Returns (vdot, dvdot, info)."""
    n, n_dir = len(c), len(dc)
    A = [[float(H[i][j]) for j in range(n)] for i in range(n)]
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        col = []
        for i in range(j, n):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            col.append(s)
        if not col[0] > 0.0:
            return np.full(n, np.nan), np.full((n_dir, n), np.nan), j + 1
        L[j][j] = math.sqrt(col[0])
        for i in range(j + 1, n):
            L[i][j] = col[i - j] / L[j][j]

    def solve(rhs):
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
        return x

    vd = solve([(float(f[i]) - float(c[i])) + (float(tau[i]) if tau is not None else 0.0) for i in range(n)])
    out = []
    for d in range(n_dir):
        r = []
        for i in range(n):
            t = float(dH[d][i][0]) * vd[0]
            for j in range(1, n):
                t = t + float(dH[d][i][j]) * vd[j]
            r.append(((float(df[d][i]) - float(dc[d][i])) + (float(dtau[d][i]) if dtau is not None else 0.0)) - t)
        out.append(solve(r))
    return np.array(vd), np.array(out).reshape(n_dir, n), 0


# ---- running error numbers, with the quotient ------------------------------------------------------------------------------------
class E:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = float(v), float(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    def __add__(self, o):
        o = E.of(o); z = self.v + o.v
        return E(z, self.e + o.e + U1 * abs(z))

    def __sub__(self, o):
        o = E.of(o); z = self.v - o.v
        return E(z, self.e + o.e + U1 * abs(z))

    def __neg__(self):
        return E(-self.v, self.e)

    def __mul__(self, o):
        o = E.of(o); z = self.v * o.v
        return E(z, abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e + U1 * abs(z))

    def __truediv__(self, o):
        o = E.of(o); z = self.v / o.v
        assert abs(o.v) > 2 * o.e
        return E(z, (self.e + abs(z) * o.e) / (abs(o.v) - o.e) * (1 + 4 * EPS) + U1 * abs(z))

    def __rtruediv__(self, o):
        return E.of(o) / self


class _Running:
    """The number type of the bound: E numbers, cos and sin within eps of exact plus the angle's error."""
    def num(self, x): return E(x)

    def cos_sin(self, th):
        return E(math.cos(th.v), EPS + th.e), E(math.sin(th.v), EPS + th.e)


def dyn_dual_bound(mech, inertia, g, q, v, dq, dv):
    """((value parts as arrays), (bounds of the value parts), (partial parts), (bounds of the partial parts)), each (qdot, H, c)."""
    qd, H, c = dyn_dual_numbers(mech, inertia, g, q, v, dq, dv, N=_Running())
    pick = lambda part, f: (np.array([f(getattr(e, part)) for e in qd]), np.array([[f(getattr(e, part)) for e in row] for row in H]),
                            np.array([f(getattr(e, part)) for e in c]))
    val, err = (lambda a: a.v), (lambda a: a.e)
    return pick("v", val), pick("v", err), pick("d", val), pick("d", err)


def _seeds(mech, rng, n_dir):
    return rng.uniform(-1, 1, (n_dir, mech["nv"])), rng.uniform(-1, 1, (n_dir, mech["nv"]))


# ---- 1. ABI --------------------------------------------------------------------------------------------------------------------
def test_dual_dynamics_symbols_are_declared_exported_and_bound(pfc):
    hdr = open(os.path.join(ROOT, "include", "pfc.h")).read()
    assert "no Dual sibling yet" not in hdr
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
    for name, _ in NAMES[:4]:
        a = getattr(L, name).argtypes
        assert a[1] is C.c_int and a[2] is C.c_int, name                                    # n_scene, n_dir
    for name, _ in NAMES[4:]:
        a = getattr(L, name).argtypes
        assert a[1] is C.c_int and a[2] is C.c_int and a[5] is C.c_int, name                # n_items, n_dir, n_scene
    M = pfc.scenario.MechanismScenario
    for meth in ("dynamics_dual", "dynamics_dual_device", "accelerations_dual", "accelerations_dual_device",
                 "state_derivative_dual_device", "state_derivative_dual_device_more", "state_derivative_dual"):
        assert callable(getattr(M, meth)), meth


def test_dual_dynamics_kernels_are_built_from_their_header():
    csrc = os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc")
    for kernel in ("k_dynamics", "k_dynamics_dual", "k_accel", "k_accel_dual"):
        holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip"))
                   and re.search(r"__global__ void (__launch_bounds__\(\w+\) )?" + kernel + r"\(", open(os.path.join(csrc, f)).read())]
        assert holders == ["pfc_dyn.h"], (kernel, holders)
    dyn = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "pfc_dyn.h")).read())      # the code, without its comments
    # one statement of the five stages, instantiated twice; one factorisation and one pair of substitutions, used by both solves
    assert len(re.findall(r"void dyn_stages\(", dyn)) == 1
    assert "dyn_stages<double>" in dyn and "dyn_stages<ScatDual>" in dyn
    assert len(re.findall(r"\baccel_factor\(", dyn)) == 3 and len(re.findall(r"\baccel_solve<", dyn)) == 3
    assert len(re.findall(r"sqrt\(", dyn)) == 1
    assert "atomic" not in dyn.replace("no atomics", "")


# ---- 2. the scalar statements --------------------------------------------------------------------------------------------------
def test_value_parts_are_the_bytes_of_the_value_statements():
    rng = np.random.default_rng(20261201)
    for k in range(16):
        mech = (mech_a(), mech_b(), mech_c(), mech_a(seed=6))[k % 4]
        q, v = random_state(mech, rng, k // 4)
        inertia = random_inertia(mech, rng)
        dq, dv = _seeds(mech, rng, 2)
        trig = None
        if k % 2:
            trig = {float(q[mech["off"][b]]): (0.25 + 0.01 * b, -0.5) for b, t in enumerate(mech["joint_type"]) if t == REVOLUTE}
        got = dyn_dual_scalar(mech, inertia, GRAVITY, q, v, dq[0], dv[0], trig, part="v")
        ref = dyn_scalar(mech, inertia, GRAVITY, q, v, trig)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref)), k
        if trig is None:      # and the running-error numbers carry the same bytes, values and partials
            val, _, par, _ = dyn_dual_bound(mech, inertia, GRAVITY, q, v, dq[0], dv[0])
            assert all(a.tobytes() == b.tobytes() for a, b in zip(val, ref)), k
            assert all(a.tobytes() == b.tobytes() for a, b in zip(par, dyn_dual_scalar(mech, inertia, GRAVITY, q, v, dq[0], dv[0]))), k
        _, dH, dc = dyn_dual_scalar(mech, inertia, GRAVITY, q, v, dq[0], dv[0], trig)
        _, H, c = ref
        f, tau, df, dtau = rng.standard_normal(mech["nv"]), rng.standard_normal(mech["nv"]), rng.standard_normal((1, mech["nv"])), None
        vd, dvd, info = chol_dual_scalar(H, c, f, [dH], [dc], df, tau, dtau)
        ref_v, ref_i = chol_scalar(H, c, f, tau)
        assert info == ref_i == 0 and vd.tobytes() == ref_v.tobytes() and np.isfinite(dvd).all()
        # a NULL dtau is + 0.0: the bytes of an array of zeros
        assert chol_dual_scalar(H, c, f, [dH], [dc], df, tau, np.zeros((1, mech["nv"])))[1].tobytes() == dvd.tobytes()


def test_null_seeds_are_the_bytes_of_zero_arrays():
    mech = mech_a()
    rng = np.random.default_rng(3)
    q, v = random_state(mech, rng)
    q, v = q[None], v[None]
    inertia = random_inertia(mech, rng)
    dq, dv = rng.uniform(-1, 1, (1, 2, 10)), rng.uniform(-1, 1, (1, 2, 10))
    for a, b in ((dq, None), (None, dv)):
        got = dyn_dual_reference(mech, inertia, GRAVITY, q, v, a, b)
        ref = dyn_dual_reference(mech, inertia, GRAVITY, q, v, a if a is not None else np.zeros_like(dq), b if b is not None else np.zeros_like(dv))
        assert all(g.tobytes() == r.tobytes() for g, r in zip(got, ref))
        assert np.abs(got[0]).max() > 0 and np.abs(got[2]).max() > 0
        assert (np.abs(got[1]).max() > 0) == (a is not None)      # H does not depend on v
    assert dyn_dual_reference(mech, inertia, GRAVITY, q, v, dq, dv)[1].shape == (1, 2, 10, 10)


# ---- 3. the partials against a 50-digit evaluation -----------------------------------------------------------------------------
def _exact_arrays(mech, inertia, g, q, v, dq, dv, exact):
    qd, H, c = dyn_dual_numbers(mech, inertia, g, q, v, dq, dv, N=exact)
    return (np.array([e.d for e in qd], dtype=object), np.array([[e.d for e in row] for row in H], dtype=object),
            np.array([e.d for e in c], dtype=object))


def test_partials_agree_with_a_50_digit_evaluation():
    rng = np.random.default_rng(20261202)
    exact = _Exact()
    worst, largest, n_lt, n_gt = 0.0, 0.0, 0, 0
    for k in range(12):
        mech = (mech_a(), mech_c(), mech_a(seed=6))[k % 3]
        q, v = random_state(mech, rng, k // 3)
        for b, t in enumerate(mech["joint_type"]):
            if t == FLOATING:
                p = np.linalg.norm(q[mech["off"][b]:mech["off"][b] + 3])
                n_lt += p < 1; n_gt += 1 < p < 3
        inertia = random_inertia(mech, rng)
        g = np.array(GRAVITY) if k % 2 else rng.uniform(-10, 10, 3)
        dq, dv = _seeds(mech, rng, 2)
        for d in range(2):
            got = dyn_dual_scalar(mech, inertia, g, q, v, dq[d], dv[d])
            ref = _exact_arrays(mech, inertia, g, q, v, dq[d], dv[d], exact)
            _, _, par, bnd = dyn_dual_bound(mech, inertia, g, q, v, dq[d], dv[d])
            for name, a, p_, r, b in zip(("dqdot", "dH", "dc"), got, par, ref, bnd):
                assert a.tobytes() == p_.tobytes()
                diff = np.abs(a - r).astype(np.float64)      # the difference is formed in 50 digits
                assert (diff <= b).all(), (k, d, name, np.argwhere(diff > b)[:4], diff.max(), b.max())
                nz = b > 0
                if nz.any():
                    worst = max(worst, float((diff[nz] / b[nz]).max()))
                largest = max(largest, float(b.max()))
                assert np.abs(r.astype(np.float64)).max() > 0
    print(f"dqdot, dH, dc: largest error / bound over 12 states x 2 directions {worst:.3f}; largest bound {largest:.2e}; "
          f"MRP |p| < 1: {n_lt}, in (1, 3): {n_gt}")
    assert n_lt >= 2 and n_gt >= 2
    assert largest < 1e-7      # a rounding bound: ten times dyn_bound's ceiling on the values, the partials being as large again


def _solve_bounds(mp, H, c, f, tau, dH, dc, df, dtau, vd):
    """(k, lmin, vdot*, [dvdot*], [e_r], [e_r without the e_v term], e_v) of the module docstring, in mpmath."""
    n = len(c)
    u = mp.mpf(2) ** -53
    gam = lambda m: m * u / (1 - m * u)
    M = lambda a: mp.matrix([[mp.mpf(float(e))] for e in a])
    Hm = mp.matrix(np.asarray(H).tolist())
    ev = mp.eigsy(Hm, eigvals_only=True)
    lmin, kappa = min(ev), max(ev) / min(ev)
    kk = n * gam(3 * n + 1) * kappa / (1 - n * gam(n + 1))
    rhs = M(f) - M(c) + M(tau)
    vs = mp.lu_solve(Hm, rhs)
    e_rhs = mp.norm(gam(2) * M(np.abs(f) + np.abs(c) + np.abs(tau)))
    e_v = 2 * kk * (mp.norm(vs) + e_rhs / lmin) + e_rhs / lmin
    outs = []
    for d in range(len(dc)):
        dHm = mp.matrix(np.asarray(dH[d]).tolist())
        rs = M(df[d]) - M(dc[d]) + M(dtau[d]) - dHm * vs
        xs = mp.lu_solve(Hm, rs)
        form = mp.norm(gam(3) * M(np.abs(df[d]) + np.abs(dc[d]) + np.abs(dtau[d])) + gam(n + 1) * M(np.abs(dH[d]) @ np.abs(vd)))
        dH2 = mp.sqrt(max(mp.eigsy(dHm.T * dHm, eigvals_only=True)))
        outs.append((xs, form + dH2 * e_v, form))
    return kk, lmin, Hm, vs, outs, e_v


def test_solve_partials_against_fifty_digits_and_their_residual():
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(20261203)
    worst, worst_res = 0.0, 0.0
    for k in range(6):
        mech = (mech_a(), mech_b(), mech_c())[k % 3]
        q, v = random_state(mech, rng, k)
        inertia = random_inertia(mech, rng)
        n, n_dir = mech["nv"], 2
        dq, dv = _seeds(mech, rng, n_dir)
        _, H, c = dyn_scalar(mech, inertia, GRAVITY, q, v)
        part = [dyn_dual_scalar(mech, inertia, GRAVITY, q, v, dq[d], dv[d]) for d in range(n_dir)]
        dH, dc = [p[1] for p in part], [p[2] for p in part]
        f, tau = rng.standard_normal(n), rng.standard_normal(n)
        df, dtau = rng.standard_normal((n_dir, n)), rng.standard_normal((n_dir, n))
        vd, dvd, info = chol_dual_scalar(H, c, f, dH, dc, df, tau, dtau)
        assert info == 0
        kk, lmin, Hm, vs, outs, e_v = _solve_bounds(mp, H, c, f, tau, dH, dc, df, dtau, vd)
        assert kk < 0.5
        col = lambda a: mp.matrix([[mp.mpf(float(e))] for e in a])
        assert mp.norm(col(vd) - vs) <= e_v
        for d, (xs, e_r, form) in enumerate(outs):
            bound = 2 * kk * (mp.norm(xs) + e_r / lmin) + e_r / lmin
            err = mp.norm(col(dvd[d]) - xs)
            assert err <= bound, (k, d, float(err), float(bound))
            worst = max(worst, float(err / bound))
            res = Hm * col(dvd[d]) + mp.matrix(np.asarray(dH[d]).tolist()) * col(vd) - (col(df[d]) - col(dc[d]) + col(dtau[d]))
            rb = mp.sqrt(max(mp.eigsy(Hm.T * Hm, eigvals_only=True))) * 2 * kk * (mp.norm(xs) + e_r / lmin) + form
            assert mp.norm(res) <= rb, (k, d, float(mp.norm(res)), float(rb))
            worst_res = max(worst_res, float(mp.norm(res) / rb))
    print(f"dvdot: largest error / bound {worst:.2e}; residual / bound {worst_res:.2e}")


# ---- 4. independent of the formulation -----------------------------------------------------------------------------------------
def _numpy_dynamics(pfc, mech, inertia, g, q, v):
    return pfc.scenario.joint_dynamics(mech["parent"], mech["joint_type"], mech["x_p_j"], mech["axis"], inertia, g, q, v)


def test_partials_are_the_central_differences_of_joint_dynamics(pfc):
    """Central differences of scenario.joint_dynamics (NumPy, the matrix formulation) along (dq, dv) in Float64 at h = 2e-3 and 1e-3.
    The error must fall as h^2 (a ratio of 4, asserted within [3.5, 4.5] where the finer error is a thousand times above the rounding
    floor eps scale / h) and the finer one must lie below h^2 times the scale: truncation is h^2 / 6 times a third directional
    derivative, and with |dq|, |dv| <= 1 per coordinate (nv <= 10: |direction|^3 <= 10^1.5 nv^1.5) each derivative of an entry of H or c
    is below the entry's magnitude sum times the direction's length, as test_bias_is_the_sum_formula... argues for the columns.
    scale: max |H| (for dH), max |c| + max |H| (for dc, which is quadratic in v), times nv^1.5."""
    rng = np.random.default_rng(21)
    seen = 0
    for k in range(6):
        mech = (mech_a(), mech_c())[k % 2]
        q, v = random_state(mech, rng, 2 * k)       # |p| < 1
        inertia = random_inertia(mech, rng)
        g = np.array(GRAVITY)
        dq, dv = _seeds(mech, rng, 1)
        dqd, dH, dc = dyn_dual_scalar(mech, inertia, g, q, v, dq[0], dv[0])
        fd = []
        for h in (2e-3, 1e-3):
            p = _numpy_dynamics(pfc, mech, inertia, g, q + h * dq[0], v + h * dv[0])
            m = _numpy_dynamics(pfc, mech, inertia, g, q - h * dq[0], v - h * dv[0])
            fd.append([(a - b) / (2 * h) for a, b in zip(p, m)])
        _, H, c = dyn_scalar(mech, inertia, g, q, v)
        big = mech["nv"] ** 1.5
        for name, a, s in (("dqdot", dqd, big * (1 + np.abs(v).max())), ("dH", dH, big * np.abs(H).max()),
                           ("dc", dc, big * (np.abs(c).max() + np.abs(H).max()))):
            i = ("dqdot", "dH", "dc").index(name)
            e1, e2 = np.abs(fd[0][i].reshape(a.shape) - a), np.abs(fd[1][i].reshape(a.shape) - a)
            assert (e2 <= 1e-6 * s + 1e-9).all(), (k, name, e2.max(), s)
            for idx in np.argwhere(e2 > 1e3 * EPS * s / 1e-3):
                seen += 1
                r = e1[tuple(idx)] / e2[tuple(idx)]
                assert 3.5 <= r <= 4.5, (k, name, idx, r)
    assert seen >= 10


def test_dH_is_symmetric_to_the_bit_and_positive_zero_across_branches():
    rng = np.random.default_rng(22)
    for k in range(6):
        mech = (mech_a(), mech_b(), mech_c())[k % 3]
        q, v = random_state(mech, rng, k)
        dq, dv = _seeds(mech, rng, 1)
        _, dH, _ = dyn_dual_scalar(mech, random_inertia(mech, rng), GRAVITY, q, v, dq[0], dv[0])
        assert dH.tobytes() == np.ascontiguousarray(dH.T).tobytes()
    mech = mech_a()
    q, v = random_state(mech, rng)
    dq, dv = _seeds(mech, rng, 1)
    _, dH, _ = dyn_dual_scalar(mech, random_inertia(mech, rng), GRAVITY, q, v, dq[0], dv[0])
    related = {6: range(0, 8), 7: range(0, 8), 8: list(range(0, 6)) + [8], 9: [9]}      # as test_dynamics_abi: the branches of (A)
    for i, rel in related.items():
        for j in range(10):
            if j not in rel:
                assert dH[i, j].tobytes() == np.float64(0.0).tobytes() and dH[j, i].tobytes() == np.float64(0.0).tobytes()   # +0.0
    assert (dH[6, :8] != 0).any() and (dH[8, :6] != 0).any()


def test_bias_partial_along_v_is_twice_the_velocity_part():
    """c(q, v) = C(q)[v, v] + G(q) with C bilinear: along dq = 0, dv = v the derivative is 2 C[v, v] = 2 (c(q, v) - c(q, 0)).  Bound: the
    running-error bound of dc, plus twice those of c(q, v) and c(q, 0), plus the rounding of the difference and the doubling,
    1.5 eps (|c(q, v)| + |c(q, 0)|) 2."""
    rng = np.random.default_rng(23)
    worst = 0.0
    for k in range(8):
        mech = (mech_a(), mech_c(), mech_b(), mech_a(seed=6))[k % 4]
        q, v = random_state(mech, rng, k // 4)
        inertia = random_inertia(mech, rng)
        z = np.zeros(mech["nv"])
        val, ev, par, ed = dyn_dual_bound(mech, inertia, GRAVITY, q, v, z, v)
        val0, ev0, _, _ = dyn_dual_bound(mech, inertia, GRAVITY, q, z, z, z)
        ref = 2.0 * (val[2] - val0[2])
        bound = ed[2] + 2 * (ev[2] + ev0[2]) + 3 * EPS * (np.abs(val[2]) + np.abs(val0[2]))
        diff = np.abs(par[2] - ref)
        assert (diff <= bound).all(), (k, diff, bound)
        worst = max(worst, float((diff / np.maximum(bound, 1e-300)).max()))
        assert np.abs(ref).max() > 0 and bound.max() < 1e-8
    print(f"dc along v against 2 (c(q, v) - c(q, 0)): largest difference / bound {worst:.3f}")


def test_power_balance_with_the_exact_mass_matrix_rate():
    """With dq = qdot(q, v), dv = 0, dH is Hdot and  v'c = 1/2 v' Hdot v + dV/dt,  V = -sum_b g . (R_b cp_b + m_b t_b), dV/dt from the
    pose partials of kin_dual_scalar along the same direction.  qdot is rounded (eps relative per coordinate: dyn_bound's Bq), which
    moves the right-hand side by its derivative along that error -- below eps times the magnitude sum of the right-hand side's terms,
    every one of which is linear in the direction.  Bound: the running-error bounds of c (in v'c) and of dH (in v' dH v), the
    roundings of the two contractions (gamma_(nv+2) and gamma_(2 nv + 2) on their magnitude sums), the pose partials' bound
    kin_dual_bound in dV/dt, and the 16 eps of qdot on the magnitude sums."""
    rng = np.random.default_rng(24)
    worst = 0.0
    for k in range(6):
        mech = (mech_a(), mech_c(), mech_b())[k % 3]
        q, v = random_state(mech, rng, 2 * k)
        inertia = random_inertia(mech, rng)
        g = np.array(GRAVITY)
        nv, z = mech["nv"], np.zeros(mech["nv"])
        qd, _, _ = dyn_scalar(mech, inertia, g, q, v)
        val, ev, par, ed = dyn_dual_bound(mech, inertia, g, q, v, qd, z)
        c, dH = val[2], par[1]
        xd, _, _ = KD._partials_one(mech, q, v, qd, z)
        ex, _, _ = KD.kin_dual_bound(mech, q, v, qd, z, 0)
        dV, dV_mag, dV_err = 0.0, 0.0, 0.0
        for b in range(mech["n_body"]):
            dR, dt = K._split(xd[b])
            cp, m = inertia[b, 9:12], inertia[b, 12]
            dV -= float(g @ (dR @ cp + m * dt))
            dV_mag += float(np.abs(g) @ (np.abs(dR) @ np.abs(cp) + m * np.abs(dt)))
            dV_err += float(np.abs(g) @ (np.full((3, 3), ex[b, 0]) @ np.abs(cp) + m * np.full(3, ex[b, 9])))
        lhs, rhs = float(v @ c), 0.5 * float(v @ dH @ v) + dV
        quad_mag = 0.5 * float(np.abs(v) @ np.abs(dH) @ np.abs(v))
        bound = (float(np.abs(v) @ ev[2]) + 0.5 * float(np.abs(v) @ ed[1] @ np.abs(v)) + (nv + 2) * EPS * float(np.abs(v) @ np.abs(c))
                 + (2 * nv + 2) * EPS * quad_mag + dV_err + 8 * EPS * dV_mag + 16 * EPS * (quad_mag + dV_mag))
        assert abs(lhs - rhs) <= bound, (k, lhs, rhs, bound)
        worst = max(worst, abs(lhs - rhs) / bound)
        assert bound < 1e-8 * (1 + abs(lhs))
    print(f"power balance with the exact Hdot: largest difference / bound {worst:.3f}")


# ---- 5. closed forms -----------------------------------------------------------------------------------------------------------
def test_point_mass_pendulum_partial():
    """c = m g l sin(theta): dc / dtheta = m g l cos(theta); H = m l^2 is constant: dH = 0 to rounding (16 eps relative, as the values)."""
    m, l, g = 0.7, 0.4, 9.81
    mech = make_mech([-1], [REVOLUTE], [WORLD_X], [[0.0, 1.0, 0.0]])
    rec = make_inertia(m, [0.0, 0.0, -l], np.zeros((3, 3))).reshape(1, 13)
    for th in (-2.5, -0.3, 0.0, 0.9, 3.0):
        dqd, dH, dc = dyn_dual_scalar(mech, rec, (0.0, 0.0, -g), [th], [1.3], [1.0], [0.0])
        assert dqd[0] == 0.0
        assert abs(dc[0] - m * g * l * math.cos(th)) <= 16 * EPS * m * g * l
        assert abs(dH[0, 0]) <= 16 * EPS * m * l * l
        dqd, _, _ = dyn_dual_scalar(mech, rec, (0.0, 0.0, -g), [th], [1.3], [0.0], [0.5])
        assert dqd[0] == 0.5


def test_prismatic_mass_on_a_revolute_arm_partial():
    """H = diag(m r^2, m): dH / dr = diag(2 m r, 0); c = [2 m r rdot thdot + m g r cos th, -m r thdot^2 + m g sin th]:
    dc / dr = [2 m rdot thdot + m g cos th, -m thdot^2]; 32 eps of the values' scale, as the value test."""
    m, g = 1.3, 9.81
    mech = make_mech([-1, 0], [REVOLUTE, PRISMATIC], [WORLD_X, WORLD_X], [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    rec = np.zeros((2, 13)); rec[1, 12] = m
    rng = np.random.default_rng(25)
    for _ in range(10):
        th, r, thd, rd = rng.uniform(-3, 3), rng.uniform(0.2, 2), rng.uniform(-1, 1), rng.uniform(-1, 1)
        _, dH, dc = dyn_dual_scalar(mech, rec, (0.0, -g, 0.0), [th, r], [thd, rd], [0.0, 1.0], [0.0, 0.0])
        scale = m * (1 + r) ** 2 * (1 + g)
        assert np.abs(dH - np.diag([2 * m * r, 0.0])).max() <= 32 * EPS * scale
        assert np.abs(dc - [2 * m * rd * thd + m * g * math.cos(th), -m * thd * thd]).max() <= 32 * EPS * scale


def test_free_body_qdot_partial():
    """pdot = 1/4 ((1 - p.p) w + 2 p x w + 2 (p.w) p):  d pdot along dp = 1/4 (-2 (p.dp) w + 2 dp x w + 2 (dp.w) p + 2 (p.w) dp); about
    20 roundings on terms below (1 + |p|^2) |w| |dp|: 32 eps of that."""
    mech = make_mech([-1], [FLOATING], [WORLD_X], [[0, 0, 0]])
    rng = np.random.default_rng(26)
    for k in range(10):
        q, v = random_state(mech, rng, k)
        dp = rng.uniform(-1, 1, 3)
        dq = np.concatenate([dp, np.zeros(3)])
        dqd, _, _ = dyn_dual_scalar(mech, random_inertia(mech, rng), GRAVITY, q, v, dq, np.zeros(6))
        p, w = q[:3], v[:3]
        ref = 0.25 * (-2 * (p @ dp) * w + 2 * np.cross(dp, w) + 2 * (dp @ w) * p + 2 * (p @ w) * dp)
        scale = (1 + p @ p) * np.linalg.norm(w) * np.linalg.norm(dp)
        assert np.abs(dqd[:3] - ref).max() <= 32 * EPS * scale, (k, np.abs(dqd[:3] - ref).max(), scale)
        # tdot = R(p) u: along dv = e_k of the linear part the partial is R's column k, the value statement's bytes
        dv = np.zeros(6); dv[4] = 1.0
        dqd, _, _ = dyn_dual_scalar(mech, random_inertia(mech, rng), GRAVITY, q, v, np.zeros(6), dv)
        xj, _ = K._joint(FLOATING, [0.0] * 3, [float(e) for e in q], [0.0] * 6, None)
        assert np.array_equal(dqd[3:], np.asarray(xj[3:6])) and not dqd[:3].any()


# ---- 6. a failed pivot ---------------------------------------------------------------------------------------------------------
def test_massless_moving_body_flags_its_pivot_and_all_partials_are_nan():
    mech = mech_c()      # b3 massless makes pivot 4 zero
    rng = np.random.default_rng(16)
    q, v = random_state(mech, rng)
    inertia = random_inertia(mech, rng, massless=(3,))
    _, H, c = dyn_scalar(mech, inertia, GRAVITY, q, v)
    dq, dv = _seeds(mech, rng, 3)
    part = [dyn_dual_scalar(mech, inertia, GRAVITY, q, v, dq[d], dv[d]) for d in range(3)]
    assert H[3, 3] == 0.0
    vd, dvd, info = chol_dual_scalar(H, c, np.zeros(4), [p[1] for p in part], [p[2] for p in part], np.zeros((3, 4)))
    assert info == 4 and np.isnan(vd).all() and dvd.shape == (3, 4) and np.isnan(dvd).all()
