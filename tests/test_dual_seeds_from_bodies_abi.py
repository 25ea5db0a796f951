"""pfc_dual_seeds_from_bodies[_device], pfc_eval_dual_bodies_device[_more]: the C ABI, and the scalar statement of the seeds kernel's
arithmetic (k_dual_seeds_from_bodies, csrc/pfc_bodies.h) that tests/test_gpu_dual_seeds_from_bodies.py compares bytes with -- without
a device.

The statement, `seeds_scalar`, is items_scalar's statements (tests/test_items_from_bodies_abi.py, duplicated here) run on a (value,
partial) number with ForwardDiff's rules: sum and difference componentwise, unary minus on both parts, the product
{a.v b.v, a.d b.v + a.v b.d} (the order of _mul_partials), no fma.

It is checked against the matrix form of the derivative in NumPy (`seeds_matrix`).  Bound, elementwise (`seeds_bound`): every partial
entry is, on both sides, a sum of products a_k b_k (a value times a partial) that is exactly the same sum in exact arithmetic; the
sides differ in association, in the order of the additions and in whether BLAS contracts a product into an fma.  On either side a
product goes through its multiplication and then through at most 5 additions -- in the statement the sum of the two halves of a
Dual product (1), the 3-term dot product (2) and the translation or cross term added last (1); in the matrix form the dot or cross
product (2) and the three additions that join the four vectors of d_lin (3) -- so 8 roundings bound both with room: each side is
within gamma_8 = 8u / (1 - 8u) (u = eps / 2) of the exact sum, times sum_k |a_k| |b_k|, and two such values differ by at most
2 gamma_8 < 9 eps times that sum ("E").  Where an operand was itself
computed -- the values t2w, R21, t21, ang and the partials dt2w, dR21, dt21, dang -- the two sides' operands differ by their own
bound, which is carried through the product with the magnitude bound of the other operand.  (d = tw_2 - tw_1 and its partial are one
subtraction, the same on both sides: no bound of their own.)  Products of two bounds are O(eps^2) and lie in the slack between
2 gamma_8 and 9 eps.  Nothing in the bound is fitted to an observed difference."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from test_items_from_bodies_abi import EPS, WORLD_X, items_scalar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = (("pfc_dual_seeds_from_bodies_device", 15), ("pfc_dual_seeds_from_bodies", 14), ("pfc_eval_dual_bodies_device", 27),
         ("pfc_eval_dual_bodies_device_more", 18))
E = 9 * EPS


class D:
    """One partial of a ForwardDiff.Dual: value v and partial d."""
    __slots__ = ("v", "d")

    def __init__(self, v, d=0.0):
        self.v, self.d = float(v), float(d)

    def __add__(self, o): return D(self.v + o.v, self.d + o.d)
    def __sub__(self, o): return D(self.v - o.v, self.d - o.d)
    def __neg__(self): return D(-self.v, -self.d)
    def __mul__(self, o): return D(self.v * o.v, self.d * o.v + self.v * o.d)


def seeds_scalar(x1, tw1, x2, tw2, dx1, dtw1, dx2, dtw2):
    """pose (24) and twist (6) of one item as lists of D from the world pose / twist of body 1 and body 2 and their partials for one
    direction: the statements of bodies_item in csrc/pfc_bodies.h (items_scalar's, on D)."""
    x1, tw1, x2, tw2 = ([D(v, d) for v, d in zip(a, b)] for a, b in ((x1, dx1), (tw1, dtw1), (x2, dx2), (tw2, dtw2)))
    pose, twist = [None] * 24, [None] * 6
    t2w = [-((x2[3 * r] * x2[9] + x2[3 * r + 1] * x2[10]) + x2[3 * r + 2] * x2[11]) for r in range(3)]
    for c in range(3):
        for r in range(3):
            pose[3 * c + r] = (x2[3 * r] * x1[3 * c] + x2[3 * r + 1] * x1[3 * c + 1]) + x2[3 * r + 2] * x1[3 * c + 2]
    for r in range(3):
        pose[9 + r] = ((x2[3 * r] * x1[9] + x2[3 * r + 1] * x1[10]) + x2[3 * r + 2] * x1[11]) + t2w[r]
    for c in range(3):
        for r in range(3):
            pose[12 + 3 * c + r] = pose[3 * r + c]
    for r in range(3):
        pose[21 + r] = -((pose[3 * r] * pose[9] + pose[3 * r + 1] * pose[10]) + pose[3 * r + 2] * pose[11])
    d = [tw2[e] - tw1[e] for e in range(6)]
    ang = [(x2[3 * r] * d[0] + x2[3 * r + 1] * d[1]) + x2[3 * r + 2] * d[2] for r in range(3)]
    lin = [(x2[3 * r] * d[3] + x2[3 * r + 1] * d[4]) + x2[3 * r + 2] * d[5] for r in range(3)]
    twist[0:3] = ang
    twist[3] = lin[0] + (t2w[1] * ang[2] - t2w[2] * ang[1])
    twist[4] = lin[1] + (t2w[2] * ang[0] - t2w[0] * ang[2])
    twist[5] = lin[2] + (t2w[0] * ang[1] - t2w[1] * ang[0])
    return pose, twist


def seeds_reference(bind, x_w_b, twist_w_b, d_x_w_b, d_twist_w_b, n_dir, ins_ids=None, scene=None):
    """The three outputs of pfc_dual_seeds_from_bodies by seeds_scalar, in the ABI's layouts: d_pose (n,n_dir,24), d_twist
    (n,n_dir,6), d_x_w_r2 (n,n_dir,12).  bind (n_ins,2); x_w_b (n_scene,n_body,12); twist_w_b (n_scene,n_body,6); d_x_w_b
    (n_scene,n_body,n_dir,12) or None (zeros); d_twist_w_b (n_scene,n_body,n_dir,6) or None; ins_ids / scene (n,) or None."""
    bind = np.asarray(bind)
    n = len(ins_ids) if ins_ids is not None else (len(scene) if scene is not None else len(bind))
    d_pose, d_twist, d_x_w_r2 = np.zeros((n, n_dir, 24)), np.zeros((n, n_dir, 6)), np.zeros((n, n_dir, 12))
    Z12, Z6 = [0.0] * 12, [0.0] * 6
    for i in range(n):
        b1, b2 = (int(v) for v in bind[int(ins_ids[i]) if ins_ids is not None else i])
        sc = int(scene[i]) if scene is not None else 0
        for k in range(n_dir):
            def st(b):
                if b < 0:
                    return WORLD_X, [0.0] * 6, Z12, Z6
                return (x_w_b[sc, b], twist_w_b[sc, b], d_x_w_b[sc, b, k] if d_x_w_b is not None else Z12,
                        d_twist_w_b[sc, b, k] if d_twist_w_b is not None else Z6)
            (x1, tw1, dx1, dtw1), (x2, tw2, dx2, dtw2) = st(b1), st(b2)
            pose, twist = seeds_scalar(x1, tw1, x2, tw2, dx1, dtw1, dx2, dtw2)
            d_pose[i, k] = [q.d for q in pose]
            d_twist[i, k] = [q.d for q in twist]
            d_x_w_r2[i, k] = dx2
    return d_pose, d_twist, d_x_w_r2


def _split(x):
    x = np.asarray(x, dtype=np.float64)
    return x[:9].reshape(3, 3, order="F"), x[9:]


def seeds_matrix(x1, tw1, x2, tw2, dx1, dtw1, dx2, dtw2):
    """The partials of pose (24) and twist (6) by the matrix form of the derivative."""
    (R1, t1), (R2, t2), (dR1, dt1), (dR2, dt2) = _split(x1), _split(x2), _split(dx1), _split(dx2)
    tw = np.asarray(tw2, dtype=np.float64) - np.asarray(tw1, dtype=np.float64)
    dtw = np.asarray(dtw2, dtype=np.float64) - np.asarray(dtw1, dtype=np.float64)
    R2w, dR2w = R2.T, dR2.T
    t2w = -(R2w @ t2)
    dt2w = -(dR2w @ t2 + R2w @ dt2)
    R21 = R2w @ R1
    t21 = R2w @ t1 + t2w
    dR21 = dR2w @ R1 + R2w @ dR1
    dt21 = dR2w @ t1 + R2w @ dt1 + dt2w
    dt12 = -(dR21.T @ t21 + R21.T @ dt21)
    ang = R2w @ tw[:3]
    dang = dR2w @ tw[:3] + R2w @ dtw[:3]
    dlin = dR2w @ tw[3:] + R2w @ dtw[3:] + np.cross(dt2w, ang) + np.cross(t2w, dang)
    dp = np.concatenate([dR21.reshape(-1, order="F"), dt21, dR21.T.reshape(-1, order="F"), dt12])
    return dp, np.concatenate([dang, dlin])


def _abs_cross(a, b):
    return np.array([a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]])


def seeds_bound(x1, tw1, x2, tw2, dx1, dtw1, dx2, dtw2):
    """Elementwise (bound, sum of |terms|) for the partials of pose (24) and twist (6): E times the sum of |a| |b| over the products
    of each entry, an operand's own bound carried through where it was computed (module docstring).  Returns (bp, sp, bt, st)."""
    a = lambda v: np.abs(np.asarray(v, dtype=np.float64))
    (A1, t1), (A2c, t2), (dA1, dt1), (dA2c, dt2) = _split(a(x1)), _split(a(x2)), _split(a(dx1)), _split(a(dx2))
    A2, dA2 = A2c.T, dA2c.T                          # |R2w|, |dR2w|
    d, dd = a(tw2) + a(tw1), a(dtw2) + a(dtw1)       # |tw_2 - tw_1| <= |tw_2| + |tw_1|, likewise the partial
    # values, as items_bound
    t2w = A2 @ t2;                       b_t2w = E * t2w
    R21 = A2 @ A1;                       b_R21 = E * R21
    t21 = A2 @ t1 + t2w;                 b_t21 = E * t21 + b_t2w
    ang = A2 @ d[:3];                    b_ang = E * ang
    # partials
    dt2w = dA2 @ t2 + A2 @ dt2;          b_dt2w = E * dt2w
    dR21 = dA2 @ A1 + A2 @ dA1;          b_dR21 = E * dR21
    dt21 = dA2 @ t1 + A2 @ dt1 + dt2w;   b_dt21 = E * dt21 + b_dt2w
    dt12 = dR21.T @ t21 + R21.T @ dt21
    b_dt12 = E * dt12 + b_dR21.T @ t21 + dR21.T @ b_t21 + b_R21.T @ dt21 + R21.T @ b_dt21
    dang = dA2 @ d[:3] + A2 @ dd[:3];    b_dang = E * dang
    dlin = dA2 @ d[3:] + A2 @ dd[3:] + _abs_cross(dt2w, ang) + _abs_cross(t2w, dang)
    b_dlin = (E * dlin + _abs_cross(b_dt2w, ang) + _abs_cross(dt2w, b_ang) + _abs_cross(b_t2w, dang) + _abs_cross(t2w, b_dang))
    F = lambda M: M.reshape(-1, order="F")
    bp = np.concatenate([F(b_dR21), b_dt21, F(b_dR21.T), b_dt12])
    sp = np.concatenate([F(dR21), dt21, F(dR21.T), dt12])
    return bp, sp, np.concatenate([b_dang, b_dlin]), np.concatenate([dang, dlin])


def _random_pair(pfc, rng, k):
    """States and partials of two bodies: rotations from QR, |t| <= 10, standard-normal twists and partials; a third of the pairs
    with body 1's partials zero; the world (R = I, t = 0, zeros) on either side now and then."""
    Cf = pfc.configs
    st = []
    for side in range(2):
        R, t = Cf.random_rotation(rng), rng.uniform(-1, 1, 3) * rng.uniform(0, 10)
        st.append([np.concatenate([R.reshape(-1, order="F"), t]), rng.standard_normal(6), rng.standard_normal(12), rng.standard_normal(6)])
    if k % 3 == 0:
        st[0][2], st[0][3] = np.zeros(12), np.zeros(6)
    if k % 20 == 7:
        st[0] = [np.array(WORLD_X), np.zeros(6), np.zeros(12), np.zeros(6)]
    if k % 20 == 13:
        st[1] = [np.array(WORLD_X), np.zeros(6), np.zeros(12), np.zeros(6)]
    (x1, tw1, dx1, dtw1), (x2, tw2, dx2, dtw2) = st
    return x1, tw1, x2, tw2, dx1, dtw1, dx2, dtw2


def test_seed_symbols_are_declared_exported_and_bound(pfc):
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
    for name, _ in NAMES:
        a = getattr(L, name).argtypes
        assert a[1] is C.c_int and a[2] is C.c_int and a[5] is C.c_int and a[6] is C.c_int, name      # n_items, n_dir, n_scene, n_body
    M = pfc.scenario.MechanismScenario
    for meth in ("dual_seeds_from_bodies", "dual_seeds_from_bodies_device", "eval_dual_bodies_device", "eval_dual_bodies_device_more",
                 "force_all_elastic_intersections_dual_bodies"):
        assert callable(getattr(M, meth)), meth


def test_seeds_kernel_is_built_from_a_listed_header(pfc):
    csrc = os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc")
    holders = [f for f in sorted(os.listdir(csrc)) if f.endswith(".h") and "void k_dual_seeds_from_bodies(" in
               open(os.path.join(csrc, f)).read().replace("__launch_bounds__(kBodiesWave) ", "")]
    assert len(holders) == 1, holders
    srcs = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "_lib.py")).read()
    assert f'"{holders[0]}"' in srcs      # a change of the kernel rebuilds the library
    assert f'#include "{holders[0]}"' in open(os.path.join(csrc, "pfc_hip.hip")).read()
    # one definition of the (value, partial) type and of its product rule for the scatter and the seeds
    text = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip")))
    assert len(re.findall(r"struct ScatDual\s*\{", text)) == 1
    assert len(re.findall(r"operator\*\(ScatDual", text)) == 1


def test_value_parts_are_the_bytes_of_items_scalar(pfc):
    rng = np.random.default_rng(20261019)
    for k in range(40):
        args = _random_pair(pfc, rng, k)
        pose, twist = seeds_scalar(*args)
        pose_v, twist_v = items_scalar(*args[:4])
        assert np.array([q.v for q in pose]).tobytes() == np.array(pose_v).tobytes(), k
        assert np.array([q.v for q in twist]).tobytes() == np.array(twist_v).tobytes(), k


def test_partials_agree_with_the_matrix_form(pfc):
    rng = np.random.default_rng(20261020)
    worst = worst_rel = 0.0
    for k in range(300):
        args = _random_pair(pfc, rng, k)
        pose, twist = seeds_scalar(*args)
        dp, dt = seeds_matrix(*args)
        bp, sp, bt, st = seeds_bound(*args)
        ep = np.abs(np.array([q.d for q in pose]) - dp)
        et = np.abs(np.array([q.d for q in twist]) - dt)
        assert (ep <= bp).all(), (k, ep, bp)
        assert (et <= bt).all(), (k, et, bt)
        for e, b, s in ((ep, bp, sp), (et, bt, st)):
            on = s > 0
            assert not e[~on].any() and not b[~on].any()
            if on.any():
                worst = max(worst, float((e[on] / b[on]).max()))
                worst_rel = max(worst_rel, float((e[on] / s[on]).max()) / EPS)
                assert (b[on] < 1e-12 * s[on]).all(), (k, (b[on] / s[on]).max())      # a rounding bound, not a loose one
    print(f"over 300 pairs: largest difference / bound {worst:.3f}, largest difference {worst_rel:.2f} eps x sum|terms|")


def test_reference_layout_world_and_null_partials():
    """seeds_reference: with the world on one side the seeds are the other body's; on both sides zero; None is zeros."""
    rng = np.random.default_rng(3)
    n_dir = 3
    x = rng.standard_normal((2, 3, 12)); tw = rng.standard_normal((2, 3, 6))
    dx = rng.standard_normal((2, 3, n_dir, 12)); dtw = rng.standard_normal((2, 3, n_dir, 6))
    bind = [(-1, 1), (2, -1), (-1, -1), (0, 2)]
    ids, sc = [0, 1, 2, 1, 3], [0, 0, 1, 1, 1]
    d_pose, d_twist, d_x = seeds_reference(bind, x, tw, dx, dtw, n_dir, ids, sc)
    assert d_pose.shape == (5, n_dir, 24) and d_twist.shape == (5, n_dir, 6) and d_x.shape == (5, n_dir, 12)
    # body 1 the world: R_r1_r2 = R_w_r2, x_rw_r2 = x_w_b2 -- and so their partials
    assert np.array_equal(d_pose[0, :, 12:21], dx[0, 1, :, :9]) and np.array_equal(d_x[0], dx[0, 1])
    # body 2 the world: x_r2_r1 = x_w_r1, twist = -tw_1, x_rw_r2 constant
    assert np.array_equal(d_pose[1, :, :12], dx[0, 2]) and np.array_equal(d_twist[1], -dtw[0, 2]) and not d_x[1].any()
    assert np.array_equal(d_pose[3, :, :12], dx[1, 2]) and np.array_equal(d_twist[3], -dtw[1, 2])      # the same in scene 1
    assert not d_pose[2].any() and not d_twist[2].any() and not d_x[2].any()                            # the world on both sides
    assert np.array_equal(d_x[4], dx[1, 2]) and d_pose[4].any() and d_twist[4].any()
    # None: the arrays of zeros
    for a, b in ((None, dtw), (dx, None), (None, None)):
        got = seeds_reference(bind, x, tw, a, b, n_dir, ids, sc)
        ref = seeds_reference(bind, x, tw, a if a is not None else np.zeros_like(dx), b if b is not None else np.zeros_like(dtw), n_dir,
                              ids, sc)
        for g, r in zip(got, ref):
            assert g.tobytes() == r.tobytes()
    assert not any(q.any() for q in seeds_reference(bind, x, tw, None, None, n_dir, ids, sc))
    # without ids: item i = instruction i in scene 0
    got = seeds_reference(bind, x, tw, dx, dtw, n_dir)
    assert got[0].shape == (4, n_dir, 24) and np.array_equal(got[2][3], dx[0, 2])
