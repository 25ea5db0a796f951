"""pfc_set_instruction_bodies, pfc_items_from_bodies[_device], pfc_eval_bodies[_device]: the C ABI, and the scalar statement of the
kernel's arithmetic (csrc/pfc_bodies.h) that tests/test_gpu_items_from_bodies.py compares bytes with -- without a device.

The statement is checked here against scenario.relative_pose / relative_twist (NumPy matrix products).  Bound, elementwise: both
sides evaluate a 3-term dot product sum_k a_k b_k with 3 products and at most 3 additions (the translation / cross term included),
so each is within gamma_3 = 3u / (1 - 3u) (u = eps / 2) of the exact sum, times sum |a_k| |b_k|, whatever the order and whether or
not BLAS contracts a product into an fma; two such values differ by at most 2 gamma_3 < 4 eps times that sum.  Where an operand was
itself computed (t2w in t21 and lin, R12 and t21 in t12, ang in lin), the two sides' operands differ by their own bound, which is
carried through the product: that is `items_bound`."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = (("pfc_set_instruction_bodies", 4), ("pfc_items_from_bodies_device", 14), ("pfc_items_from_bodies", 13),
         ("pfc_eval_bodies_device", 18), ("pfc_eval_bodies", 17))
EPS = float(np.finfo(np.float64).eps)
WORLD_X = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


def items_scalar(x1, tw1, x2, tw2):
    """pose (24) and twist (6) of one item from the world pose (12: R column-major, t) and twist (6) of body 1 and body 2: Python
    floats, every dot product summed left to right, no fma -- the statements of bodies_item in csrc/pfc_bodies.h."""
    x1, tw1, x2, tw2 = ([float(v) for v in a] for a in (x1, tw1, x2, tw2))
    pose, twist = [0.0] * 24, [0.0] * 6
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


def items_reference(bind, x_w_b, twist_w_b, ins_ids=None, scene=None):
    """The five outputs of pfc_items_from_bodies by items_scalar.  bind (n_ins,2); x_w_b (n_scene,n_body,12); twist_w_b
    (n_scene,n_body,6); ins_ids / scene (n,) or None."""
    bind = np.asarray(bind)
    n_body = x_w_b.shape[1]
    n = len(ins_ids) if ins_ids is not None else (len(scene) if scene is not None else len(bind))
    pose, twist, x_w_r2 = np.zeros((n, 24)), np.zeros((n, 6)), np.zeros((n, 12))
    body_1, body_2 = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for i in range(n):
        b1, b2 = (int(v) for v in bind[int(ins_ids[i]) if ins_ids is not None else i])
        sc = int(scene[i]) if scene is not None else 0
        st = lambda b: (x_w_b[sc, b], twist_w_b[sc, b]) if b >= 0 else (WORLD_X, [0.0] * 6)
        (x1, tw1), (x2, tw2) = st(b1), st(b2)
        pose[i], twist[i] = items_scalar(x1, tw1, x2, tw2)
        x_w_r2[i] = x2
        off = sc * n_body if scene is not None else 0
        body_1[i] = b1 + off if b1 >= 0 else -1
        body_2[i] = b2 + off if b2 >= 0 else -1
    return pose, twist, x_w_r2, body_1, body_2


def _abs_cross(a, b):
    return np.array([a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]])


def items_bound(x1, tw1, x2, tw2):
    """Elementwise bound (pose 24, twist 6) on the difference of two evaluations of the item's expressions in Float64: 4 eps times
    the sum of |a| |b| over the products of each entry, an operand's own bound carried through where it was computed."""
    x1, tw1, x2, tw2 = (np.abs(np.asarray(a, dtype=np.float64)) for a in (x1, tw1, x2, tw2))
    A2 = x2[:9].reshape(3, 3)                    # |R2w| (row-major reading of the column-major R_w2)
    A1 = x1[:9].reshape(3, 3, order="F")         # |R_w1|
    e = 4 * EPS
    b_t2w = e * (A2 @ x2[9:])
    t2w = A2 @ x2[9:]
    b_R21 = e * (A2 @ A1)
    t21 = A2 @ x1[9:] + t2w
    b_t21 = e * t21 + b_t2w
    R21 = A2 @ A1
    b_t12 = e * (R21.T @ t21) + b_R21.T @ t21 + R21.T @ b_t21
    d = tw2 + tw1                                # |tw_2 - tw_1| <= |tw_2| + |tw_1|
    ang = A2 @ d[:3]
    b_ang = e * ang
    b_lin = e * (A2 @ d[3:] + _abs_cross(t2w, ang)) + _abs_cross(b_t2w, ang) + _abs_cross(t2w, b_ang)
    bp = np.concatenate([b_R21.reshape(-1, order="F"), b_t21, b_R21.T.reshape(-1, order="F"), b_t12])
    return bp, np.concatenate([b_ang, b_lin])


def test_bodies_symbols_are_declared_exported_and_bound(pfc):
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
    assert L.pfc_set_instruction_bodies.argtypes[1:] == [C.c_int] * 3
    for name in ("pfc_items_from_bodies_device", "pfc_items_from_bodies", "pfc_eval_bodies_device", "pfc_eval_bodies"):
        a = getattr(L, name).argtypes
        assert a[1] is C.c_int and a[4] is C.c_int and a[5] is C.c_int, name      # n_items, n_scene, n_body
    M = pfc.scenario.MechanismScenario
    for meth in ("set_instruction_bodies", "items_from_bodies", "force_all_elastic_intersections_bodies", "items_from_bodies_device",
                 "eval_bodies_device"):
        assert callable(getattr(M, meth)), meth


def test_bodies_kernel_is_built_from_its_header(pfc):
    srcs = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "_lib.py")).read()
    assert '"pfc_bodies.h"' in srcs      # a change of the kernel rebuilds the library
    src = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc", "pfc_hip.hip")).read()
    assert '#include "pfc_bodies.h"' in src


def test_scalar_statement_agrees_with_relative_pose_and_twist(pfc):
    S, Cf = pfc.scenario, pfc.configs
    rng = np.random.default_rng(20260107)
    worst = 0.0
    for k in range(200):
        R1, R2 = Cf.random_rotation(rng), Cf.random_rotation(rng)
        t1, t2 = (rng.uniform(-1, 1, 3) * rng.uniform(0, 10) for _ in range(2))
        tw1, tw2 = rng.standard_normal(6), rng.standard_normal(6)
        if k % 10 == 0:      # the world on one side, as the kernel states it
            R1, t1, tw1 = np.eye(3), np.zeros(3), np.zeros(6)
        if k % 10 == 5:
            R2, t2, tw2 = np.eye(3), np.zeros(3), np.zeros(6)
        x1 = np.concatenate([R1.reshape(-1, order="F"), t1]); x2 = np.concatenate([R2.reshape(-1, order="F"), t2])
        pose, twist = items_scalar(x1, tw1, x2, tw2)
        bp, bt = items_bound(x1, tw1, x2, tw2)
        dp = np.abs(np.array(pose) - S.relative_pose(R1, t1, R2, t2))
        dt = np.abs(np.array(twist) - S.relative_twist(R2, t2, tw1, tw2))
        assert (dp <= bp).all(), (k, dp, bp)
        assert (dt <= bt).all(), (k, dt, bt)
        worst = max(worst, float((dp / np.maximum(bp, 1e-300)).max()), float((dt / np.maximum(bt, 1e-300)).max()))
    print(f"largest difference / bound over 200 pairs: {worst:.3f}")
    assert (bp < 1e-12).all() and (bt < 1e-12).all()      # the bound is a rounding bound, not a loose one


def test_reference_layout_and_world_body():
    """items_reference: the world gives the other body's pose (inverted on side 2), ids are offset by scene."""
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 3, 12)); tw = rng.standard_normal((2, 3, 6))
    bind = [(-1, 1), (2, -1), (-1, -1)]
    pose, twist, x_w_r2, b1, b2 = items_reference(bind, x, tw, ins_ids=[0, 1, 2, 1], scene=[0, 0, 1, 1])
    assert np.array_equal(pose[1, :12], x[0, 2]) and np.array_equal(twist[1], -tw[0, 2])      # body 2 the world: x_r2_r1 = x_w_r1
    assert np.array_equal(pose[0, 12:21], x[0, 1, :9])                                      # body 1 the world: R_r1_r2 = R_w_r2
    assert np.array_equal(pose[2], np.array(WORLD_X * 2)) and not twist[2].any()
    assert np.array_equal(x_w_r2[0], x[0, 1]) and np.array_equal(x_w_r2[1], WORLD_X)
    assert b1.tolist() == [-1, 2, -1, 5] and b2.tolist() == [1, -1, -1, -1]
