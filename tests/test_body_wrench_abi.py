"""Applied body wrenches (pfc_body_wrench_device, pfc_body_wrench_dual_device, pfc_radau_set_body_wrenches,
pfc_radau_clear_body_wrenches): the symbols, and the scalar statements of include/pfc.h in Python floats
(scenario.body_wrench_tau, scenario.body_wrench_tau_partials) against formulations that share nothing with them but
scenario.joint_kinematics.  tests/test_gpu_body_wrench.py compares the device with these statements in bytes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import test_kinematics_abi as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = K.EPS
NAMES = [("pfc_body_wrench_device", 18), ("pfc_body_wrench_dual_device", 21), ("pfc_radau_set_body_wrenches", 8),
         ("pfc_radau_clear_body_wrenches", 1), ("pfc_radau_stage_times", 2)]
NV = 8


def test_body_wrench_symbols_are_declared_exported_and_bound(pfc):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfc.h")).read(), flags=re.S)
    for name, n_args in NAMES:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        res, args = pfc._lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, name
    sig = pfc._lib.SIGNATURES
    assert sig["pfc_body_wrench_device"][1][1:7] == [C.c_int] * 6 and sig["pfc_body_wrench_device"][1][7] is C.c_void_p
    assert sig["pfc_body_wrench_dual_device"][1][1:8] == [C.c_int] * 7 and sig["pfc_body_wrench_dual_device"][1][8] is C.c_void_p
    assert sig["pfc_radau_set_body_wrenches"][1][1] is C.c_int and sig["pfc_radau_set_body_wrenches"][1][5] is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", pfc._lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pfc_[a-z_0-9]+)", out))
    assert {name for name, _ in NAMES} <= exported
    M = pfc.scenario.MechanismScenario
    for meth in ("radau_set_body_wrenches", "radau_clear_body_wrenches", "body_wrench_device", "body_wrench_dual_device"):
        assert callable(getattr(M, meth)), meth
    assert callable(pfc.scenario.body_wrench_tau) and callable(pfc.scenario.body_wrench_tau_partials)
    src = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc", "pfc_body_wrench.h")).read().split("#pragma once")[1]
    assert "fma(" not in src and "__shared__" not in src and "atomic" not in src and "__shfl" not in src
    assert "scat_world<T>" in src and "scat_tau<double>" in src and "scat_tau<ScatDual>" in src      # the shared statements


# ---- the mechanism of tests/test_gpu_feedback.py: world -> prismatic z -> revolute y, and an MRP-floating box ---------------------
def arm_box_mech():
    x = np.tile(np.array(K.WORLD_X), (3, 1))
    x[0, 9:] = [0.5, 0.0, 0.3]
    return K.make_mech([-1, 0, -1], [K.PRISMATIC, K.REVOLUTE, K.FLOATING], x, [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]])


def _kin(pfc, mech, q, v):
    return pfc.scenario.joint_kinematics(mech["parent"], mech["joint_type"], mech["x_p_j"], mech["axis"], q, v)


def _random_state(rng):
    q, v = rng.uniform(-1.0, 1.0, NV), rng.uniform(-1.0, 1.0, NV)
    q[2:5] = K._unit(rng) * rng.uniform(0.0, 0.9)          # the box's MRP, |p| < 1
    return q, v


def _wrenches(rng):
    """Four wrenches: both frames on the arm (its path holds coordinates 0 and 1 only) and on the box, offset points."""
    return dict(body=[1, 1, 2, 2], frame=[0, 1, 0, 1], point=rng.uniform(-0.5, 0.5, (4, 3)).tolist(),
                seg_t=[0.0], seg_w=rng.uniform(-2.0, 2.0, (1, 4, 6)).tolist())


def _world_loads(x_w_b, w):
    """Per wrench (r, F, M) in world by matrix products, and their magnitudes (|r|, |F|, |M|) for the bounds."""
    out = []
    for k, b in enumerate(w["body"]):
        R, t = np.asarray(x_w_b[b][:9]).reshape(3, 3, order="F"), np.asarray(x_w_b[b][9:])
        p, l = np.asarray(w["point"][k]), np.asarray(w["seg_w"][0][k])
        r, ar = R @ p + t, np.abs(R) @ np.abs(p) + np.abs(t)
        if w["frame"][k] == 1:
            F, M, aF, aM = R @ l[3:], R @ l[:3], np.abs(R) @ np.abs(l[3:]), np.abs(R) @ np.abs(l[:3])
        else:
            F, M, aF, aM = l[3:], l[:3], np.abs(l[3:]), np.abs(l[:3])
        out.append((r, F, M, ar, aF, aM))
    return out


def _abs_cross(a, b):
    return np.array([a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]])


def _tau_scale(jac, w, loads):
    """Per coordinate the sum of the magnitudes of the products of tau_j = sum_k J_k[j] . [M + r x F; F]."""
    scale = np.zeros(NV)
    for k, b in enumerate(w["body"]):
        _, _, _, ar, aF, aM = loads[k]
        scale += np.abs(jac[b]) @ np.concatenate([aM + _abs_cross(ar, aF), aF])
    return scale


def test_virtual_power_identity(pfc):
    """tau . v = sum_k F_k . (velocity of the application point) + M_k . omega_k, with the point's velocity v_O + omega x r from
    joint_kinematics' twist [omega; v_O] (world, about the origin) and F, M, r from matrix products.  Both sides are sums of
    products of the same magnitudes; the bound is 64 eps times the sum of those magnitudes, computed from the inputs (the longest
    chain of either side has fewer than 64 roundings: 3 + 3 + 6 + n_w + nv per coordinate on the left, the twist's own sums on the
    right)."""
    S = pfc.scenario
    rng = np.random.default_rng(20261021)
    mech = arm_box_mech()
    worst = 0.0
    for case in range(40):
        q, v = _random_state(rng)
        w = _wrenches(rng)
        x_w_b, tw, jac = _kin(pfc, mech, q, v)
        tau = np.array(S.body_wrench_tau(x_w_b.tolist(), jac.tolist(), 0.0, None, **w))
        loads = _world_loads(x_w_b, w)
        lhs, rhs = float(tau @ v), 0.0
        mag = float(_tau_scale(jac, w, loads) @ np.abs(v))
        for k, b in enumerate(w["body"]):
            r, F, M, ar, aF, aM = loads[k]
            om, vo = tw[b][:3], tw[b][3:]
            rhs += float(F @ (vo + np.cross(om, r)) + M @ om)
            mag += float(aF @ (np.abs(vo) + _abs_cross(np.abs(om), ar)) + aM @ np.abs(om))
        assert abs(lhs - rhs) <= 64.0 * EPS * mag, (case, lhs, rhs, mag)
        assert mag > 1.0                                                      # the identity is not 0 = 0
        worst = max(worst, abs(lhs - rhs) / (EPS * mag))
    print("virtual power: worst |lhs - rhs| = %.2f eps x magnitudes" % worst)


def test_partials_of_the_statement_against_central_differences(pfc):
    """body_wrench_tau_partials along every configuration coordinate (dx_w_b and djac from joint_kinematics_partials) against
    central differences of body_wrench_tau through joint_kinematics at h = 2e-3 and 1e-3 -- the rule of test_dynamics_abi's
    derivative check: the finer error lies below h^2 times the magnitude sum of tau's products, and where it is a thousand times
    above the rounding floor eps |terms| / h the two errors have a ratio of 4 within [3.5, 4.5].  A direction along an MRP
    coordinate is scaled by 1/4: dR/dp turns the box at 4 / (1 + |p|^2) rad per unit of p, and the rule's truncation argument is
    for motions whose twist is at most 1."""
    S = pfc.scenario
    rng = np.random.default_rng(7)
    mech = arm_box_mech()
    args = (mech["parent"], mech["joint_type"], mech["x_p_j"], mech["axis"])
    seen = 0
    for case in range(6):
        q, v = _random_state(rng)
        w = _wrenches(rng)
        x_w_b, _, jac = _kin(pfc, mech, q, v)
        scale = _tau_scale(jac, w, _world_loads(x_w_b, w))
        for i in range(NV):
            dq = np.zeros(NV)
            dq[i] = 0.25 if 2 <= i < 5 else 1.0
            dx, _, dJ = S.joint_kinematics_partials(*args, q, v, dq[None, :], None)
            an = np.array(S.body_wrench_tau_partials(x_w_b.tolist(), jac.tolist(), dx[:, 0].tolist(), dJ[:, 0].tolist(), 0.0, None, **w))
            err = []
            for h in (2e-3, 1e-3):
                xp, _, Jp = _kin(pfc, mech, q + h * dq, v)
                xm, _, Jm = _kin(pfc, mech, q - h * dq, v)
                fd = (np.array(S.body_wrench_tau(xp.tolist(), Jp.tolist(), 0.0, None, **w)) -
                      np.array(S.body_wrench_tau(xm.tolist(), Jm.tolist(), 0.0, None, **w))) / (2.0 * h)
                err.append(np.abs(fd - an))
            assert (err[1] <= 1e-6 * scale).all(), (case, i, err[1], scale)
            for j in range(NV):
                if err[1][j] > 1e3 * EPS * scale[j] / 1e-3:
                    seen += 1
                    assert 3.5 <= err[0][j] / err[1][j] <= 4.5, (case, i, j, err[0][j], err[1][j])
    assert seen >= 10


def test_partials_add_to_dtau_in_and_constants_have_none(pfc):
    S = pfc.scenario
    rng = np.random.default_rng(3)
    mech = arm_box_mech()
    q, v = _random_state(rng)
    w = _wrenches(rng)
    x_w_b, _, jac = _kin(pfc, mech, q, v)
    zx, zJ = np.zeros_like(x_w_b).tolist(), np.zeros_like(jac).tolist()
    # a direction that moves nothing: every partial is a zero, and dtau_in comes back
    d0 = S.body_wrench_tau_partials(x_w_b.tolist(), jac.tolist(), zx, zJ, 0.0, None, **w)
    assert all(e == 0.0 for e in d0)
    din = rng.standard_normal(NV).tolist()
    d1 = S.body_wrench_tau_partials(x_w_b.tolist(), jac.tolist(), zx, zJ, 0.0, din, **w)
    assert d1 == din
    # no wrench: tau_in copied, a signed zero survives; None: +0.0
    none = dict(body=[], frame=[], point=[], seg_t=[0.0], seg_w=[[]])
    out = S.body_wrench_tau(x_w_b.tolist(), jac.tolist(), 0.0, [-0.0] * NV, **none)
    assert np.asarray(out).tobytes() == np.full(NV, -0.0).tobytes()
    assert np.asarray(S.body_wrench_tau(x_w_b.tolist(), jac.tolist(), 0.0, None, **none)).tobytes() == np.zeros(NV).tobytes()
    # a wrench on the arm leaves the box's coordinates alone: its Jacobian columns there are +0.0
    arm = dict(body=[1], frame=[1], point=[[0.1, 0.2, 0.3]], seg_t=[0.0], seg_w=[[[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]]])
    out = S.body_wrench_tau(x_w_b.tolist(), jac.tolist(), 0.0, None, **arm)
    assert out[0] != 0.0 and out[1] != 0.0 and all(e == 0.0 for e in out[2:])


@pytest.mark.parametrize("t, seg", [(-5.0, 0), (0.9999999999999999, 0), (1.0, 1), (1.5, 1), (2.0, 2), (9.0, 2)])
def test_a_time_on_a_segment_start_reads_the_new_segment(pfc, t, seg):
    """seg = the number of j >= 1 with seg_t[j] <= t; entry 0 is not read."""
    S = pfc.scenario
    x_w_b = [K.WORLD_X]
    jac = [[[0.0, 0.0, 0.0, 1.0, 0.0, 0.0]]]                                  # one prismatic coordinate along x
    w = dict(body=[0], frame=[0], point=[[0.0, 0.0, 0.0]], seg_t=[123.0, 1.0, 2.0],
             seg_w=[[[0.0, 0.0, 0.0, 10.0, 0.0, 0.0]], [[0.0, 0.0, 0.0, 20.0, 0.0, 0.0]], [[0.0, 0.0, 0.0, 30.0, 0.0, 0.0]]])
    assert S.body_wrench_tau(x_w_b, jac, t, None, **w) == [10.0 * (seg + 1)]
    assert S.body_wrench_tau(x_w_b, jac, t, [0.5], **w) == [0.5 + 10.0 * (seg + 1)]
