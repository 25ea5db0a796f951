"""The gripper program on the device (pfc_radau_program_device, pfc_radau_set_program, pfc_radau_clear_program,
pfc_radau_program_state; kernel k_radau_program): bytes against the scalar statement (scenario.gripper_program_step fed the angle the
device stored; tests/test_radau_program_abi.py), the device's atan2 against a 40-digit one, and the device route against the host
route, integrate_scenario_radau(discrete_controller=(gripper_program_fn(..), dt, t_last0)), on configs.pencil_gripper().
Every handle runs with option fixed_order: bytes are compared."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_radau as G
import test_gpu_radau_control as T
from test_gpu_items_from_bodies import GUARD, Guarded, _dev, _torch

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
INF = float("inf")
TAU_SOFT, TAU_HARD = 0.3, 2.5
ATAN2_ULP = 6.0      # OpenCL's full-profile bound for double atan2, the only published one (the cos / sin test uses its 4)
_bits = G._bits


def _rotation(axis, theta):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(theta) * K + (1.0 - math.cos(theta)) * (K @ K)


def _fill(g, a):
    a = np.ascontiguousarray(a).reshape(-1)
    g.t[GUARD:GUARD + a.size] = _dev(a)


@pytest.fixture(scope="module")
def scen(pfc):
    m = pfc.configs.build_scenario(pfc.configs.c1_boxes())      # the part needs a handle, not a mechanism
    yield m
    m.close()


# ---- 1. the part ------------------------------------------------------------------------------------------------------------------
KINDS = ["not due", "first fire", "tie", "tie + 1 ulp", "finite below", "finite above", "last, dt 0", "retired", "parked"]


@pytest.mark.parametrize("n_scene", [9, 70])
@pytest.mark.parametrize("nv,n_act,n_grip", [(1, 1, 0), (10, 4, 2), (64, 64, 64)])
def test_program_part_is_the_statement_in_bytes(pfc, scen, nv, n_act, n_grip, n_scene):
    """Scene s is of kind KINDS[s % 9]; 70 scenes cross a wave.  Three instructions per scene, three bodies, body 1 watched.  The
    expected values come from gripper_program_step fed the angle the device stored; everything else is compared bit for bit."""
    torch = _torch()
    S = pfc.scenario
    n_ins, n_body, body = 3, 3, 1
    rng = np.random.default_rng(1000 * nv + n_scene)
    grip = rng.permutation(nv)[:n_grip].astype(np.int32) if n_grip < nv else rng.permutation(nv).astype(np.int32)
    theta = rng.uniform(0.3, math.pi - 0.3, n_scene)
    x_w_b = rng.standard_normal((n_scene, n_body, 12))
    for s in range(n_scene):
        for b in range(n_body):
            x_w_b[s, b, :9] = _rotation(rng.standard_normal(3), theta[s] if b == body else rng.uniform(0, math.pi)).reshape(-1, order="F")
    prog_dt = np.full((n_scene, n_ins), INF)
    prog_slip = np.full((n_scene, n_ins), INF)
    prog_q = rng.standard_normal((n_scene, n_ins, n_act))
    t, t_last = np.zeros(n_scene), np.zeros(n_scene)
    cursor = np.zeros((n_scene, 2), dtype=np.int32)
    pstate = np.zeros((n_scene, 4))
    istate = np.zeros((n_scene, 8), dtype=np.int32)
    for s in range(n_scene):
        kind, lap = KINDS[s % 9], s // 9
        pstate[s] = [0.5, 0.125 * lap, 0.77, 1.5]                           # t0, rot_0, the last angle, the last tau_grip
        cursor[s] = [0, lap]
        t[s] = 0.75 + lap
        t_last[s] = t[s] if lap % 2 == 0 else t[s] - 0.004                 # equality fires, as the controller's clock does
        if kind == "not due":
            t_last[s] = math.nextafter(t[s], INF)
            prog_dt[s, 0] = 0.0                                            # it would pop
        elif kind == "first fire":
            pstate[s] = [INF, INF, 0.0, 0.0]
            prog_dt[s, 0], prog_slip[s, 0] = 0.0, -INF                     # t - t0 = 0 is not above 0
        elif kind in ("tie", "tie + 1 ulp"):
            pstate[s, 0] = t[s] - 0.25
            prog_dt[s, 0] = 0.25
            assert t[s] - pstate[s, 0] == 0.25
            prog_slip[s, 0] = 0.0 if lap % 2 == 0 else -0.0
            prog_slip[s, 1] = INF if lap % 2 == 0 else 0.3                  # a pop onto a finite slip: rot_0 = angle, soft
            if kind == "tie + 1 ulp":
                t[s] = math.nextafter(t[s], INF)
        elif kind in ("finite below", "finite above"):
            cursor[s, 0] = 1
            prog_slip[s, 1] = 0.2
            pstate[s, 1] = theta[s] - 0.1 if kind == "finite below" else theta[s] + 0.4
            if lap % 2:
                pstate[s, 1] = theta[s] + 0.1 if kind == "finite below" else theta[s] - 0.4
        elif kind == "last, dt 0":
            cursor[s, 0] = n_ins - 1
            prog_dt[s, n_ins - 1], prog_slip[s, n_ins - 1] = 0.0, (0.2 if lap % 2 == 0 else -0.1)
            pstate[s, 1] = INF if lap % 2 == 0 else theta[s]               # rot_0 = +inf, or a negative slip: hard
        else:
            prog_dt[s, 0] = 0.0
            istate[s, 5 if kind == "retired" else 7] = 5 if kind == "retired" else 1
    seg_q0, seg_ff0 = rng.standard_normal((n_scene, n_act)), rng.standard_normal((n_scene, nv))
    g_cur, g_st = Guarded(n_scene, 2, True), Guarded(n_scene, 4)
    g_q, g_ff = Guarded(n_scene, n_act), Guarded(n_scene, nv)
    for g, a in ((g_cur, cursor), (g_st, pstate), (g_q, seg_q0), (g_ff, seg_ff0)):
        _fill(g, a)
    ins = [_dev(a) for a in (grip, prog_dt, prog_q, prog_slip, t, t_last, x_w_b, istate)]
    p = [a.data_ptr() if a.numel() else 0 for a in ins]
    scen.radau_program_device(n_scene, n_body, nv, n_act, n_ins, body, n_grip, p[0], TAU_SOFT, TAU_HARD, p[1], p[2], p[3], p[4], p[5], p[6],
                              p[7], g_cur.ptr, g_st.ptr, g_q.ptr, g_ff.ptr)
    torch.cuda.synchronize()
    got_cur, got_st = g_cur.rows().reshape(n_scene, 2), g_st.rows().reshape(n_scene, 4)
    got_q, got_ff = g_q.rows().reshape(n_scene, n_act), g_ff.rows().reshape(n_scene, nv)
    e_cur, e_st, e_q, e_ff = cursor.copy(), pstate.copy(), seg_q0.copy(), seg_ff0.copy()
    seen, margin = {}, INF
    for s in range(n_scene):
        kind = KINDS[s % 9]
        if kind in ("not due", "retired", "parked"):
            assert t_last[s] <= t[s] or kind == "not due"
            continue
        angle = float(got_st[s, 2])
        assert abs(angle - theta[s]) < 1e-13, (s, angle, theta[s])           # the watched body's, not a neighbour's
        rec = dict(cursor=int(cursor[s, 0]), pops=int(cursor[s, 1]), t0=pstate[s, 0], rot_0=pstate[s, 1], angle=pstate[s, 2], tau_grip=pstate[s, 3])
        new, q_row, tau_grip = S.gripper_program_step(rec, t[s], angle, prog_dt[s].tolist(), prog_q[s].tolist(), prog_slip[s].tolist(),
                                                      TAU_SOFT, TAU_HARD)
        e_cur[s] = [new["cursor"], new["pops"]]
        e_st[s] = [new["t0"], new["rot_0"], new["angle"], new["tau_grip"]]
        e_q[s] = q_row
        e_ff[s, grip] = tau_grip
        sl = prog_slip[s, new["cursor"]]
        if math.isfinite(sl) and sl != 0.0 and math.isfinite(new["rot_0"]):
            margin = min(margin, abs(abs(angle - new["rot_0"]) - sl))
        seen.setdefault(kind, []).append((new["cursor"] - rec["cursor"], tau_grip))
    assert margin > 1e-9                                                   # no finite-slip decision of these inputs hinges on a rounding
    assert seen["first fire"][0] == (0, 0.0) and seen["tie"][0] == (0, TAU_HARD) and seen["tie + 1 ulp"][0] == (1, TAU_SOFT)
    assert seen["finite below"][0] == (0, TAU_SOFT) and seen["finite above"][0] == (0, TAU_HARD) and seen["last, dt 0"][0] == (0, TAU_HARD)
    if n_scene > 9:
        assert seen["tie"][1] == (0, TAU_HARD) and seen["tie + 1 ulp"][1] == (1, TAU_SOFT) and seen["last, dt 0"][1] == (0, TAU_HARD)
    assert got_cur.tolist() == e_cur.tolist()
    assert _bits(got_st) == _bits(e_st), np.argwhere(got_st != e_st)[:4]
    assert _bits(got_q) == _bits(e_q) and _bits(got_ff) == _bits(e_ff)


# ---- 2. the device's angle --------------------------------------------------------------------------------------------------------
def test_device_angle_is_within_the_published_atan2_bound(pfc, scen):
    """130 rotations: angles k pi / 127 about random axes, k = 0 .. 127, then the identity and a half turn as exact matrices.  Against
    mpmath.atan2 (40 digits) of the statement's own s and w in Python floats; the bound is OpenCL's full-profile 6 ulp.
    Measured on an MI355X: 1.090 ulp at the worst (the figure is printed; DESIGN.md holds it)."""
    import mpmath
    torch = _torch()
    S = pfc.scenario
    rng = np.random.default_rng(77)
    mats = [_rotation(rng.standard_normal(3), math.pi * k / 127) for k in range(128)] + [np.eye(3), np.diag([1.0, -1.0, -1.0])]
    n = len(mats)
    x_w_b = np.zeros((n, 1, 12))
    for s, R in enumerate(mats):
        x_w_b[s, 0, :9] = R.reshape(-1, order="F")
    g_cur, g_st = Guarded(n, 2, True), Guarded(n, 4)
    _fill(g_cur, np.zeros((n, 2), dtype=np.int32)); _fill(g_st, np.tile([INF, INF, 0.0, 0.0], (n, 1)))
    d = [_dev(a) for a in (np.full((n, 1), INF), np.full((n, 1), -INF), np.zeros(n), np.zeros(n), x_w_b)]
    scen.radau_program_device(n, 1, 1, 0, 1, 0, 0, 0, TAU_SOFT, TAU_HARD, d[0].data_ptr(), 0, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                              d[4].data_ptr(), 0, g_cur.ptr, g_st.ptr, 0, 0)
    torch.cuda.synchronize()
    got = g_st.rows().reshape(n, 4)[:, 2]
    mpmath.mp.dps = 40
    worst = 0.0
    for s in range(n):
        sv, wv = S.rotation_angle_terms(x_w_b[s, 0, :9].tolist())
        ref = mpmath.atan2(mpmath.mpf(sv), mpmath.mpf(wv))
        err = abs(mpmath.mpf(float(got[s])) - ref) / mpmath.mpf(math.ulp(float(ref))) if ref != 0 else (0.0 if got[s] == 0.0 else INF)
        worst = max(worst, float(err))
        assert 0.0 <= got[s] <= math.pi
    print("largest atan2 error on the device: %.3f ulp over %d rotations" % (worst, n))
    assert got[n - 2] == 0.0 and got[n - 1] == math.pi
    assert worst <= ATAN2_ULP


# ---- 3. device route = host route on the pencil scene -----------------------------------------------------------------------------
# The controller's period in this test.  With the pad and plane contacts of this scene the integrator's steps are 1e-5 .. 5e-3 (it
# starts from h_max = 0.01, fails and restarts at a hundredth; measured: 25 batch steps reach t = 0.0085), so pencil_gripper()'s own
# period, 0.01, does not come round once in 25 steps; with 2e-4 the controller is due at most steps and not at all of them.
PENCIL_DT = 2.0e-4


def _short_program(d):
    """Two scenes: the first instructions of pencil_gripper() with durations of 2 - 5 controller periods, differing per scene; the
    slips run through -inf, +inf, 0, +inf, 0: every non-finite class is reached within three pops."""
    p, dt = d["program"], PENCIL_DT
    periods = np.array([[2, 3, 2, 4, 5, INF], [3, 2, 4, 2, 3, INF]])
    return periods * dt, np.broadcast_to(p["prog_q"][[0, 1, 2, 3, 4, 5]], (2, 6, 4)).copy(), np.tile([-INF, INF, 0.0, INF, 0.0, INF], (2, 1))


def _pencil_run(pfc, route, max_steps=25):
    d = pfc.configs.pencil_gripper()
    m = pfc.configs.build_gripper_scenario(d, fixed_order=True)
    r, c, p = d["radau"], d["controller"], d["program"]
    assert m.radau_configure(2, [0, 1, 2, 3], h0=r["h0"], h_max=r["h_max"], h_min=r["h_min"]) == 20
    x0 = np.tile(d["x0"], (2, 1))
    x0[1, 0] = 0.09                                                         # the second scene starts a centimetre lower
    m.radau_set_state(x0)
    prog_dt, prog_q, prog_slip = _short_program(d)
    if route == "device":
        m.radau_set_controller(c["act"], c["kp"], c["kd"], PENCIL_DT, [0.0], c["seg_q"], c["seg_ff"], c["a_max"], c["t_last0"])
        m.radau_set_program(p["body"], p["grip"], p["tau_soft"], p["tau_hard"], prog_dt, prog_q, prog_slip)
        out = m.integrate_scenario_radau(INF, max_steps)
        st, rec, tau = m.radau_controller_state(), m.radau_program_state(), m.radau_get_tau()[0]
    else:
        fn = m.gripper_program_fn(c["act"], c["kp"], c["kd"], c["seg_ff"], p["body"], p["grip"], p["tau_soft"], p["tau_hard"], prog_dt, prog_q,
                                  prog_slip, c["a_max"])
        out = m.integrate_scenario_radau(INF, max_steps, discrete_controller=(fn, PENCIL_DT, c["t_last0"]))
        st, tau = m.radau_host_controller_state(), m.radau_host_tau()
        rec = {k: np.array([r_[k] for r_ in fn.records]) for k in fn.records[0]}
    m.close()
    return out, st, rec, tau, prog_slip


def test_device_route_is_the_host_route_on_the_pencil_scene(pfc):
    (dev, dev_st, dev_rec, dev_tau, prog_slip), (host, host_st, host_rec, host_tau, _) = _pencil_run(pfc, "device"), _pencil_run(pfc, "host")
    print("pops", dev_rec["pops"].tolist(), "cursor", dev_rec["cursor"].tolist(), "fires", dev_st[1].tolist(), "t end", [float(tr[0][-1]) for tr in dev],
          "tau_grip", dev_rec["tau_grip"].tolist())
    for s in range(2):
        assert dev[s][0].size == host[s][0].size == 26
        assert _bits(dev[s][0]) == _bits(host[s][0]), s
        assert _bits(dev[s][1]) == _bits(host[s][1]), (s, np.abs(dev[s][1] - host[s][1]).max())
        assert dev_rec["pops"][s] >= 3
        reached = set(prog_slip[s, :dev_rec["cursor"][s] + 1].tolist())
        assert {-INF, 0.0, INF} <= reached, reached
    assert _bits(dev_st[0]) == _bits(host_st[0]) and dev_st[1].tolist() == host_st[1].tolist()
    assert dev_rec["cursor"].tolist() == host_rec["cursor"].tolist() and dev_rec["pops"].tolist() == host_rec["pops"].tolist()
    assert _bits(dev_rec["t0"]) == _bits(host_rec["t0"].astype(np.float64)) and _bits(dev_rec["tau_grip"]) == _bits(host_rec["tau_grip"].astype(np.float64))
    assert _bits(dev_tau) == _bits(host_tau), np.abs(dev_tau - host_tau).max()
    for key in ("rot_0", "angle"):      # host math.atan2 against the device's: the bound of the angle test
        a, b = dev_rec[key], host_rec[key].astype(np.float64)
        assert np.isfinite(a).all() and (np.abs(a - b) <= ATAN2_ULP * np.array([math.ulp(v) for v in b])).all(), (key, a, b)


# ---- 4. chained = parts -----------------------------------------------------------------------------------------------------------
SLIDER_X0 = np.array([[T.R + 1e-3, 0.0, 0.0, 0.0], [T.R + 2e-3, 0.01, 0.0, 0.0]])
SLIDER_DT = 2.0e-4      # below the first steps (h0 = 1e-4, doubling): the controller is due at most tops, not at all of them
SLIDER_CTL = dict(act=[0, 1], kp=[400.0, 10.0], kd=[40.0, 1.0], dt=SLIDER_DT, seg_t=[0.0], seg_q=[[T.R, 0.0]], seg_ff=[[0.1, 0.0]], a_max=[2.0, INF],
                  t_last0=0.0)
SLIDER_PROG = dict(body=1, grip=[1], tau_soft=0.03, tau_hard=0.25, prog_dt=[[0.0005, 0.001, INF], [0.001, 0.0005, INF]],
                   prog_q=[[[T.R, 0.0], [T.R - 1e-3, 0.01], [T.R + 1e-3, 0.0]]] * 2, prog_slip=[[-INF, 0.0, INF], [INF, -INF, 0.0]])


def _slider2(pfc):
    m = T._slider(pfc, two=True)
    assert m.radau_configure(2, [0]) == 4
    m.radau_set_state(SLIDER_X0)
    return m


def test_chained_step_is_the_parts(pfc):
    """Six batch steps of a handle with a controller and a program (A) against the same steps assembled from the parts: per step
    pfc_kinematics_device, pfc_radau_program_device, pfc_dynamics_device and pfc_radau_control_device on caller buffers at the
    committed (q, v, t), then the step of a handle without a controller (B) given that tau.  State, rule state, tau, the clock,
    the counters, the records: the same bytes after every step."""
    torch = _torch()
    A, B = _slider2(pfc), _slider2(pfc)
    A.radau_set_controller(**SLIDER_CTL)
    A.radau_set_program(**SLIDER_PROG)
    ns, nb, nv, na, ni = 2, 2, 2, 2, 3
    c, p = SLIDER_CTL, SLIDER_PROG
    d = {k: _dev(np.asarray(v, dtype=np.float64)) for k, v in dict(kp=c["kp"], kd=c["kd"], a_max=c["a_max"], seg_t=np.zeros((ns, 1)), prog_dt=p["prog_dt"],
                                                                   prog_q=p["prog_q"], prog_slip=p["prog_slip"]).items()}
    act, grip = _dev(np.asarray(c["act"], dtype=np.int32)), _dev(np.asarray(p["grip"], dtype=np.int32))
    seg_q, seg_ff = _dev(np.tile(np.asarray(c["seg_q"]), (ns, 1))), _dev(np.tile(np.asarray(c["seg_ff"]), (ns, 1)))
    t_last, fires = _dev(np.zeros(ns)), _dev(np.zeros(ns, dtype=np.int32))
    cursor, pstate = _dev(np.zeros((ns, 2), dtype=np.int32)), _dev(np.tile([INF, INF, 0.0, 0.0], (ns, 1)))
    tau = _dev(np.zeros((3 * ns, nv)))
    x_w_b, tw, H, cc = (_dev(np.zeros(k)) for k in (ns * nb * 12, ns * nb * 6, ns * nv * nv, ns * nv))
    pops = 0
    for step in range(6):
        x, t = B.radau_get_state()
        q, v, tt = _dev(x[:, :nv].copy()), _dev(x[:, nv:2 * nv].copy()), _dev(t)
        B.kinematics_device(ns, q.data_ptr(), v.data_ptr(), x_w_b.data_ptr(), tw.data_ptr(), 0)
        B.radau_program_device(ns, nb, nv, na, ni, p["body"], 1, grip.data_ptr(), p["tau_soft"], p["tau_hard"], d["prog_dt"].data_ptr(),
                               d["prog_q"].data_ptr(), d["prog_slip"].data_ptr(), tt.data_ptr(), t_last.data_ptr(), x_w_b.data_ptr(), 0,
                               cursor.data_ptr(), pstate.data_ptr(), seg_q.data_ptr(), seg_ff.data_ptr())
        B.dynamics_device(ns, q.data_ptr(), v.data_ptr(), x_w_b.data_ptr(), tw.data_ptr(), 0, H.data_ptr(), cc.data_ptr())
        B.radau_control_device(ns, nv, nv, na, 1, c["dt"], act.data_ptr(), d["kp"].data_ptr(), d["kd"].data_ptr(), d["a_max"].data_ptr(),
                               d["seg_t"].data_ptr(), seg_q.data_ptr(), seg_ff.data_ptr(), tt.data_ptr(), q.data_ptr(), v.data_ptr(), H.data_ptr(),
                               cc.data_ptr(), 0, t_last.data_ptr(), fires.data_ptr(), tau.data_ptr())
        torch.cuda.synchronize()
        tau_h = tau.cpu().numpy().reshape(3, ns, nv)
        B.radau_set_tau(tau_h[0])
        ra, rb = A.radau_step(), B.radau_step()
        assert ra["flags"].tolist() == rb["flags"].tolist() == [0, 0]
        assert T._snapshot(A) == T._snapshot(B), step
        assert _bits(A.radau_get_tau()) == _bits(tau_h), step
        st, rec = A.radau_controller_state(), A.radau_program_state()
        assert _bits(st[0]) == _bits(t_last.cpu().numpy()) and st[1].tolist() == fires.cpu().numpy().tolist()
        cur, ps = cursor.cpu().numpy(), pstate.cpu().numpy()
        assert rec["cursor"].tolist() == cur[:, 0].tolist() and rec["pops"].tolist() == cur[:, 1].tolist()
        assert _bits(np.stack([rec["t0"], rec["rot_0"], rec["angle"], rec["tau_grip"]], axis=1)) == _bits(ps), step
        pops = int(cur[:, 1].sum())
    print("pops in six steps:", pops, "fires:", fires.cpu().numpy().tolist())
    assert pops >= 2                                                       # the program moved: the segment the law read was rewritten
    A.close(); B.close()


# ---- 5. lifetime and refusals -----------------------------------------------------------------------------------------------------
def test_lifetime_and_refusals(pfc):
    import ctypes as C
    L = pfc._lib
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    nan = float("nan")

    def refused(call, status, word):
        with pytest.raises(L.PFCError) as e:
            call()
        assert e.value.status == status and word in str(e.value), str(e.value)

    m = T._slider(pfc, two=True)
    refused(lambda: m.radau_set_program(**SLIDER_PROG), L.ERR_STATE, "pfc_radau_configure")
    refused(lambda: m.radau_program_state(), L.ERR_STATE, "pfc_radau_configure")
    assert m.radau_configure(2, [0]) == 4
    m.radau_set_state(SLIDER_X0)
    refused(lambda: m.radau_set_program(**SLIDER_PROG), L.ERR_STATE, "without a controller")
    m.radau_set_controller(**dict(SLIDER_CTL, seg_t=[0.0, 1.0], seg_q=[[T.R, 0.0]] * 2, seg_ff=[[0.1, 0.0]] * 2))
    refused(lambda: m.radau_set_program(**SLIDER_PROG), L.ERR_BAD_ARG, "n_seg = 2")
    m.radau_set_controller(**dict(SLIDER_CTL, seg_ff=None))
    refused(lambda: m.radau_set_program(**SLIDER_PROG), L.ERR_BAD_ARG, "no seg_ff block")
    refused(lambda: m.radau_program_state(), L.ERR_STATE, "without a program")
    m.radau_set_controller(**SLIDER_CTL)
    m.radau_set_program(**SLIDER_PROG)
    rec = m.radau_program_state()
    assert rec["cursor"].tolist() == rec["pops"].tolist() == [0, 0] and rec["t0"].tolist() == rec["rot_0"].tolist() == [INF, INF]
    assert rec["angle"].tolist() == rec["tau_grip"].tolist() == [0.0, 0.0]
    for _ in range(5):
        m.radau_step()

    def everything():
        st, rec = m.radau_controller_state(), m.radau_program_state()
        return T._snapshot(m) + _bits(st[0]) + _bits(st[1]) + b"".join(_bits(rec[k]) for k in sorted(rec)) + _bits(m.radau_get_tau())

    before = everything()
    assert m.radau_program_state()["pops"].sum() >= 1 and np.isfinite(m.radau_program_state()["t0"]).all()
    bad = [(dict(body=2), "body"), (dict(body=-1), "body"), (dict(grip=[5]), "not one of"), (dict(grip=[1, 1]), "repeated"),
           (dict(grip=[0, 1, 0]), "n_grip"), (dict(tau_soft=nan), "tau_soft"), (dict(tau_hard=INF), "tau_hard"),
           (dict(prog_q=[[[T.R, 0.0], [nan, 0.0], [T.R, 0.0]]] * 2), "setpoint"), (dict(prog_q=[[[T.R, INF]] * 3] * 2), "setpoint"),
           (dict(prog_dt=[0.1, -1e-9, INF]), "prog_dt"), (dict(prog_dt=[0.1, nan, INF]), "prog_dt"), (dict(prog_slip=[0.0, nan, INF]), "prog_slip")]
    for change, word in bad:
        refused(lambda: m.radau_set_program(**dict(SLIDER_PROG, **change)), L.ERR_BAD_ARG, word)
        assert everything() == before, (change, word)
    one, gi = np.ones(16), np.ones(2, dtype=np.int32)
    rc = L.lib().pfc_radau_set_program(m._h, 1, 1, gi.ctypes.data_as(ip), 0.1, 0.2, 0, *[one.ctypes.data_as(dp)] * 3)
    assert rc == L.ERR_BAD_ARG and "n_ins" in L.lib().pfc_last_error(m._h).decode() and everything() == before
    # the part
    g = [Guarded(1, 2, True), Guarded(1, 4), Guarded(1, 2), Guarded(1, 2)]
    d_, di = _dev(np.ones(32)), _dev(np.zeros(8, dtype=np.int32))
    a = [d_.data_ptr()] * 6 + [0]
    for (n_body, nv, n_act, n_ins, body, n_grip, ts), word in (((2, 65, 1, 1, 0, 1, 0.1), "PFC_MAX_NV_SOLVE"), ((2, 0, 0, 1, 0, 0, 0.1), "PFC_MAX_NV_SOLVE"),
                                                             ((2, 2, 3, 1, 0, 1, 0.1), "n_act"), ((2, 2, 1, 0, 0, 1, 0.1), "n_ins"),
                                                             ((2, 2, 1, 1, 2, 1, 0.1), "body"), ((2, 2, 1, 1, -1, 1, 0.1), "body"),
                                                             ((2, 2, 1, 1, 0, 3, 0.1), "n_grip"), ((2, 2, 1, 1, 0, 1, nan), "tau_soft")):
        refused(lambda: m.radau_program_device(1, n_body, nv, n_act, n_ins, body, n_grip, di.data_ptr(), ts, 0.2, *a, *[o.ptr for o in g]),
                L.ERR_BAD_ARG, word)
    refused(lambda: m.radau_program_device(1, 2, 2, 1, 1, 0, 1, di.data_ptr(), 0.1, 0.2, *a, g[0].ptr, 0, g[2].ptr, g[3].ptr), L.ERR_BAD_ARG,
            "null buffer")
    _torch().cuda.synchronize()
    assert all(o.untouched() for o in g)
    assert everything() == before
    # the previous program is still in force
    pops = m.radau_program_state()["pops"].copy()
    for _ in range(12):
        m.radau_step()
    assert (m.radau_program_state()["pops"] > pops).any()
    # set_state keeps the program and resets the records
    m.radau_set_state(SLIDER_X0, [0.5, 0.7])
    rec = m.radau_program_state()
    assert rec["cursor"].tolist() == rec["pops"].tolist() == [0, 0] and rec["t0"].tolist() == rec["rot_0"].tolist() == [INF, INF]
    assert rec["angle"].tolist() == rec["tau_grip"].tolist() == [0.0, 0.0]
    m.radau_step()
    assert m.radau_program_state()["t0"].tolist() == [0.5, 0.7]             # t_last0 = 0.0 <= t: due, the first fire latches t
    # set_controller, configure and clear_program end the program
    m.radau_set_controller(**SLIDER_CTL)
    refused(lambda: m.radau_program_state(), L.ERR_STATE, "without a program")
    m.radau_set_program(**SLIDER_PROG)
    m.radau_clear_controller()
    refused(lambda: m.radau_program_state(), L.ERR_STATE, "without a program")
    m.radau_set_controller(**SLIDER_CTL)
    m.radau_set_program(**SLIDER_PROG)
    m.radau_configure(2, [0])
    refused(lambda: m.radau_program_state(), L.ERR_STATE, "without a program")
    m.radau_set_state(SLIDER_X0)
    m.radau_set_controller(**SLIDER_CTL)
    m.radau_set_program(**SLIDER_PROG)
    m.radau_program_state()
    m.radau_clear_program()
    refused(lambda: m.radau_program_state(), L.ERR_STATE, "without a program")
    m.radau_clear_program()                                                # nothing to clear: not an error
    m.close()


def test_a_cleared_program_leaves_the_step_as_it_was(pfc):
    snaps = []
    for cleared in (False, True):
        m = _slider2(pfc)
        m.radau_set_controller(**SLIDER_CTL)
        if cleared:
            m.radau_set_program(**SLIDER_PROG)
            for _ in range(5):                                             # the program rewrites the segment ...
                m.radau_step()
            assert m.radau_program_state()["pops"].sum() >= 1
            m.radau_clear_program()                                        # ... and its removal puts it back
            m.radau_set_state(SLIDER_X0)
        for _ in range(5):
            assert m.radau_step()["flags"].tolist() == [0, 0]
        st = m.radau_controller_state()
        snaps.append(T._snapshot(m) + _bits(st[0]) + _bits(st[1]) + _bits(m.radau_get_tau()))
        m.close()
    assert snaps[0] == snaps[1]


_NINS = [1001, 2003, 3001]
_SIZES = [8 * (2 * 2 * k + 2 * k * 2 + 4 * 2) for k in _NINS]      # 2 scenes, n_act 2: prog_dt, prog_slip (2 n_ins each), prog_q (4 n_ins), 8


def child():
    """The child process: a program, its replacement, the clearing, a third dropped by set_controller's replacement, the close."""
    import pfc_pkg
    pfc = pfc_pkg.load()
    m = _slider2(pfc)
    m.radau_set_controller(**SLIDER_CTL)

    def set_(n_ins):
        m.radau_set_program(1, [1], 0.03, 0.25, np.full(n_ins, 0.001), np.tile([T.R, 0.0], (n_ins, 1)), np.zeros(n_ins))

    set_(_NINS[0])
    m.radau_step()
    set_(_NINS[1])
    m.radau_step()
    m.radau_clear_program()
    m.radau_step()
    set_(_NINS[2])
    m.radau_set_controller(**SLIDER_CTL)
    m.radau_step()
    m.close()


def test_every_program_block_is_freed_once():
    env = dict(os.environ, PFC_LOG_ALLOC="1")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_gpu_radau_program as t; t.child()"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    alloc = re.compile(r"^pfc alloc (0x[0-9a-f]+) \.\. 0x[0-9a-f]+ \((\d+) bytes, element (\d)\)$")
    free = re.compile(r"^pfc free (0x[0-9a-f]+)$")
    live, blocks, most, partner = {}, [], 0, False
    for ln in r.stderr.splitlines():
        a, f = alloc.match(ln), free.match(ln)
        if a and a.group(3) == "8" and int(a.group(2)) in _SIZES:
            assert a.group(1) not in live, ln
            live[a.group(1)] = int(a.group(2))
            blocks.append(int(a.group(2)))
            partner = True                                                 # the block of grip and the cursors follows at once
        elif a and partner:
            assert a.group(3) == "4" and int(a.group(2)) == 4 * (1 + 4) and a.group(1) not in live, ln
            live[a.group(1)] = int(a.group(2))
            partner = False
        elif f and f.group(1) in live:
            del live[f.group(1)]
        most = max(most, len(live))
    assert blocks == _SIZES, blocks                                        # each call allocated its blocks, in the order of the calls
    assert not live and most <= 4, (live, most)                            # the old pair goes when the new one is there; none is left
