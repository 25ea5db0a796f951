"""The discrete controller on the device (pfc_radau_control_device, pfc_radau_set_controller, pfc_radau_clear_controller,
pfc_radau_controller_state): bytes against the scalar statement (scenario.discrete_clock, scenario.computed_torque_pd;
tests/test_radau_control_abi.py) and against the host route, integrate_scenario_radau(discrete_controller=...), which drives the
same step through radau_set_tau one batch step at a time.

The mechanism of the integrations: world -> prismatic z -> a rigid box (half-width 0.05, 0.8 kg) over the one-tet half plane
(E = 1e6), regularized friction, quadrature rule 2; NX = 2.  Every handle runs with option fixed_order: bytes are compared."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_dynamics_abi as D
import test_gpu_radau as G
import test_kinematics_abi as K
from test_gpu_items_from_bodies import Guarded, _dev, _torch

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
INF = float("inf")
R, MASS = 0.05, 0.8
_bits = G._bits


def _slider(pfc, two=False):
    """The box on its vertical slide over the half plane; `two`: a second body (0.1 kg) on a prismatic x joint of the box, nv = 2."""
    Cf = pfc.configs
    plane = Cf.G.as_tet_emesh(Cf.G.emesh_half_plane())
    box = Cf.G.as_tri_emesh(Cf.G.emesh_box(R))
    ins = [Cf.InsSpec(1, 0, "regularized", chi=0.5, mu_d=0.3, n_quad_rule=2)]
    w = Cf.Workload("slider", [Cf._mesh("plane", plane, 1.0e6), Cf._mesh("box", box)], ins, np.zeros(1, dtype=np.int32),
                    np.zeros((1, 24)), np.zeros((1, 6)), np.zeros((1, 6)))
    m = Cf.build_scenario(w)
    m.set_option("fixed_order", 1)
    nb = 2 if two else 1
    mech = K.make_mech([-1, 0][:nb], [K.PRISMATIC] * nb, [K.WORLD_X] * nb, [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]][:nb])
    m.set_mechanism(mech["parent"], mech["joint_type"], mech["x_p_j"], mech["axis"])
    m.set_instruction_bodies(0, 0, -1)
    Ic = np.eye(3) * (2.0 / 3.0) * MASS * R * R
    inert = [D.make_inertia(MASS, [0.0, 0.0, 0.0], Ic), D.make_inertia(0.1, [0.0, 0.0, 0.0], Ic / 8)][:nb]
    m.set_inertia(np.array(inert).reshape(nb, 13), D.GRAVITY)
    return m


@pytest.fixture(scope="module")
def scen(pfc):
    m = pfc.configs.build_scenario(pfc.configs.c1_boxes())      # the part needs a handle, not a mechanism
    yield m
    m.close()


# ---- 1. the part ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv,n_act", [(nv, na) for nv in (1, 7, 64) for na in sorted({0, 1, nv})])
def test_control_part_is_the_statement_in_bytes(pfc, scen, nv, n_act):
    """Five scenes: 0 is not due (nothing of it is written), 1 fires once with t_last == t and a segment that starts exactly at t,
    2 fires three times, 3 is retired and 4 parked (both due, both untouched).  Scene 1 clamps upwards and scene 2 downwards on the
    even actuated entries; the odd ones have a_max = +inf."""
    torch = _torch()
    S = pfc.scenario
    m = scen
    n_scene, n_seg, dt = 5, 3, 0.01
    rng = np.random.default_rng(100 * nv + n_act)
    act = np.arange(nv, dtype=np.int32) if n_act == nv else np.array([nv // 2][:n_act], dtype=np.int32)
    kp, kd = rng.uniform(50.0, 200.0, n_act), rng.uniform(1.0, 20.0, n_act)
    a_max = np.where(np.arange(n_act) % 2 == 0, 0.5, INF)
    q, v = rng.standard_normal((n_scene, nv)), rng.standard_normal((n_scene, nv))
    H, c = rng.standard_normal((n_scene, nv, nv)), rng.standard_normal((n_scene, nv))
    t = np.array([0.25, 0.5, 0.75, 1.0, 1.25])
    t_last = np.array([0.25 + 1e-9, 0.5, 0.75 - 2.5 * dt, 0.9, 1.0])
    seg_t = np.array([[9.0, 0.1, 0.3], [9.0, 0.5, 0.6], [9.0, 0.2, 0.75000001], [9.0, 0.0, 0.5], [9.0, 0.0, 0.5]])
    seg_q = rng.standard_normal((n_scene, n_seg, n_act))
    seg_q[1, 1] = q[1, act] + 10.0                                         # e = -10: acc far above a_max
    seg_q[2, 1] = q[2, act] - 10.0                                         # e = +10: far below -a_max
    seg_ff = rng.standard_normal((n_scene, n_seg, nv))
    istate = np.zeros((n_scene, 8), dtype=np.int32)
    istate[3, 5], istate[4, 7] = 5, 1
    tau0 = rng.standard_normal((3 * n_scene, nv))
    fires0 = np.array([3, 1, 4, 1, 5], dtype=np.int32)
    g_tl, g_f, g_tau = Guarded(n_scene, 1), Guarded(n_scene, 1, True), Guarded(3 * n_scene, nv)
    g_tl.t[16:16 + n_scene] = _dev(t_last)
    g_f.t[16:16 + n_scene] = _dev(fires0)
    g_tau.t[16:16 + tau0.size] = _dev(tau0.reshape(-1))
    ins = [_dev(a) for a in (act, kp, kd, a_max, seg_t, seg_q, seg_ff, t, q, v, H, c, istate)]
    ptr = [a.data_ptr() if a.numel() else 0 for a in ins]
    for ff in (True, False):
        args = list(ptr)
        if not ff:
            args[6] = 0
            g_tl.t[16:16 + n_scene] = _dev(t_last); g_f.t[16:16 + n_scene] = _dev(fires0); g_tau.t[16:16 + tau0.size] = _dev(tau0.reshape(-1))
        m.radau_control_device(n_scene, nv, nv, n_act, n_seg, dt, *args, g_tl.ptr, g_f.ptr, g_tau.ptr)
        torch.cuda.synchronize()
        e_tl, e_f, e_tau = t_last.copy(), fires0.copy(), tau0.copy()
        for s in (0, 1, 2):
            tl, k = S.discrete_clock(t_last[s], t[s], dt)
            if k == 0:
                continue
            e_tl[s], e_f[s] = tl, fires0[s] + k
            tau = S.computed_torque_pd(q[s].tolist(), v[s].tolist(), H[s].tolist(), c[s].tolist(), float(t[s]), act.tolist(), kp.tolist(),
                                       kd.tolist(), seg_t[s].tolist(), seg_q[s].tolist(), seg_ff[s].tolist() if ff else None, a_max.tolist())
            for r in range(3):
                e_tau[r * n_scene + s] = tau
        assert (e_f - fires0).tolist() == [0, 1, 3, 0, 0]
        assert _bits(g_tl.rows()) == _bits(e_tl) and g_f.rows().tolist() == e_f.tolist()
        got = g_tau.rows().reshape(3 * n_scene, nv)
        assert _bits(got) == _bits(e_tau), np.argwhere(got != e_tau)[:4]
    if n_act:      # the clamps were active, on either side, and the segment of scene 1 was the one that starts at t
        raw1 = -(kd[0] * v[1, act[0]]) - kp[0] * (q[1, act[0]] - seg_q[1, 1, 0])
        raw2 = -(kd[0] * v[2, act[0]]) - kp[0] * (q[2, act[0]] - seg_q[2, 1, 0])
        assert raw1 > 0.5 and raw2 < -0.5 and seg_t[1, 1] == t[1] and seg_t[2, 2] > t[2]


# ---- 2. device route = host route -------------------------------------------------------------------------------------------------
ACT, KP, KD, DT = [0], [400.0], [40.0], 0.004
X0 = np.array([[R + 1.0e-3, 0.0], [R + 2.0e-3, -0.05], [R + 5.0e-4, 0.0]])
SEG_Q = np.array([[[R - 1.0e-3], [R - 2.5e-3]], [[R - 2.0e-3], [R + 1.0e-3]], [[R - 5.0e-4], [R - 3.0e-3]]])
SEG_FF = np.array([[[-0.5], [0.2]], [[0.0], [-0.3]], [[0.1], [0.1]]])
A_MAX = [0.5]
MAX_STEPS = 30


def _integrate(pfc, route, seg_t, t_final, max_steps=MAX_STEPS, x0=X0, dt=DT, t_last0=0.0, seg_q=SEG_Q, seg_ff=SEG_FF, a_max=A_MAX,
               kp=KP, kd=KD, keep=False, rule=None, **cfg):
    m = _slider(pfc)
    assert m.radau_configure(x0.shape[0], [0], **cfg) == 2
    m.radau_set_state(x0)
    if rule is not None:
        m.radau_set_rule_state(rule=rule)
    if route == "device":
        m.radau_set_controller(ACT, kp, kd, dt, seg_t, seg_q, seg_ff, a_max, t_last0)
        out = m.integrate_scenario_radau(t_final, max_steps)
        st = m.radau_controller_state()
    else:
        fn = m.computed_torque_pd_fn(ACT, kp, kd, seg_t, seg_q, seg_ff, a_max)
        out = m.integrate_scenario_radau(t_final, max_steps, discrete_controller=(fn, dt, t_last0))
        st = m.radau_host_controller_state()
    if keep:
        return out, st, m
    m.close()
    return out, st


def _mid(t, k):
    assert t.size > k + 1
    return 0.5 * (t[k] + t[k + 1])


def test_device_route_is_the_host_route_in_bytes(pfc):
    """Three scenes with different setpoints, switch times and ends.  A first run without switches gives the t values between
    which the switch times are placed, a second the t values between which the ends are placed; then both routes."""
    never = np.array([[0.0, INF]] * 3)
    free, _ = _integrate(pfc, "device", never, INF, max_steps=14)
    seg_t = np.array([[0.0, _mid(free[s][0], k)] for s, k in enumerate((6, 9, 12))])
    run, _ = _integrate(pfc, "device", seg_t, INF)
    assert all(tr[0].size == MAX_STEPS + 1 for tr in run)
    t_final = np.array([_mid(run[0][0], 18), _mid(run[1][0], 24), INF])
    (dev, dev_st, A), (host, host_st) = _integrate(pfc, "device", seg_t, t_final, keep=True), _integrate(pfc, "host", seg_t, t_final)
    assert [tr[0].size for tr in dev] == [tr[0].size for tr in host] == [20, 26, MAX_STEPS + 1]
    for s in range(3):
        assert _bits(dev[s][0]) == _bits(host[s][0]), s
        assert _bits(dev[s][1]) == _bits(host[s][1]), (s, np.abs(dev[s][1] - host[s][1]).max())
        for a in (seg_t[s, 1], t_final[s]):      # mid-gap: no decision hinges on a rounding
            assert not np.isfinite(a) or np.abs(dev[s][0] - a).min() > 1e-7
        assert dev[s][0][-1] > seg_t[s, 1]                                # the switch happened inside the run
    assert _bits(dev_st[0]) == _bits(host_st[0]) and dev_st[1].tolist() == host_st[1].tolist() and (dev_st[1] > 5).all()
    # contact: the box starts above the plane (no wrench) and is driven into it (a wrench, contributing pairs)
    in_contact = []
    for s in range(3):
        x = dev[s][1]
        wrench = A.force_all_elastic_intersections_state(x[:, 0:1], x[:, 1:2], ins_ids=[0] * x.shape[0],
                                                         scene=np.arange(x.shape[0], dtype=np.int32))[0]
        touching = np.abs(wrench).max(axis=1) > 0.0
        assert not touching[0]
        in_contact.append(int(touching.sum()))
    print("rows in contact per scene:", in_contact, "fires:", dev_st[1].tolist())
    assert max(in_contact) >= 3
    A.close()


# ---- 3. hold ----------------------------------------------------------------------------------------------------------------------
H_MAX = 2.0 ** -7


@pytest.mark.parametrize("case", ["dt = 4 h_max", "dt = h_max / 3"])
def test_hold_semantics(pfc, case):
    """One scene half a metre above the plane, h = h_max = 2^-7 from the first step (a gentle law: the step size stays at its cap, so
    t = k h_max exactly).  dt = 4 h_max, t_last0 = t = 0: fires at steps 0, 4, 8 -- at step 4 with t_last == t -- and tau is held
    in between.  dt = h_max / 3 with t_last0 = -dt / 2: one fire at step 0, three per step afterwards.  Counters and clock are the
    statement's after every step, and the trajectory is the host route's, whose tau is held by construction."""
    S = pfc.scenario
    dt, t0 = (4 * H_MAX, None) if case == "dt = 4 h_max" else (H_MAX / 3, -H_MAX / 6)
    x0, n_steps = np.array([[0.5, 0.0]]), 9
    kw = dict(seg_q=np.array([[[0.501]]]), seg_ff=None, a_max=None, kp=[4.0], kd=[4.0])
    m = _slider(pfc)
    m.radau_configure(1, [0], h0=H_MAX, h_max=H_MAX)
    m.radau_set_state(x0)
    m.radau_set_controller(ACT, kw["kp"], kw["kd"], dt, [0.0], kw["seg_q"], None, None, t0)
    tl, total, counts, vs = 0.0 if t0 is None else t0, 0, [], [0.0]
    assert m.radau_controller_state()[0][0] == tl
    for k in range(n_steps):
        assert m.radau_get_state()[1][0] == k * H_MAX                      # h stayed at its cap
        tl, f = S.discrete_clock(tl, k * H_MAX, dt)
        total += f
        counts.append(f)
        m.radau_step()
        st = m.radau_controller_state()
        assert st[0][0] == tl and st[1][0] == total, (k, st, tl, total)
        vs.append(m.radau_get_state()[0][0, 1])
    assert counts == ([1, 0, 0, 0, 1, 0, 0, 0, 1] if t0 is None else [1] + [3] * 8)
    if t0 is None:      # out of contact vdot = tau / m - g: a held tau gives equal velocity increments, to what Newton leaves of a
        dv = np.diff(vs)  # state (sqrt(tol_newton) = 1e-8 each); the fire at step 4 changes the increment by a tenth of 3e-5
        print("velocity increments", dv)
        assert np.abs(dv[1:4] - dv[0]).max() <= 2e-8 and abs(dv[4] - dv[0]) > 1e-6
    m.close()
    dev, dev_st = _integrate(pfc, "device", [0.0], INF, n_steps, x0, dt, t0, h0=H_MAX, h_max=H_MAX, **kw)
    host, host_st = _integrate(pfc, "host", [0.0], INF, n_steps, x0, dt, t0, h0=H_MAX, h_max=H_MAX, **kw)
    assert _bits(dev[0][0]) == _bits(host[0][0]) and _bits(dev[0][1]) == _bits(host[0][1])
    assert dev_st[1].tolist() == host_st[1].tolist() == [total] and _bits(dev_st[0]) == _bits(host_st[0]) == _bits(np.array([tl]))


# ---- 4. analytic ------------------------------------------------------------------------------------------------------------------
# Largest deviations measured on the host route (the step as it was, driven through radau_set_tau) with these inputs on an MI355X,
# the same in two runs: 2.864375403532904e-14 m/s^2 -- the cancellation in (v1 - v0) / h at h = 1e-4 -- and 1.1102230246251565e-16 m,
# the spacing of doubles at q = 0.5.
HOST_DEV_ACC, HOST_DEV_Q = 2.864375403532904e-14, 1.1102230246251565e-16


def analytic_deviation(pfc, route):
    """Out of contact H = m and c = m g, so vdot = acc, the law's clamped PD acceleration at the row where the controller fired -- it
    fires at every step: dt = 1e-5 is below every step size.  Returns the largest |(v1 - v0) / (t1 - t0) - acc| and
    |q1 - (q0 + h v0 + acc h^2 / 2)| over 12 steps under rule 2 from the start (order 5: exact for a constant acceleration)."""
    S = pfc.scenario
    x0 = np.array([[0.5, 0.1]])
    kw = dict(seg_q=np.array([[[0.52]]]), seg_ff=None, a_max=[1.0], kp=[100.0], kd=[5.0])
    (out, st, m) = _integrate(pfc, route, [0.0], INF, 12, x0, 1e-5, 0.0, keep=True, rule=2, **kw)
    m.close()
    t, x = out[0]
    assert t.size == 13
    d_acc, d_q, clamped = 0.0, 0.0, 0
    for k in range(12):
        h = t[k + 1] - t[k]
        raw = (-(5.0 * x[k, 1])) - 100.0 * (x[k, 0] - 0.52)
        acc = min(max(raw, -1.0), 1.0)
        clamped += raw != acc
        d_acc = max(d_acc, abs((x[k + 1, 1] - x[k, 1]) / h - acc))
        d_q = max(d_q, abs(x[k + 1, 0] - (x[k, 0] + h * x[k, 1] + 0.5 * acc * h * h)))
    assert 0 < clamped < 12 and st[1][0] > 12
    return d_acc, d_q


def test_free_motion_follows_the_law(pfc):
    """The host route deviates from the law's acceleration by at most 2.86e-14 m/s^2 and from its parabola by at most 1.11e-16 m
    (HOST_DEV_ACC, HOST_DEV_Q: measured, see above); the device route is allowed four times that.  Measured on the device route:
    the same two figures, as the two routes agree in bytes."""
    d_acc, d_q = analytic_deviation(pfc, "device")
    print("device route: |dv/dt - acc| <=", d_acc, " |q - parabola| <=", d_q)
    assert d_acc <= 4 * HOST_DEV_ACC and d_q <= 4 * HOST_DEV_Q


# ---- 5. no controller -------------------------------------------------------------------------------------------------------------
def _snapshot(m):
    rs = m.radau_rule_state()
    x, t = m.radau_get_state()
    return b"".join(_bits(a) for a in (x, t, rs["h"], rs["rule"], rs["cooldown"], rs["theta"], rs["psi_k"], rs["x_err_norm"],
                                       rs["x_err_norm_next"]))


def test_a_cleared_controller_leaves_the_step_as_it_was(pfc):
    L = pfc._lib
    x0 = np.array([[R - 1.0e-3, 0.0], [R + 1.0e-3, -0.1]])
    snaps = []
    for cleared in (False, True):
        m = _slider(pfc)
        m.radau_configure(2, [0])
        m.radau_set_state(x0)
        if cleared:
            m.radau_set_controller(ACT, KP, KD, DT, [0.0], [[R]], [[3.0]], A_MAX, 0.0)
            assert m.radau_controller_state()[1].tolist() == [0, 0]
            m.radau_clear_controller()
        with pytest.raises(L.PFCError) as e:                               # the handle holds no controller: the step's body skips it
            m.radau_controller_state()
        assert e.value.status == L.ERR_STATE
        for _ in range(3):
            assert m.radau_step()["flags"].tolist() == [0, 0]
        snaps.append(_snapshot(m))
        m.close()
    assert snaps[0] == snaps[1]


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(pfc):
    import ctypes as C
    L = pfc._lib
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

    def refused(call, status, word):
        with pytest.raises(L.PFCError) as e:
            call()
        assert e.value.status == status and word in str(e.value), str(e.value)

    m = _slider(pfc, two=True)
    good = dict(act=[0, 1], kp=[400.0, 10.0], kd=[40.0, 1.0], dt=DT, seg_t=[0.0, 0.02], seg_q=[[R, 0.0], [R + 1e-3, 0.01]],
                seg_ff=[[0.1, 0.0], [0.0, 0.1]], a_max=[2.0, INF], t_last0=0.0)
    refused(lambda: m.radau_set_controller(**good), L.ERR_STATE, "pfc_radau_configure")
    refused(lambda: m.radau_controller_state(), L.ERR_STATE, "pfc_radau_configure")
    assert m.radau_configure(2, [0]) == 4
    refused(lambda: m.radau_controller_state(), L.ERR_STATE, "without a controller")
    m.radau_set_state(np.array([[R + 1e-3, 0.0, 0.0, 0.0], [R + 2e-3, 0.01, 0.0, 0.0]]))
    m.radau_set_controller(**good)
    for _ in range(2):
        m.radau_step()

    def everything():
        st = m.radau_controller_state()
        return _snapshot(m) + _bits(st[0]) + _bits(st[1])

    before = everything()
    assert m.radau_controller_state()[1].tolist() == [1, 1]                # t = 0 and 1e-4 against t_last = 0, 0.004
    nan = float("nan")
    bad = [(dict(act=[0, 2]), "below nv"), (dict(act=[-1, 0]), "below nv"), (dict(act=[1, 0]), "increasing"), (dict(act=[1, 1]), "increasing"),
           (dict(kp=[nan, 1.0]), "gain"), (dict(kd=[1.0, INF]), "gain"), (dict(a_max=[0.0, 1.0]), "a_max"), (dict(a_max=[1.0, -2.0]), "a_max"),
           (dict(a_max=[nan, 1.0]), "a_max"), (dict(dt=0.0), "dt"), (dict(dt=-1.0), "dt"), (dict(dt=INF), "dt"), (dict(dt=nan), "dt"),
           (dict(dt=1e-7), "PFC_RADAU_MAX_FIRES"), (dict(seg_t=[0.0, 0.02, 0.01], seg_q=[[R, 0.0]] * 3, seg_ff=None), "decrease"),
           (dict(seg_t=[0.0, nan]), "decrease"), (dict(seg_q=[[R, 0.0], [nan, 0.0]]), "setpoint"), (dict(seg_ff=[[0.1, 0.0], [0.0, INF]]), "feed-forward"),
           (dict(t_last0=[0.0, nan]), "t_last0")]
    for change, word in bad:
        refused(lambda: m.radau_set_controller(**dict(good, **change)), L.ERR_BAD_ARG, word)
        assert everything() == before, (change, word)
    one = np.ones(8)
    iz = np.zeros(2, dtype=np.int32)
    for n_act, n_seg in ((2, 0), (2, -1), (3, 1), (-1, 1)):
        rc = L.lib().pfc_radau_set_controller(m._h, n_act, iz.ctypes.data_as(ip), *[one.ctypes.data_as(dp)] * 3, DT, None, n_seg,
                                              *[one.ctypes.data_as(dp)] * 3)
        assert rc == L.ERR_BAD_ARG and everything() == before, (n_act, n_seg, rc)
    # a coordinate of a floating joint
    B = G._box_scenario(pfc, True)
    B.radau_configure(1, [0])
    refused(lambda: B.radau_set_controller([2], [1.0], [1.0], DT, [0.0], [[0.0]]), L.ERR_BAD_ARG, "floating or fixed")
    refused(lambda: B.radau_controller_state(), L.ERR_STATE, "without a controller")
    B.close()
    # the part
    g = [Guarded(1, 1), Guarded(1, 1, True), Guarded(3, 2)]
    d = _dev(np.ones(8)); di = _dev(np.zeros(8, dtype=np.int32))
    a = [di.data_ptr()] + [d.data_ptr()] * 11 + [0]
    for (nq, nv, n_act, n_seg, dt), word in (((2, 65, 1, 1, DT), "PFC_MAX_NV_SOLVE"), ((2, 0, 0, 1, DT), "PFC_MAX_NV_SOLVE"), ((2, 2, 3, 1, DT), "n_act"),
                                             ((2, 2, 1, 0, DT), "n_seg"), ((2, 2, 1, 1, 0.0), "dt"), ((2, 2, 1, 1, nan), "dt")):
        refused(lambda: m.radau_control_device(1, nq, nv, n_act, n_seg, dt, *a, *[o.ptr for o in g]), L.ERR_BAD_ARG, word)
    refused(lambda: m.radau_control_device(1, 2, 2, 1, 1, DT, *a, g[0].ptr, 0, g[2].ptr), L.ERR_BAD_ARG, "null buffer")
    _torch().cuda.synchronize()
    assert all(o.untouched() for o in g)
    # the previous controller is still in force: the next steps fire as its clock says
    assert everything() == before
    fired = m.radau_controller_state()[1].copy()
    for _ in range(8):
        t = m.radau_get_state()[1]                                         # the t the clock sees at the top of the step
        m.radau_step()
    assert ((m.radau_controller_state()[1] - fired) >= 1).all() and (m.radau_controller_state()[0] > t).all()
    # set_state keeps law and schedule and starts the clock again; configure drops the controller
    m.radau_set_state(np.array([[R + 1e-3, 0.0, 0.0, 0.0], [R + 2e-3, 0.01, 0.0, 0.0]]), [0.5, 0.7])
    st = m.radau_controller_state()
    assert st[0].tolist() == [0.0, 0.0] and st[1].tolist() == [0, 0]      # t_last0 was given: 0.0
    m.radau_set_controller(**dict(good, t_last0=None))
    assert m.radau_controller_state()[0].tolist() == [0.5, 0.7]            # NULL: the scenes' t now
    m.radau_set_state(np.array([[R + 1e-3, 0.0, 0.0, 0.0], [R + 2e-3, 0.01, 0.0, 0.0]]), [0.25, 0.125])
    assert m.radau_controller_state()[0].tolist() == [0.25, 0.125]
    m.radau_configure(2, [0])
    refused(lambda: m.radau_controller_state(), L.ERR_STATE, "without a controller")
    m.close()


# ---- 7. ownership -----------------------------------------------------------------------------------------------------------------
_SEGS = [1001, 2003, 3001, 4001]
_SIZES = [8 * (3 + 4 * k + 2) for k in _SEGS]      # n_act 1, 2 scenes, no feed-forward: 3 + 2 n_seg + 2 n_seg + 2 doubles


def child():
    """The child process: a controller, its replacement, the clearing, a third, a reconfiguration, a fourth, the close."""
    import pfc_pkg
    pfc = pfc_pkg.load()
    m = _slider(pfc)
    x0 = np.array([[R + 1e-3, 0.0], [R + 2e-3, 0.0]])

    def set_(n_seg):
        m.radau_set_controller(ACT, KP, KD, DT, np.concatenate([[0.0], np.arange(1, n_seg)]), np.full((n_seg, 1), R), None, None, 0.0)

    m.radau_configure(2, [0])
    m.radau_set_state(x0)
    set_(_SEGS[0])
    m.radau_step()
    set_(_SEGS[1])
    m.radau_step()
    m.radau_clear_controller()
    m.radau_step()
    set_(_SEGS[2])
    m.radau_configure(2, [0], n_chunk=16)
    m.radau_set_state(x0)
    set_(_SEGS[3])
    m.radau_step()
    assert m.radau_controller_state()[1].tolist() == [1, 1]
    m.close()


def test_every_controller_block_is_freed_once():
    env = dict(os.environ, PFC_LOG_ALLOC="1")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_gpu_radau_control as t; t.child()"
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
            partner = True                                                 # the block of act and the counters follows at once
        elif a and partner:
            assert a.group(3) == "4" and int(a.group(2)) == 4 * (1 + 2) and a.group(1) not in live, ln
            live[a.group(1)] = int(a.group(2))
            partner = False
        elif f and f.group(1) in live:
            del live[f.group(1)]
        most = max(most, len(live))
    assert blocks == _SIZES, blocks                                        # each call allocated its blocks, in the order of the calls
    assert not live and most <= 4, (live, most)                            # the old pair goes when the new one is there; none is left
