"""Applied body wrenches on the device (pfc_body_wrench_device, pfc_body_wrench_dual_device, pfc_radau_set_body_wrenches,
pfc_radau_clear_body_wrenches; kernels k_body_wrench, k_body_wrench_dual): bytes against the scalar statements
(scenario.body_wrench_tau, scenario.body_wrench_tau_partials; tests/test_body_wrench_abi.py), the batch step with wrenches set
against the same step assembled from the public parts on caller buffers, the partials in -J against finite differences, and the
physics of a pushed box.

The mechanism, the states and the assembled step are those of tests/test_gpu_feedback.py: world -> prismatic z -> revolute y and one
MRP-floating box (half-width 0.05, 0.8 kg) over the one-tet half plane, nq = nv = 8, NX = 16, three bodies; option fixed_order."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_dynamics_abi as D
import test_gpu_feedback as FB
import test_radau_abi as R
from test_gpu_feedback import NV, NX, PAR, _bits, _ptr, _sync
from test_gpu_items_from_bodies import Guarded, _dev, _torch

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
INF = float("inf")
NB = 3
G = 9.81
MG = FB.BOX_MASS * G


@pytest.fixture(scope="module")
def scen(pfc):
    m = pfc.configs.build_scenario(pfc.configs.c1_boxes())      # the parts need a handle, not a mechanism
    yield m
    m.close()


# ---- 1. the value part, 2. the Dual part ------------------------------------------------------------------------------------------
def _part_case(rows, n_w, n_seg, seed, n_scene=1):
    """rows rows of three bodies and nv = 8 that read the schedules of n_scene scenes.  The wrenches sit on body 1 (frame 0), body 2
    (frame 1) and body 0 (frame 1): both frames in one call with n_w = 3.  Body 1's Jacobian holds coordinates 0 and 1 only (+0.0
    elsewhere, as pfc_kinematics_device writes a path), coordinate 3's column is zero for every body and tau_in holds -0.0 there; row
    0 sits exactly on a segment start."""
    rng = np.random.default_rng(seed)
    d = dict(body=np.array([1, 2, 0][:n_w], dtype=np.int32), frame=np.array([0, 1, 1][:n_w], dtype=np.int32),
             point=rng.uniform(-0.5, 0.5, (n_w, 3)), seg_t=np.tile(np.array([9.0, 0.25, 0.5][:n_seg]), (n_scene, 1)),
             seg_w=rng.standard_normal((n_scene, n_seg, n_w, 6)), t=rng.uniform(0.0, 0.75, rows),
             x_w_b=rng.standard_normal((rows, NB, 12)), jac=rng.standard_normal((rows, NB, NV, 6)), tau_in=rng.standard_normal((rows, NV)))
    d["t"][0] = 0.25
    d["jac"][:, 1, 2:] = 0.0
    d["jac"][:, :, 3] = 0.0
    d["tau_in"][:, 3] = -0.0
    return n_scene, d


def _tables(dev, n_seg):
    return [_ptr(dev["body"]), _ptr(dev["frame"]), _ptr(dev["point"]), _ptr(dev["seg_t"]) if n_seg > 1 else 0, _ptr(dev["seg_w"])]


@pytest.mark.parametrize("rows", [1, 3, 65])
@pytest.mark.parametrize("n_w", [0, 1, 3])
@pytest.mark.parametrize("n_seg", [1, 3])
def test_value_part_is_the_statement_in_bytes(pfc, scen, rows, n_w, n_seg):
    S = pfc.scenario
    # 65 rows: 13 stage-scene blocks over the schedules of 5 scenes, more rows than a wave has lanes
    n_scene, d = _part_case(rows, n_w, n_seg, 1000 * rows + 10 * n_w + n_seg, 5 if rows == 65 else 1)
    dev = {k: _dev(a) for k, a in d.items()}
    for ti in (False, True):
        out = Guarded(rows, NV)
        scen.body_wrench_device(rows, n_scene, NB, NV, n_w, n_seg, *_tables(dev, n_seg), _ptr(dev["t"]), _ptr(dev["x_w_b"]), _ptr(dev["jac"]),
                                _ptr(dev["tau_in"]) if ti else 0, out.ptr)
        _sync()
        ref = np.zeros((rows, NV))
        for r in range(rows):
            sc = r % n_scene
            ref[r] = S.body_wrench_tau(d["x_w_b"][r].tolist(), d["jac"][r].tolist(), float(d["t"][r]), d["tau_in"][r].tolist() if ti else None,
                                       d["body"].tolist(), d["frame"].tolist(), d["point"].tolist(), d["seg_t"][sc].tolist(),
                                       d["seg_w"][sc].tolist())
        got = out.rows().reshape(rows, NV)
        assert _bits(got) == _bits(ref), (ti, np.argwhere(got != ref)[:4])
        if n_w == 0:
            assert _bits(got) == _bits(d["tau_in"] if ti else np.zeros((rows, NV)))      # copied: -0.0 survives; +0.0 without tau_in
            assert not ti or math.copysign(1.0, got[0, 3]) == -1.0
        else:
            assert (got[:, 3] == 0.0).all()                                   # the zero column: -0.0 plus a sum of signed zeros
            assert np.abs(got[:, :2]).min() > 0.0
    if n_seg > 1 and n_w > 0:                                                 # row 0 read the segment that starts at its t
        assert d["seg_t"][0, 1] == d["t"][0]
        ref0 = S.body_wrench_tau(d["x_w_b"][0].tolist(), d["jac"][0].tolist(), 0.25, d["tau_in"][0].tolist(), d["body"].tolist(),
                                 d["frame"].tolist(), d["point"].tolist(), [0.0], d["seg_w"][0][1:2].tolist())
        assert _bits(got[0]) == _bits(ref0)
    if n_w == 1:                                                              # body 1's path: the box's coordinates get tau_in back
        assert _bits(got[:, 4:]) == _bits(d["tau_in"][:, 4:] + 0.0)


@pytest.mark.parametrize("n_dir", [1, 6, 16])
def test_dual_part_is_the_statement_in_bytes(pfc, scen, n_dir):
    """Three scenes with schedules of their own, three wrenches, three segments; dtau_in NULL and given."""
    S = pfc.scenario
    ns, n_w, n_seg = 3, 3, 3
    n_scene, d = _part_case(ns, n_w, n_seg, 50 + n_dir, ns)
    rng = np.random.default_rng(n_dir)
    dx, dJ, din = rng.standard_normal((ns, NB, n_dir, 12)), rng.standard_normal((ns, NB, n_dir, NV, 6)), rng.standard_normal((ns, n_dir, NV))
    dJ[:, 1, :, 2:] = 0.0
    dJ[:, :, :, 3] = 0.0
    dev = {k: _dev(a) for k, a in d.items()}
    ddx, ddJ, ddin = _dev(dx), _dev(dJ), _dev(din)
    for use_in in (False, True):
        out = Guarded(ns * n_dir, NV)
        scen.body_wrench_dual_device(ns, n_dir, n_scene, NB, NV, n_w, n_seg, *_tables(dev, n_seg), _ptr(dev["t"]), _ptr(dev["x_w_b"]),
                                     _ptr(dev["jac"]), _ptr(ddx), _ptr(ddJ), _ptr(ddin) if use_in else 0, out.ptr)
        _sync()
        ref = np.zeros((ns, n_dir, NV))
        for s in range(ns):
            for k in range(n_dir):
                ref[s, k] = S.body_wrench_tau_partials(d["x_w_b"][s].tolist(), d["jac"][s].tolist(), dx[s, :, k].tolist(), dJ[s, :, k].tolist(),
                                                       float(d["t"][s]), din[s, k].tolist() if use_in else None, d["body"].tolist(),
                                                       d["frame"].tolist(), d["point"].tolist(), d["seg_t"][s].tolist(), d["seg_w"][s].tolist())
        got = out.rows().reshape(ns, n_dir, NV)
        assert _bits(got) == _bits(ref), (use_in, np.argwhere(got != ref)[:4])
        assert np.abs(got[:, :, :2]).min() > 0.0
        if not use_in:
            assert (got[:, :, 3] == 0.0).all()
    # no wrench: dtau_in copied, or +0.0
    for use_in in (False, True):
        out = Guarded(ns * n_dir, NV)
        scen.body_wrench_dual_device(ns, n_dir, n_scene, NB, NV, 0, 1, 0, 0, 0, 0, 0, _ptr(dev["t"]), 0, 0, 0, 0, _ptr(ddin) if use_in else 0, out.ptr)
        _sync()
        assert _bits(out.rows().reshape(ns, n_dir, NV)) == _bits(din if use_in else np.zeros((ns, n_dir, NV)))


def test_parts_refuse_bad_sizes_before_any_launch(pfc, scen):
    L = pfc._lib
    n_scene, d = _part_case(2, 1, 1, 5, 2)
    dev = {k: _dev(a) for k, a in d.items()}
    z = _dev(np.zeros(2 * NB * 17 * NV * 6))
    out = Guarded(2 * 17, NV)
    tab = _tables(dev, 1)

    def value(rows=2, n_scene=2, n_body=NB, nv=NV, n_w=1, n_seg=1, t=None, o=None):
        scen.body_wrench_device(rows, n_scene, n_body, nv, n_w, n_seg, *tab, _ptr(dev["t"]) if t is None else t, _ptr(dev["x_w_b"]),
                                _ptr(dev["jac"]), 0, out.ptr if o is None else o)

    def dual(n_dir, **kw):
        a = dict(dict(rows=2, n_scene=2, n_body=NB, nv=NV, n_w=1, n_seg=1), **kw)
        scen.body_wrench_dual_device(a["rows"], n_dir, a["n_scene"], a["n_body"], a["nv"], a["n_w"], a["n_seg"], *tab, _ptr(dev["t"]),
                                     _ptr(dev["x_w_b"]), _ptr(dev["jac"]), _ptr(z), _ptr(z), 0, out.ptr)

    bad = [(lambda: dual(0), "n_dir"), (lambda: dual(17), "n_dir"), (lambda: value(nv=0), "PFC_MAX_NV_SOLVE"), (lambda: value(nv=65), "PFC_MAX_NV_SOLVE"),
           (lambda: dual(2, nv=65), "PFC_MAX_NV_SOLVE"), (lambda: value(n_w=-1), "n_w"), (lambda: dual(2, n_w=-1), "n_w"),
           (lambda: value(n_seg=0), "n_seg"), (lambda: dual(2, n_seg=0), "n_seg"), (lambda: value(n_scene=0), "n_scene"),
           (lambda: value(rows=3), "multiple"), (lambda: dual(2, rows=3), "multiple"), (lambda: value(n_body=0), "n_body"),
           (lambda: value(t=0), "null buffer"), (lambda: value(o=0), "null buffer")]
    for call, word in bad:
        with pytest.raises(L.PFCError) as e:
            call()
        assert e.value.status == L.ERR_BAD_ARG and word in str(e.value), (word, str(e.value))
    with pytest.raises(L.PFCError) as e:      # a null table with a wrench to apply
        scen.body_wrench_device(2, 2, NB, NV, 1, 1, 0, tab[1], tab[2], 0, tab[4], _ptr(dev["t"]), _ptr(dev["x_w_b"]), _ptr(dev["jac"]), 0, out.ptr)
    assert e.value.status == L.ERR_BAD_ARG and "null buffer" in str(e.value)
    _sync()
    assert out.untouched()


# ---- the step from its parts ------------------------------------------------------------------------------------------------------
class _Behind:
    """The scenario as FB.Parts calls it, with the wrench parts issued in front of either solve -- where the driver issues them: after
    the dynamics and after the law -- and the solve reading their outputs."""

    def __init__(self, m, parts):
        self._m, self._p = m, parts

    def __getattr__(self, name):
        return getattr(self._m, name)

    def accelerations_device(self, rows, H, c, f, tau, vdot, info):
        P = self._p
        P.push_value(rows, P.t_now, tau)
        self._m.accelerations_device(rows, H, c, f, _ptr(P.wtaus), vdot, info)

    def accelerations_dual_device(self, ns, nd, H, c, f, tau, dH, dc, df, dtau, vdot, dvdot, info):
        P = self._p
        if vdot:                      # a first chunk: the value as well, at the scenes' t
            P.push_value(ns, P.t, tau)
        P.push_dual(ns, nd, dtau)
        self._m.accelerations_dual_device(ns, nd, H, c, f, _ptr(P.wtaus), dH, dc, df, _ptr(P.wdtau), vdot, dvdot, info)


class PushParts(FB.Parts):
    """FB.Parts with applied body wrenches push = dict(body, frame, point, seg_t (ns, n_seg), seg_w (ns, n_seg, n_w, 6))."""

    def __init__(self, m, x0, t0, law, push, **kw):
        super().__init__(m, x0, t0, law, **kw)
        torch = _torch()
        self.push = push
        self.pdev = {k: _dev(np.asarray(push[k], dtype=np.int32 if k in ("body", "frame") else np.float64)) for k in push}
        rows = self.q.shape[0]
        self.wtaus = torch.zeros((rows, NV), dtype=torch.float64, device=self.q.device)
        self.wdtau = torch.zeros((self.ns * self.n_chunk, NV), dtype=torch.float64, device=self.q.device)
        self.t_now = self.ts
        self.m = _Behind(m, self)
        _sync()

    def _head(self):
        d = self.pdev
        n_seg = d["seg_t"].shape[-1]
        return [self.ns, NB, NV, int(d["body"].numel()), n_seg, _ptr(d["body"]), _ptr(d["frame"]), _ptr(d["point"]), _ptr(d["seg_t"]), _ptr(d["seg_w"])]

    def push_value(self, rows, t, tau_in):
        self._m().body_wrench_device(rows, *self._head(), _ptr(t), _ptr(self.kin[0]), _ptr(self.kin[2]), tau_in, _ptr(self.wtaus))

    def push_dual(self, ns, nd, dtau_in):
        self._m().body_wrench_dual_device(ns, nd, *self._head(), _ptr(self.t), _ptr(self.kin[0]), _ptr(self.kin[2]), _ptr(self.dkin[0]),
                                          _ptr(self.dkin[2]), dtau_in, _ptr(self.wdtau))

    def _m(self):
        return self.m._m

    def value_chain(self, rows, t):
        self.t_now = t
        super().value_chain(rows, t)


def _push(ns, n_seg=1, seg_t1=INF, seed=23, scale=1.0):
    """A world-frame load at an offset point of the arm and a body-frame load at a corner of the box, per scene and segment."""
    rng = np.random.default_rng(seed)
    seg_t = np.zeros((ns, n_seg))
    if n_seg > 1:
        seg_t[:, 1] = seg_t1
    seg_w = scale * rng.uniform(-1.0, 1.0, (ns, n_seg, 2, 6)) * np.array([0.05, 0.05, 0.05, 3.0, 3.0, 3.0])
    return dict(body=[1, 2], frame=[0, 1], point=[[0.2, 0.03, -0.1], [0.05, -0.05, 0.05]], seg_t=seg_t, seg_w=seg_w)


def _handle(pfc, x0, t0=None, rule=None, h=None, law=None, push=None):
    m = FB._handle(pfc, x0, t0, rule, h, law)
    if push is not None:
        m.radau_set_body_wrenches(**push)
    return m


@pytest.mark.parametrize("case", ["one segment", "a boundary inside the step", "a law and wrenches"])
def test_step_with_wrenches_is_its_parts(pfc, case):
    """Two scenes at rule 2 with different h, three batch steps, against the step assembled from the public parts.  `a boundary inside
    the step`: the second segment starts at t0 + h0 / 2, strictly between the first and the last stage time of the first step.  `a
    law and wrenches`: the parts run the law's kernels, then the wrenches' on the law's outputs -- the order the header states."""
    ns = 2
    x0, t0, h, rule = FB._states(ns), np.array([0.0, 0.25]), np.array([1e-4, 2e-4]), np.array([2, 2], dtype=np.int32)
    law = FB._law(ns) if case == "a law and wrenches" else None
    push = _push(ns, n_seg=2, seg_t1=t0 + 0.5 * h) if case == "a boundary inside the step" else _push(ns)
    A, B = _handle(pfc, x0, t0, rule, h, law, push), FB._arm_box(pfc)
    P = PushParts(B, x0, t0, law, push, rule=rule, h=h)
    for step in range(3):
        ra, rb = A.radau_step(), P.step()
        assert ra["flags"].tolist() == rb["flags"].tolist() == [0] * ns, step
        assert ra["iters"].tolist() == rb["iters"].tolist() and ra["attempts"].tolist() == rb["attempts"].tolist(), step
        FB._same(FB._handle_snapshot(A), P.snapshot(), step)
        assert _bits(A.radau_stage_times()) == _bits(P.times[-1]), step
        if step == 0 and case == "a boundary inside the step":
            ts = P.times[0]
            assert ((ts[0] < push["seg_t"][:, 1]) & (push["seg_t"][:, 1] < ts[2])).all()
    summed = P.wtaus.cpu().numpy()[:3 * ns]
    assert np.abs(summed).max() > 0.1                                         # the wrenches were at work
    if law is not None:                                                       # on top of the law's torque, not in place of it
        assert np.abs(P.taus.cpu().numpy()).max() > 1.0 and _bits(summed) != _bits(P.taus.cpu().numpy()[:3 * ns])
    A.close(); B.close()


def test_partials_of_the_wrenches_reach_the_jacobian(pfc):
    """One scene, a world-frame force at an offset point of the revolute arm and a body-frame force at a corner of the floating box.
    -J's vdot rows for the columns of the arm angle and the box's MRP (states 1 .. 4) against central differences of the value
    chain with the wrenches included.  The tolerance is test_partials_of_the_law_reach_the_jacobian's: at most four times the
    error the same check shows with the wrenches cleared on the same scene (both printed; DESIGN.md holds the figures measured on
    an MI355X); the error is the largest absolute difference over the block divided by the block's largest magnitude.  The set and
    the cleared blocks differ by more than the cleared check's absolute error: a dropped dtau would show."""
    x0, t0 = FB._states(1), np.array([0.125])
    cols, eps = [1, 2, 3, 4], 1e-5
    push = dict(body=[1, 2], frame=[0, 1], point=[[0.3, 0.0, -0.1], [0.05, -0.05, 0.05]], seg_t=np.zeros((1, 1)),
                seg_w=np.array([[[[0.0, 0.0, 0.0, 8.0, -5.0, 20.0], [0.0, 0.0, 0.0, 10.0, 15.0, -5.0]]]]))
    err, blocks, abs_err = {}, {}, {}
    for name in ("cleared", "set"):
        B = FB._arm_box(pfc)
        P = PushParts(B, x0, t0, None, push, cap=2 * len(cols)) if name == "set" else FB.Parts(B, x0, t0, None, cap=2 * len(cols))
        P.unpack()
        P.jacobian()
        J = -P.neg_J_kept[0][cols][:, NV:2 * NV]                               # [column][vdot row]
        fd = FB._fd_columns(P, x0[0], float(t0[0]), cols, eps)
        abs_err[name] = float(np.abs(fd - J).max())
        err[name] = abs_err[name] / float(np.abs(J).max())
        blocks[name] = J
        B.close()
    diff = float(np.abs(blocks["set"] - blocks["cleared"]).max())
    print("finite-difference check of -J's vdot rows, relative error: wrenches cleared %.3e, set %.3e; the blocks differ by %.3e, "
          "the cleared check's absolute error is %.3e" % (err["cleared"], err["set"], diff, abs_err["cleared"]))
    assert diff > abs_err["cleared"], (diff, abs_err)
    assert err["set"] <= 4.0 * err["cleared"], err


# ---- 5. physics, free bodies ------------------------------------------------------------------------------------------------------
def _free_box_state():
    x = np.zeros((1, NX))
    x[0, 1] = 0.2
    x[0, 7] = 5.0                                                             # 5 m above the plane: no contact
    return x


def test_a_force_that_cancels_gravity_leaves_the_box_at_rest(pfc):
    """A world force +m g z at the box's centre of mass, from rest to t = 0.2: every step commits, and the box's position, attitude
    and velocity stay within the integrator's tol_a of the start (the slide and the arm, which nothing holds, fall meanwhile)."""
    x0 = _free_box_state()
    m = _handle(pfc, x0, push=dict(body=[2], frame=[0], point=[[0.0, 0.0, 0.0]], seg_t=[0.0], seg_w=[[[0.0, 0.0, 0.0, 0.0, 0.0, MG]]]))
    steps, t = 0, 0.0
    while t < 0.2 and steps < 400:
        assert m.radau_step()["flags"].tolist() == [0], steps
        x, tt = m.radau_get_state()
        t, steps = float(tt[0]), steps + 1
        box = np.concatenate([x[0, 2:8] - x0[0, 2:8], x[0, 10:16]])
        assert np.abs(box).max() <= PAR["tol_a"], (steps, t, box)
    print("hover: %d steps to t = %.4f, largest box deviation %.3e; the slide fell %.4f m" % (steps, t, np.abs(box).max(), x0[0, 0] - x[0, 0]))
    assert t >= 0.2 and abs(x[0, 0] - x0[0, 0]) > 0.1                         # the slide and the arm, not held, fell 0.2 m meanwhile
    m.close()


def test_a_body_frame_moment_spins_the_box_up_linearly(pfc):
    """Zero gravity, a body-frame moment M about z on the box with its isotropic inertia I: omega_z(t) = M t / I, linear in t and so
    integrated exactly; within tol_r |omega_z| + tol_a at the end."""
    x0 = _free_box_state()
    m = FB._arm_box(pfc)
    Ib = (2.0 / 3.0) * FB.BOX_MASS * FB.BOX_R * FB.BOX_R
    inert = [D.make_inertia(0.5, [0.0, 0.0, 0.0], np.eye(3) * 1e-3), D.make_inertia(0.3, [0.1, 0.0, 0.02], np.diag([2e-4, 1e-3, 1e-3])),
             D.make_inertia(FB.BOX_MASS, [0.0, 0.0, 0.0], np.eye(3) * Ib)]
    m.set_inertia(np.array(inert).reshape(3, 13), (0.0, 0.0, 0.0))
    assert m.radau_configure(1, [0]) == NX
    m.radau_set_state(x0)
    M = 1.0e-3
    m.radau_set_body_wrenches([2], [1], [[0.02, -0.01, 0.03]], [0.0], [[[0.0, 0.0, M, 0.0, 0.0, 0.0]]])
    steps, t = 0, 0.0
    while t < 0.2 and steps < 400:
        assert m.radau_step()["flags"].tolist() == [0], steps
        x, tt = m.radau_get_state()
        t, steps = float(tt[0]), steps + 1
    want = M * t / Ib
    print("spin-up: %d steps to t = %.4f, omega_z = %.9e, M t / I = %.9e" % (steps, t, x[0, 12], want))
    assert t >= 0.2 and abs(x[0, 12] - want) <= PAR["tol_r"] * abs(want) + PAR["tol_a"], (x[0, 12], want)
    assert np.abs(x[0, 10:12]).max() <= PAR["tol_a"] and np.abs(x[0, 13:16]).max() <= PAR["tol_a"]      # a pure moment: nothing else moves
    m.close()


# ---- 6. physics, contact ----------------------------------------------------------------------------------------------------------
def test_a_pushed_box_sticks_below_the_friction_cone_and_slides_above_it(pfc):
    """The box rests on the plane (mu_d = 0.3), level and at the depth where the pressure field carries it: the half plane's field
    is E z per metre and the footprint is (2 r)^2, so m g = E (2 r)^2 d.  Two scenes in one batch, pushed along x at the centre of
    mass to t = 0.1 with F_low = 0.5 mu m g and F_high = 2 mu m g."""
    mu, ns = 0.3, 2
    depth = MG / (1.0e6 * (2.0 * FB.BOX_R) ** 2)
    x0 = np.zeros((ns, NX))
    x0[:, 1] = 0.2
    x0[:, 7] = FB.BOX_R - depth
    F = np.array([0.5 * mu * MG, 2.0 * mu * MG])
    seg_w = np.zeros((ns, 1, 1, 6))
    seg_w[:, 0, 0, 3] = F
    m = _handle(pfc, x0, push=dict(body=[2], frame=[0], point=[[0.0, 0.0, 0.0]], seg_t=np.zeros((ns, 1)), seg_w=seg_w))
    m.radau_set_end([0.1, 0.1], 0)
    steps, t = 0, np.zeros(ns)
    while (t < 0.1).any() and steps < 2000:
        flags = m.radau_step()["flags"].tolist()
        assert all(f == 0 or (f == 6 and t[i] >= 0.1) for i, f in enumerate(flags)), (steps, flags, t)
        x, t = m.radau_get_state()
        steps += 1
    dx = x[:, 5] - x0[:, 5]
    print("pushed box: %d batch steps, t = %s, x_low = %.6e m, x_high = %.6e m, frictionless bound %.6e m, z - z0 = %s"
          % (steps, t.tolist(), dx[0], dx[1], 0.5 * (F[1] / FB.BOX_MASS) * t[1] ** 2, (x[:, 7] - x0[:, 7]).tolist()))
    assert (t >= 0.1).all()
    assert dx[1] <= 0.5 * (F[1] / FB.BOX_MASS) * t[1] ** 2
    assert dx[1] >= 10.0 * dx[0]
    assert dx[1] > 0.0
    m.close()


# ---- 7. life cycle ----------------------------------------------------------------------------------------------------------------
def test_cleared_wrenches_leave_the_step_as_it_was(pfc):
    x0 = FB._states(2)
    snaps = []
    for cleared in (False, True):
        m = _handle(pfc, x0, push=_push(2) if cleared else None)
        if cleared:
            m.radau_step()
            m.radau_clear_body_wrenches()
            m.radau_set_state(x0)
        for _ in range(2):
            assert m.radau_step()["flags"].tolist() == [0, 0]
        snaps.append(FB._handle_snapshot(m))
        m.close()
    FB._same(snaps[0], snaps[1], "cleared")


def test_a_parked_scene_is_left_alone_with_wrenches_set(pfc):
    x0 = FB._states(3)
    m = _handle(pfc, x0, push=_push(3))
    m.radau_set_end([1.5e-4, INF, INF], 0)                                    # scene 0 parks at its second commit
    flags = [m.radau_step()["flags"].tolist() for _ in range(3)]
    assert flags[2] == [6, 0, 0], flags
    before = FB._handle_snapshot(m)
    for _ in range(3):
        assert m.radau_step()["flags"].tolist() == [6, 0, 0]
    after = FB._handle_snapshot(m)
    for k in before:
        assert _bits(before[k][0]) == _bits(after[k][0]), k
        assert k not in ("x", "t") or _bits(before[k][1:]) != _bits(after[k][1:]), k      # the others went on
    m.close()


def test_refusals_keep_the_previous_wrenches(pfc):
    L = pfc._lib
    nan = float("nan")

    def refused(call, status, word):
        with pytest.raises(L.PFCError) as e:
            call()
        assert e.value.status == status and word in str(e.value), str(e.value)
        assert L.lib().pfc_last_error(m._h)

    m = FB._arm_box(pfc)
    w6 = [[0.01, 0.0, 0.02, 1.0, -2.0, 0.5], [0.0, 0.03, 0.0, 0.5, 0.5, 1.5]]
    good = dict(body=[1, 2], frame=[0, 1], point=[[0.2, 0.0, -0.1], [0.05, 0.05, 0.0]], seg_t=[0.0, 2e-4], seg_w=[w6, [w6[1], w6[0]]])
    refused(lambda: m.radau_set_body_wrenches(**good), L.ERR_STATE, "pfc_radau_configure")
    refused(lambda: m.radau_clear_body_wrenches(), L.ERR_STATE, "pfc_radau_configure")
    x0 = FB._states(2)
    assert m.radau_configure(2, [0]) == NX
    m.radau_set_state(x0)
    refused(lambda: m.radau_stage_times(), L.ERR_STATE, "without a law")
    m.radau_set_body_wrenches(**good)
    assert not m.radau_stage_times().any()                                    # before the first step with them
    m.radau_step()
    assert m.radau_stage_times().any()                                        # answered without a law
    bad_w = [list(w6[0]), list(w6[1])]
    bad_w[1][4] = INF
    bad = [(dict(body=[1, 3]), "body"), (dict(body=[-1, 2]), "body"), (dict(frame=[0, 2]), "frame"), (dict(frame=[-1, 1]), "frame"),
           (dict(point=[[0.2, nan, 0.0], [0.0, 0.0, 0.0]]), "point"), (dict(point=[[0.2, 0.0, 0.0], [INF, 0.0, 0.0]]), "point"),
           (dict(seg_w=[w6, bad_w]), "load"), (dict(seg_t=[0.0, nan]), "decrease"),
           (dict(seg_t=[0.0, 2.0, 1.0], seg_w=[w6, w6, w6]), "decrease")]
    for change, word in bad:
        refused(lambda: m.radau_set_body_wrenches(**dict(good, **change)), L.ERR_BAD_ARG, word)
    one, iz = np.ones(64), np.array([1, 1], dtype=np.int32)      # sizes the wrapper cannot express: the entry itself
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    for n_w, n_seg, word in ((2, 0, b"n_seg"), (2, -1, b"n_seg"), (-1, 1, b"n_w")):
        rc = L.lib().pfc_radau_set_body_wrenches(m._h, n_w, iz.ctypes.data_as(ip), iz.ctypes.data_as(ip), one.ctypes.data_as(dp), n_seg,
                                                 one.ctypes.data_as(dp), one.ctypes.data_as(dp))
        assert rc == L.ERR_BAD_ARG and word in L.lib().pfc_last_error(m._h)
    # the previous wrenches are in force: the next steps are those of a handle that was given `good` and never a bad one
    ref = _handle(pfc, x0, push=good)
    ref.radau_step()
    for _ in range(2):
        assert m.radau_step()["flags"].tolist() == ref.radau_step()["flags"].tolist() == [0, 0]
    FB._same(FB._handle_snapshot(m), FB._handle_snapshot(ref), "after refusals")
    # and they matter: a handle without them is elsewhere
    bare = _handle(pfc, x0)
    for _ in range(3):
        bare.radau_step()
    assert _bits(FB._handle_snapshot(bare)["x"]) != _bits(FB._handle_snapshot(ref)["x"])
    # pfc_radau_set_state keeps them, a later configure drops them: the step is a fresh handle's
    m.radau_set_state(x0); ref.radau_configure(2, [0]); ref.radau_set_state(x0); ref.radau_set_body_wrenches(**good)
    m.radau_step(); ref.radau_step()
    FB._same(FB._handle_snapshot(m), FB._handle_snapshot(ref), "after set_state")
    m.radau_configure(2, [0])
    m.radau_set_state(x0)
    refused(lambda: m.radau_stage_times(), L.ERR_STATE, "without a law")
    fresh = _handle(pfc, x0)
    m.radau_step(); fresh.radau_step()
    FB._same(FB._handle_snapshot(m), FB._handle_snapshot(fresh), "after configure")
    for h in (m, ref, fresh, bare):
        h.close()


# The wrenches' two blocks on two scenes of the arm-box (nv = 8, n_chunk = 6), packed: n_w = 2, n_seg = 2:
#   doubles  point 6 + seg_t 4 + seg_w 48 + summed tau 3 x 2 x 8 = 48 + partials 2 x 6 x 8 = 96 + stage times 6 = 208;  ints 2 + 2 = 4
_BLOCKS = [(8 * 208, 8), (4 * 4, 4)]


def alloc_child():
    """The child process: set, replace, clear and set again, each between two marks in the log; a step; the close."""
    import pfc_pkg
    pfc = pfc_pkg.load()
    m = FB._arm_box(pfc)
    m.radau_configure(2, [0])
    m.radau_set_state(FB._states(2))
    w6 = [[0.01, 0.0, 0.02, 1.0, -2.0, 0.5], [0.0, 0.03, 0.0, 0.5, 0.5, 1.5]]
    good = dict(body=[1, 2], frame=[0, 1], point=[[0.2, 0.0, -0.1], [0.05, 0.05, 0.0]], seg_t=[0.0, 2e-4], seg_w=[w6, [w6[1], w6[0]]])

    def marked(name, call):
        print(f"mark {name}", file=sys.stderr, flush=True)
        call()
        print("mark end", file=sys.stderr, flush=True)

    marked("set", lambda: m.radau_set_body_wrenches(**good))
    marked("replace", lambda: m.radau_set_body_wrenches(**good))
    marked("clear", lambda: m.radau_clear_body_wrenches())
    marked("step", lambda: m.radau_step())
    marked("again", lambda: m.radau_set_body_wrenches(**good))
    assert m.radau_step()["flags"].tolist() == [0, 0]
    m.close()


def test_wrench_blocks_have_their_sizes_and_are_freed_once():
    """PFC_LOG_ALLOC=1: setting allocates the two packed blocks (doubles first), replacing allocates the new pair before it frees the
    old one, clearing frees the pair, a step without wrenches allocates nothing of theirs, and every block is freed exactly once by
    the close."""
    env = dict(os.environ, PFC_LOG_ALLOC="1")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_gpu_body_wrench as t; t.alloc_child()"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    alloc = re.compile(r"^pfc alloc (0x[0-9a-f]+) \.\. 0x[0-9a-f]+ \((\d+) bytes, element (\d+)\)$")
    free = re.compile(r"^pfc free (0x[0-9a-f]+)$")
    call, events, live = None, {}, set()
    for ln in r.stderr.splitlines():
        a, f = alloc.match(ln), free.match(ln)
        if ln.startswith("mark "):
            call = None if ln == "mark end" else ln[5:]
        elif a:
            assert a.group(1) not in live, f"allocated twice without a free in between: {ln}"
            live.add(a.group(1))
            if call:
                events.setdefault(call, []).append(("alloc", a.group(1), int(a.group(2)), int(a.group(3))))
        elif f:
            assert f.group(1) in live, f"freed without a live allocation (a second free?): {ln}"
            live.remove(f.group(1))
            if call:
                events.setdefault(call, []).append(("free", f.group(1)))
    assert not live, f"{len(live)} blocks never freed"
    sizes = lambda ev: [(e[2], e[3]) for e in ev if e[0] == "alloc"]
    assert [e[0] for e in events["set"]] == ["alloc", "alloc"] and sizes(events["set"]) == _BLOCKS
    first = [e[1] for e in events["set"]]
    assert [e[0] for e in events["replace"]] == ["alloc", "alloc", "free", "free"] and sizes(events["replace"]) == _BLOCKS
    assert sorted(e[1] for e in events["replace"][2:]) == sorted(first)      # the old pair, after the new one was had
    second = [e[1] for e in events["replace"][:2]]
    assert [e[0] for e in events["clear"]] == ["free", "free"] and sorted(e[1] for e in events["clear"]) == sorted(second)
    # the first step grows the handle's own work lists; none of that is the wrenches' double block (a size nothing else has)
    assert all((e[2], e[3]) != _BLOCKS[0] for e in events.get("step", []) if e[0] == "alloc")
    assert sizes(events["again"]) == _BLOCKS
