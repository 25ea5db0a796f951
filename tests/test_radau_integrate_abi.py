"""Integration to per-scene end times (pfc_radau_set_end, pfc_radau_integrate, pfc_radau_trajectory[_rows],
pfc_radau_finish_end_device) without a device: the scalar statement of what the end adds to the step of tests/test_radau_abi.py, and
what pins it.

The statement: `arm_end` (k_radau_jac's arming: a retired scene is left alone, a parked one gets exit flag 6, the others are armed),
`set_end_scalar` (row 0, the parked marks cleared), `record_and_park` (what k_radau_finish<true> adds at a commit: the row, the park
decision, the live count) and the batch driver `integrate_batch`, which arms only unparked scenes, feeds parked scenes at their
committed x and records after `finish_scalar`.  tests/test_gpu_radau_integrate.py compares bytes with it.

What pins it: for a `de` that does not depend on the batch, every scene's (data_time, data_state) is what the reference's loop
(integrate_scenario_radau, src/example_integrator.jl: step, store, stop when t_final < t, at most max_steps steps) returns on
`radau_step_scalar`, and, to 1e-10, on `reference_step`, the NumPy restatement of the reference's own step."""
import ctypes as C
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import test_dynamics_abi as D
import test_kinematics_abi as K
import test_radau_abi as R
from test_radau_abi import (ATTEMPTS, DEFAULTS, EXIT, ITER, KITER, PHASE, factor_scalar, finish_scalar, new_records,
                            newton_scalar)

ROOT = K.ROOT
INF = float("inf")
PARKED = 7      # kRadIntSpare: the parked mark
NAMES = (("pfc_radau_set_end", 3), ("pfc_radau_integrate", 4), ("pfc_radau_trajectory_rows", 2), ("pfc_radau_trajectory", 6),
         ("pfc_radau_finish_end_device", 34))


# ---- the statement ------------------------------------------------------------------------------------------------------------------
def arm_end(st):
    """The arming of k_radau_jac: exit flag 5 -- nothing; parked -- exit flag 6, attempts 0; else armed for a first attempt."""
    if st["istate"][EXIT] == 5:
        return
    if st["istate"][PARKED] != 0:
        st["istate"][EXIT], st["istate"][ATTEMPTS] = 6, 0
        return
    R.arm(st)


def set_end_scalar(xs, ts, recs, max_rows):
    """pfc_radau_set_end: the trajectories (lists of (t, x) rows) with row 0 = the state now; no scene is parked."""
    for st in recs:
        st["istate"][PARKED] = 0
    return [[(float(ts[s]), [float(e) for e in xs[s]])] if max_rows > 0 else [] for s in range(len(xs))]


def record_and_park(st, traj, x, t, t_final, max_rows):
    """What k_radau_finish<true> adds at a commit (after principal_value!): the row, the park decision.  Returns 1 if the scene goes
    on (it is counted live), 0 if it parked."""
    park = t_final < t                                  # strict: the reference's `if t_final < t_cumulative`
    if max_rows > 0:
        row = len(traj)
        if row < max_rows:
            traj.append((t, list(x)))
        if row + 1 >= max_rows:
            park = True
    if park:
        st["istate"][PARKED] = 1
        return 0
    return 1


def batch_step_end(de_batch, de_dual_batch, xs, ts, recs, trajs, t_final, max_rows, mrp_off=(), **par):
    """One batch step with ends, in the evaluation shapes of pfc_radau_step (R.radau_step_batch): the Jacobian of all n_scene scenes,
    the arming of the unparked ones, attempts until none is armed again -- a scene that is not iterating, parked ones included, is
    fed at its committed x --, and after each finish_scalar that committed, the row and the park decision.  Returns (xs, ts, live)."""
    p = dict(DEFAULTS, **par)
    ns, n = len(xs), len(xs[0])
    xs = [[float(e) for e in x] for x in xs]
    ts = list(ts)
    neg_J = [[[0.0] * n for _ in range(n)] for _ in range(ns)]
    xdot0 = None
    for j0 in range(0, n, p["n_chunk"]):
        seeds = [[1.0 if i == j else 0.0 for i in range(n)] for j in range(j0, min(j0 + p["n_chunk"], n))]
        xd, dxd = de_dual_batch(xs, seeds)
        if j0 == 0:
            xdot0 = [[float(e) for e in row] for row in xd]
        for s in range(ns):
            for d, col in enumerate(dxd[s]):
                for i in range(n):
                    neg_J[s][i][j0 + d] = -float(col[i])
    for st in recs:
        arm_end(st)
    X = [[list(xs[s]) for s in range(ns)] for _ in range(3)]
    F_keep = [[None] * ns for _ in range(3)]
    facs = [None] * ns
    live = 0
    iterating = lambda s: recs[s]["istate"][ITER] == 1
    while any(st["istate"][PHASE] == 1 for st in recs):
        for s in range(ns):
            if iterating(s):
                facs[s] = factor_scalar(neg_J[s], recs[s]["h"], recs[s]["rule"])
        while any(iterating(s) for s in range(ns)):
            rows = []
            for k in range(3):
                for s in range(ns):
                    start = recs[s]["istate"][KITER] == 0
                    if iterating(s) and start:
                        X[k][s] = list(xs[s])
                    rows.append(list(xs[s]) if (not iterating(s) or start) else list(X[k if recs[s]["rule"] == 2 else 0][s]))
            F = de_batch(rows)
            for s in range(ns):
                if iterating(s):
                    NS = 3 if recs[s]["rule"] == 2 else 1
                    for k in range(NS):
                        F_keep[k][s] = [float(e) for e in F[k * ns + s]]
                    newton_scalar(recs[s], facs[s], xs[s], [X[k][s] for k in range(NS)], [F_keep[k][s] for k in range(NS)],
                                  p["tol_newton"], p["k_iter_max"])
        for s in range(ns):
            st = recs[s]
            if st["istate"][PHASE] == 1 and st["istate"][ITER] == 0:
                NS = 3 if st["rule"] == 2 else 1
                xs[s], ts[s] = finish_scalar(st, facs[s], xs[s], ts[s], [X[k][s] for k in range(NS)], [F_keep[k][s] for k in range(NS)],
                                             xdot0[s], mrp_off, p["tol_a"], p["tol_r"], p["h_max"], p["h_min"], p["k_iter_max"],
                                             p["max_rule"], p["cooldown"])
                if st["istate"][PHASE] == 0 and st["istate"][EXIT] == 0:      # committed (not re-armed, not retired)
                    live += record_and_park(st, trajs[s], xs[s], ts[s], t_final[s], max_rows)
    return xs, ts, live


def integrate_batch(de_batch, de_dual_batch, xs, ts, recs, t_final, max_rows, max_steps, trajs=None, mrp_off=(), **par):
    """pfc_radau_set_end (unless `trajs` of an earlier call are handed back: the integration goes on) and pfc_radau_integrate: batch
    steps until no scene is live -- neither retired nor parked -- or max_steps were taken.  Returns (xs, ts, trajs, steps, live)."""
    if trajs is None:
        trajs = set_end_scalar(xs, ts, recs, max_rows)
    live = sum(1 for st in recs if st["istate"][EXIT] != 5 and st["istate"][PARKED] == 0)
    steps = 0
    while live > 0 and steps < max_steps:
        xs, ts, live = batch_step_end(de_batch, de_dual_batch, xs, ts, recs, trajs, t_final, max_rows, mrp_off, **par)
        steps += 1
    return xs, ts, trajs, steps, live


# ---- the reference's loop on one scene ---------------------------------------------------------------------------------------------
def scene_loop(de, de_dual, x, t, st, t_final, max_steps, **par):
    """integrate_scenario_radau on R.radau_step_scalar: rows (t, x); stops after the step that leaves t_final < t."""
    rows = [(float(t), [float(e) for e in x])]
    for _ in range(max_steps):
        x, t = R.radau_step_scalar(de, de_dual, x, t, st, **par)
        if st["istate"][EXIT] == 5:      # the reference throws here
            break
        rows.append((t, list(x)))
        if t_final < t:
            break
    return rows


def reference_loop(de, jac, x, t, rs, t_final, max_steps, **par):
    """The same loop on R.reference_step."""
    x = np.array(x, dtype=np.float64)
    rows = [(float(t), x.copy())]
    for _ in range(max_steps):
        x, h, _ = R.reference_step(de, jac, x, rs, **par)
        t = t + h
        rows.append((t, x.copy()))
        if t_final < t:
            break
    return rows


def _lift(de, de_dual):
    def dual_batch(rows, seeds):
        out = [de_dual(r, seeds) for r in rows]
        return [o[0] for o in out], [o[1] for o in out]
    return (lambda rows: [de(r) for r in rows]), dual_batch


def mid_gap(rows, k):
    """An end time in the middle of the gap before row k of a free run, and the assertion that no recorded t is nearer than 10 % of
    that step: the park decision cannot hinge on a rounding.  The scene then stops with k + 1 rows."""
    tf = 0.5 * (rows[k - 1][0] + rows[k][0])
    h = rows[k][0] - rows[k - 1][0]
    assert min(abs(tf - r[0]) for r in rows) >= 0.1 * h
    return tf


def _pendulum():
    m, l, g = 0.7, 0.4, 9.81
    mech = K.make_mech([-1], [K.REVOLUTE], [K.WORLD_X], [[0.0, 1.0, 0.0]])
    rec = D.make_inertia(m, [0.0, 0.0, -l], np.zeros((3, 3))).reshape(1, 13)
    return R._mech_de(mech, rec, (0.0, 0.0, -g))


def _stiff():
    return R._synthetic(lambda x: R.M_STIFF @ x, lambda x: R.M_STIFF)


def _records(h0, rule, cool=DEFAULTS["cooldown"]):
    st = new_records(h0=h0, cooldown=cool)
    st["rule"] = rule
    return st


def _moving(st):
    """What of a scene's records must stay byte for byte while it is parked."""
    return copy.deepcopy((st["h"], st["rule"], st["cool"], st["enorm"], st["nstate"]))


CASES = {
    # three pendulum scenes that need different iteration counts and (the third) attempts: R.test_the_batch_statement_is_..
    "pendulum": (_pendulum, [[0.9, -0.4], [0.0, 0.0], [2.5, 30.0]], [1e-4, 2e-3, 0.01], [2, 2, 2]),
    "stiff": (_stiff, [[1.0, -2.0], [0.5, 0.25], [-3.0, 1.0]], [1e-4, 2e-4, 5e-5], [1, 2, 1]),
}
MAX_ROWS = 6
STOP_ROW = [2, 4, None]      # scene 0 stops with 3 rows, scene 1 with 5, scene 2 by the row budget with 6


def _ends(de, de_dual, x0, h0, rules, cool):
    free = [scene_loop(de, de_dual, x0[s], 0.0, _records(h0[s], rules[s], cool), INF, MAX_ROWS - 1, cooldown=cool) for s in range(3)]
    assert all(len(f) == MAX_ROWS for f in free)
    return [INF if k is None else mid_gap(free[s], k) for s, k in enumerate(STOP_ROW)]


@pytest.mark.parametrize("case", sorted(CASES))
def test_integrate_batch_is_the_references_loop_scene_by_scene(case):
    make, x0, h0, rules = CASES[case]
    de, de_dual = make()
    cool = 2                                            # a rule change within the run
    t_final = _ends(de, de_dual, x0, h0, rules, cool)
    want = [scene_loop(de, de_dual, x0[s], 0.0, _records(h0[s], rules[s], cool), t_final[s], MAX_ROWS - 1, cooldown=cool) for s in range(3)]
    assert [len(w) for w in want] == [3, 5, 6]
    de_b, dual_b = _lift(de, de_dual)
    recs = [_records(h0[s], rules[s], cool) for s in range(3)]
    xs, ts, trajs, steps, live = integrate_batch(de_b, dual_b, x0, [0.0] * 3, recs, t_final, MAX_ROWS, 1, cooldown=cool)
    frozen = {}
    while live > 0:
        for s in range(3):
            if recs[s]["istate"][PARKED] and s not in frozen:
                frozen[s] = (_moving(recs[s]), list(xs[s]), ts[s], copy.deepcopy(trajs[s]), steps)
        xs, ts, trajs, more, live = integrate_batch(de_b, dual_b, xs, ts, recs, t_final, MAX_ROWS, 1, trajs=trajs, cooldown=cool)
        steps += more
    assert steps == 5 and trajs == want                 # equal as Python floats
    assert len({len(tr) for tr in trajs}) == 3
    assert [frozen[s][4] for s in (0, 1)] == [2, 4]     # the batch steps after which scenes 0 and 1 were parked
    for s, (mov, x, t, tr, _) in frozen.items():        # a parked scene's record is unchanged by the later batch steps
        assert _moving(recs[s]) == mov and xs[s] == x and ts[s] == t and trajs[s] == tr
        assert recs[s]["istate"][EXIT] == 6 and recs[s]["istate"][ATTEMPTS] == 0
    assert recs[2]["istate"][EXIT] == 0 and recs[2]["istate"][PARKED] == 1      # the arriving step's flag stays 0
    assert [tr[-1][0] for tr in trajs] == ts and [tr[-1][1] for tr in trajs] == xs
    # one call does what the single steps did
    recs1 = [_records(h0[s], rules[s], cool) for s in range(3)]
    one = integrate_batch(de_b, dual_b, x0, [0.0] * 3, recs1, t_final, MAX_ROWS, 100, cooldown=cool)
    assert one[2] == trajs and one[3:] == (5, 0) and one[0] == xs


@pytest.mark.parametrize("case", ["stiff", "decay"])
def test_the_same_loop_on_the_reference_restatement(case):
    """Row counts and the step at which each scene stops are equal; t and x agree to 1e-10 relative, the bound of R._both (the two
    differ in the conjugate factor, the solves and the pow: a few hundred roundings per step on well-conditioned 2 x 2 problems)."""
    if case == "stiff":
        de_np, jac = (lambda x: R.M_STIFF @ x), (lambda x: R.M_STIFF)
    else:
        de_np, jac = (lambda x: -x), (lambda x: -np.eye(2))
    _, x0, h0, rules = CASES["stiff"]
    de, de_dual = R._synthetic(de_np, jac)
    cool = 2
    t_final = _ends(de, de_dual, x0, h0, rules, cool)
    de_b, dual_b = _lift(de, de_dual)
    recs = [_records(h0[s], rules[s], cool) for s in range(3)]
    xs, ts, trajs, steps, live = integrate_batch(de_b, dual_b, x0, [0.0] * 3, recs, t_final, MAX_ROWS, MAX_ROWS - 1, cooldown=cool)
    assert (steps, live) == (5, 0)
    for s in range(3):
        ref = reference_loop(de_np, jac, x0[s], 0.0, R._ref_records(h0[s], rules[s], cool), t_final[s], MAX_ROWS - 1)
        assert len(ref) == len(trajs[s]) == [3, 5, 6][s]
        for (t, x), (tr, xr) in zip(trajs[s], ref):
            assert abs(t - tr) <= 1e-10 * max(abs(tr), 1e-300)
            assert np.abs(np.array(x) - xr).max() <= 1e-10 * max(1.0, np.abs(xr).max())


def test_edge_semantics():
    de, de_dual = _stiff()
    de_b, dual_b = _lift(de, de_dual)
    x0, h0 = [1.0, -2.0], 1e-4
    free = scene_loop(de, de_dual, x0, 0.0, _records(h0, 1), INF, 5)
    run = lambda t_final, max_rows, max_steps, t0=0.0, n=1: integrate_batch(
        de_b, dual_b, [x0] * n, [t0] * n, [_records(h0, 1) for _ in range(n)], t_final, max_rows, max_steps)
    # strict <: an end exactly on a recorded t does not stop the scene there; it takes one more step
    xs, ts, trajs, steps, live = run([free[2][0]], 10, 20)
    assert steps == 3 and live == 0 and trajs[0] == free[:4] and ts[0] == free[3][0] > free[2][0]
    # an end below the start time: the reference steps first and tests afterwards -- one step, two rows
    xs, ts, trajs, steps, live = run([0.1], 10, 20, t0=0.5)
    assert steps == 1 and live == 0 and len(trajs[0]) == 2 and trajs[0][0] == (0.5, x0) and ts[0] == 0.5 + h0
    # max_rows = 2: one step whatever the end
    xs, ts, trajs, steps, live = run([INF, 1.0], 2, 20, n=2)
    assert steps == 1 and live == 0 and [len(tr) for tr in trajs] == [2, 2] and trajs[0] == free[:2]
    # max_rows = 0: nothing is recorded, parking by time only; without an end the scene stays live
    xs, ts, trajs, steps, live = run([mid_gap(free, 3), INF], 0, 4, n=2)
    assert trajs == [[], []] and steps == 4 and live == 1 and ts == [free[3][0], free[4][0]] and xs[0] == free[3][1]
    # max_steps ends the call with the scenes live; the next call goes on
    recs = [_records(h0, 1)]
    a = integrate_batch(de_b, dual_b, [x0], [0.0], recs, [INF], 10, 2)
    assert a[3:] == (2, 1) and a[2][0] == free[:3]
    b = integrate_batch(de_b, dual_b, a[0], a[1], recs, [INF], 10, 3, trajs=a[2])
    assert b[3:] == (3, 1) and b[2][0] == free
    # nothing live: nothing is done
    recs[0]["istate"][PARKED] = 1
    before = copy.deepcopy(recs)
    c = integrate_batch(de_b, dual_b, b[0], b[1], recs, [INF], 10, 3, trajs=b[2])
    assert c[3:] == (0, 0) and recs == before


def test_a_retired_scene_records_nothing_and_is_not_live():
    # xdot = 1e10 with the Jacobian 0 (R.test_an_update_above_ten_..): every attempt diverges until h < h_min -- exit flag 5
    bad, bad_dual = R._synthetic(lambda x: np.array([1e10, 0.0]), lambda x: np.zeros((2, 2)))
    ok, ok_dual = _stiff()

    def de_b(rows):      # scene 0 of each stage is the bad one
        return [bad(r) if k % 2 == 0 else ok(r) for k, r in enumerate(rows)]

    def dual_b(rows, seeds):
        out = [(bad_dual if k % 2 == 0 else ok_dual)(r, seeds) for k, r in enumerate(rows)]
        return [o[0] for o in out], [o[1] for o in out]

    recs = [_records(1e-4, 1), _records(1e-4, 1)]
    xs, ts, trajs, steps, live = integrate_batch(de_b, dual_b, [[0.0, 0.0], [1.0, -2.0]], [0.0, 0.0], recs, [INF, INF], 4, 10)
    assert recs[0]["istate"][EXIT] == 5 and recs[0]["istate"][PARKED] == 0 and recs[0]["istate"][ATTEMPTS] == 5
    assert trajs[0] == [(0.0, [0.0, 0.0])] and xs[0] == [0.0, 0.0] and ts[0] == 0.0
    assert steps == 3 and live == 0 and len(trajs[1]) == 4
    free = scene_loop(ok, ok_dual, [1.0, -2.0], 0.0, _records(1e-4, 1), INF, 3)
    assert trajs[1] == free
    # alone, it ends the integration after the step that retired it
    recs = [_records(1e-4, 1)]
    out = integrate_batch(lambda rows: [bad(r) for r in rows], lambda rows, seeds: ([bad_dual(r, seeds)[0] for r in rows], [bad_dual(r, seeds)[1] for r in rows]),
                          [[0.0, 0.0]], [0.0], recs, [INF], 4, 10)
    assert out[3:] == (1, 0) and out[2] == [[(0.0, [0.0, 0.0])]]


# ---- exports ----------------------------------------------------------------------------------------------------------------------
def test_integrate_symbols_are_declared_exported_and_bound(pfc):
    hdr = open(os.path.join(ROOT, "include", "pfc.h")).read()
    assert "there is no per-scene stop" not in hdr
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
    for meth in ("radau_set_end", "radau_integrate", "radau_trajectory_rows", "radau_trajectory", "radau_finish_end_device",
                 "integrate_scenario_radau", "integrate_radau"):
        assert callable(getattr(M, meth)), meth
    rad = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc", "pfc_radau.h")).read()
    assert "fma(" not in rad
    assert "template <bool END> __global__ void __launch_bounds__(kRadWave) k_radau_finish(" in rad and "k_radau_set_end(" in rad
