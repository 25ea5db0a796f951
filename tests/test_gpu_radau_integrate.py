"""Integration to per-scene end times on the device (pfc_radau_set_end, pfc_radau_integrate, pfc_radau_trajectory[_rows],
pfc_radau_finish_end_device): bytes against the scalar statement of tests/test_radau_integrate_abi.py.

An evaluation's last bits depend on the batch it is part of, even under fixed_order, so no trajectory is compared with the same scene
integrated alone or with a loop in which parked scenes keep moving: the statement (S.integrate_batch) is driven by the host-form
state_derivative / state_derivative_dual of a second fixed_order handle, in the step's own evaluation shapes with parked scenes at
their committed x.  End times lie in the middle of a gap between the statement's t values (S.mid_gap asserts the distance), so no park
decision hinges on a rounding."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_radau as G
import test_radau_abi as R
import test_radau_integrate_abi as S
from test_gpu_items_from_bodies import SENTINEL, Guarded, _dev, _torch

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
INF = float("inf")
BOX_R = G.BOX_R
_bits = G._bits


@pytest.fixture(scope="module")
def scen(pfc):
    m = pfc.configs.build_scenario(pfc.configs.c1_boxes())
    yield m
    m.close()


def _host_de_batch(m):
    """de_batch and de_dual_batch of S.integrate_batch from the host forms of a handle, one item (instruction 0) per scene: the
    evaluation shapes of pfc_radau_step (tests/test_gpu_radau.py::_host_de_batch)."""
    def split(rows):
        x = np.asarray(rows, dtype=np.float64)
        return x[:, 0:6], x[:, 6:12], x[:, 12:18], [0] * x.shape[0], np.arange(x.shape[0], dtype=np.int32)

    def de_batch(rows):
        q, v, s, ids, sc = split(rows)
        qd, vd, sd, info = m.state_derivative(q, v, s, ins_ids=ids, scene=sc)[:4]
        assert not info.any()
        return np.concatenate([qd, vd, sd], axis=1).tolist()

    def de_dual_batch(rows, seeds):
        q, v, s, ids, sc = split(rows)
        n, nd = q.shape[0], len(seeds)
        sd_a = np.tile(np.array(seeds, dtype=np.float64)[None], (n, 1, 1))
        qd, vd, sd, dqd, dvd, dsd, info = m.state_derivative_dual(q, v, s, sd_a[:, :, 0:6], sd_a[:, :, 6:12], sd_a[:, :, 12:18],
                                                                    ins_ids=ids, scene=sc)[:7]
        assert not info.any()
        dsd = np.asarray(dsd).reshape(n, nd, 6)
        return (np.concatenate([qd, vd, sd], axis=1).tolist(),
                [[np.concatenate([dqd[k, d], dvd[k, d], dsd[k, d]]).tolist() for d in range(nd)] for k in range(n)])

    return de_batch, de_dual_batch


def _traj_arrays(traj):
    return np.array([r[0] for r in traj], dtype=np.float64), np.array([r[1] for r in traj], dtype=np.float64).reshape(len(traj), -1)


def _assert_state_is(m, xs, ts, recs, what):
    x, t = m.radau_get_state()
    rs = m.radau_rule_state()
    assert _bits(x) == _bits(np.array(xs)), (what, np.abs(x - np.array(xs)).max())
    assert _bits(t) == _bits(np.array(ts)), what
    assert _bits(rs["h"]) == _bits(np.array([r["h"] for r in recs])), what
    assert rs["rule"].tolist() == [r["rule"] for r in recs] and rs["cooldown"].tolist() == [r["cool"] for r in recs], what
    assert _bits(rs["x_err_norm"]) == _bits(np.array([r["enorm"][0] for r in recs])), what
    assert _bits(rs["x_err_norm_next"]) == _bits(np.array([r["enorm"][1] for r in recs])), what


def _assert_trajectories_are(m, trajs, what):
    assert m.radau_trajectory_rows().tolist() == [len(tr) for tr in trajs], what
    for s, tr in enumerate(trajs):
        t, x = m.radau_trajectory(s)
        e_t, e_x = _traj_arrays(tr)
        assert _bits(t) == _bits(e_t), (what, s)
        assert _bits(x) == _bits(e_x), (what, s, np.abs(x - e_x).max())


def _snapshot(m):
    rs = m.radau_rule_state()
    x, t = m.radau_get_state()
    return b"".join(_bits(a) for a in (x, t, rs["h"], rs["rule"], rs["cooldown"], rs["theta"], rs["psi_k"], rs["x_err_norm"],
                                       rs["x_err_norm_next"]))


# ---- 1. the part ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [1, 18, 64])
def test_finish_end_part_is_bytes_and_the_jacobian_part_arms_the_unparked(scen, nx):
    """Six scenes: 0 commits and goes on (its end is exactly the new t: the comparison is strict), 1 parks by time, 2 parks on its
    last row, 3 fails and is armed again (no row), 4 retires with flag 5 (no row), 5 is parked already (no word of it changes)."""
    torch = _torch()
    n_scene, max_rows = 6, 4
    lay = G.layout(n_scene, nx)
    nq, nv, n_ips, br = lay[2], lay[3], lay[4], lay[5]
    mrp = [0] if nq >= 3 else []
    rng = np.random.default_rng(40 + nx)
    neg_J = rng.standard_normal((n_scene, nx, nx)) * 20.0
    h = np.array([1e-4, 2e-4, 3e-4, 1e-4, 5e-8, 1e-4])
    rules = np.array([1, 2, 1, 2, 1, 2], dtype=np.int32)
    cool = np.array([5, 3, 1, 7, 4, 2], dtype=np.int32)
    fac_dev = G._factor_on_device(scen, neg_J, h, rules)
    facs = G._factor_reference(neg_J, h, rules)
    F = G._synthetic_F(lay, rng)
    x = rng.standard_normal((n_scene, nx)) * 0.3
    X = np.tile(x, (3, 1)) + 1e-3 * rng.standard_normal((3 * n_scene, nx))
    if mrp:
        X[0, :3] = [0.9, -0.8, 0.3]                                        # scene 0 (rule 1): the row holds x after principal_value!
    xdot0 = rng.standard_normal((n_scene, nx))
    t = 0.1 * np.arange(n_scene)
    t_final = np.array([t[0] + h[0], t[1] + 0.5 * h[1], INF, 0.0, INF, 0.0])
    rows0 = np.array([1, 1, 3, 2, 1, 2], dtype=np.int32)
    enorm = rng.uniform(0.1, 1.0, (n_scene, 2))
    recs = [R.new_records() for _ in range(n_scene)]
    for s, r in enumerate(recs):
        R.arm(r)
        r["h"], r["rule"], r["cool"], r["enorm"] = float(h[s]), int(rules[s]), int(cool[s]), [float(e) for e in enorm[s]]
        r["istate"][R.ITER], r["istate"][R.KITER] = 0, 3 + s
    for s, f in enumerate([0, 0, 0, 3, 1, 0]):
        recs[s]["istate"][R.FLAG] = f
    recs[5]["istate"][R.PHASE], recs[5]["istate"][R.EXIT], recs[5]["istate"][R.ATTEMPTS], recs[5]["istate"][S.PARKED] = 0, 6, 0, 1
    nstate, istate = G._records_arrays(recs)
    d_F = _dev(np.array([G._F_of(lay, *F, ss) for ss in range(3 * n_scene)]))
    bufs = [Guarded(n_scene, nx), Guarded(n_scene, 1), Guarded(n_scene, 1), Guarded(n_scene, 1, True), Guarded(n_scene, 1, True),
            Guarded(n_scene, 2), Guarded(n_scene, 8), Guarded(n_scene, 8, True), Guarded(1, 1, True)]
    for b, a in zip(bufs, (x, t, h, rules, cool, enorm, nstate, istate)):
        b.t[16:16 + a.size] = _dev(a.reshape(-1))
    traj, g_rows, g_live = Guarded(n_scene * max_rows, 1 + nx), Guarded(n_scene, 1, True), Guarded(1, 1, True)      # traj: poison everywhere
    g_rows.t[16:16 + n_scene] = _dev(rows0)
    g_live.t[16:17] = _dev(np.array([7], dtype=np.int32))                  # the call adds to it
    d_xdot0, d_X, d_tf = _dev(xdot0), _dev(X), _dev(t_final)
    scen.radau_finish_end_device(lay, mrp, (1e-4, 1e-4, 0.01, 1e-8), 15, 2, 10, d_F.data_ptr(), d_xdot0.data_ptr(), d_X.data_ptr(),
                                 fac_dev[0].ptr, fac_dev[2].ptr, *[b.ptr for b in bufs], d_tf.data_ptr(), traj.ptr, g_rows.ptr, max_rows,
                                 g_live.ptr)
    torch.cuda.synchronize()
    # the statement
    e_x, e_t = x.copy(), t.copy()
    e_traj = np.full((n_scene, max_rows, 1 + nx), SENTINEL)
    trajs = [[None] * int(k) for k in rows0]
    live = 7
    for s, r in enumerate(recs):
        NS = 3 if rules[s] == 2 else 1
        Xs = [[float(e) for e in X[k * n_scene + s]] for k in range(NS)]
        Fs = [G._F_of(lay, *F, k * n_scene + s) for k in range(NS)]
        was_open = r["istate"][R.PHASE] == 1
        e_x[s], e_t[s] = R.finish_scalar(r, facs[s], [float(e) for e in x[s]], float(t[s]), Xs, Fs, [float(e) for e in xdot0[s]], mrp_off=tuple(mrp))
        if was_open and r["istate"][R.PHASE] == 0 and r["istate"][R.EXIT] == 0:
            live += S.record_and_park(r, trajs[s], [float(e) for e in e_x[s]], float(e_t[s]), float(t_final[s]), max_rows)
            e_traj[s, len(trajs[s]) - 1] = [trajs[s][-1][0]] + trajs[s][-1][1]
    e_n, e_i = G._records_arrays(recs)
    assert [r["istate"][R.EXIT] for r in recs] == [0, 0, 0, 3, 5, 6] and [r["istate"][S.PARKED] for r in recs] == [0, 1, 1, 0, 0, 1]
    assert [len(tr) for tr in trajs] == [2, 2, 4, 2, 1, 2] and live == 8
    if mrp:
        assert e_traj[0, 1, 1] == -(0.9 / ((0.9 * 0.9 + 0.8 * 0.8) + 0.3 * 0.3))
    got = [b.rows() for b in bufs]
    assert _bits(got[0]) == _bits(e_x) and _bits(got[1]) == _bits(e_t)
    assert _bits(got[2]) == _bits(np.array([r["h"] for r in recs])), (got[2], [r["h"] for r in recs])
    assert got[3].tolist() == [r["rule"] for r in recs] and got[4].tolist() == [r["cool"] for r in recs]
    assert _bits(got[5]) == _bits(np.array([r["enorm"] for r in recs]))
    assert _bits(got[6].reshape(e_n.shape)) == _bits(e_n) and np.array_equal(got[7].reshape(e_i.shape), e_i), (got[7], e_i)
    assert int(got[8][0]) == 1                                             # scene 3 was armed for another attempt
    assert g_rows.rows().tolist() == [len(tr) for tr in trajs] and int(g_live.rows()[0]) == live
    assert _bits(traj.rows()) == _bits(e_traj), np.argwhere(traj.rows().reshape(e_traj.shape) != e_traj)[:4]
    # the Jacobian part, chunk 0, on these records: it arms exactly the unparked scenes that are not retired
    n_dir = min(6, nx)
    dqd, dvd = rng.standard_normal((n_scene, n_dir, nq)), rng.standard_normal((n_scene, n_dir, nv))
    dsd = rng.standard_normal((n_scene, n_ips, n_dir, 6))
    qd, vd, sd = rng.standard_normal((n_scene, nq)), rng.standard_normal((n_scene, nv)), rng.standard_normal((n_scene * n_ips, 6))
    d_in = [_dev(a) for a in (dqd, dvd, dsd, qd, vd, sd)]
    g_J, g_xd = Guarded(n_scene, nx * nx), Guarded(n_scene, nx)
    scen.radau_jacobian_device(lay, 0, 6, *[a.data_ptr() if a.numel() else 0 for a in d_in], g_J.ptr, g_xd.ptr, bufs[6].ptr, bufs[7].ptr)
    torch.cuda.synchronize()
    for r in recs:
        S.arm_end(r)
    e_n, e_i = G._records_arrays(recs)
    assert e_i[:, R.ITER].tolist() == [1, 0, 0, 1, 0, 0] and e_i[:, R.EXIT].tolist() == [0, 6, 6, 3, 5, 6]
    assert e_i[:, R.ATTEMPTS].tolist()[1:3] == [0, 0]
    assert _bits(bufs[6].rows().reshape(e_n.shape)) == _bits(e_n) and np.array_equal(bufs[7].rows().reshape(e_i.shape), e_i), (bufs[7].rows(), e_i)
    g_J.rows(); g_xd.rows()                                                # guard words


# ---- 2, 3. a whole integration ----------------------------------------------------------------------------------------------------
MAX_ROWS, STOP_ROW = 6, [2, 4, None]      # scene 0 stops with 3 rows, scene 1 with 5, scene 2 on its row budget with 6


def _three_boxes():
    """1 mm and 2 mm in the ground, and one released 1 cm above it."""
    return G._box_states(3, [BOX_R - 1e-3, BOX_R - 2e-3, BOX_R + 1e-2], [0.0, -0.02, 0.0])


def _start(m, x0, rules=(2, 1, 1)):
    m.radau_configure(len(x0), [0], cooldown=2)
    m.radau_set_state(x0)
    m.radau_set_rule_state(rule=list(rules))


def _statement_records(rules=(2, 1, 1)):
    recs = [R.new_records(cooldown=2) for _ in rules]
    for r, rule in zip(recs, rules):
        r["rule"] = rule
    return recs


@pytest.fixture(scope="module")
def whole(pfc):
    """The statement's integration of the three boxes, computed once: a free run whose t values decide the two finite end times, then
    the run to those ends."""
    B = G._box_scenario(pfc, True)
    de_batch, de_dual_batch = _host_de_batch(B)
    x0 = _three_boxes()
    start = [x0[s].tolist() for s in range(3)]
    free = S.integrate_batch(de_batch, de_dual_batch, start, [0.0] * 3, _statement_records(), [INF] * 3, MAX_ROWS, MAX_ROWS - 1,
                             mrp_off=(0,), cooldown=2)
    assert [len(tr) for tr in free[2]] == [MAX_ROWS] * 3
    t_final = [INF if k is None else S.mid_gap(free[2][s], k) for s, k in enumerate(STOP_ROW)]
    recs = _statement_records()
    rules_run = []      # the rules at the start of every batch step

    xs, ts, trajs, steps, live = start, [0.0] * 3, None, 0, 3
    while live > 0 and steps < 12:
        rules_run.append([r["rule"] for r in recs])
        xs, ts, trajs, more, live = S.integrate_batch(de_batch, de_dual_batch, xs, ts, recs, t_final, MAX_ROWS, 1, trajs=trajs,
                                                      mrp_off=(0,), cooldown=2)
        steps += more
    for s, k in enumerate(STOP_ROW):      # the ends are still mid-gap in the run they were used in
        if k is not None:
            tr = trajs[s]
            assert len(tr) == k + 1 and min(abs(t_final[s] - r[0]) for r in tr) >= 0.1 * (tr[k][0] - tr[k - 1][0])
    B.close()
    return dict(x0=x0, t_final=t_final, xs=xs, ts=ts, trajs=trajs, recs=recs, steps=steps, live=live, rules_run=rules_run)


def test_whole_integration_is_the_statement_in_bytes(pfc, whole):
    A = G._box_scenario(pfc, True)
    _start(A, whole["x0"])
    A.radau_set_end(whole["t_final"], MAX_ROWS)
    assert A.radau_trajectory_rows().tolist() == [1, 1, 1]
    steps, live = A.radau_integrate(12)
    assert (steps, live) == (whole["steps"], 0) and whole["live"] == 0 and steps == 5
    rows = A.radau_trajectory_rows().tolist()
    assert rows == [3, 5, 6] and len(set(rows)) == 3
    _assert_trajectories_are(A, whole["trajs"], "trajectories")
    _assert_state_is(A, whole["xs"], whole["ts"], whole["recs"], "final state")
    assert whole["rules_run"][0] == [2, 1, 1] and any(r[1] == 2 or r[2] == 2 for r in whole["rules_run"]), whole["rules_run"]      # both rules, a change
    before = _snapshot(A)
    out = A.radau_step()                                                   # every scene is parked: nothing is done
    assert out["flags"].tolist() == [6, 6, 6] and out["attempts"].tolist() == [0, 0, 0] and out["h_taken"].tolist() == [0.0, 0.0, 0.0]
    assert _snapshot(A) == before and A.radau_trajectory_rows().tolist() == rows
    assert A.radau_integrate(3) == (0, 0)
    A.close()


def test_whole_integration_on_a_default_handle_stops_at_the_same_rows(pfc, whole):
    """Atomic sums: row counts are those of the fixed_order run, and every row is within 1e-3 in the step's own error norm (Eq. 8.21
    with the step's tol_a, tol_r), the bound tests/test_gpu_radau.py::test_step_box_on_plane.. uses for default against fixed_order."""
    Cd = G._box_scenario(pfc, False)
    _start(Cd, whole["x0"])
    Cd.radau_set_end(whole["t_final"], MAX_ROWS)
    steps, live = Cd.radau_integrate(12)
    assert (steps, live) == (5, 0) and Cd.radau_trajectory_rows().tolist() == [len(tr) for tr in whole["trajs"]]
    for s, tr in enumerate(whole["trajs"]):
        t, x = Cd.radau_trajectory(s)
        e_t, e_x = _traj_arrays(tr)
        sc = 1e-4 + np.maximum(np.abs(x), np.abs(e_x)) * 1e-4
        norm = np.sqrt((((x - e_x) / sc) ** 2).sum(axis=1) / 18)
        print("scene", s, "default vs statement: error norm per row", norm, "t difference", np.abs(t - e_t).max())
        assert (norm <= 1e-3).all(), (s, norm)
    Cd.close()


# ---- 4. no end --------------------------------------------------------------------------------------------------------------------
def test_integrate_without_an_end_is_three_steps(pfc):
    x0 = G._box_states(2, [BOX_R - 1e-3, BOX_R - 2e-3], [0.0, -0.02])
    snaps = []
    for mode in ("steps", "integrate", "set_end(None, 0)"):
        m = G._box_scenario(pfc, True)
        _start(m, x0, (2, 1))
        if mode == "steps":
            for _ in range(3):
                assert m.radau_step()["flags"].tolist() == [0, 0]
        else:
            if mode != "integrate":
                m.radau_set_end(None, 0)
                assert m.radau_trajectory_rows().tolist() == [0, 0]
            assert m.radau_integrate(3) == (3, 2)
        snaps.append(_snapshot(m))
        m.close()
    assert snaps[0] == snaps[1] == snaps[2]


# ---- 5. a retry beside a parked scene -------------------------------------------------------------------------------------------
def test_retry_beside_a_parked_scene_is_the_statement(pfc):
    """The forced-retry input of tests/test_gpu_radau.py (attempts [3, 1]) next to a free-falling scene that starts at h = 0.01 and
    ends at t = 0.005: its first step parks it.  In the second batch step it is evaluated at its committed x while scene 0 moves."""
    A, B = G._box_scenario(pfc, True), G._box_scenario(pfc, True)
    x0 = np.zeros((2, 18))
    x0[0, 5], x0[0, 11] = BOX_R - 1e-4, -3.0
    x0[1, 5], x0[1, 11] = 1.0, -0.3
    de_batch, de_dual_batch = _host_de_batch(B)
    recs = [R.new_records(h0=0.01) for _ in range(2)]
    for r in recs:
        r["rule"] = 2
    t_final, max_rows = [INF, 0.005], 4
    A.radau_configure(2, [0], h0=0.01)
    A.radau_set_state(x0)
    A.radau_set_rule_state(rule=2)
    A.radau_set_end(t_final, max_rows)
    out = A.radau_step()
    xs, ts, trajs, steps, live = S.integrate_batch(de_batch, de_dual_batch, [x0[0].tolist(), x0[1].tolist()], [0.0, 0.0], recs, t_final,
                                                   max_rows, 1, mrp_off=(0,))
    assert (steps, live) == (1, 1) and ts[1] == 0.01 and recs[1]["istate"][S.PARKED] == 1
    assert out["attempts"].tolist() == [r["istate"][R.ATTEMPTS] for r in recs] == [3, 1] and out["flags"].tolist() == [0, 0]
    assert A.radau_trajectory_rows().tolist() == [2, 2]
    _assert_state_is(A, xs, ts, recs, "batch step 1")
    _assert_trajectories_are(A, trajs, "batch step 1")
    x1, t1 = A.radau_get_state()
    out = A.radau_step()
    xs, ts, trajs, steps, live = S.integrate_batch(de_batch, de_dual_batch, xs, ts, recs, t_final, max_rows, 1, trajs=trajs, mrp_off=(0,))
    assert (steps, live) == (1, 1)
    assert out["flags"].tolist() == [r["istate"][R.EXIT] for r in recs] == [0, 6]
    assert out["attempts"].tolist() == [r["istate"][R.ATTEMPTS] for r in recs] and out["attempts"][1] == 0 and out["h_taken"][1] == 0.0
    assert out["iters"][0] == recs[0]["istate"][R.EXITITER]
    x2, t2 = A.radau_get_state()
    assert _bits(x2[1]) == _bits(x1[1]) and t2[1] == t1[1] and t2[0] > t1[0]      # only scene 0 has moved
    assert A.radau_trajectory_rows().tolist() == [3, 2]
    _assert_state_is(A, xs, ts, recs, "batch step 2")
    _assert_trajectories_are(A, trajs, "batch step 2")
    A.close(); B.close()


# ---- 6. the public call -----------------------------------------------------------------------------------------------------------
def test_integrate_scenario_radau_and_two_fresh_handles_agree(pfc):
    x0 = G._box_states(2, [BOX_R - 1e-3, BOX_R + 0.01], [0.0, -0.1], seed=9)
    t_final = np.array([1.1e-3, 5e-4])      # in the gaps of 1e-4 (2^k - 1), the t values while h doubles
    res = []
    for _ in range(2):
        m = G._box_scenario(pfc, True)
        m.radau_configure(2, [0], n_chunk=16)
        m.radau_set_state(x0)
        res.append(m.integrate_scenario_radau(t_final, max_steps=40))
        m.close()
    for s in range(2):
        (t_a, x_a), (t_b, x_b) = res[0][s], res[1][s]
        assert _bits(t_a) == _bits(t_b) and _bits(x_a) == _bits(x_b)
        assert 2 <= t_a.size < 41 and x_a.shape == (t_a.size, 18)
        assert (np.diff(t_a) > 0).all() and t_a[-1] > t_final[s] and (t_a[:-1] <= t_final[s]).all()
        assert t_a[0] == 0.0 and _bits(x_a[0]) == _bits(x0[s])
    assert res[0][0][0].size != res[0][1][0].size                          # the scenes stopped at different rows
    # the scalar form: one end for every scene
    m = G._box_scenario(pfc, True)
    m.radau_configure(2, [0], n_chunk=16)
    m.radau_set_state(x0)
    out = m.integrate_scenario_radau(5e-4, max_steps=2)                    # the row budget stops both: max_steps + 1 rows
    assert [o[0].size for o in out] == [3, 3] and all(o[0][-1] <= 5e-4 for o in out)      # t <= 1e-4 + 2e-4: h at most doubles
    m.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(pfc):
    L = pfc._lib
    import ctypes as C
    dp = C.POINTER(C.c_double)

    def refused(call, status, word):
        with pytest.raises(L.PFCError) as e:
            call()
        assert e.value.status == status and word in str(e.value), str(e.value)

    m = G._box_scenario(pfc, True)
    refused(lambda: m.radau_set_end(None, 4), L.ERR_STATE, "pfc_radau_configure")
    refused(lambda: m.radau_integrate(1), L.ERR_STATE, "pfc_radau_configure")
    x0 = G._box_states(2, [BOX_R - 1e-3, BOX_R - 2e-3], [0.0, -0.02])
    m.radau_configure(2, [0])
    refused(lambda: m.radau_set_end(None, 4), L.ERR_STATE, "pfc_radau_set_state")
    m.radau_set_state(x0)
    refused(lambda: m.radau_trajectory_rows(), L.ERR_STATE, "pfc_radau_set_end")
    refused(lambda: m.radau_trajectory(0), L.ERR_STATE, "pfc_radau_set_end")
    m.radau_set_end(None, 5)
    assert m.radau_integrate(2) == (2, 2)

    def everything():
        return _snapshot(m) + _bits(m.radau_trajectory_rows()) + b"".join(_bits(a) for s in range(2) for a in m.radau_trajectory(s))

    before = everything()
    assert m.radau_trajectory_rows().tolist() == [3, 3]
    for call, word in ((lambda: m.radau_set_end([0.1, float("nan")], 5), "NaN"), (lambda: m.radau_set_end(None, -1), "max_rows"),
                       (lambda: m.radau_set_end([0.1, 0.2], 1), "max_rows"), (lambda: m.radau_integrate(-1), "max_steps")):
        refused(call, L.ERR_BAD_ARG, word)
        assert everything() == before, word                                # the end, the rows and the state are what they were
    t_buf, x_buf = np.full(8, SENTINEL), np.full((8, 18), SENTINEL)
    for scene, row0, n in ((-1, 0, 1), (2, 0, 1), (0, -1, 1), (0, 0, -1), (0, 0, 4), (1, 3, 1), (0, 2, 2)):
        rc = L.lib().pfc_radau_trajectory(m._h, scene, row0, n, t_buf.ctypes.data_as(dp), x_buf.ctypes.data_as(dp))
        assert rc == L.ERR_BAD_ARG, (scene, row0, n, rc)
        assert (t_buf == SENTINEL).all() and (x_buf == SENTINEL).all() and everything() == before, (scene, row0, n)
    # what was refused did not end the integration: it goes on from where it was
    assert m.radau_integrate(1) == (1, 2) and m.radau_trajectory_rows().tolist() == [4, 4]
    m.close()


# ---- 8. ownership -----------------------------------------------------------------------------------------------------------------
_SIZES = [2 * k * 19 * 8 for k in (5, 11, 7, 13)]      # n_scene x max_rows x (1 + NX) doubles of the child's four trajectories


def child():
    """The child process: two ends of different sizes, an end without a trajectory, a third, a reconfiguration, a fourth, the close."""
    import pfc_pkg
    pfc = pfc_pkg.load()
    m = G._box_scenario(pfc)
    x0 = G._box_states(2, [BOX_R - 1e-3, BOX_R - 2e-3], [0.0, -0.02])
    m.radau_configure(2, [0])
    m.radau_set_state(x0)
    m.radau_set_end(None, 5)
    assert m.radau_integrate(1) == (1, 2)
    m.radau_set_end([1.0, 2.0], 11)
    m.radau_set_end(None, 0)
    m.radau_set_end(None, 7)
    m.radau_configure(2, [0], n_chunk=16)
    m.radau_set_state(x0)
    m.radau_set_end(None, 13)
    assert m.radau_integrate(1) == (1, 2) and m.radau_trajectory_rows().tolist() == [2, 2]
    m.close()


def test_every_trajectory_block_is_freed_once():
    env = dict(os.environ, PFC_LOG_ALLOC="1")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_gpu_radau_integrate as t; t.child()"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    alloc = re.compile(r"^pfc alloc (0x[0-9a-f]+) \.\. 0x[0-9a-f]+ \((\d+) bytes, element 8\)$")
    free = re.compile(r"^pfc free (0x[0-9a-f]+)$")
    live, blocks, most = {}, [], 0
    for ln in r.stderr.splitlines():
        a, f = alloc.match(ln), free.match(ln)
        if a and int(a.group(2)) in _SIZES:
            assert a.group(1) not in live, ln
            live[a.group(1)] = int(a.group(2))
            blocks.append(int(a.group(2)))
            most = max(most, len(live))
        elif f and f.group(1) in live:
            del live[f.group(1)]
    assert blocks == _SIZES, blocks                                        # each end allocated its block, in the order of the calls
    assert not live and most <= 2, (live, most)                            # the old block goes when the new one is there; none is left
