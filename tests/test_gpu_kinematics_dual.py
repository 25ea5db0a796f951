"""Dual kinematics from joint states on the device (pfc_kinematics_dual[_device], pfc_eval_dual_state_device[_more]): bytes against the
scalar statement of tests/test_kinematics_dual_abi.py fed with the device's own cos / sin, NULL inputs and outputs, the host form and
a multi-device handle, that the call is not an evaluation, the chain (q, v) + seeds -> f_generalized + partials against its parts,
and the error paths.

Tolerances: the partials of poses, twists and Jacobians, the items and the seeds are compared as bytes (values; np.array_equal does
not tell -0.0 from 0.0), and so is everything computed from them under option fixed_order.  On a default handle C1's flat patches
take clamp decisions per pass, so there wrench, sdot and their partials are compared at the suite's 1e-9 relative
(tests/test_gpu_parity.py), counts exactly, and d_f, which is linear in those partials, at rtol = 1e-9."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import test_kinematics_abi as K
import test_kinematics_dual_abi as KD
from test_gpu_dual_seeds_from_bodies import C1, _eval_dual_bodies, _results, _seed_outputs
from test_gpu_items_from_bodies import Guarded, _dev, _outputs, _torch
from test_gpu_kinematics import _c1_state, _set, _states

pytestmark = pytest.mark.gpu


def _dense(mech, n_scene, n_dir, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (n_scene, n_dir, mech["nv"])), rng.uniform(-1, 1, (n_scene, n_dir, mech["nv"]))


def _unit(mech, n_scene, n_dir, first):
    """Unit seeds over the consecutive variables first .. first + n_dir of the state [q; v], as a Radau chunk seeds them."""
    nv = mech["nv"]
    s = np.zeros((n_scene, n_dir, 2 * nv))
    for k in range(n_dir):
        s[:, k, first + k] = 1.0
    return np.ascontiguousarray(s[:, :, :nv]), np.ascontiguousarray(s[:, :, nv:])


def _cases():
    """name -> (mechanism, q, v, dq, dv).  Mechanism (A) at 6, 30, 96, 66, 330 and 1 056 (scene, body, direction) lanes: a partial wave,
    across one wave boundary, across many; mechanism (C) at 11 x 3; and unit seeds across the boundary between q and v."""
    out = {}
    for n_scene in (1, 11):
        for n_dir in (1, 5, 16):
            m = K.mech_a()
            out[f"A{n_scene}x{n_dir}"] = (m, *_states(m, n_scene, 500 + n_scene), *_dense(m, n_scene, n_dir, 600 + 16 * n_scene + n_dir))
    m = K.mech_c()
    out["C11x3"] = (m, *_states(m, 11, 511), *_dense(m, 11, 3, 700))
    m = K.mech_a()
    out["A2x5unit"] = (m, *_states(m, 2, 512), *_unit(m, 2, 5, 7))      # q[7], q[8], q[9], v[0], v[1]
    return out


CASES = _cases()


def _sync():
    """The handle's stream does not wait for the allocations and fills torch runs on the default stream: order them by hand."""
    _torch().cuda.synchronize()


@pytest.fixture(scope="module")
def scen(pfc):
    """C1's scenario, its instructions bound to the bodies of mechanism (B); every test gives it the mechanism it needs."""
    w = pfc.configs.c1_boxes()
    m = pfc.configs.build_scenario(w)
    for k, c in enumerate(w.instructions):
        m.set_instruction_bodies(k, c.id_1, c.id_2)
    yield m
    m.close()


@pytest.fixture(scope="module")
def device_trig(pfc, scen):
    """{theta: (cos theta, sin theta)} as the device computes them, read the way tests/test_gpu_kinematics.py reads them: one body,
    revolute about e_z on the world with x_p_j = I, returns R00 = cos theta and R10 = sin theta exactly."""
    a = set()
    for mech, q, _, _, _ in CASES.values():
        for b, t in enumerate(mech["joint_type"]):
            if t == K.REVOLUTE:
                a.update(float(e) for e in q[:, mech["off"][b]])
    th = np.array(sorted(a))
    _set(scen, K.make_mech([-1], [K.REVOLUTE], [K.WORLD_X], [[0.0, 0.0, 1.0]]))
    x, _, _ = scen.kinematics(th.reshape(-1, 1), np.zeros((th.size, 1)), want_jac=False)
    x = x.reshape(th.size, 12)
    assert np.array_equal(x[:, [0, 1]], x[:, [4, 3]] * [1, -1]) and (x[:, [2, 5, 6, 7, 9, 10, 11]] == 0).all()
    return {float(t): (float(x[k, 0]), float(x[k, 1])) for k, t in enumerate(th)}


@pytest.fixture(scope="module")
def references(device_trig):
    """The statement's outputs for every case, computed once and left unchanged: rows of 12, 6 and 6."""
    out = {}
    for name, (mech, q, v, dq, dv) in CASES.items():
        r = KD.kin_dual_reference(mech, q, v, dq, dv, trig=device_trig)
        out[name] = [r[0].reshape(-1, 12), r[1].reshape(-1, 6), r[2].reshape(-1, 6)]
        for a in out[name]:
            a.setflags(write=False)
    return out


def _dual_outputs(mech, n_scene, n_dir):
    nbk = n_scene * mech["n_body"] * n_dir
    return [Guarded(nbk, 12), Guarded(nbk, 6), Guarded(nbk * mech["nv"], 6)]


# ---- 1. bytes of the statement, 3. NULL outputs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_dual_kinematics_is_the_bytes_of_the_scalar_statement(pfc, scen, references, case):
    mech, q, v, dq, dv = CASES[case]
    n_scene, n_dir = dq.shape[0], dq.shape[1]
    ref = references[case]
    _set(scen, mech)
    d_q, d_v, d_dq, d_dv = _dev(q), _dev(v), _dev(dq), _dev(dv)
    head = (n_scene, n_dir, d_q.data_ptr(), d_v.data_ptr(), d_dq.data_ptr(), d_dv.data_ptr())
    got = None
    for rep in range(2):      # a second call returns the same bytes
        out = _dual_outputs(mech, n_scene, n_dir)
        _sync()
        scen.kinematics_dual_device(*head, *[o.ptr for o in out])
        _sync()
        rows = [o.rows() for o in out]      # checks the guard words
        for name, g, r in zip(("d_x_w_b", "d_twist_w_b", "d_jac"), rows, ref):
            assert np.array_equal(g, r), (name, rep, np.argwhere(g != r)[:4])
        assert got is None or all(a.tobytes() == b.tobytes() for a, b in zip(got, rows))
        got = rows
    assert all(np.abs(g).max() > 0 for g in got)
    # an output passed as NULL is untouched, the others are the same bytes: states only, Jacobians only, and two mixed ones
    for want in ((1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 0)):
        part = _dual_outputs(mech, n_scene, n_dir)
        _sync()
        scen.kinematics_dual_device(*head, *[o.ptr if k else 0 for o, k in zip(part, want)])
        _sync()
        for o, k, g in zip(part, want, got):
            assert (o.rows().tobytes() == g.tobytes()) if k else o.untouched(), want


# ---- 2. NULL inputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A11x5", "C11x3"])
def test_null_seeds_are_the_bytes_of_zero_arrays(pfc, scen, case):
    mech, q, v, dq, dv = CASES[case]
    n_scene, n_dir = dq.shape[0], dq.shape[1]
    _set(scen, mech)
    d_q, d_v, d_dq, d_dv, d_z = _dev(q), _dev(v), _dev(dq), _dev(dv), _dev(np.zeros_like(dq))
    for p_dq, p_dv in ((0, d_dv.data_ptr()), (d_dq.data_ptr(), 0)):
        a, b = _dual_outputs(mech, n_scene, n_dir), _dual_outputs(mech, n_scene, n_dir)
        _sync()
        scen.kinematics_dual_device(n_scene, n_dir, d_q.data_ptr(), d_v.data_ptr(), p_dq, p_dv, *[o.ptr for o in a])
        scen.kinematics_dual_device(n_scene, n_dir, d_q.data_ptr(), d_v.data_ptr(), p_dq or d_z.data_ptr(), p_dv or d_z.data_ptr(),
                                    *[o.ptr for o in b])
        _sync()
        for u, w in zip(a, b):
            assert u.rows().tobytes() == w.rows().tobytes()
        assert np.abs(a[1].rows()).max() > 0
    # d_v NULL is allowed when no twist partial is wanted: poses and Jacobians do not read it
    a = _dual_outputs(mech, n_scene, n_dir)
    full = _dual_outputs(mech, n_scene, n_dir)
    _sync()
    scen.kinematics_dual_device(n_scene, n_dir, d_q.data_ptr(), 0, d_dq.data_ptr(), 0, a[0].ptr, 0, a[2].ptr)
    scen.kinematics_dual_device(n_scene, n_dir, d_q.data_ptr(), d_v.data_ptr(), d_dq.data_ptr(), d_dv.data_ptr(), *[o.ptr for o in full])
    _sync()
    assert a[1].untouched() and a[0].rows().tobytes() == full[0].rows().tobytes() and a[2].rows().tobytes() == full[2].rows().tobytes()


# ---- 4. the host form and a multi-device handle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A11x5", "C11x3"])
def test_host_form_and_multi_device_handle_return_the_same_bytes(pfc, scen, references, case):
    mech, q, v, dq, dv = CASES[case]
    ref = references[case]
    _set(scen, mech)
    got = scen.kinematics_dual(q, v, dq, dv)
    for g, r in zip(got, ref):
        assert np.array_equal(g.reshape(r.shape), r)
    no_jac = scen.kinematics_dual(q, v, dq, dv, want_jac=False)
    assert no_jac[2] is None and no_jac[0].tobytes() == got[0].tobytes() and no_jac[1].tobytes() == got[1].tobytes()
    m2 = pfc.configs.build_scenario(pfc.configs.c1_boxes(), devices=[0, 0])
    _set(m2, mech)
    multi = m2.kinematics_dual(q, v, dq, dv)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(multi, got))
    out = _dual_outputs(mech, dq.shape[0], dq.shape[1])
    d_q, d_v, d_dq, d_dv = _dev(q), _dev(v), _dev(dq), _dev(dv)
    _sync()
    m2.kinematics_dual_device(dq.shape[0], dq.shape[1], d_q.data_ptr(), d_v.data_ptr(), d_dq.data_ptr(), d_dv.data_ptr(), *[o.ptr for o in out])
    _sync()
    assert all(o.rows().tobytes() == g.tobytes() for o, g in zip(out, got))
    m2.close()


# ---- 5. not an evaluation -------------------------------------------------------------------------------------------------------
def test_kinematics_dual_is_not_an_evaluation(pfc, references):
    P = C1(pfc, 6, 1)      # fixed_order: _more returns the same bytes on every call
    n, nd = P.n, P.n_dir
    mech, q, v, dq, dv = CASES["A11x5"]
    _set(P.m, mech)
    items, seeds, res = _outputs(n), _seed_outputs(n, nd), _results(n, nd)
    _eval_dual_bodies(P, 0, items, seeds, res)
    dx, dtw, ds = (_dev(a) for a in P.chunks[1])
    seeds2 = _seed_outputs(n, nd)
    _sync()
    P.m.dual_seeds_from_bodies_device(*P.head(), dx.data_ptr(), dtw.data_ptr(), *[o.ptr for o in seeds2])
    more = lambda: P.m.eval_dual_device_more(nd, seeds2[0].ptr, seeds2[1].ptr, ds.data_ptr(), res[2].data_ptr(), res[3].data_ptr())
    more()
    assert P.m.check() == 0
    reused = P.m.last_dual_reused()
    first = (res[2].cpu().numpy().copy(), res[3].cpu().numpy().copy())
    assert np.abs(first[0]).max() > 0
    res[2].zero_(); res[3].zero_()
    out = _dual_outputs(mech, 11, 5)
    d_q, d_v, d_dq, d_dv = _dev(q), _dev(v), _dev(dq), _dev(dv)
    _sync()
    P.m.kinematics_dual_device(11, 5, d_q.data_ptr(), d_v.data_ptr(), d_dq.data_ptr(), d_dv.data_ptr(), *[o.ptr for o in out])
    assert P.m.check() == 0 and P.m.last_dual_reused() == reused
    more()
    assert P.m.check() == 0 and P.m.last_dual_reused() == reused
    _sync()
    for a, b in zip(first, (res[2].cpu().numpy(), res[3].cpu().numpy())):
        assert a.tobytes() == b.tobytes()
    for o, r in zip(out, references["A11x5"]):
        assert np.array_equal(o.rows(), r)
    P.m.close()


# ---- 6. the chain equals its parts ----------------------------------------------------------------------------------------------
N_SCENE, N_BODY, NV, N_ITEMS, N_DIR = 3, 5, 24, 12, 6


class Chain:
    """C1 bound to mechanism (B) on a handle of its own, 3 scenes x 4 items, and two chunks of 6 seed directions mixing q and v."""

    def __init__(self, pfc, fixed_order):
        torch = _torch()
        w = pfc.configs.c1_boxes()
        self.m = pfc.configs.build_scenario(w)
        if fixed_order:
            self.m.set_option("fixed_order", 1)
        for k, c in enumerate(w.instructions):
            self.m.set_instruction_bodies(k, c.id_1, c.id_2)
        mech, q0, v0, _, _ = _c1_state(pfc, True)
        _set(self.m, mech)
        rng = np.random.default_rng(81)
        q = np.tile(q0, (N_SCENE, 1)); v = np.tile(v0, (N_SCENE, 1))
        q[1:, :] += 1e-4 * rng.standard_normal((2, 24)); v[1:, :] += 0.05 * rng.standard_normal((2, 24))
        self.chunks = []
        for c in range(2):      # directions 0..2: configurations only, 3..4: velocities only, 5: both
            dq, dv = rng.uniform(-1, 1, (N_SCENE, N_DIR, NV)), rng.uniform(-1, 1, (N_SCENE, N_DIR, NV))
            dq[:, 3:5] = 0.0; dv[:, 0:3] = 0.0
            self.chunks.append((_dev(dq), _dev(dv)))
        ids = np.tile(np.arange(4, dtype=np.int32), N_SCENE); scene = np.repeat(np.arange(N_SCENE, dtype=np.int32), 4)
        self.d_q, self.d_v, self.d_ids, self.d_sc = _dev(q), _dev(v), _dev(ids), _dev(scene)
        nb, n, nd = N_SCENE * N_BODY, N_ITEMS, N_DIR
        z = lambda *sh, dt=torch.float64: torch.zeros(sh, dtype=dt, device=torch.device("cuda", 0))
        self.kin = [Guarded(nb, 12), Guarded(nb, 6), Guarded(nb * NV, 6)]
        self.dkin = [Guarded(nb * nd, 12), Guarded(nb * nd, 6), Guarded(nb * nd * NV, 6)]
        self.items = _outputs(n)
        self.seeds = _seed_outputs(n, nd)
        self.res = [z(n, 6), z(n, 6), z(n, nd, 6), z(n, nd, 6), z(n, 4, dt=torch.int32)]      # wrench, sdot, d_wrench, d_sdot, counts
        self.f, self.df = Guarded(N_SCENE, NV), Guarded(N_SCENE * nd, NV)

    def head(self):
        return (N_ITEMS, N_DIR, self.d_ids.data_ptr(), self.d_sc.data_ptr(), N_SCENE, self.d_q.data_ptr(), self.d_v.data_ptr())

    def checked(self, call):
        _sync()
        for _ in range(40):
            call()
            rc = self.m.check()
            if rc == 0:
                return
        raise AssertionError(f"pfc_check: {rc}")

    def chained(self, c, with_df=True):
        dq, dv = self.chunks[c]
        r = [t.data_ptr() for t in self.res]
        self.checked(lambda: self.m.eval_dual_state_device(
            *self.head(), dq.data_ptr(), dv.data_ptr(), 0, 0, *[o.ptr for o in self.kin], *[o.ptr for o in self.dkin],
            *[o.ptr for o in self.items], *[o.ptr for o in self.seeds], *r, self.f.ptr if with_df else 0, self.df.ptr if with_df else 0))

    def parts(self, c):
        dq, dv = self.chunks[c]
        r = [t.data_ptr() for t in self.res]
        _sync()
        self.m.kinematics_device(N_SCENE, self.d_q.data_ptr(), self.d_v.data_ptr(), *[o.ptr for o in self.kin])
        self.m.kinematics_dual_device(N_SCENE, N_DIR, self.d_q.data_ptr(), self.d_v.data_ptr(), dq.data_ptr(), dv.data_ptr(),
                                      *[o.ptr for o in self.dkin])
        self.checked(lambda: self.m.eval_dual_bodies_device(
            *self.head()[:5], N_BODY, self.kin[0].ptr, self.kin[1].ptr, self.dkin[0].ptr, self.dkin[1].ptr, 0, 0,
            *[o.ptr for o in self.items], *[o.ptr for o in self.seeds], *r))
        self.scatter(True)

    def scatter(self, with_f):
        self.m.scatter_generalized_dual_device(N_ITEMS, N_DIR, self.res[0].data_ptr(), self.res[2].data_ptr(), self.items[2].ptr,
                                               self.seeds[2].ptr, self.items[3].ptr, self.items[4].ptr, self.d_sc.data_ptr(), N_SCENE, NV,
                                               self.kin[2].ptr, self.dkin[2].ptr, self.f.ptr if with_f else 0, self.df.ptr)

    def chained_more(self, c):
        dq, dv = self.chunks[c]
        _sync()
        self.m.eval_dual_state_device_more(
            *self.head(), dq.data_ptr(), dv.data_ptr(), 0, *[o.ptr for o in self.kin], *[o.ptr for o in self.dkin],
            self.items[2].ptr, self.items[3].ptr, self.items[4].ptr, self.res[0].data_ptr(), *[o.ptr for o in self.seeds],
            self.res[2].data_ptr(), self.res[3].data_ptr(), self.df.ptr)
        assert self.m.check() == 0 and self.m.last_dual_reused()

    def parts_more(self, c):
        dq, dv = self.chunks[c]
        _sync()
        self.m.kinematics_dual_device(N_SCENE, N_DIR, self.d_q.data_ptr(), self.d_v.data_ptr(), dq.data_ptr(), dv.data_ptr(),
                                      *[o.ptr for o in self.dkin])
        self.m.eval_dual_bodies_device_more(*self.head()[:5], N_BODY, self.kin[0].ptr, self.kin[1].ptr, self.dkin[0].ptr, self.dkin[1].ptr, 0,
                                            *[o.ptr for o in self.seeds], self.res[2].data_ptr(), self.res[3].data_ptr())
        assert self.m.check() == 0
        self.scatter(False)

    def snapshot(self):
        """name -> host copy of every buffer (the guard words are checked)."""
        _sync()
        names = ("x_w_b", "twist_w_b", "jac", "d_x_w_b", "d_twist_w_b", "d_jac", "pose", "twist", "x_w_r2", "body_1", "body_2", "d_pose",
                 "d_twist", "d_x_w_r2")
        out = {k: o.rows().copy() for k, o in zip(names, self.kin + self.dkin + self.items + self.seeds)}
        out.update({k: t.cpu().numpy().copy() for k, t in zip(("wrench", "sdot", "d_wrench", "d_sdot", "counts"), self.res)})
        out["f"], out["d_f"] = self.f.rows().copy(), self.df.rows().copy()
        return out


VALUES = ("x_w_b", "twist_w_b", "jac", "pose", "twist", "x_w_r2", "body_1", "body_2", "wrench", "sdot", "counts", "f")
EXACT = ("x_w_b", "twist_w_b", "jac", "d_x_w_b", "d_twist_w_b", "d_jac", "pose", "twist", "x_w_r2", "body_1", "body_2", "d_pose", "d_twist",
         "d_x_w_r2", "counts")


def test_chain_equals_its_parts_fixed_order(pfc):
    A, B = Chain(pfc, 1), Chain(pfc, 1)
    A.chained(0)
    B.parts(0)
    a, b = A.snapshot(), B.snapshot()
    assert a["counts"][:, 3].all(), "an item has no contact"
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.abs(a["d_f"]).max() > 0 and np.abs(a["f"]).max() > 0 and np.abs(a["d_wrench"]).max() > 0
    # the kinematics it leaves are the statement's (mechanism (B) has no revolute joint: no trigonometry)
    q, v = A.d_q.cpu().numpy(), A.d_v.cpu().numpy()
    dq, dv = (t.cpu().numpy() for t in A.chunks[0])
    mech = _c1_state(pfc, True)[0]
    ref = KD.kin_dual_reference(mech, q, v, dq, dv)
    for k, r, wd in zip(("d_x_w_b", "d_twist_w_b", "d_jac"), ref, (12, 6, 6)):
        assert np.array_equal(a[k], r.reshape(-1, wd)), k
    # a different chunk at the kept point: only partials are written
    A.chained_more(1)
    B.parts_more(1)
    a1, b1 = A.snapshot(), B.snapshot()
    for k in a1:
        assert a1[k].tobytes() == b1[k].tobytes(), k
    for k in VALUES:
        assert a1[k].tobytes() == a[k].tobytes(), k      # _more writes no value output
    for k in ("d_x_w_b", "d_twist_w_b", "d_jac", "d_pose", "d_twist", "d_x_w_r2", "d_wrench", "d_f"):
        assert a1[k].tobytes() != a[k].tobytes(), k      # another chunk: other partials
    A.m.close(); B.m.close()


def test_chain_on_a_default_handle(pfc):
    A, B = Chain(pfc, 0), Chain(pfc, 0)
    A.chained(0)
    B.parts(0)
    a, b = A.snapshot(), B.snapshot()
    assert a["counts"][:, 3].all(), "an item has no contact"
    for k in EXACT:
        assert a[k].tobytes() == b[k].tobytes() if k != "counts" else np.array_equal(a[k], b[k]), k
    worst = {}
    for k in ("wrench", "sdot", "d_wrench", "d_sdot"):
        u, w = a[k].reshape(N_ITEMS, -1), b[k].reshape(N_ITEMS, -1)
        worst[k] = max([H.rel_err(u[i], w[i]) for i in range(N_ITEMS) if np.linalg.norm(w[i]) > 0] or [0.0])
        assert all(not u[i].any() for i in range(N_ITEMS) if np.linalg.norm(w[i]) == 0), k
    nz = b["d_f"] != 0
    worst["d_f"] = float((np.abs(a["d_f"] - b["d_f"])[nz] / np.abs(b["d_f"])[nz]).max())
    print("chained call against its parts on a default handle, largest relative difference: "
          + ", ".join(f"{k} {e:.2e}" for k, e in worst.items()))
    assert all(worst[k] < 1e-9 for k in ("wrench", "sdot", "d_wrench", "d_sdot"))
    assert np.abs(b["d_f"]).max() > 0
    np.testing.assert_allclose(a["d_f"], b["d_f"], rtol=1e-9, atol=0)
    # d_df = NULL: no scatter runs, guarded f and d_f are untouched, the rest is as before
    Cn = Chain(pfc, 0)
    Cn.chained(0, with_df=False)
    _sync()
    assert Cn.f.untouched() and Cn.df.untouched()
    for k, o in zip(EXACT[:14], Cn.kin + Cn.dkin + Cn.items + Cn.seeds):
        assert o.rows().tobytes() == a[k].tobytes(), k
    assert np.array_equal(Cn.res[4].cpu().numpy(), a["counts"])
    A.m.close(); B.m.close(); Cn.m.close()


def test_host_array_convenience_agrees_with_the_chained_call(pfc):
    """force_all_elastic_intersections_dual_state composes the host-buffer forms of the same calls: kinematics, their partials, items
    and seeds are the chained call's bytes, counts are equal; the wrenches come from another evaluation path (pfc_eval_dual), so they,
    f and d_f -- linear in them -- are held to the suite's 1e-9 relative, per item and per scene."""
    A = Chain(pfc, 0)
    A.chained(0)
    a = A.snapshot()
    q, v = A.d_q.cpu().numpy(), A.d_v.cpu().numpy()
    dq, dv = (t.cpu().numpy() for t in A.chunks[0])
    ids, scene = A.d_ids.cpu().numpy(), A.d_sc.cpu().numpy()
    wrench, sdot, dw, dsd, counts, f, d_f, it, sd, kin, dkin = A.m.force_all_elastic_intersections_dual_state(
        q, v, None, dq, dv, ins_ids=ids, scene=scene)
    for k, got in zip(("x_w_b", "twist_w_b", "jac", "d_x_w_b", "d_twist_w_b", "d_jac", "pose", "twist", "x_w_r2", "body_1", "body_2",
                       "d_pose", "d_twist", "d_x_w_r2"),
                      list(kin) + list(dkin) + [it.pose, it.twist, it.x_w_r2, it.body_1, it.body_2, sd.d_pose, sd.d_twist, sd.d_x_w_r2]):
        assert np.ascontiguousarray(got).tobytes() == a[k].tobytes(), k
    assert np.array_equal(counts, a["counts"])
    for k, got in (("wrench", wrench), ("d_wrench", dw)):
        u, w = got.reshape(N_ITEMS, -1), a[k].reshape(N_ITEMS, -1)
        assert max(H.rel_err(u[i], w[i]) for i in range(N_ITEMS)) < 1e-9, k
    assert f.shape == (N_SCENE, NV) and d_f.shape == (N_SCENE, N_DIR, NV)
    for s in range(N_SCENE):
        assert H.rel_err(f[s], a["f"][s]) < 1e-9 and H.rel_err(d_f[s], a["d_f"].reshape(N_SCENE, N_DIR, NV)[s]) < 1e-9, s
    A.m.close()


# ---- 7. error paths -------------------------------------------------------------------------------------------------------------
def test_error_paths_write_nothing(pfc):
    """Every refused call returns before a launch: the guarded outputs are untouched."""
    torch = _torch()
    L = pfc._lib
    lib = L.lib()
    mech, q, v, dq, dv = CASES["C11x3"]
    d_q, d_v, d_dq, d_dv = _dev(q), _dev(v), _dev(dq), _dev(dv)
    out = _dual_outputs(mech, 11, 3)
    h = C.c_void_p()
    assert lib.pfc_create(0, C.byref(h)) == 0
    msg = lambda: lib.pfc_last_error(h).decode()

    def call(n_dir=3, p_v=d_v.data_ptr(), outs=None):
        o = outs or [x.ptr for x in out]
        return lib.pfc_kinematics_dual_device(h, 11, n_dir, d_q.data_ptr(), p_v, d_dq.data_ptr(), d_dv.data_ptr(), *o, None)

    _sync()
    assert call() == L.ERR_STATE and "pfc_set_mechanism" in msg()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    keep = (np.ascontiguousarray(mech["parent"], dtype=np.int32), np.ascontiguousarray(mech["joint_type"], dtype=np.int32),
            np.ascontiguousarray(mech["x_p_j"], dtype=np.float64), np.ascontiguousarray(mech["axis"], dtype=np.float64))
    assert lib.pfc_set_mechanism(h, 4, keep[0].ctypes.data_as(ip), keep[1].ctypes.data_as(ip), keep[2].ctypes.data_as(dp),
                                 keep[3].ctypes.data_as(dp)) == 0
    assert call(n_dir=0) == L.ERR_BAD_ARG and "n_dir" in msg()
    assert call(n_dir=17) == L.ERR_BAD_ARG and "n_dir" in msg()
    assert call(p_v=None) == L.ERR_BAD_ARG                                  # d_v NULL with a twist partial wanted
    assert lib.pfc_kinematics_dual_device(h, 0, 3, None, None, None, None, *[x.ptr for x in out], None) == 0      # n_scene = 0: a no-op
    torch.cuda.synchronize()
    assert all(o.untouched() for o in out)
    lib.pfc_destroy(h)

    # the chained calls: _more without a checked evaluation; an instruction bound to body 9 of a 5-body mechanism
    P = Chain(pfc, 0)
    dq1, dv1 = P.chunks[0]
    r = [Guarded(N_ITEMS, 6), Guarded(N_ITEMS, 6), Guarded(N_ITEMS * N_DIR, 6), Guarded(N_ITEMS * N_DIR, 6), Guarded(N_ITEMS, 4, True)]
    # (the value buffers _more reads are never read here: the call is refused first)
    _sync()
    rc = lib.pfc_eval_dual_state_device_more(
        P.m._h, *P.head(), dq1.data_ptr(), dv1.data_ptr(), None, *[o.ptr for o in P.kin], *[o.ptr for o in P.dkin], P.items[2].ptr,
        P.items[3].ptr, P.items[4].ptr, r[0].ptr, *[o.ptr for o in P.seeds], r[2].ptr, r[3].ptr, P.df.ptr, None)
    assert rc == L.ERR_STATE and "no checked" in lib.pfc_last_error(P.m._h).decode()
    torch.cuda.synchronize()
    assert all(o.untouched() for o in P.kin + P.dkin + P.items + P.seeds + r + [P.f, P.df])
    P.m.set_instruction_bodies(3, 9, 4)
    rc = lib.pfc_eval_dual_state_device(
        P.m._h, *P.head(), dq1.data_ptr(), dv1.data_ptr(), None, None, *[o.ptr for o in P.kin], *[o.ptr for o in P.dkin],
        *[o.ptr for o in P.items], *[o.ptr for o in P.seeds], *[o.ptr for o in r], P.f.ptr, P.df.ptr, None)
    assert rc == L.ERR_BAD_ARG and "instruction 3" in lib.pfc_last_error(P.m._h).decode()
    rc = lib.pfc_eval_dual_state_device(
        P.m._h, N_ITEMS, 17, *P.head()[2:], dq1.data_ptr(), dv1.data_ptr(), None, None, *[o.ptr for o in P.kin], *[o.ptr for o in P.dkin],
        *[o.ptr for o in P.items], *[o.ptr for o in P.seeds], *[o.ptr for o in r], P.f.ptr, P.df.ptr, None)
    assert rc == L.ERR_BAD_ARG
    torch.cuda.synchronize()
    assert all(o.untouched() for o in P.kin + P.dkin + P.items + P.seeds + r + [P.f, P.df])
    P.m.close()
