"""Dual forward dynamics on the device (pfc_dynamics_dual[_device], pfc_accelerations_dual[_device],
pfc_state_derivative_dual_device[_more]): bytes against the scalar statements of tests/test_dynamics_dual_abi.py fed with the device's
cos / sin, NULL inputs and outputs, the host forms and other handles, value parity of the solve, the refusals, the per-scene pivot
flag, that the calls are not evaluations, and the chains against their parts.

Tolerances: dqdot, dH, dc, vdot, dvdot and info are compared as bytes.  The byte comparisons feed pfc_dynamics_dual_device the poses,
twists and their partials of the statement itself (kin_reference / kin_dual_reference with the device's trigonometry), so that both
sides start from the same bytes; the run from the device's own kinematics is compared as values (np.array_equal), as
tests/test_gpu_kinematics_dual.py compares those.  Under option fixed_order every buffer of a chain is the bytes of its parts; on a
default handle f and d_f are summed with atomics, so there vdot, dvdot and what feeds them are held to the suite's 1e-9 relative."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import test_dynamics_abi as D
import test_dynamics_dual_abi as DD
import test_kinematics_abi as K
import test_kinematics_dual_abi as KD
from test_gpu_dual_seeds_from_bodies import _seed_outputs
from test_gpu_dynamics import CASES, _c4_slice, chain_mech, device_trig, scen      # noqa: F401 (the two fixtures)
from test_gpu_items_from_bodies import Guarded, _dev, _outputs, _torch
from test_gpu_kinematics import _c1_state, _raw_mech, _set, _states

pytestmark = pytest.mark.gpu


def _sync():
    _torch().cuda.synchronize()


def _dense(nv, n_scene, n_dir, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (n_scene, n_dir, nv)), rng.uniform(-1, 1, (n_scene, n_dir, nv))


def _unit(nv, n_scene, n_dir, first):
    s = np.zeros((n_scene, n_dir, 2 * nv))
    for k in range(n_dir):
        s[:, k, first + k] = 1.0
    return np.ascontiguousarray(s[:, :, :nv]), np.ascontiguousarray(s[:, :, nv:])


def _dual_cases():
    """name -> (mechanism, inertia, q, v, dq, dv): the value cases of tests/test_gpu_dynamics.py (their angles are what its device_trig
    reads) cut to the smallest shapes at which the Dual kernels can go wrong -- (A) at 1 and 11 scenes with 1, 6 and 16 directions
    (one workgroup, and n_dir accumulators from one to all sixteen), nv = 1, nv = 6, two floating bodies, the chain (C), unit seeds
    across the boundary between q and v, and the 64-link chain, where the Dual tables fill 57.6 kB of LDS and every lane owns a row."""
    out = {}
    for n in (1, 11):
        for nd in (1, 6, 16):
            m, inertia, q, v = CASES["A%d" % n]
            out[f"A{n}x{nd}"] = (m, inertia, q, v, *_dense(m["nv"], n, nd, 900 + 16 * n + nd))
    for name, ns, nd in (("rev1", 3, 2), ("float6", 3, 6), ("B2", 2, 3), ("C11", 3, 4)):
        m, inertia, q, v = CASES[name]
        out[f"{name}x{nd}"] = (m, inertia, q[:ns], v[:ns], *_dense(m["nv"], ns, nd, 950 + nd))
    m, inertia, q, v = CASES["A10"]
    out["A2x5unit"] = (m, inertia, q[:2], v[:2], *_unit(m["nv"], 2, 5, 7))      # q[7], q[8], q[9], v[0], v[1]
    m, inertia, q, v = CASES["cap64"]
    out["cap64x2"] = (m, inertia, q[:2], v[:2], *_dense(64, 2, 2, 990))
    return out


DCASES = _dual_cases()
_REF = {}


def _reference(case, trig):
    """Everything the statements give for a case, computed once and left unchanged."""
    if case not in _REF:
        mech, inertia, q, v, dq, dv = DCASES[case]
        ns, nd, nv = dq.shape[0], dq.shape[1], mech["nv"]
        x, tw, _ = K.kin_reference(mech, q, v, trig)
        dx, dtw, _ = KD.kin_dual_reference(mech, q, v, dq, dv, trig)
        _, Hm, c = D.dyn_reference(mech, inertia, D.GRAVITY, q, v, trig)
        dqd, dH, dc = DD.dyn_dual_reference(mech, inertia, D.GRAVITY, q, v, dq, dv, trig)
        rng = np.random.default_rng(5)
        f, tau, df, dtau = rng.standard_normal((ns, nv)), rng.standard_normal((ns, nv)), rng.standard_normal((ns, nd, nv)), rng.standard_normal((ns, nd, nv))
        sol = [DD.chol_dual_scalar(Hm[s], c[s], f[s], dH[s], dc[s], df[s], tau[s], dtau[s]) for s in range(ns)]
        sol0 = [DD.chol_dual_scalar(Hm[s], c[s], f[s], dH[s], dc[s], df[s], tau[s], None) for s in range(ns)]
        r = dict(x=x, tw=tw, dx=dx, dtw=dtw, H=Hm, c=c, dqd=dqd, dH=dH, dc=dc, f=f, tau=tau, df=df, dtau=dtau,
                 vd=np.array([s[0] for s in sol]), dvd=np.array([s[1] for s in sol]), info=np.array([s[2] for s in sol], dtype=np.int32),
                 dvd0=np.array([s[1] for s in sol0]))
        for a in r.values():
            a.setflags(write=False)
        _REF[case] = r
    return _REF[case]


def _dyn_dual_outputs(ns, nd, nv):
    return [Guarded(ns * nd, nv), Guarded(ns * nd * nv, nv), Guarded(ns * nd, nv)]


# ---- bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(DCASES))
def test_dual_dynamics_and_accelerations_are_the_bytes_of_the_scalar_statements(pfc, scen, device_trig, case):
    mech, inertia, q, v, dq, dv = DCASES[case]
    ns, nd, nv = dq.shape[0], dq.shape[1], mech["nv"]
    R = _reference(case, device_trig)
    ref = [R["dqd"].reshape(ns * nd, nv), R["dH"].reshape(ns * nd * nv, nv), R["dc"].reshape(ns * nd, nv)]
    _set(scen, mech)
    scen.set_inertia(inertia, D.GRAVITY)
    d_q, d_v, d_dq, d_dv = _dev(q), _dev(v), _dev(dq), _dev(dv)
    d_x, d_tw, d_dx, d_dtw = _dev(R["x"]), _dev(R["tw"]), _dev(R["dx"]), _dev(R["dtw"])
    head = (ns, nd, d_q.data_ptr(), d_v.data_ptr(), d_dq.data_ptr(), d_dv.data_ptr(), d_x.data_ptr(), d_tw.data_ptr(), d_dx.data_ptr(),
            d_dtw.data_ptr())
    got = None
    for rep in range(2):      # a second call returns the same bytes
        out = _dyn_dual_outputs(ns, nd, nv)
        _sync()
        scen.dynamics_dual_device(*head, *[o.ptr for o in out])
        _sync()
        rows = [o.rows().reshape(r.shape) for o, r in zip(out, ref)]      # checks the guard words
        for name, g, r in zip(("dqdot", "dH", "dc"), rows, ref):
            assert g.tobytes() == r.tobytes(), (name, rep, np.argwhere(g != r)[:4], np.abs(g - r).max())
        got = rows
    assert all(np.abs(g).max() > 0 for g in got)
    # each output NULL in turn: untouched, the others the same bytes
    for skip in range(3):
        part = _dyn_dual_outputs(ns, nd, nv)
        _sync()
        scen.dynamics_dual_device(*head, *[0 if k == skip else o.ptr for k, o in enumerate(part)])
        _sync()
        for k, (o, g) in enumerate(zip(part, got)):
            assert o.untouched() if k == skip else o.rows().reshape(g.shape).tobytes() == g.tobytes(), (skip, k)
    # from the device's own kinematics and their partials: the same values
    nb = ns * mech["n_body"]
    kin = [Guarded(nb, 12), Guarded(nb, 6)]
    dkin = [Guarded(nb * nd, 12), Guarded(nb * nd, 6)]
    out = _dyn_dual_outputs(ns, nd, nv)
    _sync()
    scen.kinematics_device(ns, d_q.data_ptr(), d_v.data_ptr(), kin[0].ptr, kin[1].ptr, 0)
    scen.kinematics_dual_device(ns, nd, d_q.data_ptr(), d_v.data_ptr(), d_dq.data_ptr(), d_dv.data_ptr(), dkin[0].ptr, dkin[1].ptr, 0)
    scen.dynamics_dual_device(*head[:6], kin[0].ptr, kin[1].ptr, dkin[0].ptr, dkin[1].ptr, *[o.ptr for o in out])
    _sync()
    for name, o, g in zip(("dqdot", "dH", "dc"), out, got):
        assert np.array_equal(o.rows().reshape(g.shape), g), name
    # the solve and its partials
    d_H, d_c, d_f, d_tau, d_df, d_dtau = (_dev(R[k]) for k in ("H", "c", "f", "tau", "df", "dtau"))
    d_dH, d_dc = _dev(R["dH"]), _dev(R["dc"])
    d_zero = _dev(np.zeros((ns, nd, nv)))

    def solve(p_dtau, want_vdot=True, want_info=True):
        vd, dvd, info = Guarded(ns, nv), Guarded(ns * nd, nv), Guarded(ns, 1, True)
        _sync()
        scen.accelerations_dual_device(ns, nd, d_H.data_ptr(), d_c.data_ptr(), d_f.data_ptr(), d_tau.data_ptr(), d_dH.data_ptr(),
                                       d_dc.data_ptr(), d_df.data_ptr(), p_dtau, vd.ptr if want_vdot else 0, dvd.ptr,
                                       info.ptr if want_info else 0)
        _sync()
        return vd, dvd, info

    for rep in range(2):
        vd, dvd, info = solve(d_dtau.data_ptr())
        assert vd.rows().reshape(ns, nv).tobytes() == R["vd"].tobytes() and np.array_equal(info.rows(), R["info"])
        assert dvd.rows().reshape(ns, nd, nv).tobytes() == R["dvd"].tobytes(), np.argwhere(dvd.rows().reshape(ns, nd, nv) != R["dvd"])[:4]
    # value parity: vdot is pfc_accelerations_device's bytes
    vv, vi = Guarded(ns, nv), Guarded(ns, 1, True)
    scen.accelerations_device(ns, d_H.data_ptr(), d_c.data_ptr(), d_f.data_ptr(), d_tau.data_ptr(), vv.ptr, vi.ptr)
    _sync()
    assert vv.rows().tobytes() == vd.rows().tobytes() and np.array_equal(vi.rows(), info.rows())
    # d_dtau NULL: the bytes of a zero array, and of the statement; d_vdot and d_info NULL: untouched, dvdot the same
    a, b = solve(0), solve(d_zero.data_ptr())
    assert a[1].rows().tobytes() == b[1].rows().tobytes() == R["dvd0"].reshape(ns * nd, nv).tobytes()
    vd2, dvd2, info2 = solve(d_dtau.data_ptr(), want_vdot=False, want_info=False)
    assert vd2.untouched() and info2.untouched() and dvd2.rows().tobytes() == dvd.rows().tobytes()
    # the host forms; d_dq / d_dv NULL
    h_out = scen.dynamics_dual(q, v, dq, dv, R["x"], R["tw"], R["dx"], R["dtw"])
    assert all(a.tobytes() == r.tobytes() for a, r in zip(h_out, ref))
    hv, hdv, hi = scen.accelerations_dual(R["H"], R["c"], R["f"], R["dH"], R["dc"], R["df"], R["tau"], R["dtau"])
    assert hv.tobytes() == R["vd"].tobytes() and hdv.tobytes() == R["dvd"].tobytes() and np.array_equal(hi, R["info"])
    if case in ("A11x6", "C11x4"):
        zq = _dev(np.zeros_like(dq))
        for p_dq, p_dv in ((0, d_dv.data_ptr()), (d_dq.data_ptr(), 0)):
            a, b = _dyn_dual_outputs(ns, nd, nv), _dyn_dual_outputs(ns, nd, nv)
            _sync()
            scen.dynamics_dual_device(ns, nd, head[2], head[3], p_dq, p_dv, *head[6:], *[o.ptr for o in a])
            scen.dynamics_dual_device(ns, nd, head[2], head[3], p_dq or zq.data_ptr(), p_dv or zq.data_ptr(), *head[6:], *[o.ptr for o in b])
            _sync()
            assert all(u.rows().tobytes() == w.rows().tobytes() for u, w in zip(a, b))
        for kw in ({}, {"devices": [0, 0]}):      # a fresh handle, and one over the devices [0, 0]: the same bytes
            m2 = pfc.configs.build_scenario(pfc.configs.c1_boxes(), **kw)
            _set(m2, mech)
            m2.set_inertia(inertia, D.GRAVITY)
            m_out = m2.dynamics_dual(q, v, dq, dv, R["x"], R["tw"], R["dx"], R["dtw"])
            assert all(a.tobytes() == r.tobytes() for a, r in zip(m_out, ref))
            mv, mdv, mi = m2.accelerations_dual(R["H"], R["c"], R["f"], R["dH"], R["dc"], R["df"], R["tau"], R["dtau"])
            assert mv.tobytes() == R["vd"].tobytes() and mdv.tobytes() == R["dvd"].tobytes() and np.array_equal(mi, R["info"])
            m2.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(pfc):
    L = pfc._lib
    lib = L.lib()
    h = C.c_void_p()
    assert lib.pfc_create(0, C.byref(h)) == 0
    msg = lambda: lib.pfc_last_error(h).decode()
    dp = C.POINTER(C.c_double)
    grav = np.array(D.GRAVITY)
    mech = K.mech_c()
    q, v = _states(mech, 2, 9)
    inertia = D.random_inertia(mech, np.random.default_rng(1))
    nd = 3
    d_q, d_v = _dev(q), _dev(v)
    d_dq, d_dv = (_dev(a) for a in _dense(4, 2, nd, 1))
    z = lambda *sh: _dev(np.zeros(sh))
    d_x, d_tw, d_dx, d_dtw = z(8, 12), z(8, 6), z(8 * nd, 12), z(8 * nd, 6)
    out = _dyn_dual_outputs(2, nd, 4)

    def dyn(n_dir=nd, p_dx=d_dx.data_ptr(), n_scene=2):
        return lib.pfc_dynamics_dual_device(h, n_scene, n_dir, d_q.data_ptr(), d_v.data_ptr(), d_dq.data_ptr(), d_dv.data_ptr(),
                                            d_x.data_ptr(), d_tw.data_ptr(), p_dx, d_dtw.data_ptr(), *[o.ptr for o in out], None)

    _sync()
    assert dyn() == L.ERR_STATE and "pfc_set_mechanism" in msg()
    keep, ptr = _raw_mech(mech)
    assert lib.pfc_set_mechanism(h, 4, *ptr) == 0
    assert dyn() == L.ERR_STATE and "pfc_set_inertia" in msg()
    assert lib.pfc_set_inertia(h, 4, inertia.ctypes.data_as(dp), grav.ctypes.data_as(dp)) == 0
    assert dyn(n_dir=0) == L.ERR_BAD_ARG and "n_dir" in msg()
    assert dyn(n_dir=17) == L.ERR_BAD_ARG and "n_dir" in msg()
    assert dyn(p_dx=None) == L.ERR_BAD_ARG and "null input" in msg()
    assert dyn(n_scene=0) == 0                                                    # a no-op
    acc = [Guarded(2, 4), Guarded(2 * nd, 4), Guarded(2, 1, True)]
    zz = z(2 * nd * 16)
    accel = lambda n_dir, p_df: lib.pfc_accelerations_dual_device(h, 2, n_dir, zz.data_ptr(), zz.data_ptr(), zz.data_ptr(), None, zz.data_ptr(),
                                                                  zz.data_ptr(), p_df, None, acc[0].ptr, acc[1].ptr, acc[2].ptr, None)
    assert accel(0, zz.data_ptr()) == L.ERR_BAD_ARG and accel(17, zz.data_ptr()) == L.ERR_BAD_ARG and accel(nd, None) == L.ERR_BAD_ARG
    _sync()
    assert all(o.untouched() for o in out + acc)

    # nv = 65: the solve refuses.  73 revolute links: 73 x 900 bytes of Dual tables exceed 64 KiB -- the Dual call refuses, the value
    # call on the same mechanism runs; 72 links (64 800 bytes) run in Dual.
    for n, dual_ok in ((65, True), (73, False), (72, True)):
        big = chain_mech(n)
        keep2, ptr2 = _raw_mech(big)
        assert lib.pfc_set_mechanism(h, n, *ptr2) == 0
        rec = D.random_inertia(big, np.random.default_rng(2))
        assert lib.pfc_set_inertia(h, n, rec.ctypes.data_as(dp), grav.ctypes.data_as(dp)) == 0
        qb, vb = _states(big, 1, 3)
        x, tw, _ = K.kin_reference(big, qb, vb)
        dx, dtw, _ = KD.kin_dual_reference(big, qb, vb, np.ones((1, 1, n)), None)
        b_q, b_v, b_x, b_tw, b_dx, b_dtw, b_dq = (_dev(a) for a in (qb, vb, x, tw, dx, dtw, np.ones((1, 1, n))))
        val = [Guarded(1, n), Guarded(n, n), Guarded(1, n)]
        par = _dyn_dual_outputs(1, 1, n)
        _sync()
        assert lib.pfc_dynamics_device(h, 1, b_q.data_ptr(), b_v.data_ptr(), b_x.data_ptr(), b_tw.data_ptr(), *[o.ptr for o in val], None) == 0
        rc = lib.pfc_dynamics_dual_device(h, 1, 1, b_q.data_ptr(), b_v.data_ptr(), b_dq.data_ptr(), None, b_x.data_ptr(), b_tw.data_ptr(), b_dx.data_ptr(),
                                          b_dtw.data_ptr(), *[o.ptr for o in par], None)
        _sync()
        assert np.isfinite(val[1].rows()).all() and np.abs(val[1].rows()).max() > 0
        if dual_ok:
            assert rc == 0
            dH = par[1].rows()
            assert np.isfinite(dH).all() and dH.tobytes() == np.ascontiguousarray(dH.T).tobytes()
        else:
            assert rc == L.ERR_BAD_ARG and "LDS" in msg()
            assert all(o.untouched() for o in par)
        if n == 65:
            vd, dvd, info = Guarded(1, n), Guarded(1, n), Guarded(1, 1, True)
            rc = lib.pfc_accelerations_dual_device(h, 1, 1, val[1].ptr, val[2].ptr, val[2].ptr, None, par[1].ptr, par[2].ptr, par[2].ptr, None,
                                                   vd.ptr, dvd.ptr, info.ptr, None)
            assert rc == L.ERR_BAD_ARG and "PFC_MAX_NV_SOLVE" in msg()
            _sync()
            assert vd.untouched() and dvd.untouched() and info.untouched()
    lib.pfc_destroy(h)


# ---- a failed pivot is a per-scene flag ----------------------------------------------------------------------------------------
def test_a_massless_scene_among_good_ones(pfc, scen):
    mech = K.mech_c()
    q, v = _states(mech, 3, 31)
    q[:, 1] = 0.0                                   # the revolute joint at angle 0: cos = 1, sin = 0 on any libm
    rng = np.random.default_rng(32)
    good = D.random_inertia(mech, rng)
    bad = good.copy(); bad[3] = 0.0                 # the last finger massless: pivot 4 is zero
    nd = 3
    dq, dv = _dense(4, 3, nd, 33)
    _set(scen, mech)
    f, df = rng.standard_normal((3, 4)), rng.standard_normal((3, nd, 4))
    scen.set_inertia(good, D.GRAVITY)
    _, Hg, cg = scen.dynamics(q, v)
    _, dHg, dcg = scen.dynamics_dual(q, v, dq, dv)
    scen.set_inertia(bad, D.GRAVITY)
    _, Hb, cb = scen.dynamics(q, v)
    _, dHb, dcb = scen.dynamics_dual(q, v, dq, dv)
    assert Hb[1, 3, 3] == 0.0
    Hm, cm, dHm, dcm = Hg.copy(), cg.copy(), dHg.copy(), dcg.copy()
    Hm[1], cm[1], dHm[1], dcm[1] = Hb[1], cb[1], dHb[1], dcb[1]
    vd, dvd, info = scen.accelerations_dual(Hm, cm, f, dHm, dcm, df)
    assert scen.check() == 0                         # not an error state
    gv, gdv, gi = scen.accelerations_dual(Hg, cg, f, dHg, dcg, df)
    assert np.array_equal(info, [0, 4, 0]) and not gi.any()
    nan = np.full(4, np.nan).tobytes()
    assert vd[1].tobytes() == nan and all(dvd[1, d].tobytes() == nan for d in range(nd))
    for s in (0, 2):
        assert vd[s].tobytes() == gv[s].tobytes() and dvd[s].tobytes() == gdv[s].tobytes()
        r = DD.chol_dual_scalar(Hg[s], cg[s], f[s], dHg[s], dcg[s], df[s])
        assert r[2] == 0 and vd[s].tobytes() == r[0].tobytes() and dvd[s].tobytes() == r[1].tobytes()


# ---- the chains ----------------------------------------------------------------------------------------------------------------
class Rig:
    """A scenario bound to a mechanism with inertias, n_scene scenes, two chunks of N_DIR seed directions and every buffer of the
    Dual chain behind guard words."""
    N_DIR = 6

    def __init__(self, pfc, which, fixed_order):
        torch = _torch()
        if which == "C1":
            w = pfc.configs.c1_boxes()
            self.m = pfc.configs.build_scenario(w)
            for k, c in enumerate(w.instructions):
                self.m.set_instruction_bodies(k, c.id_1, c.id_2)
            mech, q0, v0, _, _ = _c1_state(pfc, True)
            rng = np.random.default_rng(81)
            q = np.tile(q0, (3, 1)); v = np.tile(v0, (3, 1))
            q[1:, :] += 1e-4 * rng.standard_normal((2, 24)); v[1:, :] += 0.05 * rng.standard_normal((2, 24))
            inertia = D.random_inertia(mech, rng)
            ids, scene = np.tile(np.arange(4, dtype=np.int32), 3), np.repeat(np.arange(3, dtype=np.int32), 4)
        else:
            self.m, mech, inertia, q, v, ids, scene = _c4_slice(pfc)
        if fixed_order:
            self.m.set_option("fixed_order", 1)
        _set(self.m, mech)
        self.m.set_inertia(inertia, D.GRAVITY)
        self.mech, self.inertia, self.q, self.v, self.ids, self.scene = mech, inertia, q, v, ids, scene
        ns, n_body, nv, n, nd = q.shape[0], mech["n_body"], mech["nv"], ids.size, self.N_DIR
        self.ns, self.nv, self.n = ns, nv, n
        rng = np.random.default_rng(82)
        self.tau, self.dtau = rng.standard_normal((ns, nv)), rng.standard_normal((ns, nd, nv))
        self.chunks = []
        for c in range(2):      # directions 0..2: configurations only, 3..4: velocities only, 5: both
            dq, dv = rng.uniform(-1, 1, (ns, nd, nv)), rng.uniform(-1, 1, (ns, nd, nv))
            dq[:, 3:5] = 0.0; dv[:, 0:3] = 0.0
            self.chunks.append((dq, dv, _dev(dq), _dev(dv)))
        self.d_q, self.d_v, self.d_ids, self.d_sc, self.d_tau, self.d_dtau = (_dev(a) for a in (q, v, ids, scene, self.tau, self.dtau))
        nb = ns * n_body
        z = lambda *sh, dt=torch.float64: torch.zeros(sh, dtype=dt, device=torch.device("cuda", 0))
        self.kin = [Guarded(nb, 12), Guarded(nb, 6), Guarded(nb * nv, 6)]
        self.dkin = [Guarded(nb * nd, 12), Guarded(nb * nd, 6), Guarded(nb * nd * nv, 6)]
        self.items = _outputs(n)
        self.seeds = _seed_outputs(n, nd)
        self.res = [z(n, 6), z(n, 6), z(n, nd, 6), z(n, nd, 6), z(n, 4, dt=torch.int32)]      # wrench, sdot, d_wrench, d_sdot, counts
        self.f, self.df = Guarded(ns, nv), Guarded(ns * nd, nv)
        self.val = [Guarded(ns, nv), Guarded(ns * nv, nv), Guarded(ns, nv), Guarded(ns, nv), Guarded(ns, 1, True)]      # qdot H c vdot info
        self.par = [Guarded(ns * nd, nv), Guarded(ns * nd * nv, nv), Guarded(ns * nd, nv), Guarded(ns * nd, nv)]        # dqdot dH dc dvdot

    def head(self):
        return (self.n, self.N_DIR, self.d_ids.data_ptr(), self.d_sc.data_ptr(), self.ns, self.d_q.data_ptr(), self.d_v.data_ptr())

    def checked(self, call):
        _sync()
        for _ in range(40):
            call()
            rc = self.m.check()
            if rc == 0:
                return
        raise AssertionError(f"pfc_check: {rc}")

    def _p(self, group):
        return [o.ptr for o in group]

    def chained(self, c):
        _, _, dq, dv = self.chunks[c]
        r = [t.data_ptr() for t in self.res]
        self.checked(lambda: self.m.state_derivative_dual_device(
            *self.head(), dq.data_ptr(), dv.data_ptr(), 0, 0, self.d_tau.data_ptr(), self.d_dtau.data_ptr(), *self._p(self.kin),
            *self._p(self.dkin), *self._p(self.items), *self._p(self.seeds), *r, self.f.ptr, self.df.ptr, *self._p(self.val), *self._p(self.par)))

    def _dynamics_parts(self, c, first):
        _, _, dq, dv = self.chunks[c]
        state = (self.ns, self.d_q.data_ptr(), self.d_v.data_ptr())
        if first:
            self.m.dynamics_device(*state, self.kin[0].ptr, self.kin[1].ptr, *self._p(self.val[:3]))
        self.m.dynamics_dual_device(self.ns, self.N_DIR, state[1], state[2], dq.data_ptr(), dv.data_ptr(), self.kin[0].ptr, self.kin[1].ptr,
                                    self.dkin[0].ptr, self.dkin[1].ptr, *self._p(self.par[:3]))
        self.m.accelerations_dual_device(self.ns, self.N_DIR, self.val[1].ptr, self.val[2].ptr, self.f.ptr, self.d_tau.data_ptr(),
                                         self.par[1].ptr, self.par[2].ptr, self.df.ptr, self.d_dtau.data_ptr(),
                                         self.val[3].ptr if first else 0, self.par[3].ptr, self.val[4].ptr if first else 0)
        _sync()
        assert self.m.check() == 0

    def parts(self, c):
        _, _, dq, dv = self.chunks[c]
        r = [t.data_ptr() for t in self.res]
        self.checked(lambda: self.m.eval_dual_state_device(
            *self.head(), dq.data_ptr(), dv.data_ptr(), 0, 0, *self._p(self.kin), *self._p(self.dkin), *self._p(self.items),
            *self._p(self.seeds), *r, self.f.ptr, self.df.ptr))
        self._dynamics_parts(c, True)

    def _more_args(self, c):
        _, _, dq, dv = self.chunks[c]
        return (*self.head(), dq.data_ptr(), dv.data_ptr(), 0)

    def _more_tail(self):
        return (*self._p(self.kin), *self._p(self.dkin), self.items[2].ptr, self.items[3].ptr, self.items[4].ptr, self.res[0].data_ptr(),
                *self._p(self.seeds), self.res[2].data_ptr(), self.res[3].data_ptr(), self.df.ptr)

    def chained_more(self, c):
        _sync()
        self.m.state_derivative_dual_device_more(*self._more_args(c), self.d_tau.data_ptr(), self.d_dtau.data_ptr(), *self._more_tail(),
                                                 self.val[1].ptr, self.val[2].ptr, self.f.ptr, *self._p(self.par))
        assert self.m.check() == 0 and self.m.last_dual_reused()

    def parts_more(self, c):
        _sync()
        self.m.eval_dual_state_device_more(*self._more_args(c), *self._more_tail())
        assert self.m.check() == 0
        self._dynamics_parts(c, False)

    def snapshot(self):
        _sync()
        names = ("x_w_b", "twist_w_b", "jac", "d_x_w_b", "d_twist_w_b", "d_jac", "pose", "twist", "x_w_r2", "body_1", "body_2", "d_pose",
                 "d_twist", "d_x_w_r2", "f", "d_f", "qdot", "H", "c", "vdot", "info", "d_qdot", "d_H", "d_c", "d_vdot")
        out = {k: o.rows().copy() for k, o in zip(names, self.kin + self.dkin + self.items + self.seeds + [self.f, self.df] + self.val + self.par)}
        out.update({k: t.cpu().numpy().copy() for k, t in zip(("wrench", "sdot", "d_wrench", "d_sdot", "counts"), self.res)})
        return out


VALUES = ("x_w_b", "twist_w_b", "jac", "pose", "twist", "x_w_r2", "body_1", "body_2", "wrench", "sdot", "counts", "f", "qdot", "H", "c", "vdot",
          "info")
EXACT = ("x_w_b", "twist_w_b", "jac", "d_x_w_b", "d_twist_w_b", "d_jac", "pose", "twist", "x_w_r2", "body_1", "body_2", "d_pose", "d_twist",
         "d_x_w_r2", "qdot", "H", "c", "d_qdot", "d_H", "d_c")


@pytest.mark.parametrize("which", ["C1", "C4"])
def test_chain_equals_its_parts_fixed_order(pfc, which):
    A, B = Rig(pfc, which, 1), Rig(pfc, which, 1)
    A.chained(0)
    B.parts(0)
    a, b = A.snapshot(), B.snapshot()
    assert a["counts"][:, 3].all(), "an item has no contact"
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert not a["info"].any() and all(np.abs(a[k]).max() > 0 for k in ("d_f", "d_qdot", "d_H", "d_c", "d_vdot", "vdot"))
    # what it leaves is the statements' (no revolute joint in either mechanism: no trigonometry)
    dq, dv = A.chunks[0][:2]
    ns, nd, nv = A.ns, A.N_DIR, A.nv
    dqd, dH, dc = DD.dyn_dual_reference(A.mech, A.inertia, D.GRAVITY, A.q, A.v, dq, dv)
    assert np.array_equal(a["d_qdot"], dqd.reshape(ns * nd, nv)) and np.array_equal(a["d_H"], dH.reshape(-1, nv))
    assert np.array_equal(a["d_c"], dc.reshape(ns * nd, nv))
    for s in range(ns):
        r = DD.chol_dual_scalar(a["H"].reshape(ns, nv, nv)[s], a["c"][s], a["f"][s], a["d_H"].reshape(ns, nd, nv, nv)[s],
                                a["d_c"].reshape(ns, nd, nv)[s], a["d_f"].reshape(ns, nd, nv)[s], A.tau[s], A.dtau[s])
        assert r[2] == 0 and a["vdot"][s].tobytes() == r[0].tobytes() and a["d_vdot"].reshape(ns, nd, nv)[s].tobytes() == r[1].tobytes()
    # a different chunk at the kept point: only partials are written
    A.chained_more(1)
    B.parts_more(1)
    a1, b1 = A.snapshot(), B.snapshot()
    for k in a1:
        assert a1[k].tobytes() == b1[k].tobytes(), k
    for k in VALUES:
        assert a1[k].tobytes() == a[k].tobytes(), k      # _more writes no value output
    for k in ("d_x_w_b", "d_f", "d_qdot", "d_H", "d_c", "d_vdot"):
        assert a1[k].tobytes() != a[k].tobytes(), k      # another chunk: other partials
    A.m.close(); B.m.close()


@pytest.mark.parametrize("which", ["C1", "C4"])
def test_chain_on_a_default_handle_and_the_host_composition(pfc, which):
    A, B = Rig(pfc, which, 0), Rig(pfc, which, 0)
    A.chained(0)
    B.parts(0)
    a, b = A.snapshot(), B.snapshot()
    assert a["counts"][:, 3].all(), "an item has no contact"
    assert np.array_equal(a["counts"], b["counts"]) and not a["info"].any() and not b["info"].any()
    for k in EXACT:
        assert a[k].tobytes() == b[k].tobytes(), k
    ns, nd, nv, n = A.ns, A.N_DIR, A.nv, A.n
    per_item = lambda k: [H.rel_err(a[k].reshape(n, -1)[i], b[k].reshape(n, -1)[i]) for i in range(n) if np.linalg.norm(b[k].reshape(n, -1)[i]) > 0]
    per_scene = lambda x, y: max(H.rel_err(x.reshape(ns, -1)[s], y.reshape(ns, -1)[s]) for s in range(ns))
    worst = {k: max(per_item(k) or [0.0]) for k in ("wrench", "sdot", "d_wrench", "d_sdot")}
    worst.update({k: per_scene(a[k], b[k]) for k in ("f", "d_f", "vdot", "d_vdot")})
    print(f"{which}: chained call against its parts on a default handle, largest relative difference: "
          + ", ".join(f"{k} {e:.2e}" for k, e in worst.items()))
    assert all(e < 1e-9 for e in worst.values()), worst
    # the host composition: the same kinematics, qdot, H, c and their partials; the rest as close
    dq, dv = A.chunks[0][:2]
    qd, vdot, sdot, dqd, dvd, dsd, info, (f, d_f), (Hm, c), (dH, dc), (wrench, dw, counts) = A.m.state_derivative_dual(
        A.q, A.v, None, dq, dv, None, A.tau, A.dtau, A.ids, A.scene)
    for k, got in (("qdot", qd), ("H", Hm), ("c", c), ("d_qdot", dqd), ("d_H", dH), ("d_c", dc)):
        assert np.ascontiguousarray(got).tobytes() == a[k].tobytes(), k
    assert np.array_equal(counts, a["counts"]) and not info.any()
    for k, got in (("f", f), ("d_f", d_f), ("vdot", vdot), ("d_vdot", dvd)):
        assert per_scene(got, a[k]) < 1e-9, k
    assert dvd.shape == (ns, nd, nv) and dsd.shape == a["d_sdot"].shape
    A.m.close(); B.m.close()


def test_dynamics_dual_is_not_an_evaluation_and_chain_refusals_write_nothing(pfc):
    L = pfc._lib
    A = Rig(pfc, "C1", 1)
    # refused before the first launch: n_dir 17, and a handle without inertias
    r = [t.data_ptr() for t in A.res]
    _, _, dq, dv = A.chunks[0]

    def call(m, n_dir):
        with pytest.raises(L.PFCError) as e:
            m.state_derivative_dual_device(A.n, n_dir, *A.head()[2:], dq.data_ptr(), dv.data_ptr(), 0, 0, 0, 0, *A._p(A.kin), *A._p(A.dkin),
                                           *A._p(A.items), *A._p(A.seeds), *r, A.f.ptr, A.df.ptr, *A._p(A.val), *A._p(A.par))
        _sync()
        assert all(o.untouched() for o in A.kin + A.dkin + A.items + A.seeds + [A.f, A.df] + A.val + A.par)
        return e.value

    _sync()
    assert call(A.m, 17).status == L.ERR_BAD_ARG
    w = pfc.configs.c1_boxes()
    bare = pfc.configs.build_scenario(w)
    for k, c in enumerate(w.instructions):
        bare.set_instruction_bodies(k, c.id_1, c.id_2)
    _set(bare, A.mech)
    e = call(bare, A.N_DIR)
    assert e.status == L.ERR_STATE and "pfc_set_inertia" in str(e)
    with pytest.raises(L.PFCError) as e2:      # _more without a checked evaluation to extend
        A.m.state_derivative_dual_device_more(*A._more_args(1), 0, 0, *A._more_tail(), A.val[1].ptr, A.val[2].ptr, A.f.ptr, *A._p(A.par))
    _sync()
    assert e2.value.status == L.ERR_STATE and all(o.untouched() for o in A.dkin + A.seeds + [A.df] + A.par)
    bare.close()
    # after a checked Dual evaluation a pfc_dynamics_dual_device / pfc_accelerations_dual_device call still lets _more follow
    A.chained(0)
    reused = A.m.last_dual_reused()
    first = A.snapshot()
    A._dynamics_parts(0, True)
    assert A.m.check() == 0 and A.m.last_dual_reused() == reused
    again = A.snapshot()
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k
    A.chained_more(1)
    assert np.abs(A.snapshot()["d_vdot"]).max() > 0
    A.m.close()
