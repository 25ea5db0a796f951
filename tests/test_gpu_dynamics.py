"""Forward dynamics on the device (pfc_set_inertia, pfc_dynamics[_device], pfc_accelerations[_device], pfc_state_derivative[_device]):
bytes against the scalar statement of tests/test_dynamics_abi.py fed with the device's cos / sin, the refusals, the per-scene pivot
flag, the chain against its parts, and the reference's end-to-end friction test (test/test_friction.jl:92-143) through the ABI.

Tolerances: qdot, H, c, vdot and info are compared as bytes.  f_generalized is summed with atomics and is not bit-stable from call to
call (tests/test_gpu_kinematics.py), so where a chain is compared with its parts the parts' solve is given the chain's f and f itself
is compared at that file's 1e-12."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import test_dynamics_abi as D
import test_kinematics_abi as K
from test_gpu_items_from_bodies import Guarded, _dev, _torch
from test_gpu_kinematics import _c1_state, _raw_mech, _set, _states

pytestmark = pytest.mark.gpu


def chain_mech(n, seed=21):
    """n revolute bodies in a chain, links of length ~0.1 about random axes: nv = n."""
    rng = np.random.default_rng(seed)
    x = [np.concatenate([K._random_rotation(rng).reshape(-1, order="F"), K._unit(rng) * 0.1]) for _ in range(n)]
    return K.make_mech(list(range(-1, n - 1)), [K.REVOLUTE] * n, x, [K._unit(rng) for _ in range(n)])


def _cases():
    """name -> (mechanism, inertia, q, v): the smallest shapes at which the kernels can go wrong -- mechanism (A) below, at and across a
    wave of (scene, body) lanes of the kinematics kernel; nv = 1; nv = 6; the pencil's chain; C1's tree; a chain at the solve's cap."""
    out = {}
    rng = np.random.default_rng(77)
    for n in (1, 10, 11, 43):
        out["A%d" % n] = (K.mech_a(), 100 + n, n)
    out["rev1"] = (K.make_mech([-1], [K.REVOLUTE], [K.WORLD_X], [[0.0, 0.6, 0.8]]), 201, 3)
    out["float6"] = (K.make_mech([-1], [K.FLOATING], [K.WORLD_X], [[0.0, 0.0, 0.0]]), 202, 3)
    out["C11"] = (K.mech_c(), 300, 11)
    out["B2"] = (K.mech_b(), 203, 2)
    out["cap64"] = (chain_mech(D.MAX_NV_SOLVE), 204, 3)
    return {k: (m, D.random_inertia(m, rng), *_states(m, n, seed)) for k, (m, seed, n) in out.items()}


CASES = _cases()


def _angles():
    a = set()
    for mech, _, q, v in CASES.values():
        for b, t in enumerate(mech["joint_type"]):
            if t == K.REVOLUTE:
                a.update(float(e) for e in q[:, mech["off"][b]])
    return sorted(a)


@pytest.fixture(scope="module")
def scen(pfc):
    w = pfc.configs.c1_boxes()
    m = pfc.configs.build_scenario(w)
    for k, c in enumerate(w.instructions):
        m.set_instruction_bodies(k, c.id_1, c.id_2)
    yield m
    m.close()


@pytest.fixture(scope="module")
def device_trig(pfc, scen):
    """{theta: (cos theta, sin theta)} as the device computes them, read as tests/test_gpu_kinematics.py reads them."""
    th = np.array(_angles())
    _set(scen, K.make_mech([-1], [K.REVOLUTE], [K.WORLD_X], [[0.0, 0.0, 1.0]]))
    x, _, _ = scen.kinematics(th.reshape(-1, 1), np.zeros((th.size, 1)), want_jac=False)
    x = x.reshape(th.size, 12)
    return {float(t): (float(x[k, 0]), float(x[k, 1])) for k, t in enumerate(th)}


_REF = {}


def _reference(case, device_trig):
    """(qdot, H, c, f, tau, vdot, info) of a case by the scalar statement, computed once."""
    if case not in _REF:
        mech, inertia, q, v = CASES[case]
        qd, Hm, c = D.dyn_reference(mech, inertia, D.GRAVITY, q, v, trig=device_trig)
        rng = np.random.default_rng(5)
        f, tau = rng.standard_normal(c.shape), rng.standard_normal(c.shape)
        sol = [D.chol_scalar(Hm[s], c[s], f[s], tau[s]) for s in range(q.shape[0])]
        _REF[case] = (qd, Hm, c, f, tau, np.array([s[0] for s in sol]), np.array([s[1] for s in sol], dtype=np.int32))
    return _REF[case]


def _dyn_outputs(n_scene, nv):
    return [Guarded(n_scene, nv), Guarded(n_scene * nv, nv), Guarded(n_scene, nv)]


def _kin_on_device(scen, mech, q, v):
    n_scene = q.shape[0]
    d_q, d_v = _dev(q), _dev(v)
    x, tw = Guarded(n_scene * mech["n_body"], 12), Guarded(n_scene * mech["n_body"], 6)
    scen.kinematics_device(n_scene, d_q.data_ptr(), d_v.data_ptr(), x.ptr, tw.ptr, 0)
    return d_q, d_v, x, tw


# ---- bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_dynamics_and_accelerations_are_the_bytes_of_the_scalar_statement(pfc, scen, device_trig, case):
    torch = _torch()
    mech, inertia, q, v = CASES[case]
    n_scene, nv = q.shape[0], mech["nv"]
    qd_r, H_r, c_r, f, tau, vd_r, info_r = _reference(case, device_trig)
    ref = [qd_r.reshape(n_scene, nv), H_r.reshape(n_scene * nv, nv), c_r.reshape(n_scene, nv)]
    _set(scen, mech)
    scen.set_inertia(inertia, D.GRAVITY)
    torch.cuda.synchronize()
    d_q, d_v, x, tw = _kin_on_device(scen, mech, q, v)
    got = None
    for rep in range(2):      # a second call returns the same bytes
        out = _dyn_outputs(n_scene, nv)
        scen.dynamics_device(n_scene, d_q.data_ptr(), d_v.data_ptr(), x.ptr, tw.ptr, *[o.ptr for o in out])
        torch.cuda.synchronize()
        rows = [o.rows().reshape(r.shape) for o, r in zip(out, ref)]      # checks the guard words
        for name, g, r in zip(("qdot", "H", "c"), rows, ref):
            assert g.tobytes() == r.tobytes(), (name, rep, np.argwhere(g != r)[:4])
        got = rows
    # each output NULL in turn: untouched, the others the same bytes
    for skip in range(3):
        part = _dyn_outputs(n_scene, nv)
        scen.dynamics_device(n_scene, d_q.data_ptr(), d_v.data_ptr(), x.ptr, tw.ptr, *[0 if k == skip else o.ptr for k, o in enumerate(part)])
        torch.cuda.synchronize()
        for k, (o, g) in enumerate(zip(part, got)):
            assert o.untouched() if k == skip else o.rows().reshape(g.shape).tobytes() == g.tobytes(), (skip, k)
    # the solve
    d_f, d_tau = _dev(f), _dev(tau)
    sols = []
    for with_tau in (True, False):
        vd, info = Guarded(n_scene, nv), Guarded(n_scene, 1, True)
        scen.accelerations_device(n_scene, out[1].ptr, out[2].ptr, d_f.data_ptr(), d_tau.data_ptr() if with_tau else 0, vd.ptr, info.ptr)
        torch.cuda.synchronize()
        sols.append((vd.rows().reshape(n_scene, nv), info.rows()))
    assert sols[0][0].tobytes() == vd_r.tobytes() and np.array_equal(sols[0][1], info_r), np.argwhere(sols[0][0] != vd_r)[:4]
    no_tau = [D.chol_scalar(H_r[s], c_r[s], f[s]) for s in range(n_scene)]
    assert sols[1][0].tobytes() == np.array([s[0] for s in no_tau]).tobytes()
    vd = Guarded(n_scene, nv)
    scen.accelerations_device(n_scene, out[1].ptr, out[2].ptr, d_f.data_ptr(), d_tau.data_ptr(), vd.ptr, 0)      # no info wanted
    torch.cuda.synchronize()
    assert vd.rows().reshape(n_scene, nv).tobytes() == vd_r.tobytes()
    # the host forms
    hq, hH, hc = scen.dynamics(q, v)
    assert hq.tobytes() == ref[0].tobytes() and hH.tobytes() == H_r.tobytes() and hc.tobytes() == c_r.tobytes()
    hv, hi = scen.accelerations(hH, hc, f, tau)
    assert hv.tobytes() == vd_r.tobytes() and np.array_equal(hi, info_r)
    if case in ("A11", "C11"):      # a fresh handle, and one over the devices [0, 0]: the same bytes
        for kw in ({}, {"devices": [0, 0]}):
            m2 = pfc.configs.build_scenario(pfc.configs.c1_boxes(), **kw)
            _set(m2, mech)
            m2.set_inertia(inertia, D.GRAVITY)
            mq, mH, mc = m2.dynamics(q, v)
            assert mq.tobytes() == ref[0].tobytes() and mH.tobytes() == H_r.tobytes() and mc.tobytes() == c_r.tobytes()
            mv, mi = m2.accelerations(mH, mc, f, tau)
            assert mv.tobytes() == vd_r.tobytes() and np.array_equal(mi, info_r)
            m2.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(pfc):
    torch = _torch()
    L = pfc._lib
    lib = L.lib()
    h = C.c_void_p()
    assert lib.pfc_create(0, C.byref(h)) == 0
    msg = lambda: lib.pfc_last_error(h).decode()
    dp = C.POINTER(C.c_double)
    mech = K.mech_c()
    q, v = _states(mech, 2, 9)
    q[:, 1] = 0.0                                   # the revolute joint at angle 0: cos = 1, sin = 0 on any libm
    inertia = D.random_inertia(mech, np.random.default_rng(1))
    grav = np.array(D.GRAVITY)
    d_q, d_v = _dev(q), _dev(v)
    d_x, d_tw = _dev(np.zeros((8, 12))), _dev(np.zeros((8, 6)))
    out = _dyn_outputs(2, 4)
    dyn = lambda: lib.pfc_dynamics_device(h, 2, d_q.data_ptr(), d_v.data_ptr(), d_x.data_ptr(), d_tw.data_ptr(), *[o.ptr for o in out], None)
    set_in = lambda tab, n=4, g=grav: lib.pfc_set_inertia(h, n, None if tab is None else tab.ctypes.data_as(dp),
                                                          None if g is None else g.ctypes.data_as(dp))
    # before pfc_set_mechanism
    assert set_in(inertia) == L.ERR_STATE and "pfc_set_mechanism" in msg()
    assert dyn() == L.ERR_STATE
    keep, ptr = _raw_mech(mech)
    assert lib.pfc_set_mechanism(h, 4, *ptr) == 0
    # no inertias set
    assert dyn() == L.ERR_STATE and "pfc_set_inertia" in msg()
    # pfc_set_inertia's refusals
    assert set_in(inertia, n=3) == L.ERR_BAD_ARG and "n_body" in msg()
    assert set_in(None) == L.ERR_BAD_ARG and set_in(inertia, g=None) == L.ERR_BAD_ARG
    for body, col, val, word in ((2, 12, -1.0, "mass"), (1, 12, np.inf, "mass"), (3, 12, np.nan, "mass")):
        bad = inertia.copy(); bad[body, col] = val
        assert set_in(bad) == L.ERR_BAD_ARG and "body %d" % body in msg() and word in msg()
    bad = inertia.copy(); bad[2, 1] += 1e-9 * np.abs(bad[2, :9]).max()      # M10 != M01
    assert set_in(bad) == L.ERR_BAD_ARG and "body 2" in msg() and "symmetric" in msg()
    assert dyn() == L.ERR_STATE                                             # still none
    zero_mass = inertia.copy(); zero_mass[3] = 0.0                          # zero mass is allowed
    assert set_in(zero_mass) == 0 and set_in(inertia) == 0
    # a failed call leaves the previous inertias in place: the bytes are those of `inertia`
    bad = inertia.copy(); bad[0, 12] = -2.0
    assert set_in(bad) == L.ERR_BAD_ARG
    x_r, tw_r, _ = K.kin_reference(mech, q, v)
    d_x.copy_(_dev(x_r.reshape(8, 12))); d_tw.copy_(_dev(tw_r.reshape(8, 6)))
    assert lib.pfc_dynamics_device(h, 0, None, None, None, None, *[o.ptr for o in out], None) == 0      # n_scene = 0: a no-op
    torch.cuda.synchronize()
    assert all(o.untouched() for o in out)
    assert dyn() == 0
    torch.cuda.synchronize()
    qd_r, H_r, c_r = D.dyn_reference(mech, inertia, D.GRAVITY, q, v)
    assert out[0].rows().tobytes() == qd_r.tobytes() and out[1].rows().tobytes() == H_r.tobytes() and out[2].rows().tobytes() == c_r.tobytes()
    # a null input an output needs
    assert lib.pfc_dynamics_device(h, 2, d_q.data_ptr(), d_v.data_ptr(), None, d_tw.data_ptr(), None, out[1].ptr, None, None) == L.ERR_BAD_ARG
    # a later pfc_set_mechanism drops the inertias
    assert lib.pfc_set_mechanism(h, 4, *ptr) == 0
    out = _dyn_outputs(2, 4)
    assert dyn() == L.ERR_STATE
    # nv = cap + 1: the solve refuses before anything is launched; so does the chain (C1's scenario, a 65-body chain)
    big = chain_mech(D.MAX_NV_SOLVE + 1)
    keep2, ptr2 = _raw_mech(big)
    assert lib.pfc_set_mechanism(h, 65, *ptr2) == 0
    nv = 65
    vd, info = Guarded(1, nv), Guarded(1, 1, True)
    z = _dev(np.zeros(nv * nv))
    rc = lib.pfc_accelerations_device(h, 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, vd.ptr, info.ptr, None)
    assert rc == L.ERR_BAD_ARG and "PFC_MAX_NV_SOLVE" in msg()
    torch.cuda.synchronize()
    assert all(o.untouched() for o in out + [vd, info])
    lib.pfc_destroy(h)

    w = pfc.configs.c1_boxes()
    m = pfc.configs.build_scenario(w)
    for k, c in enumerate(w.instructions):
        m.set_instruction_bodies(k, c.id_1, c.id_2)
    _set(m, big)
    qb, vb = _states(big, 1, 3)
    d_qb, d_vb = _dev(qb), _dev(vb)

    def chain_call():
        bufs = [Guarded(65, 12), Guarded(65, 6), Guarded(65 * nv, 6), Guarded(4, 24), Guarded(4, 6), Guarded(4, 12), Guarded(4, 1, True),
                Guarded(4, 1, True), Guarded(4, 6), Guarded(4, 6), Guarded(4, 4, True), Guarded(1, nv), Guarded(1, nv), Guarded(nv, nv),
                Guarded(1, nv), Guarded(1, nv), Guarded(1, 1, True)]
        with pytest.raises(L.PFCError) as e:
            m.state_derivative_device(4, 0, 0, 1, d_qb.data_ptr(), d_vb.data_ptr(), 0, 0, *[o.ptr for o in bufs])
        torch.cuda.synchronize()
        assert all(o.untouched() for o in bufs)
        return e.value

    e = chain_call()
    assert e.status == L.ERR_STATE and "pfc_set_inertia" in str(e)          # no inertias
    m.set_inertia(D.random_inertia(big, np.random.default_rng(2)), D.GRAVITY)
    e = chain_call()
    assert e.status == L.ERR_BAD_ARG and "PFC_MAX_NV_SOLVE" in str(e)       # the nv cap
    m.close()


# ---- a failed pivot is a per-scene flag ----------------------------------------------------------------------------------------
def test_a_massless_scene_among_good_ones(pfc, scen):
    torch = _torch()
    mech = K.mech_c()
    q, v = _states(mech, 3, 31)
    q[:, 1] = 0.0
    rng = np.random.default_rng(32)
    good = D.random_inertia(mech, rng)
    bad = good.copy(); bad[3] = 0.0                 # the last finger massless: pivot 4 is zero
    _set(scen, mech)
    f = rng.standard_normal((3, 4))
    scen.set_inertia(good, D.GRAVITY)
    _, Hg, cg = scen.dynamics(q, v)
    scen.set_inertia(bad, D.GRAVITY)
    _, Hb, cb = scen.dynamics(q, v)
    assert Hb[1, 3, 3] == 0.0
    Hm, cm = Hg.copy(), cg.copy()
    Hm[1], cm[1] = Hb[1], cb[1]
    d_H, d_c, d_f = _dev(Hm), _dev(cm), _dev(f)
    vd, info = Guarded(3, 4), Guarded(3, 1, True)
    scen.accelerations_device(3, d_H.data_ptr(), d_c.data_ptr(), d_f.data_ptr(), 0, vd.ptr, info.ptr)
    torch.cuda.synchronize()
    assert scen.check() == 0                         # not an error state
    all_good, info_good = scen.accelerations(Hg, cg, f)
    got = vd.rows()
    assert np.array_equal(info.rows(), [0, 4, 0]) and not info_good.any()
    assert np.isnan(got[1]).all() and got[1].tobytes() == np.full(4, np.nan).tobytes()
    assert got[0].tobytes() == all_good[0].tobytes() and got[2].tobytes() == all_good[2].tobytes()
    for s in (0, 2):
        r, i = D.chol_scalar(Hg[s], cg[s], f[s])
        assert i == 0 and got[s].tobytes() == r.tobytes()


# ---- the chain equals its parts ------------------------------------------------------------------------------------------------
def _c4_slice(pfc):
    """C4's scenario (ground on the world, the 972-tet box floating) and three scenes drawn the way C4 draws them: penetration in
    (0.5, 3) mm, a tilt of a degree or two, any yaw, |v_lin| <= 0.1, |omega| <= 1.  Mechanism: body 0 the ground (fixed), body 1 the box."""
    w = pfc.configs.c2_box_on_plane(1)
    m = pfc.configs.build_scenario(w)
    m.set_instruction_bodies(0, 0, 1)
    mech = K.make_mech([-1, -1], [K.FIXED, K.FLOATING], [K.WORLD_X, K.WORLD_X], np.zeros((2, 3)))
    rng = np.random.default_rng(41)
    q, v = np.zeros((3, 6)), np.zeros((3, 6))
    for s in range(3):
        yaw = rng.uniform(0, 2 * np.pi)
        q[s, :3] = [rng.uniform(-0.004, 0.004), rng.uniform(-0.004, 0.004), np.tan(yaw / 4)]
        q[s, 3:] = [rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 0.05 - rng.uniform(0.5e-3, 3e-3)]
        v[s] = np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-0.1, 0.1, 3)])
    inertia = np.zeros((2, 13))
    inertia[1] = pfc.geometry.mesh_inertia(w.meshes[1].mesh, 400.0)
    return m, mech, inertia, q, v, np.zeros(3, dtype=np.int32), np.arange(3, dtype=np.int32)


def _c1_chain(pfc, scen):
    mech, q0, v0, _, _ = _c1_state(pfc, True)
    rng = np.random.default_rng(81)
    q = np.tile(q0, (3, 1)); v = np.tile(v0, (3, 1))
    q[1:, :] += 1e-4 * rng.standard_normal((2, 24)); v[1:, :] += 0.05 * rng.standard_normal((2, 24))
    inertia = D.random_inertia(mech, rng)
    return scen, mech, inertia, q, v, np.tile(np.arange(4, dtype=np.int32), 3), np.repeat(np.arange(3, dtype=np.int32), 4)


@pytest.mark.parametrize("which", ["C1", "C4"])
def test_chain_equals_its_parts(pfc, scen, which):
    torch = _torch()
    m, mech, inertia, q, v, ids, scene = _c1_chain(pfc, scen) if which == "C1" else _c4_slice(pfc)
    _set(m, mech)
    m.set_inertia(inertia, D.GRAVITY)
    n_scene, n_body, nv, n = q.shape[0], mech["n_body"], mech["nv"], ids.size
    nb = n_scene * n_body
    tau = np.random.default_rng(6).standard_normal((n_scene, nv))
    d_q, d_v, d_ids, d_sc, d_tau = _dev(q), _dev(v), _dev(ids), _dev(scene), _dev(tau)

    def buffers():
        return ([Guarded(nb, 12), Guarded(nb, 6), Guarded(nb * nv, 6), Guarded(n, 24), Guarded(n, 6), Guarded(n, 12), Guarded(n, 1, True),
                 Guarded(n, 1, True), Guarded(n, 6), Guarded(n, 6), Guarded(n, 4, True), Guarded(n_scene, nv)],
                [Guarded(n_scene, nv), Guarded(n_scene * nv, nv), Guarded(n_scene, nv)], [Guarded(n_scene, nv), Guarded(n_scene, 1, True)])

    ea, da, sa = buffers()
    eb, db, sb = buffers()
    torch.cuda.synchronize()      # the calls below run on the handle's own stream
    for _ in range(40):
        m.state_derivative_device(n, d_ids.data_ptr(), d_sc.data_ptr(), n_scene, d_q.data_ptr(), d_v.data_ptr(), 0, d_tau.data_ptr(),
                                  *[o.ptr for o in ea + da + sa])
        rc = m.check()
        if rc == 0:
            break
    assert rc == 0
    for _ in range(40):
        m.eval_state_device(n, d_ids.data_ptr(), d_sc.data_ptr(), n_scene, d_q.data_ptr(), d_v.data_ptr(), 0, *[o.ptr for o in eb])
        rc = m.check()
        if rc == 0:
            break
    assert rc == 0
    m.dynamics_device(n_scene, d_q.data_ptr(), d_v.data_ptr(), eb[0].ptr, eb[1].ptr, *[o.ptr for o in db])
    m.accelerations_device(n_scene, db[1].ptr, db[2].ptr, ea[11].ptr, d_tau.data_ptr(), sb[0].ptr, sb[1].ptr)      # the chain's f: see above
    torch.cuda.synchronize()
    assert m.check() == 0
    for k, (a, b) in enumerate(zip(ea[:8] + da + sa, eb[:8] + db + sb)):      # states, items, qdot, H, c, vdot, info: the same bytes
        assert a.rows().tobytes() == b.rows().tobytes(), k
    assert ea[10].rows()[:, 3].all(), "an item has no contact"
    assert np.array_equal(ea[10].rows(), eb[10].rows())
    fa, fb = ea[11].rows(), eb[11].rows()
    assert np.abs(fb).max() > 0
    np.testing.assert_allclose(fa, fb, rtol=1e-12, atol=1e-12 * np.abs(fb).max())
    assert not sa[1].rows().any() and np.isfinite(sa[0].rows()).all()
    # and against the statement: qdot, H and c from (q, v) (no revolute joint: no trigonometry), vdot from the chain's own f
    qd_r, H_r, c_r = D.dyn_reference(mech, inertia, D.GRAVITY, q, v)
    assert da[0].rows().tobytes() == qd_r.tobytes() and da[1].rows().tobytes() == H_r.tobytes() and da[2].rows().tobytes() == c_r.tobytes()
    vd_r = np.array([D.chol_scalar(H_r[s], c_r[s], fa.reshape(n_scene, nv)[s], tau[s])[0] for s in range(n_scene)])
    assert sa[0].rows().tobytes() == vd_r.tobytes()
    # the host form: the same qdot, H, c; f and vdot as close as f is
    qd_h, vd_h, _, info_h, f_h, (H_h, c_h), _ = m.state_derivative(q, v, None, tau, ids, scene)
    assert qd_h.tobytes() == qd_r.tobytes() and H_h.tobytes() == H_r.tobytes() and c_h.tobytes() == c_r.tobytes() and not info_h.any()
    np.testing.assert_allclose(f_h, fa.reshape(n_scene, nv), rtol=1e-12, atol=1e-12 * np.abs(fb).max())
    if which == "C4":
        m.close()


# ---- the reference's end-to-end friction test -----------------------------------------------------------------------------------
def test_regularized_friction_sign_through_the_abi(pfc):
    """test/test_friction.jl:92-143, the scene of tests/test_scene_kats.py::test_regularized_friction_sign: the box is a floating body
    with geometry.mesh_inertia's shell inertia (rho = 400, d = 0.09), at the penetration that balances gravity, moving at v_tol in
    +y; tau_y = 0.999 x and 1.001 x mu_d m g.  vdot[4] (index 11 of the reference's xx) is negative, then positive; |vdot_z| is
    below 1e-6 g, the existing test's rel = 1e-6 on the normal force."""
    G, S = pfc.geometry, pfc.scenario
    box_rad, Ebar, mu_d, v_tol, rho, d, mag_grav = 0.05, 1.0e9, 0.3, 1.0e-4, 400.0, 0.09, 9.8054
    plane = G.as_tet_emesh(G.emesh_half_plane())
    box = G.as_tri_emesh(G.emesh_box(box_rad)).transformed(t=[0, 0, box_rad])
    rec = G.mesh_inertia(box, rho, d)
    mass = rec[12]
    assert mass == pytest.approx(rho * d * 6 * (2 * box_rad) ** 2, rel=1e-12)
    mg = mag_grav * mass
    pene = mg / (Ebar * 4 * box_rad ** 2)
    m = S.MechanismScenario()
    i1 = m.add_contact("box", box, c_prop=None)
    i2 = m.add_contact("plane", plane, c_prop=S.ContactProperties(Ebar))
    m.add_friction_regularize(i1, i2, mu_s=mu_d, mu_d=mu_d, chi=0.5, v_tol=v_tol, n_quad_rule=2)
    m.finalize()
    m.set_instruction_bodies(0, 0, -1)      # the box is body 0, the plane the world
    m.set_mechanism([-1], [K.FLOATING], [K.WORLD_X])
    m.set_inertia(rec.reshape(1, 13), (0.0, 0.0, -mag_grav))
    q = np.array([0.0, 0.0, 0.0, 0.0, 0.0, -pene]); v = np.array([0.0, 0.0, 0.0, 0.0, v_tol, 0.0])
    signs = []
    for coe in (0.999, 1.001):
        tau = np.zeros(6); tau[4] = coe * mu_d * mg
        qd, vdot, sdot, info, f, (Hm, c), (wrench, counts) = m.state_derivative(q, v, None, tau)
        assert info[0] == 0 and counts[0, 3] > 0
        assert qd[0].tobytes() == v.tobytes()                       # p = 0: qdot = v
        assert f[0, 4] == pytest.approx(-mu_d * mg, rel=1e-4)        # the friction force on the box
        assert abs(vdot[0, 5]) <= 1e-6 * mag_grav
        signs.append(np.sign(vdot[0, 4]))
    assert signs == [-1, 1]
    m.close()
