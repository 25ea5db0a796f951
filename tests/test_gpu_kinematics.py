"""Body poses, twists and geometric Jacobians from joint states on the device (pfc_set_mechanism, pfc_kinematics[_device],
pfc_eval_state[_device]): the device's cos / sin read and measured, bytes against the scalar statement of
tests/test_kinematics_abi.py fed with them, C1 rebuilt from its joint state against the oracle, the chain state -> body states ->
items -> wrenches -> f_generalized against its parts, and the error paths.

Tolerances: poses, twists, Jacobians and items are compared as bytes (values; np.array_equal does not tell -0.0 from 0.0); the
device's cos / sin against a 40-digit value at 4 ulp (OpenCL's full-profile bound for double sin / cos, the only published one);
wrench and sdot at the suite's 1e-9 relative (tests/test_gpu_parity.py); f_generalized at 1e-12
(test_scatter_generalized_third_law): k_scatter sums with atomics, so f is not bit-stable."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import test_kinematics_abi as K
from test_gpu_items_from_bodies import Guarded, _dev, _torch, c1_world_states
from test_items_from_bodies_abi import items_reference

pytestmark = pytest.mark.gpu

N_SCENES = (1, 10, 11, 43)      # 6, 60, 66, 258 (scene, body) lanes of mechanism (A): a partial wave, across a wave boundary, across four


def _states(mech, n_scene, seed):
    rng = np.random.default_rng(seed)
    qs, vs = zip(*(K.random_state(mech, rng, k) for k in range(n_scene)))
    return np.array(qs).reshape(n_scene, mech["nv"]), np.array(vs).reshape(n_scene, mech["nv"])


def _cases():
    """(name, mechanism, q, v) of every byte comparison below: their revolute angles are what the device's cos / sin are read for."""
    out = [("A%d" % n, K.mech_a(), *_states(K.mech_a(), n, 100 + n)) for n in N_SCENES]
    out.append(("C11", K.mech_c(), *_states(K.mech_c(), 11, 300)))
    return {c[0]: c[1:] for c in out}


CASES = _cases()


def _set(m, mech):
    m.set_mechanism(mech["parent"], mech["joint_type"], mech["x_p_j"], mech["axis"])


def _angles():
    a = set()
    for mech, q, v in CASES.values():
        for b, t in enumerate(mech["joint_type"]):
            if t == K.REVOLUTE:
                a.update(float(e) for e in q[:, mech["off"][b]])
    return sorted(a)


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
    """{theta: (cos theta, sin theta)} as the device computes them, read and not assumed: one body, revolute about e_z on the world
    with x_p_j = I, returns R00 = cos theta and R10 = sin theta exactly (every other product of the statement is with 0 or 1); one
    scene per angle of CASES."""
    th = np.array(_angles())
    one = K.make_mech([-1], [K.REVOLUTE], [K.WORLD_X], [[0.0, 0.0, 1.0]])
    _set(scen, one)
    x, _, _ = scen.kinematics(th.reshape(-1, 1), np.zeros((th.size, 1)), want_jac=False)
    x = x.reshape(th.size, 12)
    assert np.array_equal(x[:, [0, 1]], x[:, [4, 3]] * [1, -1]) and (x[:, [2, 5, 6, 7, 9, 10, 11]] == 0).all()
    return {float(t): (float(x[k, 0]), float(x[k, 1])) for k, t in enumerate(th)}


# ---- 5. device trigonometry ----------------------------------------------------------------------------------------------------
def test_device_cos_sin_within_four_ulp(device_trig):
    """The library's first trigonometric calls: largest error of the device's cos / sin over the angles of this file, in ulps of
    the result.  Measured on an MI355X: 0.71 ulp ("Kinematics from joint states")."""
    import mpmath
    mpmath.mp.dps = 40
    worst = 0.0
    for th, (c, s) in device_trig.items():
        for got, f in ((c, mpmath.cos), (s, mpmath.sin)):
            ref = f(mpmath.mpf(th))
            worst = max(worst, float(abs(mpmath.mpf(got) - ref) / mpmath.mpf(float(np.spacing(abs(float(ref)))))))
    print(f"device cos / sin over {len(device_trig)} angles in [-2 pi, 2 pi]: largest error {worst:.3f} ulp")
    assert len(device_trig) > 100
    assert worst <= 4.0


# ---- 6. bytes ------------------------------------------------------------------------------------------------------------------
def _kin_outputs(mech, n_scene):
    nb = n_scene * mech["n_body"]
    return [Guarded(nb, 12), Guarded(nb, 6), Guarded(nb * mech["nv"], 6)]


@pytest.mark.parametrize("case", list(CASES))
def test_kinematics_is_the_bytes_of_the_scalar_statement(pfc, scen, device_trig, case):
    torch = _torch()
    mech, q, v = CASES[case]
    n_scene, nb, nv = q.shape[0], mech["n_body"], mech["nv"]
    ref = K.kin_reference(mech, q, v, trig=device_trig)
    ref = [ref[0].reshape(-1, 12), ref[1].reshape(-1, 6), ref[2].reshape(-1, 6)]
    _set(scen, mech)
    assert scen.mechanism_sizes() == (nb, nv, nv)
    d_q, d_v = _dev(q), _dev(v)
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    got = None
    for rep in range(2):      # a second call returns the same bytes
        out = _kin_outputs(mech, n_scene)
        scen.kinematics_device(n_scene, d_q.data_ptr(), d_v.data_ptr(), *[o.ptr for o in out], st)
        torch.cuda.synchronize()
        rows = [o.rows() for o in out]      # checks the guard words
        for name, g, r in zip(("x_w_b", "twist_w_b", "jac"), rows, ref):
            assert np.array_equal(g, r), (name, rep, np.argwhere(g != r)[:4])
        assert got is None or all(a.tobytes() == b.tobytes() for a, b in zip(got, rows))
        got = rows
    # an output passed as NULL is untouched, the others are the same bytes: states only, jac only, and two mixed ones
    for want in ((1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 0)):
        part = _kin_outputs(mech, n_scene)
        scen.kinematics_device(n_scene, d_q.data_ptr(), d_v.data_ptr(), *[o.ptr if k else 0 for o, k in zip(part, want)], st)
        torch.cuda.synchronize()
        for o, k, g in zip(part, want, got):
            assert (o.rows().tobytes() == g.tobytes()) if k else o.untouched(), want
    # the host form, and a handle over the devices [0, 0]: the same bytes
    hx, htw, hj = scen.kinematics(q, v)
    assert hx.tobytes() == got[0].tobytes() and htw.tobytes() == got[1].tobytes() and hj.tobytes() == got[2].tobytes()
    if case in ("A11", "C11"):
        m2 = pfc.configs.build_scenario(pfc.configs.c1_boxes(), devices=[0, 0])
        _set(m2, mech)
        assert m2.mechanism_sizes() == (nb, nv, nv)
        mx, mtw, mj = m2.kinematics(q, v)
        assert mx.tobytes() == got[0].tobytes() and mtw.tobytes() == got[1].tobytes() and mj.tobytes() == got[2].tobytes()
        m2.close()


# ---- 7. C1 from its joint state ------------------------------------------------------------------------------------------------
def _c1_state(pfc, tilted):
    """Mechanism (B) with the rotations of c1_world_states in its joint_poses, and the joint state that reproduces those states
    (p = 0) or tilts the boxes (|p| ~ 0.05) and moves them."""
    x, tw = c1_world_states(pfc)
    mech = K.mech_b(rot=x[0, :, :9])
    q, v = np.zeros(24), np.zeros(24)
    rng = np.random.default_rng(8)
    for b in range(1, 5):
        o = 6 * (b - 1)
        q[o + 3:o + 6] = x[0, b, 9:]
        v[o:o + 3] = tw[0, b, :3]
        if tilted:
            q[o:o + 3] = K._unit(rng) * 0.05
            v[o:o + 6] = np.concatenate([tw[0, b, :3] + 0.3 * rng.standard_normal(3), 0.05 * rng.standard_normal(3)])
    return mech, q, v, x, tw


@pytest.mark.parametrize("tilted", [False, True])
def test_c1_from_its_joint_state_against_the_oracle(pfc, scen, tilted):
    from oracle import oracle as O
    mech, q, v, x_c1, tw_c1 = _c1_state(pfc, tilted)
    _set(scen, mech)
    wrench, sdot, counts, f, it, (x, tw, jac) = scen.force_all_elastic_intersections_state(q, v)
    if not tilted:
        assert x.tobytes() == x_c1.tobytes() and tw.tobytes() == tw_c1.tobytes()
    xr, twr, jr = K.kin_reference(mech, q, v)      # no revolute joint: no trigonometry
    assert np.array_equal(x, xr) and np.array_equal(tw, twr) and np.array_equal(jac, jr)
    w = pfc.configs.c1_boxes()
    bind = [(c.id_1, c.id_2) for c in w.instructions]
    pose_r, twist_r, x_w_r2, b1, b2 = items_reference(bind, xr, twr)
    assert np.array_equal(it.pose, pose_r) and np.array_equal(it.twist, twist_r) and np.array_equal(it.x_w_r2, x_w_r2)
    assert np.array_equal(it.body_1, b1) and np.array_equal(it.body_2, b2)
    w.pose, w.twist = pose_r, twist_r
    ref = H.oracle_run(pfc, w, debug=False)
    for k, r in enumerate(ref):
        print(f"item {k}: counts {counts[k]} oracle {r.counts} wrench rel {H.rel_err(wrench[k], r.wrench):.2e}")
        assert np.array_equal(counts[k], r.counts), (k, counts[k], r.counts)
        assert r.counts[3] > 0
        assert H.rel_err(wrench[k], r.wrench) < 1e-9, k
        assert H.rel_err(sdot[k], r.sdot) < 1e-9 or np.linalg.norm(r.sdot) == 0, k
    f_ref = O.scatter_generalized(np.array([r.wrench for r in ref]), x_w_r2, b1, b2, jr, None, n_scene=1)
    print(f"f_generalized against the oracle's: largest difference {np.abs(f - f_ref).max():.2e} of {np.abs(f_ref).max():.2e}")
    if tilted:      # the friction wrench is there, and the Jacobians' cross terms t x R[:,k]
        assert min(np.abs(np.array([r.wrench for r in ref])[:, 3:5]).max(axis=1)) > 1e-3
        assert all(np.abs(jr[b, 6 * (b - 1):6 * (b - 1) + 3, 3:]).max() > 0 for b in range(1, 5))
    assert np.abs(f_ref).max() > 0
    np.testing.assert_allclose(f, f_ref, rtol=1e-12, atol=1e-12 * np.abs(f_ref).max())


# ---- 8. the chain equals its parts ---------------------------------------------------------------------------------------------
def test_chain_equals_its_parts(pfc, scen):
    torch = _torch()
    mech, q0, v0, _, _ = _c1_state(pfc, True)
    _set(scen, mech)
    n_scene, n_body, nv, n = 3, 5, 24, 12
    rng = np.random.default_rng(81)
    q = np.tile(q0, (n_scene, 1)); v = np.tile(v0, (n_scene, 1))
    q[1:, :] += 1e-4 * rng.standard_normal((2, 24)); v[1:, :] += 0.05 * rng.standard_normal((2, 24))
    ids = np.tile(np.arange(4, dtype=np.int32), n_scene); scene = np.repeat(np.arange(n_scene, dtype=np.int32), 4)
    dev = torch.device("cuda", 0)
    z = lambda *sh, dt=torch.float64: torch.zeros(sh, dtype=dt, device=dev)
    d_q, d_v, d_ids, d_sc = _dev(q), _dev(v), _dev(ids), _dev(scene)
    nb = n_scene * n_body

    def buffers():
        return ([Guarded(nb, 12), Guarded(nb, 6), Guarded(nb * nv, 6)],
                [Guarded(n, 24), Guarded(n, 6), Guarded(n, 12), Guarded(n, 1, True), Guarded(n, 1, True)],
                [z(n, 6), z(n, 6), z(n, 4, dt=torch.int32)], Guarded(n_scene, nv))

    ka, ia, ea, fa = buffers()
    kb, ib, eb, fb = buffers()
    torch.cuda.synchronize()      # the calls below run on the handle's own stream
    for _ in range(40):
        scen.eval_state_device(n, d_ids.data_ptr(), d_sc.data_ptr(), n_scene, d_q.data_ptr(), d_v.data_ptr(), 0, *[o.ptr for o in ka],
                               *[o.ptr for o in ia], *[t.data_ptr() for t in ea], fa.ptr)
        rc = scen.check()
        if rc == 0:
            break
    assert rc == 0
    scen.kinematics_device(n_scene, d_q.data_ptr(), d_v.data_ptr(), *[o.ptr for o in kb])
    for _ in range(40):
        scen.eval_bodies_device(n, d_ids.data_ptr(), d_sc.data_ptr(), n_scene, n_body, kb[0].ptr, kb[1].ptr, 0, *[o.ptr for o in ib],
                                *[t.data_ptr() for t in eb])
        rc = scen.check()
        if rc == 0:
            break
    assert rc == 0
    scen.scatter_generalized_device(n, eb[0].data_ptr(), ib[2].ptr, ib[3].ptr, ib[4].ptr, d_sc.data_ptr(), n_scene, nv, kb[2].ptr, fb.ptr)
    torch.cuda.synchronize()
    for a, b in zip(ka + ia, kb + ib):      # states and items: the same bytes
        assert a.rows().tobytes() == b.rows().tobytes()
    xr, twr, jr = K.kin_reference(mech, q, v)
    assert np.array_equal(ka[0].rows(), xr.reshape(-1, 12)) and np.array_equal(ka[2].rows(), jr.reshape(-1, 6))
    (wa, sa, ca), (wb, sb, cb) = ([t.cpu().numpy() for t in e] for e in (ea, eb))
    assert ca[:, 3].all(), "an item has no contact"
    assert np.array_equal(ca, cb)
    assert max(H.rel_err(wa[k], wb[k]) for k in range(n)) < 1e-9
    for k in range(n):
        assert H.rel_err(sa[k], sb[k]) < 1e-9 if np.linalg.norm(sb[k]) > 0 else not sa[k].any()
    f1, f2 = fa.rows(), fb.rows()
    assert np.abs(f2).max() > 0
    # k_scatter sums with atomics: f is not bit-stable from call to call
    np.testing.assert_allclose(f1, f2, rtol=1e-12, atol=1e-12 * np.abs(f2).max())
    # d_f = NULL: no scatter, a guarded f is untouched; the rest is as it was
    kc, ic, ec, fc = buffers()
    for _ in range(40):
        scen.eval_state_device(n, d_ids.data_ptr(), d_sc.data_ptr(), n_scene, d_q.data_ptr(), d_v.data_ptr(), 0, *[o.ptr for o in kc],
                               *[o.ptr for o in ic], *[t.data_ptr() for t in ec], 0)
        rc = scen.check()
        if rc == 0:
            break
    assert rc == 0
    torch.cuda.synchronize()
    assert fc.untouched()
    for a, c in zip(ka + ia, kc + ic):
        assert a.rows().tobytes() == c.rows().tobytes()
    assert np.array_equal(ec[2].cpu().numpy(), ca)


# ---- 9. error paths ------------------------------------------------------------------------------------------------------------
def _raw_mech(mech):
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    keep = (np.ascontiguousarray(mech["parent"], dtype=np.int32), np.ascontiguousarray(mech["joint_type"], dtype=np.int32),
            np.ascontiguousarray(mech["x_p_j"], dtype=np.float64), np.ascontiguousarray(mech["axis"], dtype=np.float64))
    return keep, (keep[0].ctypes.data_as(ip), keep[1].ctypes.data_as(ip), keep[2].ctypes.data_as(dp), keep[3].ctypes.data_as(dp))


def test_error_paths_write_nothing(pfc):
    torch = _torch()
    L = pfc._lib
    lib = L.lib()
    h = C.c_void_p()
    assert lib.pfc_create(0, C.byref(h)) == 0
    mech = K.mech_c()
    q, v = _states(mech, 2, 9)
    q[:, 1] = 0.0                                   # the revolute joint at angle 0: cos = 1, sin = 0 on any libm
    d_q, d_v = _dev(q), _dev(v)
    out = _kin_outputs(mech, 2)
    msg = lambda: lib.pfc_last_error(h).decode()
    # kinematics before pfc_set_mechanism
    assert lib.pfc_kinematics_device(h, 2, d_q.data_ptr(), d_v.data_ptr(), *[o.ptr for o in out], None) == L.ERR_STATE
    assert "pfc_set_mechanism" in msg()
    assert lib.pfc_mechanism_sizes(h, None, None, None) == L.ERR_STATE
    # bad tables: the message names the body, the handle keeps no mechanism
    def bad(**kw):
        m = dict(mech); m.update({k: np.array(a) for k, a in kw.items()})
        keep, ptr = _raw_mech(m)
        return lib.pfc_set_mechanism(h, len(m["parent"]), *ptr)
    assert bad(parent=[-1, 0, 2, 1]) == L.ERR_BAD_ARG and "body 2" in msg()              # a parent >= b
    assert bad(parent=[-1, -2, 1, 1]) == L.ERR_BAD_ARG and "body 1" in msg()             # a parent < -1
    assert bad(joint_type=[2, 1, 2, 7]) == L.ERR_BAD_ARG and "body 3" in msg()           # joint type 7
    ax = mech["axis"].copy(); ax[1] = 0.0
    assert bad(axis=ax) == L.ERR_BAD_ARG and "body 1" in msg()                           # a zero axis
    keep, ptr = _raw_mech(mech)
    assert lib.pfc_set_mechanism(h, 0, *ptr) == L.ERR_BAD_ARG                            # n_body = 0
    assert lib.pfc_set_mechanism(h, 4, ptr[0], None, ptr[2], ptr[3]) == L.ERR_BAD_ARG    # a null table
    assert lib.pfc_kinematics_device(h, 2, d_q.data_ptr(), d_v.data_ptr(), *[o.ptr for o in out], None) == L.ERR_STATE
    # a good one: kinematics needs no pfc_finalize, pfc_eval_state_device does
    assert lib.pfc_set_mechanism(h, 4, *ptr) == 0
    nb, nq, nv = C.c_int(), C.c_int(), C.c_int()
    assert lib.pfc_mechanism_sizes(h, C.byref(nb), C.byref(nq), C.byref(nv)) == 0 and (nb.value, nq.value, nv.value) == (4, 4, 4)
    assert lib.pfc_kinematics_device(h, 0, None, None, *[o.ptr for o in out], None) == 0   # n_scene = 0: a no-op
    torch.cuda.synchronize()
    assert all(o.untouched() for o in out)
    items = [Guarded(1, 24), Guarded(1, 6), Guarded(1, 12), Guarded(1, 1, True), Guarded(1, 1, True)]
    res = [Guarded(1, 6), Guarded(1, 6), Guarded(1, 4, True), Guarded(2, 4)]
    rc = lib.pfc_eval_state_device(h, 1, None, None, 2, d_q.data_ptr(), d_v.data_ptr(), None, *[o.ptr for o in out], *[o.ptr for o in items],
                                   *[o.ptr for o in res], None)
    assert rc == L.ERR_STATE and "pfc_finalize" in msg()
    torch.cuda.synchronize()
    assert all(o.untouched() for o in out + items + res)
    assert lib.pfc_kinematics_device(h, 2, d_q.data_ptr(), d_v.data_ptr(), *[o.ptr for o in out], None) == 0
    torch.cuda.synchronize()
    for o, r, wd in zip(out, K.kin_reference(mech, q, v), (12, 6, 6)):
        assert np.array_equal(o.rows(), r.reshape(-1, wd))
    lib.pfc_destroy(h)

    # an instruction bound to body 9 of a 5-body mechanism
    w = pfc.configs.c1_boxes()
    m = pfc.configs.build_scenario(w)
    for k, c in enumerate(w.instructions):
        m.set_instruction_bodies(k, c.id_1, c.id_2)
    mb, qb, vb, _, _ = _c1_state(pfc, False)
    _set(m, mb)
    m.set_instruction_bodies(3, 9, 4)
    d_qb, d_vb = _dev(qb), _dev(vb)
    kin = _kin_outputs(mb, 1)
    items = [Guarded(4, 24), Guarded(4, 6), Guarded(4, 12), Guarded(4, 1, True), Guarded(4, 1, True)]
    res = [Guarded(4, 6), Guarded(4, 6), Guarded(4, 4, True), Guarded(1, 24)]
    with pytest.raises(L.PFCError) as e:
        m.eval_state_device(4, 0, 0, 1, d_qb.data_ptr(), d_vb.data_ptr(), 0, *[o.ptr for o in kin], *[o.ptr for o in items], *[o.ptr for o in res])
    assert e.value.status == L.ERR_BAD_ARG and "instruction 3" in str(e.value)
    with pytest.raises(L.PFCError) as e:
        m.force_all_elastic_intersections_state(qb, vb)
    assert e.value.status == L.ERR_BAD_ARG and "instruction 3" in str(e.value)
    torch.cuda.synchronize()
    assert all(o.untouched() for o in kin + items + res)
    m.set_instruction_bodies(3, 3, 4)
    # a second pfc_set_mechanism with another nv takes effect on the next call
    assert m.mechanism_sizes() == (5, 24, 24)
    x1, _, _ = m.kinematics(qb, vb)
    two = K.make_mech([-1, 0], [K.PRISMATIC, K.PRISMATIC], [K.WORLD_X, K.WORLD_X], [[0, 0, 1], [1, 0, 0]])
    _set(m, two)
    assert m.mechanism_sizes() == (2, 2, 2)
    q2, v2 = np.array([[0.25, -1.5]]), np.array([[1.0, 2.0]])
    x2, tw2, j2 = m.kinematics(q2, v2)
    r2 = K.kin_reference(two, q2, v2)
    assert x2.shape == (1, 2, 12) and x1.shape == (1, 5, 12)
    assert np.array_equal(x2, r2[0]) and np.array_equal(tw2, r2[1]) and np.array_equal(j2, r2[2])
    # NaN in q reaches that scene's outputs only; pfc_check stays OK
    ma = K.mech_c()
    _set(m, ma)
    qn, vn = _states(ma, 3, 11)
    qn[:, 1] = 0.0                                  # the revolute joint at angle 0: cos = 1, sin = 0 on any libm
    ref = K.kin_reference(ma, qn, vn)
    qn[1, 0] = np.nan
    xn, twn, jn = m.kinematics(qn, vn)
    assert np.isnan(xn[1]).any() and np.isnan(jn.reshape(3, -1)[1]).any()
    for s in (0, 2):
        assert np.array_equal(xn[s], ref[0][s]) and np.array_equal(twn[s], ref[1][s])
        assert np.array_equal(jn.reshape(3, -1)[s], ref[2].reshape(3, -1)[s])
    assert m.check() == 0
    m.close()
