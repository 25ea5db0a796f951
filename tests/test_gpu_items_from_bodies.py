"""Contact items from body states on the device (pfc_set_instruction_bodies, pfc_items_from_bodies[_device],
pfc_eval_bodies[_device]): bytes against the scalar statement of tests/test_items_from_bodies_abi.py, C1 rebuilt from its world
states against the oracle, the chain body states -> items -> wrenches -> f_generalized against its parts, and the error paths.

Tolerances: the items are compared as bytes (values; np.array_equal does not tell -0.0 from 0.0); against relative_pose /
relative_twist under items_bound (derived in the ABI test file); wrench and sdot at the suite's 1e-9 relative
(tests/test_gpu_parity.py); the scatter at 1e-12 (test_scatter_generalized_third_law)."""
import numpy as np
import pytest

import helpers as H
from test_items_from_bodies_abi import WORLD_X, items_bound, items_reference

pytestmark = pytest.mark.gpu

GUARD = 16                  # guard words in front of and behind every device output
SENTINEL = -7.0e77
ISENTINEL = -77777


def _torch():
    import torch
    return torch


def _dev(a, dt=None):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).to(torch.device("cuda", 0))


class Guarded:
    """A device array of n x width behind GUARD sentinel words on either side; ptr is the address of its first row."""

    def __init__(self, n, width, integer=False):
        torch = _torch()
        self.n, self.width, self.fill = n, width, ISENTINEL if integer else SENTINEL
        self.t = torch.full((n * width + 2 * GUARD,), self.fill, dtype=torch.int32 if integer else torch.float64,
                            device=torch.device("cuda", 0))
        self.ptr = self.t.data_ptr() + GUARD * self.t.element_size()

    def rows(self):
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == self.fill).all() and (a[a.size - GUARD:] == self.fill).all(), "guard words overwritten"
        a = a[GUARD:a.size - GUARD]
        return a.reshape(self.n, self.width) if self.width > 1 else a

    def untouched(self):
        return bool((self.t == self.fill).all().item())


def _outputs(n):
    return [Guarded(n, 24), Guarded(n, 6), Guarded(n, 12), Guarded(n, 1, True), Guarded(n, 1, True)]


def _random_states(pfc, rng, n_scene, n_body):
    x = np.zeros((n_scene, n_body, 12)); tw = rng.standard_normal((n_scene, n_body, 6))
    for s in range(n_scene):
        for b in range(n_body):
            x[s, b, :9] = pfc.configs.random_rotation(rng).reshape(-1, order="F")
            x[s, b, 9:] = rng.uniform(-1, 1, 3) * rng.uniform(0, 10)
    return x, tw


# ---- 1. bits ---------------------------------------------------------------------------------------------------------
N_INS_BITS = 260


@pytest.fixture(scope="module")
def bound_c1(pfc):
    """C1's meshes under 260 instructions (its four, repeated) bound to random bodies of 5, the world on side 1, on side 2 and
    on both among them."""
    w = pfc.configs.c1_boxes()
    w.instructions = w.instructions * (N_INS_BITS // 4)
    m = pfc.configs.build_scenario(w)
    rng = np.random.default_rng(31)
    bind = rng.integers(-1, 5, (N_INS_BITS, 2)).astype(np.int32)
    bind[0] = (-1, 3); bind[1] = (2, -1); bind[2] = (-1, -1); bind[3] = (4, 0)
    for k in range(N_INS_BITS):
        m.set_instruction_bodies(k, bind[k, 0], bind[k, 1])
    yield m, bind
    m.close()


@pytest.mark.parametrize("ids_given", [True, False])
@pytest.mark.parametrize("n_scene", [1, 3])
@pytest.mark.parametrize("n_items", [1, 63, 64, 65, 257])
def test_items_are_the_bytes_of_the_scalar_statement(pfc, bound_c1, n_items, n_scene, ids_given):
    torch = _torch()
    m, bind = bound_c1
    n, n_body = n_items, 5
    rng = np.random.default_rng(1000 * n_items + 10 * n_scene + ids_given)
    x, tw = _random_states(pfc, rng, n_scene, n_body)
    ids = scene = None
    if ids_given:
        ids = rng.integers(0, N_INS_BITS, n).astype(np.int32); ids[:min(n, 4)] = np.arange(min(n, 4))
        scene = rng.integers(0, n_scene, n).astype(np.int32)
    ref = items_reference(bind, x, tw, ids, scene) if ids_given else items_reference(bind[:n], x, tw)
    assert (ref[3] == -1).any() or n < 3
    d_x, d_tw = _dev(x), _dev(tw)
    d_ids = _dev(ids) if ids_given else None
    d_sc = _dev(scene) if ids_given else None
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr() if t is not None else 0
    out = _outputs(n)
    m.items_from_bodies_device(n, p(d_ids), p(d_sc), n_scene, n_body, d_x.data_ptr(), d_tw.data_ptr(), *[o.ptr for o in out], st)
    torch.cuda.synchronize()
    got = [o.rows() for o in out]
    for name, g, r in zip(("pose", "twist", "x_w_r2", "body_1", "body_2"), got, ref):
        assert np.array_equal(g, r), (name, np.argwhere(g != r)[:4])
    # x_w_r2 is the gathered input, the ids are offset by scene * n_body
    for i in range(n):
        b2 = bind[ids[i] if ids_given else i, 1]; sc = scene[i] if ids_given else 0
        assert np.array_equal(got[2][i], x[sc, b2] if b2 >= 0 else WORLD_X)
        assert got[4][i] == (b2 + sc * n_body if b2 >= 0 else -1)
    # outputs passed as NULL are not written, the wanted ones are the same bytes
    for want in ((0, 1, 0, 0, 1), (1, 0, 1, 1, 0)):
        part = _outputs(n)
        m.items_from_bodies_device(n, p(d_ids), p(d_sc), n_scene, n_body, d_x.data_ptr(), d_tw.data_ptr(),
                                   *[o.ptr if k else 0 for o, k in zip(part, want)], st)
        torch.cuda.synchronize()
        for o, k, g in zip(part, want, got):
            if k:
                assert o.rows().tobytes() == g.tobytes()
            else:
                assert o.untouched()
    # the host entry point: the same bytes
    it = m.items_from_bodies(x, tw, ids, scene) if ids_given else m.items_from_bodies(x, tw, ins_ids=np.arange(n, dtype=np.int32))
    for g, hst in zip(got, (it.pose, it.twist, it.x_w_r2, it.body_1, it.body_2)):
        assert np.ascontiguousarray(hst).tobytes() == g.tobytes()


# ---- world states of the scenes ----------------------------------------------------------------------------------------
def c1_world_states(pfc):
    """The five world poses and twists configs.c1_boxes() builds its items from (plane, box_1 .. box_4; body = mesh id)."""
    Cf = pfc.configs
    r, pen = 0.05, 0.001
    z = [0.0, r - pen, 3 * r - 2 * pen, 5 * r - 3 * pen, 7 * r - 4 * pen]
    x = np.zeros((1, 5, 12)); tw = np.zeros((1, 5, 6))
    for b in range(5):
        R = np.eye(3) if b == 0 else Cf.rot_z(0.1 * b)
        x[0, b, :9] = R.reshape(-1, order="F"); x[0, b, 11] = z[b]
        tw[0, b, 2] = float(b)
    return x, tw


def states_from_items(pfc, w, world_side, rng):
    """Body states that reproduce a workload's items up to rounding: one scene per item, body 0 on side 1 and body 1 on side 2.
    world_side[ins] in (0, 1, 2): neither body of the instruction is the world / body 1 is / body 2 is.  Returns (x, tw, bind)."""
    n = w.n_items
    x = np.zeros((n, 2, 12)); tw = np.zeros((n, 2, 6))
    x[:, :, [0, 4, 8]] = 1.0
    for k in range(n):
        side = world_side[int(w.ins_ids[k])]
        R21 = w.pose[k, :9].reshape(3, 3, order="F"); t21 = w.pose[k, 9:12]
        if side == 2:
            R2, t2 = np.eye(3), np.zeros(3)
        elif side == 1:
            R2, t2 = w.pose[k, 12:21].reshape(3, 3, order="F"), w.pose[k, 21:24]
        else:
            R2, t2 = pfc.configs.random_rotation(rng), rng.standard_normal(3)
        R1, t1 = R2 @ R21, R2 @ t21 + t2
        # twist_r2_r1_r2 = transform(tw_2 - tw_1, x_r2_rw)  =>  tw_2 - tw_1 = transform(twist, x_rw_r2)
        ang = R2 @ w.twist[k, :3]
        d = np.concatenate([ang, R2 @ w.twist[k, 3:] + np.cross(t2, ang)])
        tw2 = np.zeros(6) if side == 2 else (d if side == 1 else rng.standard_normal(6))
        tw1 = tw2 - d
        x[k, 0] = np.concatenate([R1.reshape(-1, order="F"), t1]); x[k, 1] = np.concatenate([R2.reshape(-1, order="F"), t2])
        tw[k, 0], tw[k, 1] = tw1, tw2
        if side == 1:
            x[k, 0] = WORLD_X; tw[k, 0] = 0.0      # (not read: the instruction is bound to -1 there)
    bind = [(-1 if s == 1 else 0, -1 if s == 2 else 1) for s in world_side]
    return x, tw, bind


def _bind(m, bind):
    for k, (b1, b2) in enumerate(bind):
        m.set_instruction_bodies(k, b1, b2)


# ---- 2. C1 from world states -----------------------------------------------------------------------------------------
def test_c1_from_world_states_against_relative_pose_and_oracle(pfc):
    torch = _torch()
    w = pfc.configs.c1_boxes()
    x, tw = c1_world_states(pfc)
    bind = [(c.id_1, c.id_2) for c in w.instructions]
    m = pfc.configs.build_scenario(w)
    _bind(m, bind)
    n = w.n_items
    d_x, d_tw = _dev(x), _dev(tw)
    out = _outputs(n)
    z = lambda *sh, dt=torch.float64: torch.zeros(sh, dtype=dt, device=torch.device("cuda", 0))
    o_w, o_sd, o_ct = z(n, 6), z(n, 6), z(n, 4, dt=torch.int32)
    torch.cuda.synchronize()
    for _ in range(40):
        m.eval_bodies_device(n, 0, 0, 1, 5, d_x.data_ptr(), d_tw.data_ptr(), 0, *[o.ptr for o in out], o_w.data_ptr(), o_sd.data_ptr(),
                             o_ct.data_ptr())
        rc = m.check()
        if rc == 0:
            break
    assert rc == 0
    pose, twist = out[0].rows(), out[1].rows()
    for k in range(n):
        b1, b2 = bind[k]
        bp, bt = items_bound(x[0, b1], tw[0, b1], x[0, b2], tw[0, b2])
        assert (np.abs(pose[k] - w.pose[k]) <= bp).all(), (k, np.abs(pose[k] - w.pose[k]), bp)
        assert (np.abs(twist[k] - w.twist[k]) <= bt).all(), (k, np.abs(twist[k] - w.twist[k]), bt)
    wrench, sdot, counts = o_w.cpu().numpy(), o_sd.cpu().numpy(), o_ct.cpu().numpy()
    ref = H.oracle_run(pfc, w, debug=False)
    for k, r in enumerate(ref):
        print(f"item {k}: counts {counts[k]} oracle {r.counts} wrench rel {H.rel_err(wrench[k], r.wrench):.2e}")
        assert np.array_equal(counts[k], r.counts), (k, counts[k], r.counts)
        assert H.rel_err(wrench[k], r.wrench) < 1e-9, k
        assert H.rel_err(sdot[k], r.sdot) < 1e-9 or np.linalg.norm(r.sdot) == 0, k
    m.close()


# ---- 3. the chain equals its parts -----------------------------------------------------------------------------------
def _chain_scene(pfc, name):
    Cf = pfc.configs
    rng = np.random.default_rng(7)
    if name == "c1":
        w = Cf.c1_boxes()
        x, tw = c1_world_states(pfc)
        return w, x, tw, [(c.id_1, c.id_2) for c in w.instructions], None
    if name == "c2":
        w = Cf.c2_box_on_plane(n_scenes=64)
        x, tw, bind = states_from_items(pfc, w, [1], rng)      # the plane is the world
    else:
        w = Cf.vol_vol(n_poses=4, model="bristle")
        x, tw, bind = states_from_items(pfc, w, [2, 0], rng)   # the box on the world's half-plane; two free spheres
    return w, x, tw, bind, np.arange(w.n_items, dtype=np.int32)


@pytest.mark.parametrize("fixed_order", [1, 0])
@pytest.mark.parametrize("name", ["c1", "c2", "vol_vol"])
def test_chain_equals_its_parts(pfc, name, fixed_order):
    torch = _torch()
    w, x, tw, bind, scene = _chain_scene(pfc, name)
    n, n_scene, n_body, nv = w.n_items, x.shape[0], x.shape[1], 12
    m = pfc.configs.build_scenario(w)
    m.set_option("fixed_order", fixed_order)
    _bind(m, bind)
    dev = torch.device("cuda", 0)
    z = lambda *sh, dt=torch.float64: torch.zeros(sh, dtype=dt, device=dev)
    d_x, d_tw, d_ids, d_s = _dev(x), _dev(tw), _dev(w.ins_ids), _dev(w.s)
    d_sc = _dev(scene) if scene is not None else None
    sc_p = d_sc.data_ptr() if scene is not None else 0
    out = _outputs(n)
    a = [z(n, 6), z(n, 6), z(n, 4, dt=torch.int32)]
    b = [z(n, 6), z(n, 6), z(n, 4, dt=torch.int32)]
    torch.cuda.synchronize()      # the calls below run on the handle's own stream
    for _ in range(40):
        m.eval_bodies_device(n, d_ids.data_ptr(), sc_p, n_scene, n_body, d_x.data_ptr(), d_tw.data_ptr(), d_s.data_ptr(),
                             *[o.ptr for o in out], *[t.data_ptr() for t in a])
        rc = m.check()
        if rc == 0:
            break
    assert rc == 0
    for _ in range(40):
        m.eval_device(n, d_ids.data_ptr(), out[0].ptr, out[1].ptr, d_s.data_ptr(), *[t.data_ptr() for t in b])
        rc = m.check()
        if rc == 0:
            break
    assert rc == 0
    (wa, sa, ca), (wb, sb, cb) = ([t.cpu().numpy() for t in q] for q in (a, b))
    assert ca[:, 3].any(), "the scene has no contact"
    assert np.array_equal(ca, cb)
    if fixed_order:
        assert wa.tobytes() == wb.tobytes() and sa.tobytes() == sb.tobytes() and ca.tobytes() == cb.tobytes()
    else:
        ew = max(H.rel_err(wa[k], wb[k]) for k in range(n) if np.linalg.norm(wb[k]) > 0)
        es = max([H.rel_err(sa[k], sb[k]) for k in range(n) if np.linalg.norm(sb[k]) > 0] or [0.0])
        print(f"{name}: eval_bodies_device against eval_device, largest per-item relative difference: wrench {ew:.2e}, sdot {es:.2e}")
        assert ew < 1e-9 and es < 1e-9
    # the kernel's x_w_r2 / body ids feed the device scatter; against the host scatter on the host-formed copies
    pose_r, twist_r, x_r, b1_r, b2_r = items_reference(bind, x, tw, w.ins_ids, scene)
    got = [o.rows() for o in out]
    assert np.array_equal(got[0], pose_r) and np.array_equal(got[1], twist_r)
    jac = np.random.default_rng(9).standard_normal((n_scene * n_body, nv, 6))
    d_jac, d_f = _dev(jac), z(n_scene, nv)
    torch.cuda.synchronize()
    m.scatter_generalized_device(n, a[0].data_ptr(), out[2].ptr, out[3].ptr, out[4].ptr, sc_p, n_scene, nv, d_jac.data_ptr(), d_f.data_ptr(),
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    f = d_f.cpu().numpy()
    ref = m.scatter_generalized(wa, x_r, b1_r, b2_r, jac, scene, n_scene=n_scene)
    assert np.abs(ref).max() > 0
    np.testing.assert_allclose(f, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
    m.close()


# ---- 4. not an evaluation --------------------------------------------------------------------------------------------
def test_items_from_bodies_is_not_an_evaluation(pfc):
    torch = _torch()
    w = pfc.configs.c1_boxes()
    x, tw = c1_world_states(pfc)
    m = pfc.configs.build_scenario(w)
    _bind(m, [(c.id_1, c.id_2) for c in w.instructions])
    n, nd = w.n_items, 6
    rng = np.random.default_rng(4)
    dev = torch.device("cuda", 0)
    z = lambda *sh, dt=torch.float64: torch.zeros(sh, dtype=dt, device=dev)
    t = [_dev(w.ins_ids), _dev(w.pose), _dev(w.twist), _dev(w.s)]
    sd = [_dev(rng.standard_normal((n, nd, 24)) * 1e-2), _dev(rng.standard_normal((n, nd, 6)) * 0.1), _dev(rng.standard_normal((n, nd, 6)) * 1e-3)]
    o_w, o_sd, o_ct, o_dw, o_dsd = z(n, 6), z(n, 6), z(n, 4, dt=torch.int32), z(n, nd, 6), z(n, nd, 6)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(40):
        m.eval_dual_device(n, nd, *[q.data_ptr() for q in t], *[q.data_ptr() for q in sd], o_w.data_ptr(), o_sd.data_ptr(), o_dw.data_ptr(),
                           o_dsd.data_ptr(), o_ct.data_ptr(), st)
        rc = m.check()
        if rc == 0:
            break
    assert rc == 0
    first = (o_dw.cpu().numpy().copy(), o_dsd.cpu().numpy().copy())
    d_x, d_tw = _dev(x), _dev(tw)
    out = _outputs(n)
    m.items_from_bodies_device(n, 0, 0, 1, 5, d_x.data_ptr(), d_tw.data_ptr(), *[o.ptr for o in out], st)
    o_dw.zero_(); o_dsd.zero_()
    m.eval_dual_device_more(nd, *[q.data_ptr() for q in sd], o_dw.data_ptr(), o_dsd.data_ptr(), st)
    assert m.check() == 0
    assert m.last_dual_reused()
    assert np.abs(first[0]).max() > 0
    scale = np.abs(first[0]).max()
    assert np.abs(o_dw.cpu().numpy() - first[0]).max() <= 1e-9 * scale      # the same chunk at the same point (test_gpu_dual's tolerance)
    assert np.array_equal(out[0].rows(), items_reference([(c.id_1, c.id_2) for c in w.instructions], x, tw)[0])
    m.close()


# ---- 5. errors ---------------------------------------------------------------------------------------------------------
def test_errors_and_rebinding(pfc):
    torch = _torch()
    L = pfc._lib
    w = pfc.configs.c1_boxes()
    x, tw = c1_world_states(pfc)
    m = pfc.configs.build_scenario(w)
    bind = [(c.id_1, c.id_2) for c in w.instructions]
    _bind(m, bind[:3])                               # instruction 3 never bound
    with pytest.raises(L.PFCError) as e:
        m.items_from_bodies(x, tw)
    assert e.value.status == L.ERR_STATE and "instruction 3" in str(e.value)
    d_x, d_tw = _dev(x), _dev(tw)
    out = _outputs(4)
    with pytest.raises(L.PFCError) as e:
        m.items_from_bodies_device(4, 0, 0, 1, 5, d_x.data_ptr(), d_tw.data_ptr(), *[o.ptr for o in out])
    assert e.value.status == L.ERR_STATE and "instruction 3" in str(e.value)
    with pytest.raises(L.PFCError) as e:
        m.force_all_elastic_intersections_bodies(x, tw)
    assert e.value.status == L.ERR_STATE
    it = m.items_from_bodies(x, tw, ins_ids=[0, 1, 2])      # the bound ones alone are fine on the host form
    assert np.array_equal(it.pose, items_reference(bind[:3], x, tw)[0])
    m.set_instruction_bodies(3, *bind[3])
    # host form: a body id >= n_body, a scene id >= n_scene, an instruction id out of range: BAD_ARG, nothing written
    lib, h = L.lib(), m._h
    import ctypes as C
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    pose = np.full((4, 24), SENTINEL); twist = np.full((4, 6), SENTINEL); xr = np.full((4, 12), SENTINEL)
    b1 = np.full(4, ISENTINEL, dtype=np.int32); b2 = np.full(4, ISENTINEL, dtype=np.int32)
    outs = (pose.ctypes.data_as(dp), twist.ctypes.data_as(dp), xr.ctypes.data_as(dp), b1.ctypes.data_as(ip), b2.ctypes.data_as(ip))
    xs, tws = np.ascontiguousarray(x[:, :4]), np.ascontiguousarray(tw[:, :4])      # four bodies: instruction 3 names body 4
    ids = np.arange(4, dtype=np.int32); sc = np.array([0, 0, 1, 0], dtype=np.int32); bad = np.array([0, 1, 4, 2], dtype=np.int32)
    for args in ((None, None, 1, 4, xs, tws), (ids.ctypes.data_as(ip), sc.ctypes.data_as(ip), 1, 5, x, tw),
                 (bad.ctypes.data_as(ip), None, 1, 5, x, tw)):
        rc = lib.pfc_items_from_bodies(h, 4, args[0], args[1], args[2], args[3], args[4].ctypes.data_as(dp), args[5].ctypes.data_as(dp), *outs)
        assert rc == L.ERR_BAD_ARG, rc
        assert (pose == SENTINEL).all() and (twist == SENTINEL).all() and (xr == SENTINEL).all()
        assert (b1 == ISENTINEL).all() and (b2 == ISENTINEL).all()
    # n_items = 0
    assert lib.pfc_items_from_bodies(h, 0, None, None, 1, 5, x.ctypes.data_as(dp), tw.ctypes.data_as(dp), *outs) == 0
    m.items_from_bodies_device(0, 0, 0, 1, 5, d_x.data_ptr(), d_tw.data_ptr(), *[o.ptr for o in out])
    torch.cuda.synchronize()
    assert all(o.untouched() for o in out)
    # rebinding after finalize takes effect on the next call
    it0 = m.items_from_bodies(x, tw)
    m.set_instruction_bodies(1, 4, -1)
    bind2 = list(bind); bind2[1] = (4, -1)
    it1 = m.items_from_bodies(x, tw)
    r0, r1 = items_reference(bind, x, tw), items_reference(bind2, x, tw)
    assert np.array_equal(it0.pose, r0[0]) and np.array_equal(it1.pose, r1[0]) and not np.array_equal(it0.pose[1], it1.pose[1])
    assert it1.body_1[1] == 4 and it1.body_2[1] == -1
    m.close()


# ---- 6. multi-device handle over {0, 0} ------------------------------------------------------------------------------
def test_multi_device_handle_gives_the_same_items(pfc):
    w, x, tw, bind, scene = _chain_scene(pfc, "c2")
    res = []
    for devices in (None, [0, 0]):
        m = pfc.configs.build_scenario(w, devices=devices)
        _bind(m, bind)
        it = m.items_from_bodies(x, tw, w.ins_ids, scene)
        wrench, sdot, counts, it2 = m.force_all_elastic_intersections_bodies(x, tw, w.s, w.ins_ids, scene)
        if devices is not None:
            assert m.last_shards() == 2
        for a, b in zip((it.pose, it.twist, it.x_w_r2, it.body_1, it.body_2), (it2.pose, it2.twist, it2.x_w_r2, it2.body_1, it2.body_2)):
            assert a.tobytes() == b.tobytes()
        res.append((it, wrench, sdot, counts))
        m.close()
    (i0, w0, s0, c0), (i1, w1, s1, c1) = res
    for a, b in zip((i0.pose, i0.twist, i0.x_w_r2, i0.body_1, i0.body_2), (i1.pose, i1.twist, i1.x_w_r2, i1.body_1, i1.body_2)):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(c0, c1) and c0[:, 3].all()
    assert max(H.rel_err(w1[k], w0[k]) for k in range(w.n_items)) < 1e-9
    assert np.array_equal(s0, s1)      # regularized items: zeros
