"""Dual seeds of contact items from body states on the device (pfc_dual_seeds_from_bodies[_device],
pfc_eval_dual_bodies_device[_more]): bytes against the scalar statement of tests/test_dual_seeds_from_bodies_abi.py, the chain
body states + partials -> items + seeds -> Dual evaluation against its parts, the consumers of the three layouts, and the error paths.

Tolerances: seeds, items and everything computed from them under option fixed_order are compared as bytes (values: np.array_equal
does not tell -0.0 from 0.0).  On a default handle C1's flat patches take clamp decisions per pass, so there only the values are
compared, at the suite's 1e-9 relative (tests/test_gpu_parity.py), and counts exactly."""
import ctypes as C

import numpy as np
import pytest

from test_dual_seeds_from_bodies_abi import seeds_reference
from test_gpu_items_from_bodies import Guarded, _dev, _outputs, _random_states, _torch, c1_world_states
from test_items_from_bodies_abi import items_reference

pytestmark = pytest.mark.gpu

N_INS_BITS = 260
N_BODY = 5


def _seed_outputs(n, n_dir):
    return [Guarded(n * n_dir, 24), Guarded(n * n_dir, 6), Guarded(n * n_dir, 12)]


def _p(t):
    return t.data_ptr() if t is not None else 0


def _z(*sh, dt=None):
    torch = _torch()
    return torch.zeros(sh, dtype=dt or torch.float64, device=torch.device("cuda", 0))


def _sync():
    """The handle's stream does not wait for the allocations and fills torch runs on the default stream: order them by hand."""
    _torch().cuda.synchronize()


def _checked(m, call):
    """call() then check(), re-issued while the check asks for it (PFC_ERR_OVERFLOW: the work lists grew)."""
    _sync()
    for _ in range(40):
        call()
        rc = m.check()
        if rc == 0:
            return
    raise AssertionError(f"pfc_check: {rc}")


@pytest.fixture(scope="module")
def bound_c1(pfc):
    """C1's meshes under 260 instructions (its four, repeated) bound to random bodies of 5, the world on side 1, on side 2 and
    on both among them."""
    w = pfc.configs.c1_boxes()
    w.instructions = w.instructions * (N_INS_BITS // 4)
    m = pfc.configs.build_scenario(w)
    rng = np.random.default_rng(31)
    bind = rng.integers(-1, N_BODY, (N_INS_BITS, 2)).astype(np.int32)
    bind[0] = (-1, 3); bind[1] = (2, -1); bind[2] = (-1, -1); bind[3] = (4, 0)
    for k in range(N_INS_BITS):
        m.set_instruction_bodies(k, bind[k, 0], bind[k, 1])
    yield m, bind
    m.close()


def _random_partials(rng, n_scene, n_dir):
    return rng.standard_normal((n_scene, N_BODY, n_dir, 12)), rng.standard_normal((n_scene, N_BODY, n_dir, 6))


# ---- 1. bytes of the statement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids_given", [True, False])
@pytest.mark.parametrize("n_scene", [1, 3])
@pytest.mark.parametrize("n_items,n_dir", [(1, 1), (4, 16), (5, 13), (17, 16), (65, 3)])
def test_seeds_are_the_bytes_of_the_scalar_statement(pfc, bound_c1, n_items, n_dir, n_scene, ids_given):
    torch = _torch()
    m, bind = bound_c1
    n = n_items
    rng = np.random.default_rng(100000 * n_items + 100 * n_dir + 10 * n_scene + ids_given)
    x, tw = _random_states(pfc, rng, n_scene, N_BODY)
    dx, dtw = _random_partials(rng, n_scene, n_dir)
    ids = scene = None
    if ids_given:
        ids = rng.integers(0, N_INS_BITS, n).astype(np.int32); ids[:min(n, 4)] = np.arange(min(n, 4))
        scene = rng.integers(0, n_scene, n).astype(np.int32)
    b = bind if ids_given else bind[:n]
    ref = seeds_reference(b, x, tw, dx, dtw, n_dir, ids, scene)
    d_x, d_tw, d_dx, d_dtw = _dev(x), _dev(tw), _dev(dx), _dev(dtw)
    d_ids = _dev(ids) if ids_given else None
    d_sc = _dev(scene) if ids_given else None
    st = torch.cuda.current_stream().cuda_stream
    head = (n, n_dir, _p(d_ids), _p(d_sc), n_scene, N_BODY, d_x.data_ptr(), d_tw.data_ptr())
    out = _seed_outputs(n, n_dir)
    _sync()
    m.dual_seeds_from_bodies_device(*head, d_dx.data_ptr(), d_dtw.data_ptr(), *[o.ptr for o in out], st)
    torch.cuda.synchronize()
    got = [o.rows() for o in out]
    for name, g, r in zip(("d_pose", "d_twist", "d_x_w_r2"), got, ref):
        r = r.reshape(g.shape)
        assert np.array_equal(g, r), (name, np.argwhere(g != r)[:4])
    assert np.abs(got[0]).max() > 0 or n < 3
    # outputs passed as NULL are not written, the wanted ones are the same bytes
    for want in ((0, 1, 0), (1, 0, 1), (0, 0, 1)):
        part = _seed_outputs(n, n_dir)
        _sync()
        m.dual_seeds_from_bodies_device(*head, d_dx.data_ptr(), d_dtw.data_ptr(), *[o.ptr if k else 0 for o, k in zip(part, want)], st)
        torch.cuda.synchronize()
        for o, k, g in zip(part, want, got):
            if k:
                assert o.rows().tobytes() == g.tobytes()
            else:
                assert o.untouched()
    # NULL partial arrays: the bytes of arrays of zeros
    zx, ztw = _z(*dx.shape), _z(*dtw.shape)
    for px, ptw, rx, rtw in ((0, d_dtw.data_ptr(), None, dtw), (d_dx.data_ptr(), 0, dx, None), (0, 0, None, None)):
        a, bz = _seed_outputs(n, n_dir), _seed_outputs(n, n_dir)
        _sync()
        m.dual_seeds_from_bodies_device(*head, px, ptw, *[o.ptr for o in a], st)
        m.dual_seeds_from_bodies_device(*head, px or zx.data_ptr(), ptw or ztw.data_ptr(), *[o.ptr for o in bz], st)
        torch.cuda.synchronize()
        rz = seeds_reference(b, x, tw, rx, rtw, n_dir, ids, scene)
        for oa, ob, r in zip(a, bz, rz):
            assert oa.rows().tobytes() == ob.rows().tobytes()
            assert np.array_equal(oa.rows(), r.reshape(oa.rows().shape))
    # the host entry point: the same bytes
    sd = (m.dual_seeds_from_bodies(x, tw, dx, dtw, ids, scene) if ids_given else
          m.dual_seeds_from_bodies(x, tw, dx, dtw, ins_ids=np.arange(n, dtype=np.int32)))
    for g, hst in zip(got, sd):
        assert hst.shape[:2] == (n, n_dir) and np.ascontiguousarray(hst).tobytes() == g.tobytes()
    sd = m.dual_seeds_from_bodies(x, tw, None, dtw, ids if ids_given else np.arange(n, dtype=np.int32), scene)
    for r, hst in zip(seeds_reference(b, x, tw, None, dtw, n_dir, ids, scene), sd):
        assert np.array_equal(hst, r)


def test_items_with_ids_out_of_range_write_nothing(pfc, bound_c1):
    torch = _torch()
    m, bind = bound_c1
    n, n_dir, n_scene = 70, 5, 2
    rng = np.random.default_rng(77)
    x, tw = _random_states(pfc, rng, n_scene, N_BODY)
    dx, dtw = _random_partials(rng, n_scene, n_dir)
    ids = rng.integers(0, N_INS_BITS, n).astype(np.int32)
    scene = rng.integers(0, n_scene, n).astype(np.int32)
    ref = seeds_reference(bind, x, tw, dx, dtw, n_dir, ids, scene)
    bad_ids, bad_sc = ids.copy(), scene.copy()
    bad_ids[3] = N_INS_BITS; bad_ids[66] = -1; bad_sc[9] = n_scene; bad_sc[64] = -5
    bad = [3, 9, 64, 66]
    out = _seed_outputs(n, n_dir)
    t = [_dev(q) for q in (bad_ids, bad_sc, x, tw, dx, dtw)]
    _sync()
    m.dual_seeds_from_bodies_device(n, n_dir, t[0].data_ptr(), t[1].data_ptr(), n_scene, N_BODY, *[q.data_ptr() for q in t[2:]],
                                    *[o.ptr for o in out], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for o, r in zip(out, ref):
        g = o.rows().reshape(r.shape)
        assert (g[bad] == o.fill).all()
        ok = np.setdiff1d(np.arange(n), bad)
        assert np.array_equal(g[ok], r[ok])


# ---- C1 and its world states -------------------------------------------------------------------------------------------
class C1:
    """C1 on a handle bound to its world states, with one box's pose and twist seeded in some directions (the others all zero)."""

    def __init__(self, pfc, n_dir, fixed_order, devices=None, seed=5):
        self.w = w = pfc.configs.c1_boxes()
        self.x, self.tw = c1_world_states(pfc)
        self.bind = [(c.id_1, c.id_2) for c in w.instructions]
        self.m = pfc.configs.build_scenario(w, devices=devices)
        if fixed_order:
            self.m.set_option("fixed_order", 1)
        for k, (b1, b2) in enumerate(self.bind):
            self.m.set_instruction_bodies(k, b1, b2)
        self.n, self.n_dir = w.n_items, n_dir
        self.chunks = [self.chunk(np.random.default_rng(seed + c), n_dir) for c in range(2)]
        self.d_x, self.d_tw, self.d_s = _dev(self.x), _dev(self.tw), _dev(w.s)
        self.items = items_reference(self.bind, self.x, self.tw)

    def chunk(self, rng, n_dir):
        """(dx, dtw, ds): box_2 (body 2, on either side of an instruction) seeded in every direction but each third one."""
        dx = np.zeros((1, N_BODY, n_dir, 12)); dtw = np.zeros((1, N_BODY, n_dir, 6))
        on = [k for k in range(n_dir) if k % 3 != 2]
        dx[0, 2, on] = rng.standard_normal((len(on), 12)) * 1e-2
        dtw[0, 2, on] = rng.standard_normal((len(on), 6)) * 0.1
        return dx, dtw, rng.standard_normal((self.w.n_items, n_dir, 6)) * 1e-3

    def seeds(self, c):
        dx, dtw, _ = self.chunks[c]
        return seeds_reference(self.bind, self.x, self.tw, dx, dtw, self.n_dir)

    def head(self):
        return (self.n, self.n_dir, 0, 0, 1, N_BODY, self.d_x.data_ptr(), self.d_tw.data_ptr())


def _results(n, n_dir):
    torch = _torch()
    return [_z(n, 6), _z(n, 6), _z(n, n_dir, 6), _z(n, n_dir, 6), _z(n, 4, dt=torch.int32)]      # wrench, sdot, d_wrench, d_sdot, counts


def _eval_dual_bodies(P, c, items, seeds, res):
    dx, dtw, ds = (_dev(q) for q in P.chunks[c])
    _checked(P.m, lambda: P.m.eval_dual_bodies_device(*P.head(), dx.data_ptr(), dtw.data_ptr(), P.d_s.data_ptr(), ds.data_ptr(),
                                                      *[o.ptr for o in items], *[o.ptr for o in seeds], res[0].data_ptr(),
                                                      res[1].data_ptr(), res[2].data_ptr(), res[3].data_ptr(), res[4].data_ptr()))


def _eval_dual_parts(P, c, res):
    """pfc_eval_dual_device fed items and seeds from the host statement."""
    pose, twist = _dev(P.items[0]), _dev(P.items[1])
    sd = P.seeds(c)
    dp, dt, ds = _dev(sd[0]), _dev(sd[1]), _dev(P.chunks[c][2])
    _checked(P.m, lambda: P.m.eval_dual_device(P.n, P.n_dir, 0, pose.data_ptr(), twist.data_ptr(), P.d_s.data_ptr(), dp.data_ptr(),
                                               dt.data_ptr(), ds.data_ptr(), res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(),
                                               res[3].data_ptr(), res[4].data_ptr()))


# ---- 2. not an evaluation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed_order", [1, 0])
def test_dual_seeds_from_bodies_is_not_an_evaluation(pfc, fixed_order):
    torch = _torch()
    P = C1(pfc, 6, fixed_order)
    n, nd = P.n, P.n_dir
    res = _results(n, nd)
    _eval_dual_parts(P, 0, res)
    sd = P.seeds(1)
    dp, dt, ds = _dev(sd[0]), _dev(sd[1]), _dev(P.chunks[1][2])
    more = lambda: P.m.eval_dual_device_more(nd, dp.data_ptr(), dt.data_ptr(), ds.data_ptr(), res[2].data_ptr(), res[3].data_ptr())
    _sync()
    more()
    assert P.m.check() == 0
    first = (res[2].cpu().numpy().copy(), res[3].cpu().numpy().copy())
    assert np.abs(first[0]).max() > 0
    dx, dtw, _ = (_dev(q) for q in P.chunks[1])
    out = _seed_outputs(n, nd)
    res[2].zero_(); res[3].zero_()
    _sync()
    P.m.dual_seeds_from_bodies_device(*P.head(), dx.data_ptr(), dtw.data_ptr(), *[o.ptr for o in out])
    more()
    assert P.m.check() == 0
    assert P.m.last_dual_reused()
    torch.cuda.synchronize()
    for a, b in zip(first, (res[2].cpu().numpy(), res[3].cpu().numpy())):
        if fixed_order:
            assert np.array_equal(a, b)
        else:      # the same chunk at the same point (test_gpu_dual's tolerance)
            assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max()
    for o, r in zip(out, sd):
        assert np.array_equal(o.rows(), r.reshape(o.rows().shape))
    P.m.close()


# ---- 3. the chain equals its parts, bytes under fixed_order ---------------------------------------------------------------
@pytest.mark.parametrize("n_dir", [6, 16])
def test_chain_equals_its_parts_fixed_order(pfc, n_dir):
    torch = _torch()
    A, B = C1(pfc, n_dir, 1), C1(pfc, n_dir, 1)
    n = A.n
    items, seeds, ra, rb = _outputs(n), _seed_outputs(n, n_dir), _results(n, n_dir), _results(n, n_dir)
    _eval_dual_bodies(A, 0, items, seeds, ra)
    _eval_dual_parts(B, 0, rb)
    torch.cuda.synchronize()
    a, b = [t.cpu().numpy() for t in ra], [t.cpu().numpy() for t in rb]
    assert a[4][:, 3].any(), "the scene has no contact"
    for name, u, v in zip(("wrench", "sdot", "d_wrench", "d_sdot", "counts"), a, b):
        assert u.tobytes() == v.tobytes(), name
    assert np.abs(a[2]).max() > 0
    # the item and seed buffers it leaves: the bytes of the stand-alone calls (and of the statement)
    dx, dtw, _ = (_dev(q) for q in A.chunks[0])
    items1, seeds1 = _outputs(n), _seed_outputs(n, n_dir)
    _sync()
    A.m.items_from_bodies_device(n, 0, 0, 1, N_BODY, A.d_x.data_ptr(), A.d_tw.data_ptr(), *[o.ptr for o in items1])
    A.m.dual_seeds_from_bodies_device(*A.head(), dx.data_ptr(), dtw.data_ptr(), *[o.ptr for o in seeds1])
    torch.cuda.synchronize()
    for o, o1 in zip(items + seeds, items1 + seeds1):
        assert o.rows().tobytes() == o1.rows().tobytes()
    for o, r in zip(items + seeds, list(A.items) + list(A.seeds(0))):
        assert np.array_equal(o.rows(), np.asarray(r).reshape(o.rows().shape))
    # a different chunk at the kept point
    dx, dtw, ds = (_dev(q) for q in A.chunks[1])
    seeds2 = _seed_outputs(n, n_dir)
    _sync()
    A.m.eval_dual_bodies_device_more(*A.head(), dx.data_ptr(), dtw.data_ptr(), ds.data_ptr(), *[o.ptr for o in seeds2],
                                     ra[2].data_ptr(), ra[3].data_ptr())
    assert A.m.check() == 0 and A.m.last_dual_reused()
    sd = B.seeds(1)
    dp, dt = _dev(sd[0]), _dev(sd[1])
    _sync()
    B.m.eval_dual_device_more(n_dir, dp.data_ptr(), dt.data_ptr(), ds.data_ptr(), rb[2].data_ptr(), rb[3].data_ptr())
    assert B.m.check() == 0
    torch.cuda.synchronize()
    for k in (2, 3):
        u, v = ra[k].cpu().numpy(), rb[k].cpu().numpy()
        print(f"_more output {k}: largest |chain - parts| {np.abs(u - v).max():.3e} of {np.abs(v).max():.3e}; against the first chunk "
              f"{np.abs(u - a[k]).max():.3e}")
        assert u.tobytes() == v.tobytes()
    assert ra[2].cpu().numpy().tobytes() != a[2].tobytes()      # (C1's instructions are regularized: sdot and its partials are zero)
    for o, r in zip(seeds2, sd):
        assert np.array_equal(o.rows(), r.reshape(o.rows().shape))
    for k in (0, 1, 4):      # no value output is written by _more
        assert ra[k].cpu().numpy().tobytes() == a[k].tobytes()
    A.m.close(); B.m.close()


# ---- 4. the chain on a default handle ------------------------------------------------------------------------------------
def test_chain_on_a_default_handle(pfc):
    import helpers as H
    torch = _torch()
    n_dir = 6
    P = C1(pfc, n_dir, 0)
    n = P.n
    items, seeds, ra = _outputs(n), _seed_outputs(n, n_dir), _results(n, n_dir)
    _eval_dual_bodies(P, 0, items, seeds, ra)
    torch.cuda.synchronize()
    wa, sa, ca = ra[0].cpu().numpy(), ra[1].cpu().numpy(), ra[4].cpu().numpy()
    got_seeds = [o.rows().copy() for o in seeds]
    vb = [_z(n, 6), _z(n, 6), _z(n, 4, dt=torch.int32)]
    items_b = _outputs(n)
    _checked(P.m, lambda: P.m.eval_bodies_device(n, 0, 0, 1, N_BODY, P.d_x.data_ptr(), P.d_tw.data_ptr(), P.d_s.data_ptr(),
                                                 *[o.ptr for o in items_b], *[t.data_ptr() for t in vb]))
    torch.cuda.synchronize()
    wb, sb, cb = (t.cpu().numpy() for t in vb)
    assert cb[:, 3].any() and np.array_equal(ca, cb)
    ew = max(H.rel_err(wa[k], wb[k]) for k in range(n) if np.linalg.norm(wb[k]) > 0)
    es = max([H.rel_err(sa[k], sb[k]) for k in range(n) if np.linalg.norm(sb[k]) > 0] or [0.0])
    print(f"eval_dual_bodies_device against eval_bodies_device, largest per-item relative difference: wrench {ew:.2e}, sdot {es:.2e}")
    assert ew < 1e-9 and es < 1e-9
    dx, dtw, _ = (_dev(q) for q in P.chunks[0])
    seeds1 = _seed_outputs(n, n_dir)
    _sync()
    P.m.dual_seeds_from_bodies_device(*P.head(), dx.data_ptr(), dtw.data_ptr(), *[o.ptr for o in seeds1])
    torch.cuda.synchronize()
    for g, o1 in zip(got_seeds, seeds1):
        assert g.tobytes() == o1.rows().tobytes()
    for o, ob in zip(items, items_b):
        assert o.rows().tobytes() == ob.rows().tobytes()
    P.m.close()


# ---- 5. the consumers accept the layouts ---------------------------------------------------------------------------------
def test_consumers_accept_the_layouts(pfc):
    torch = _torch()
    n_dir, nv = 6, 12
    P = C1(pfc, n_dir, 1)
    n = P.n
    items, seeds, ra = _outputs(n), _seed_outputs(n, n_dir), _results(n, n_dir)
    _eval_dual_bodies(P, 0, items, seeds, ra)
    rng = np.random.default_rng(9)
    jac, djac = rng.standard_normal((N_BODY, nv, 6)), rng.standard_normal((N_BODY, n_dir, nv, 6)) * 1e-2
    d_jac, d_djac, d_f, d_df = _dev(jac), _dev(djac), _z(1, nv), _z(1, n_dir, nv)
    d_L = _z(n, 12, 36)
    _sync()
    P.m.scatter_generalized_dual_device(n, n_dir, ra[0].data_ptr(), ra[2].data_ptr(), items[2].ptr, seeds[2].ptr, items[3].ptr,
                                        items[4].ptr, 0, 1, nv, d_jac.data_ptr(), d_djac.data_ptr(), d_f.data_ptr(), d_df.data_ptr())
    # the local Jacobian at the kept point, applied to kernel seeds and to statement seeds
    P.m.local_jacobian_device(d_L.data_ptr())
    assert P.m.check() == 0
    torch.cuda.synchronize()
    sd = P.seeds(0)
    _, _, x_r, b1_r, b2_r = P.items
    f_ref, df_ref = P.m.scatter_generalized_dual(ra[0].cpu().numpy(), ra[2].cpu().numpy(), x_r, sd[2], b1_r, b2_r, jac, djac)
    assert np.abs(f_ref).max() > 0 and np.abs(df_ref).max() > 0
    assert np.array_equal(d_f.cpu().numpy(), f_ref) and np.array_equal(d_df.cpu().numpy(), df_ref)
    dp, dt, ds = _dev(sd[0]), _dev(sd[1]), _dev(P.chunks[0][2])
    ka, kb = [_z(n, n_dir, 6), _z(n, n_dir, 6)], [_z(n, n_dir, 6), _z(n, n_dir, 6)]
    _sync()
    P.m.apply_local_jacobian_device(n, n_dir, d_L.data_ptr(), seeds[0].ptr, seeds[1].ptr, ds.data_ptr(), ka[0].data_ptr(), ka[1].data_ptr())
    P.m.apply_local_jacobian_device(n, n_dir, d_L.data_ptr(), dp.data_ptr(), dt.data_ptr(), ds.data_ptr(), kb[0].data_ptr(), kb[1].data_ptr())
    torch.cuda.synchronize()
    assert np.abs(kb[0].cpu().numpy()).max() > 0
    for u, v in zip(ka, kb):
        assert np.array_equal(u.cpu().numpy(), v.cpu().numpy())
    P.m.close()


# ---- 6. errors -----------------------------------------------------------------------------------------------------------
def test_errors(pfc):
    torch = _torch()
    L = pfc._lib
    lib = L.lib()
    n_dir = 4
    P = C1(pfc, n_dir, 0)
    n = P.n
    dx, dtw, ds = (_dev(q) for q in P.chunks[0])
    seeds = _seed_outputs(n, n_dir)
    dw, dsd = _z(n, n_dir, 6), _z(n, n_dir, 6)
    st = torch.cuda.current_stream().cuda_stream
    _sync()

    def seeds_call(m_h, n_items=n, nd=n_dir, n_body=N_BODY):
        return lib.pfc_dual_seeds_from_bodies_device(m_h, n_items, nd, None, None, 1, n_body, P.d_x.data_ptr(), P.d_tw.data_ptr(),
                                                     dx.data_ptr(), dtw.data_ptr(), *[o.ptr for o in seeds], st)

    def more_call(n_items=n):
        return lib.pfc_eval_dual_bodies_device_more(P.m._h, n_items, n_dir, None, None, 1, N_BODY, P.d_x.data_ptr(), P.d_tw.data_ptr(),
                                                    dx.data_ptr(), dtw.data_ptr(), ds.data_ptr(), *[o.ptr for o in seeds],
                                                    dw.data_ptr(), dsd.data_ptr(), st)

    # before pfc_finalize
    h = C.c_void_p()
    assert lib.pfc_create(0, C.byref(h)) == 0
    assert seeds_call(h) == L.ERR_STATE
    lib.pfc_destroy(h)
    # n_dir out of range, a body >= n_body (instruction 3 names body 4)
    assert seeds_call(P.m._h, nd=0) == L.ERR_BAD_ARG and seeds_call(P.m._h, nd=17) == L.ERR_BAD_ARG
    assert seeds_call(P.m._h, n_body=4) == L.ERR_BAD_ARG
    hx = np.ascontiguousarray(P.x[:, :4]); htw = np.ascontiguousarray(P.tw[:, :4])
    with pytest.raises(L.PFCError) as e:
        P.m.dual_seeds_from_bodies(hx, htw, P.chunks[0][0][:, :4], P.chunks[0][1][:, :4])
    assert e.value.status == L.ERR_BAD_ARG
    with pytest.raises(L.PFCError) as e:      # the host form checks every id
        P.m.dual_seeds_from_bodies(P.x, P.tw, *P.chunks[0][:2], ins_ids=[0, 1, 4, 2])
    assert e.value.status == L.ERR_BAD_ARG
    with pytest.raises(L.PFCError) as e:
        P.m.dual_seeds_from_bodies(P.x, P.tw, *P.chunks[0][:2], ins_ids=[0, 1, 2, 3], scene=[0, 0, 1, 0])
    assert e.value.status == L.ERR_BAD_ARG
    # _more without a kept evaluation, then with one of another size: nothing is written
    assert more_call() == L.ERR_STATE
    res = _results(n, n_dir)
    _eval_dual_parts(P, 0, res)
    assert more_call(n - 1) == L.ERR_BAD_ARG
    torch.cuda.synchronize()
    assert all(o.untouched() for o in seeds)
    assert more_call() == 0 and P.m.check() == 0      # and the kept point is still there
    # n_items = 0 is a no-op
    seeds = _seed_outputs(n, n_dir)
    _sync()
    assert seeds_call(P.m._h, n_items=0) == 0
    torch.cuda.synchronize()
    assert all(o.untouched() for o in seeds)
    P.m.close()
    # an instruction without bodies
    w = pfc.configs.c1_boxes()
    m = pfc.configs.build_scenario(w)
    for k, (b1, b2) in enumerate(P.bind[:3]):
        m.set_instruction_bodies(k, b1, b2)
    with pytest.raises(L.PFCError) as e:
        m.dual_seeds_from_bodies_device(n, n_dir, 0, 0, 1, N_BODY, P.d_x.data_ptr(), P.d_tw.data_ptr(), dx.data_ptr(), dtw.data_ptr(),
                                        *[o.ptr for o in seeds], st)
    assert e.value.status == L.ERR_STATE and "instruction 3" in str(e.value)
    with pytest.raises(L.PFCError) as e:
        m.dual_seeds_from_bodies(P.x, P.tw, *P.chunks[0][:2])
    assert e.value.status == L.ERR_STATE and "instruction 3" in str(e.value)
    torch.cuda.synchronize()
    assert all(o.untouched() for o in seeds)
    m.close()


def test_multi_device_handle_gives_the_same_seeds(pfc):
    torch = _torch()
    n_dir = 5
    got = []
    for devices in (None, [0, 0]):
        P = C1(pfc, n_dir, 0, devices=devices)
        dx, dtw, _ = (_dev(q) for q in P.chunks[0])
        out = _seed_outputs(P.n, n_dir)
        _sync()
        P.m.dual_seeds_from_bodies_device(*P.head(), dx.data_ptr(), dtw.data_ptr(), *[o.ptr for o in out],
                                          torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got.append([o.rows().copy() for o in out])
        P.m.close()
    for a, b, r in zip(got[0], got[1], P.seeds(0)):
        assert a.tobytes() == b.tobytes() and np.array_equal(a, r.reshape(a.shape))
    assert np.abs(got[0][0]).max() > 0
