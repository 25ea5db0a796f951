"""pfc_scatter_generalized_dual[_device]: addGeneralizedForcesThirdLaw! on Dual numbers (non_friction.jl:267-286 in a Jacobian
chunk), summed in the reference's item order.  Values against the oracle's pfo_scatter_generalized bit for bit, partials against a
Dual restatement of its statements bit for bit and against central differences of the value scatter."""
import numpy as np
import pytest

from helpers import oracle_ins, oracle_meshes
from test_oracle_dual import tangents

pytestmark = pytest.mark.gpu


class D:
    """ForwardDiff.Dual over the directions: v the value, d the partials (broadcast against v); d(a b) = da b + a db."""
    __slots__ = ("v", "d")

    def __init__(self, v, d):
        self.v, self.d = v, d

    def __add__(self, o):
        return D(self.v + o.v, self.d + o.d)

    def __sub__(self, o):
        return D(self.v - o.v, self.d - o.d)

    def __mul__(self, o):
        return D(self.v * o.v, self.d * o.v + self.v * o.d)


def _world(w, x):
    """pfo_scatter_generalized's transform(wrench, x_rw_r2), on D: [R ang + t x lin; R lin]."""
    lx = (x[0] * w[3] + x[3] * w[4]) + x[6] * w[5]
    ly = (x[1] * w[3] + x[4] * w[4]) + x[7] * w[5]
    lz = (x[2] * w[3] + x[5] * w[4]) + x[8] * w[5]
    return [((x[0] * w[0] + x[3] * w[1]) + x[6] * w[2]) + (x[10] * lz - x[11] * ly),
            ((x[1] * w[0] + x[4] * w[1]) + x[7] * w[2]) + (x[11] * lx - x[9] * lz),
            ((x[2] * w[0] + x[5] * w[1]) + x[8] * w[2]) + (x[9] * ly - x[10] * lx), lx, ly, lz]


def restate(wrench, d_wrench, x_w_r2, d_x_w_r2, body_1, body_2, jac, d_jac, scene=None, n_scene=1, f0=None, df0=None):
    """The Dual scatter written out: items in order, +tau(body 2) then -tau(body 1), vectorised over (direction, coordinate)."""
    n, nd = d_wrench.shape[0], d_wrench.shape[1]
    n_body, nv = jac.shape[0], jac.shape[1]
    dx = np.zeros((n, nd, 12)) if d_x_w_r2 is None else d_x_w_r2
    dj = np.zeros((n_body, nd, nv, 6)) if d_jac is None else d_jac
    f = np.zeros((n_scene, nv)) if f0 is None else f0.copy()
    df = np.zeros((n_scene, nd, nv)) if df0 is None else df0.copy()
    for i in range(n):
        w = [D(wrench[i, e], d_wrench[i, :, e][:, None]) for e in range(6)]
        x = [D(x_w_r2[i, e], dx[i, :, e][:, None]) for e in range(12)]
        o = _world(w, x)
        s = 0 if scene is None else int(scene[i])
        for b, sign in ((int(body_2[i]), 1), (int(body_1[i]), -1)):
            if b < 0:
                continue
            J = [D(jac[b, :, e], dj[b, :, :, e]) for e in range(6)]
            tau = ((J[0] * o[0] + J[1] * o[1]) + J[2] * o[2]) + ((J[3] * o[3] + J[4] * o[4]) + J[5] * o[5])
            if sign > 0:
                f[s] = f[s] + tau.v; df[s] = df[s] + tau.d
            else:
                f[s] = f[s] - tau.v; df[s] = df[s] - tau.d
    return f, df


def random_case(pfc, rng, n=64, n_scene=8, n_body=5, nv=18, nd=6, shuffle=True):
    x = np.zeros((n, 12))
    for k in range(n):
        x[k, :9] = pfc.configs.random_rotation(rng).reshape(-1, order="F"); x[k, 9:] = rng.standard_normal(3)
    scene = rng.integers(0, n_scene, size=n).astype(np.int32) if shuffle else (np.arange(n) * n_scene // max(n, 1)).astype(np.int32)
    return dict(wrench=rng.standard_normal((n, 6)), d_wrench=rng.standard_normal((n, nd, 6)), x_w_r2=x,
                d_x_w_r2=rng.standard_normal((n, nd, 12)), body_1=rng.integers(-1, n_body, size=n).astype(np.int32),
                body_2=rng.integers(-1, n_body, size=n).astype(np.int32), jac=rng.standard_normal((n_body, nv, 6)),
                d_jac=rng.standard_normal((n_body, nd, nv, 6)), scene=scene, n_scene=n_scene)


@pytest.fixture(scope="module")
def m(pfc):
    s = pfc.configs.build_scenario(pfc.configs.c1_boxes())
    yield s
    s.close()


def _dev(a, dt=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).to(torch.device("cuda", 0))


def _device_call(m, c, f0=None, df0=None, accumulate=False, stream=0, with_f=True):
    """The device form on copies of case c; returns (f, d_f) after a synchronisation."""
    import torch
    n, nd = c["d_wrench"].shape[0], c["d_wrench"].shape[1]
    nv = c["jac"].shape[1]
    t = {k: _dev(c[k]) for k in ("wrench", "d_wrench", "x_w_r2", "jac")}
    for k in ("d_x_w_r2", "d_jac"):
        t[k] = None if c[k] is None else _dev(c[k])
    for k in ("body_1", "body_2"):
        t[k] = _dev(c[k], torch.int32)
    t_sc = None if c["scene"] is None else _dev(c["scene"], torch.int32)
    f = _dev(np.zeros((c["n_scene"], nv)) if f0 is None else f0)
    df = _dev(np.zeros((c["n_scene"], nd, nv)) if df0 is None else df0)
    p = lambda x: 0 if x is None else x.data_ptr()
    torch.cuda.synchronize()      # (the copies and fills above are ordered on the current stream, the call may use another)
    m.scatter_generalized_dual_device(n, nd, p(t["wrench"]), p(t["d_wrench"]), p(t["x_w_r2"]), p(t["d_x_w_r2"]), p(t["body_1"]),
                                      p(t["body_2"]), p(t_sc), c["n_scene"], nv, p(t["jac"]), p(t["d_jac"]),
                                      f.data_ptr() if with_f else 0, df.data_ptr(), accumulate, stream)
    torch.cuda.synchronize()
    return f.cpu().numpy(), df.cpu().numpy()


def _host(m, c):
    return m.scatter_generalized_dual(c["wrench"], c["d_wrench"], c["x_w_r2"], c["d_x_w_r2"], c["body_1"], c["body_2"], c["jac"],
                                      c["d_jac"], c["scene"], c["n_scene"])


def _oracle_f(O, c):
    return O.scatter_generalized(c["wrench"], c["x_w_r2"], c["body_1"], c["body_2"], c["jac"], c["scene"], c["n_scene"])


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_values_are_the_oracles_bits(pfc, O, m):
    """f against pfo_scatter_generalized bit for bit: shuffled, non-contiguous scene ids; bodies -1; both bodies movable; no items."""
    rng = np.random.default_rng(1)
    c = random_case(pfc, rng, n_scene=8)
    c["n_scene"] = 11                                   # scene ids interleaved over the items; scenes 8 .. 10 have none
    c["body_1"][::3] = -1; c["body_2"][1::5] = -1
    cases = [c]
    b = dict(c); b["body_1"] = rng.integers(0, 5, size=64).astype(np.int32); b["body_2"] = rng.integers(0, 5, size=64).astype(np.int32)
    cases.append(b)
    e = random_case(pfc, rng, n=0, nd=3)
    cases.append(e)
    for k, cc in enumerate(cases):
        f, df = _host(m, cc)
        ref = _oracle_f(O, cc)
        assert np.array_equal(f, ref), k
        rf, rdf = restate(**{key: cc[key] for key in cc})
        assert np.array_equal(rf, ref) and np.array_equal(df, rdf), k
        fd, dfd = _device_call(m, cc)
        assert np.array_equal(fd, ref) and np.array_equal(dfd, rdf), k
    assert not _host(m, e)[0].any() and _host(m, e)[1].shape == (e["n_scene"], 3, 18)
    # accumulate onto non-zero content: that content is the first term of every sum
    f0 = rng.standard_normal((c["n_scene"], 18)); df0 = rng.standard_normal((c["n_scene"], 6, 18))
    fd, dfd = _device_call(m, c, f0, df0, accumulate=True)
    rf, rdf = restate(**c, f0=f0, df0=df0)
    assert np.array_equal(fd, rf) and np.array_equal(dfd, rdf)
    # d_f only (f NULL): the same partials
    _, dfn = _device_call(m, c, with_f=False)
    assert np.array_equal(dfn, restate(**c)[1])


@pytest.mark.parametrize("nd", [1, 6, 16])
def test_partials_are_the_restatements_bits(pfc, m, nd):
    c = random_case(pfc, np.random.default_rng(100 + nd), nd=nd)
    f, df = _host(m, c)
    rf, rdf = restate(**c)
    assert np.array_equal(f, rf) and np.array_equal(df, rdf)


def test_partials_against_central_differences(pfc, O, m):
    """The map is a polynomial of degree 4 in (w, X, J): its central difference along (dw, dX, dJ) has an O(h^2) error."""
    c = random_case(pfc, np.random.default_rng(7), nd=3)
    _, df = _host(m, c)
    h = 1e-5
    for k in range(3):
        def at(sg):
            return O.scatter_generalized(c["wrench"] + sg * h * c["d_wrench"][:, k], c["x_w_r2"] + sg * h * c["d_x_w_r2"][:, k],
                                         c["body_1"], c["body_2"], c["jac"] + sg * h * c["d_jac"][:, k], c["scene"], c["n_scene"])
        fd = (at(1.0) - at(-1.0)) / (2 * h)
        scale = np.abs(df[:, k]).max()
        assert np.abs(df[:, k] - fd).max() <= 1e-8 * scale, (k, np.abs(df[:, k] - fd).max() / scale)


def test_null_partials_are_zero_arrays(pfc, m):
    c = random_case(pfc, np.random.default_rng(8))
    for drop in (("d_x_w_r2",), ("d_jac",), ("d_x_w_r2", "d_jac")):
        a, z = dict(c), dict(c)
        for k in drop:
            a[k] = None; z[k] = np.zeros_like(c[k])
        fa, dfa = _host(m, a)
        fz, dfz = _host(m, z)
        assert _same(fa, fz) and _same(dfa, dfz), drop
        ga, dga = _device_call(m, a)
        assert _same(ga, fz) and _same(dga, dfz), drop
        assert _same(dfa, restate(**a)[1]), drop


def test_same_bytes_across_calls_handles_forms_and_devices(pfc, m):
    c = random_case(pfc, np.random.default_rng(9), n=256, n_scene=5, n_body=7, nv=40)
    f, df = _host(m, c)
    outs = [_host(m, c), _device_call(m, c)]
    import torch
    s = torch.cuda.Stream()
    outs.append(_device_call(m, c, stream=s.cuda_stream))
    for devices in (None, [0, 0]):
        h = pfc.configs.build_scenario(pfc.configs.c1_boxes(), devices=devices)
        outs += [_host(h, c), _device_call(h, c)]
        h.close()
    for k, (g, dg) in enumerate(outs):
        assert _same(g, f) and _same(dg, df), k


def test_device_chain_of_a_jacobian(pfc):
    """pfc_eval_dual_device -> scatter -> pfc_eval_dual_device_more -> scatter (accumulate) on one stream; each device scatter
    against the host scatter of the wrenches that evaluation left in HBM."""
    import torch
    w = pfc.configs.c2_box_on_plane(256, montecarlo=True)
    n, nv = w.n_items, 6
    rng = np.random.default_rng(31)
    m = pfc.configs.build_scenario(w)
    x = np.zeros((n, 12))
    for k in range(n):
        x[k, :9] = pfc.configs.random_rotation(rng).reshape(-1, order="F"); x[k, 9:] = rng.standard_normal(3)
    jac = rng.standard_normal((n, nv, 6))
    body_1 = np.full(n, -1, dtype=np.int32); body_2 = np.arange(n, dtype=np.int32)
    scene = rng.permutation(n).astype(np.int32)
    t_ins, t_pose, t_tw, t_s = _dev(w.ins_ids, torch.int32), _dev(w.pose), _dev(w.twist), _dev(w.s)
    t_x, t_j, t_b1, t_b2, t_sc = _dev(x), _dev(jac), _dev(body_1, torch.int32), _dev(body_2, torch.int32), _dev(scene, torch.int32)
    st = torch.cuda.current_stream().cuda_stream
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=torch.device("cuda", 0))

    def seeds(nd):
        return [_dev(rng.standard_normal((n, nd, 24)) * 1e-2), _dev(rng.standard_normal((n, nd, 6)) * 0.1),
                _dev(rng.standard_normal((n, nd, 6)) * 1e-3)]

    o_w, o_sd, o_ct = z(n, 6), z(n, 6), z(n, 4, dt=torch.int32)
    s1 = seeds(6)
    o_dw, o_dsd = z(n, 6, 6), z(n, 6, 6)
    ev = lambda: m.eval_dual_device(n, 6, t_ins.data_ptr(), t_pose.data_ptr(), t_tw.data_ptr(), t_s.data_ptr(), s1[0].data_ptr(),
                                    s1[1].data_ptr(), s1[2].data_ptr(), o_w.data_ptr(), o_sd.data_ptr(), o_dw.data_ptr(),
                                    o_dsd.data_ptr(), o_ct.data_ptr(), st)
    for _ in range(40):      # the first evaluations of a handle size its lists (ERR_OVERFLOW: issue again)
        ev()
        if m.check() == 0:
            break
    f1, df1, f2, df2 = z(n, nv), z(n, 6, nv), z(n, nv), z(n, 4, nv)
    ev()
    m.scatter_generalized_dual_device(n, 6, o_w.data_ptr(), o_dw.data_ptr(), t_x.data_ptr(), 0, t_b1.data_ptr(), t_b2.data_ptr(),
                                      t_sc.data_ptr(), n, nv, t_j.data_ptr(), 0, f1.data_ptr(), df1.data_ptr(), False, st)
    assert m.check() == 0      # (eval_dual_device_more extends a checked evaluation)
    s2 = seeds(4)
    o_dw2, o_dsd2 = z(n, 4, 6), z(n, 4, 6)
    m.eval_dual_device_more(4, s2[0].data_ptr(), s2[1].data_ptr(), s2[2].data_ptr(), o_dw2.data_ptr(), o_dsd2.data_ptr(), st)
    m.scatter_generalized_dual_device(n, 4, o_w.data_ptr(), o_dw2.data_ptr(), t_x.data_ptr(), 0, t_b1.data_ptr(), t_b2.data_ptr(),
                                      t_sc.data_ptr(), n, nv, t_j.data_ptr(), 0, f2.data_ptr(), df2.data_ptr(), True, st)
    assert m.check() == 0
    torch.cuda.synchronize()
    wv = o_w.cpu().numpy()
    assert np.abs(wv).max() > 0
    for dw, f, df in ((o_dw, f1, df1), (o_dw2, f2, df2)):
        hf, hdf = m.scatter_generalized_dual(wv, dw.cpu().numpy(), x, None, body_1, body_2, jac, None, scene, n)
        assert _same(f.cpu().numpy(), hf) and _same(df.cpu().numpy(), hdf)
        assert np.abs(hdf).max() > 0
    m.close()


def _c5_bodies(w):
    ids = np.array([[w.instructions[int(k)].id_1, w.instructions[int(k)].id_2] for k in w.ins_ids])
    return (ids[:, 0] // 2).astype(np.int32), (ids[:, 1] // 2).astype(np.int32)      # meshes b{i}_tri, b{i}_tet per body


def test_reproducible_jacobian_end_to_end(pfc, O):
    """C5 with 27 bodies (351 items, nv 162), option fixed_order: pfc_eval_dual then the Dual scatter gives the same bytes on two
    handles, and agrees with the Dual oracle's wrenches through the restatement."""
    w = pfc.configs.c5_pile(n_side=3)
    n, nd = w.n_items, 6
    rng = np.random.default_rng(41)
    body_1, body_2 = _c5_bodies(w)
    n_body = int(max(body_1.max(), body_2.max())) + 1
    nv = 6 * n_body
    Rb = [pfc.configs.random_rotation(rng) for _ in range(n_body)]
    tb = rng.standard_normal((n_body, 3))
    x = np.array([np.concatenate([Rb[b].reshape(-1, order="F"), tb[b]]) for b in body_2])
    dx = rng.standard_normal((n, nd, 12)) * 1e-2
    jac = rng.standard_normal((n_body, nv, 6)); d_jac = rng.standard_normal((n_body, nd, nv, 6)) * 1e-2
    dq = rng.standard_normal((n, nd, 6)) * np.array([1, 1, 1, 0.05, 0.05, 0.05])
    d_twist = rng.standard_normal((n, nd, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1])
    d_s = rng.standard_normal((n, nd, 6)) * 1e-3
    d_pose = np.zeros((n, nd, 24))
    for k in range(n):
        d_pose[k] = tangents(w.pose[k][:9].reshape(3, 3, order="F"), w.pose[k][9:12], dq[k])
    outs = []
    for _ in range(2):
        m = pfc.configs.build_scenario(w)
        m.set_option("fixed_order", 1)
        wr, _, dw, _, _ = m.force_all_elastic_intersections_dual(w.pose, w.twist, w.s, d_pose, d_twist, d_s, w.ins_ids)
        outs.append(m.scatter_generalized_dual(wr, dw, x, dx, body_1, body_2, jac, d_jac))
        m.close()
    assert _same(outs[0][0], outs[1][0]) and _same(outs[0][1], outs[1][1])
    om = oracle_meshes(w)
    rw, rdw = np.zeros((n, 6)), np.zeros((n, nd, 6))
    for k in range(n):
        c = w.instructions[int(w.ins_ids[k])]
        st, rw[k], _, rdw[k], _ = O.evaluate_dual(om[c.id_1], om[c.id_2], oracle_ins(pfc, c), w.pose[k], w.twist[k], w.s[k],
                                                  d_pose[k], d_twist[k], d_s[k])
        assert st == 0
    rf, rdf = restate(rw, rdw, x, dx, body_1, body_2, jac, d_jac)
    f, df = outs[0]
    assert np.abs(rf).max() > 0
    assert np.abs(f - rf).max() <= 1e-9 * np.abs(rf).max()
    for k in range(nd):      # test_gpu_dual.py's tolerance on wrench partials
        assert np.abs(df[:, k] - rdf[:, k]).max() <= 1e-6 * np.abs(rdf[:, k]).max(), k


def test_full_size_c5(pfc, m):
    """C5 shape: 2 016 items of 64 free bodies, nv 384, Dual(6), with d_x_w_r2 and d_jac: the device form against the restatement."""
    w = pfc.configs.c5_pile(n_side=4)
    rng = np.random.default_rng(51)
    body_1, body_2 = _c5_bodies(w)
    c = random_case(pfc, rng, n=w.n_items, n_scene=1, n_body=64, nv=384, nd=6)
    c.update(body_1=body_1, body_2=body_2, scene=None)
    rf, rdf = restate(**c)
    f, df = _device_call(m, c)
    assert np.array_equal(f, rf) and np.array_equal(df, rdf)
    g, dg = _host(m, c)
    assert _same(g, f) and _same(dg, df)


def test_bad_arguments_leave_the_handle_usable(pfc, m):
    import ctypes as C
    L = pfc._lib.lib()
    c = random_case(pfc, np.random.default_rng(61), nd=4)
    n, nv, nb = 64, 18, 5
    P = lambda a, t=C.c_double: np.ascontiguousarray(a, dtype=np.float64 if t is C.c_double else np.int32).ctypes.data_as(C.POINTER(t))
    args = dict(wrench=P(c["wrench"]), d_wrench=P(c["d_wrench"]), x=P(c["x_w_r2"]), dx=P(c["d_x_w_r2"]), b1=P(c["body_1"], C.c_int),
                b2=P(c["body_2"], C.c_int), sc=P(c["scene"], C.c_int), jac=P(c["jac"]), djac=P(c["d_jac"]))
    f, df = np.zeros((8, nv)), np.zeros((8, 16, nv))
    fp, dfp = f.ctypes.data_as(C.POINTER(C.c_double)), df.ctypes.data_as(C.POINTER(C.c_double))

    def call(nd=4, n_scene=8, **kw):
        a = dict(args, **kw)
        return L.pfc_scatter_generalized_dual(m._h, n, nd, a["wrench"], a["d_wrench"], a["x"], a["dx"], a["b1"], a["b2"], a["sc"],
                                              n_scene, nb, nv, a["jac"], a["djac"], fp, kw.get("dfp", dfp))

    bad_b = c["body_2"].copy(); bad_b[9] = nb
    bad_s = c["scene"].copy(); bad_s[3] = 8
    neg_s = c["scene"].copy(); neg_s[5] = -1
    for kw in (dict(nd=0), dict(nd=17), dict(wrench=None), dict(d_wrench=None), dict(x=None), dict(b1=None), dict(jac=None),
               dict(dfp=None), dict(b2=P(bad_b, C.c_int)), dict(sc=P(bad_s, C.c_int)), dict(sc=P(neg_s, C.c_int)), dict(n_scene=0)):
        assert call(**kw) == pfc._lib.ERR_BAD_ARG, kw
    dev = L.pfc_scatter_generalized_dual_device
    assert dev(m._h, n, 0, None, None, None, None, None, None, None, 8, nv, None, None, None, None, 0, None) == pfc._lib.ERR_BAD_ARG
    assert dev(m._h, n, 17, None, None, None, None, None, None, None, 8, nv, None, None, None, None, 0, None) == pfc._lib.ERR_BAD_ARG
    assert dev(m._h, n, 4, None, None, None, None, None, None, None, 8, nv, None, None, None, None, 0, None) == pfc._lib.ERR_BAD_ARG
    assert dev(m._h, 1 << 16, 4, None, None, None, None, None, None, None, 1 << 15, nv, None, None, None, None, 0,
               None) == pfc._lib.ERR_BAD_ARG      # n_scene * n_items >= 2^31
    assert call() == pfc._lib.OK
    rf, rdf = restate(**c)
    assert np.array_equal(f, rf) and np.array_equal(df.reshape(-1)[:8 * 4 * nv].reshape(8, 4, nv), rdf)
