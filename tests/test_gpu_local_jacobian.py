"""Per-item contact Jacobians (pfc_local_jacobian[_device]) and their application to further Dual chunks
(pfc_apply_local_jacobian[_device]): L against the partials pfc_eval_dual_device_more returns for unit seeds (bytes, under
fixed_order), against the Dual oracle, and against central differences; apply against _more.

Tolerances are those of tests/test_gpu_dual.py: the oracle at 1e-6 (wrench) / 1e-5 (ṡ) of the item's largest partial; apply
against _more at 1e-9 / 1e-7 of the array's largest entry (test_dual_linear_in_seed).  Default handles form K per Dual pass from
atomically summed sums, so scenes with flat patches (C5, where decompose_K! clamps an eigenvalue) run on fixed_order handles.  On C5
the ṡ comparisons use 1e-6, the tolerance tests/test_gpu_scale.py uses for ṡ there: its ill-conditioned K̄^{-1/2} amplifies the
rounding that differs between one Dual pass over a seed and a sum of unit-seed columns."""
import ctypes as C

import numpy as np
import pytest

from helpers import oracle_ins, oracle_meshes
from test_oracle_dual import pose_of, tangents

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _dev(a, dt=None):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).to(torch.device("cuda", 0))


def _z(*shape, dt=None):
    torch = _torch()
    return torch.zeros(shape, dtype=dt or torch.float64, device=torch.device("cuda", 0))


def _with_state(w, seed):
    w.s[:] = np.random.default_rng(seed).standard_normal((w.n_items, 6)) * 1e-3
    return w


def _c5_bodies(w):
    ids = np.array([[w.instructions[int(k)].id_1, w.instructions[int(k)].id_2] for k in w.ins_ids])
    return ids[:, 0] // 2, ids[:, 1] // 2      # meshes b{i}_tri, b{i}_tet per body


SMALL = {
    "c3": lambda C5: C5.c3_blob_tool(4, seed=8, n_div_blob=6, n_div_tool=4),
    "vv_reg": lambda C5: C5.vol_vol(4, n_div=3, model="regularized"),
    "vv_br": lambda C5: C5.vol_vol(4, n_div=3, model="bristle"),
    "c1": lambda C5: C5.c1_boxes(),
    "c2": lambda C5: C5.c2_box_on_plane(48, montecarlo=True),
}


class Point:
    """A handle at a workload's point on the device: the first chunk of a Jacobian (eval_dual_device, re-issued until checked)."""

    def __init__(self, pfc, w, options=None, devices=None, seed=0):
        torch = _torch()
        self.m = pfc.configs.build_scenario(w, devices=devices)
        for name, value in (options or {}).items():
            self.m.set_option(name, value)
        self.w, self.n = w, w.n_items
        n = self.n
        self.st = torch.cuda.current_stream().cuda_stream
        rng = np.random.default_rng(seed)
        self.t = [_dev(w.ins_ids, torch.int32), _dev(w.pose), _dev(w.twist), _dev(w.s)]
        sd = [_dev(rng.standard_normal((n, 6, 24)) * 1e-2), _dev(rng.standard_normal((n, 6, 6)) * 0.1),
              _dev(rng.standard_normal((n, 6, 6)) * 1e-3)]
        self.o_w, self.o_sd, o_ct, o_dw, o_dsd = _z(n, 6), _z(n, 6), _z(n, 4, dt=torch.int32), _z(n, 6, 6), _z(n, 6, 6)
        for _ in range(40):      # the first evaluations of a handle size its lists (ERR_OVERFLOW: issue again)
            self.m.eval_dual_device(n, 6, self.t[0].data_ptr(), self.t[1].data_ptr(), self.t[2].data_ptr(), self.t[3].data_ptr(),
                                    sd[0].data_ptr(), sd[1].data_ptr(), sd[2].data_ptr(), self.o_w.data_ptr(), self.o_sd.data_ptr(),
                                    o_dw.data_ptr(), o_dsd.data_ptr(), o_ct.data_ptr(), self.st)
            rc = self.m.check()
            if rc == 0:
                break
        assert rc == 0
        self.counts = o_ct.cpu().numpy()

    def L(self):
        L = _z(self.n, 12, 36)
        self.m.local_jacobian_device(L.data_ptr(), self.st)
        assert self.m.check() == 0
        return L

    def more(self, dp, dt, ds):
        nd = dp.shape[1]
        dw, dsd = _z(self.n, nd, 6), _z(self.n, nd, 6)
        self.m.eval_dual_device_more(nd, dp.data_ptr(), dt.data_ptr(), ds.data_ptr() if ds is not None else 0, dw.data_ptr(),
                                     dsd.data_ptr(), self.st)
        assert self.m.check() == 0
        return dw, dsd

    def apply(self, L, dp, dt, ds, stream=None):
        nd = dp.shape[1]
        dw, dsd = _z(self.n, nd, 6), _z(self.n, nd, 6)
        self.m.apply_local_jacobian_device(self.n, nd, L.data_ptr(), dp.data_ptr(), dt.data_ptr(), ds.data_ptr() if ds is not None else 0,
                                           dw.data_ptr(), dsd.data_ptr(), stream or self.st)
        _torch().cuda.synchronize()
        return dw, dsd

    def close(self):
        self.m.close()


def unit_seeds(n):
    """The three unit-seed chunks (16 + 16 + 4 directions) whose partials are L's columns."""
    out = []
    for p in range(3):
        cols = np.arange(16 * p, min(16 * p + 16, 36))
        E = np.zeros((cols.size, 36))
        E[np.arange(cols.size), cols] = 1.0
        S = np.ascontiguousarray(np.broadcast_to(E, (n, cols.size, 36)))
        out.append((cols, S[..., :24], S[..., 24:30], S[..., 30:]))
    return out


def L_from_more(P):
    L = np.zeros((P.n, 12, 36))
    for cols, a, b, c in unit_seeds(P.n):
        dw, dsd = P.more(_dev(a), _dev(b), _dev(c))
        L[:, :6, cols] = dw.cpu().numpy().transpose(0, 2, 1)
        L[:, 6:, cols] = dsd.cpu().numpy().transpose(0, 2, 1)
    return L


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("scene", ["c3", "vol_vol", "c5"])
def test_L_is_the_bytes_of_more_with_unit_seeds(pfc, scene):
    C5 = pfc.configs
    w = {"c3": lambda: C5.c3_blob_tool(4, seed=8, n_div_blob=6, n_div_tool=4), "vol_vol": lambda: C5.vol_vol(4, n_div=3, model="bristle"),
         "c5": lambda: C5.c5_pile(n_side=3)}[scene]()
    _with_state(w, 1)
    P = Point(pfc, w, options={"fixed_order": 1})
    L = P.L().cpu().numpy()
    Lm = L_from_more(P)      # (_more at the same point still works after the L build)
    assert np.abs(L).max() > 0
    assert _same(L, Lm)
    assert _same(P.L().cpu().numpy(), L)      # and L again after _more
    P.close()


@pytest.mark.parametrize("scene", ["bristle", "regularized", "tet_tet_regularized", "tet_tet_bristle"])
def test_L_against_the_dual_oracle(pfc, O, scene):
    C5 = pfc.configs
    w = {"bristle": lambda: C5.c3_blob_tool(5, seed=4, n_div_blob=5, n_div_tool=3),
         "regularized": lambda: C5.c2_box_on_plane(8, montecarlo=True),
         "tet_tet_regularized": lambda: C5.vol_vol(4, n_div=3, model="regularized"),
         "tet_tet_bristle": lambda: C5.vol_vol(4, n_div=3, model="bristle")}[scene]()
    _with_state(w, 2)
    m = pfc.configs.build_scenario(w)
    wr, sd, L, counts = m.local_jacobian(w.pose, w.twist, w.s, w.ins_ids)
    wr0, sd0, counts0 = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    m.close()
    np.testing.assert_allclose(wr, wr0, rtol=1e-11, atol=1e-11 * np.abs(wr0).max())
    np.testing.assert_allclose(sd, sd0, rtol=1e-7, atol=1e-7 * max(np.abs(sd0).max(), 1e-300))
    assert np.array_equal(counts, counts0)
    om = oracle_meshes(w)
    eye = np.eye(36)
    n_contact = 0
    for k in range(w.n_items):
        c = w.instructions[int(w.ins_ids[k])]
        st, _, _, rdw, rdsd = O.evaluate_dual(om[c.id_1], om[c.id_2], oracle_ins(pfc, c), w.pose[k], w.twist[k], w.s[k],
                                              eye[:, :24], eye[:, 24:30], eye[:, 30:])
        assert st == 0
        n_contact += counts[k, 3] > 0
        sw = max(np.abs(rdw).max(), 1e-300)
        assert np.abs(L[k, :6].T - rdw).max() <= 1e-6 * sw, (k, np.abs(L[k, :6].T - rdw).max() / sw)
        ss = max(np.abs(rdsd).max(), 1e-300)
        assert np.abs(L[k, 6:].T - rdsd).max() <= 1e-5 * ss, (k, np.abs(L[k, 6:].T - rdsd).max() / ss)
    assert n_contact > 0


def _seed_sets(pfc, w, rng, P):
    """(name, d_pose, d_twist, d_s) chunks: dense random (n_dir 1, 6, 16), consistent tangents, one body's items only."""
    n = w.n_items
    out = []
    for nd in (1, 6, 16):
        dp = rng.standard_normal((n, nd, 24)) * 1e-2
        dt = rng.standard_normal((n, nd, 6)) * 0.1
        ds = rng.standard_normal((n, nd, 6)) * 1e-3
        if nd > 1:
            dp[:, 1] = 0; dt[:, 1] = 0; ds[:, 1] = 0      # one zero key per item
        out.append((f"dense{nd}", dp, dt, ds))
    dq = rng.standard_normal((n, 6, 6)) * np.array([1, 1, 1, 0.05, 0.05, 0.05])
    dp = np.stack([tangents(w.pose[k][:9].reshape(3, 3, order="F"), w.pose[k][9:12], dq[k]) for k in range(n)])
    out.append(("tangents", dp, rng.standard_normal((n, 6, 6)) * 0.1, None))
    if w.name.startswith("C5"):
        b1, b2 = _c5_bodies(w)
        sel = (b1 == 4) | (b2 == 4)
    else:
        sel = np.arange(n) % 3 == 0
    dp = rng.standard_normal((n, 6, 24)) * 1e-2 * sel[:, None, None]
    dt = rng.standard_normal((n, 6, 6)) * 0.1 * sel[:, None, None]
    ds = rng.standard_normal((n, 6, 6)) * 1e-3 * sel[:, None, None]
    assert 0 < sel.sum() < n
    out.append(("one_body", dp, dt, ds))
    return out


def _check_apply_against_more(pfc, w, options, seed, sd_tol=1e-7):
    _with_state(w, seed)
    P = Point(pfc, w, options=options, seed=seed)
    L = P.L()
    rng = np.random.default_rng(seed)
    for name, dp, dt, ds in _seed_sets(pfc, w, rng, P):
        t = [_dev(dp), _dev(dt), None if ds is None else _dev(ds)]
        mw, msd = [a.cpu().numpy() for a in P.more(*t)]
        aw, asd = [a.cpu().numpy() for a in P.apply(L, *t)]
        sw = max(np.abs(mw).max(), 1e-300)
        assert np.abs(mw).max() > 0 or not name.startswith("dense"), name
        assert np.abs(aw - mw).max() <= 1e-9 * sw, (name, np.abs(aw - mw).max() / sw)
        assert np.abs(asd - msd).max() <= sd_tol * max(np.abs(msd).max(), 1e-300), (name, np.abs(asd - msd).max() / np.abs(msd).max())
        zero = ~((dp != 0).any(axis=2) | (dt != 0).any(axis=2) | ((ds != 0).any(axis=2) if ds is not None else False))
        if zero.any():
            for a in (aw, asd, mw, msd):
                assert (a[zero] == 0).all(), name
    P.close()


@pytest.mark.parametrize("scene", sorted(SMALL))
def test_apply_equals_more_default_handles(pfc, scene):
    _check_apply_against_more(pfc, SMALL[scene](pfc.configs), None, 3)


@pytest.mark.parametrize("scene", ["c5", "c1"])
def test_apply_equals_more_fixed_order(pfc, scene):
    w = pfc.configs.c5_pile(n_side=3) if scene == "c5" else pfc.configs.c1_boxes()
    _check_apply_against_more(pfc, w, {"fixed_order": 1}, 4, sd_tol=1e-6 if scene == "c5" else 1e-7)


def test_nan_seeds_propagate(pfc):
    w = _with_state(SMALL["c3"](pfc.configs), 5)
    P = Point(pfc, w)
    L = P.L()
    n = w.n_items
    dp, dt, ds = np.zeros((n, 2, 24)), np.zeros((n, 2, 6)), np.zeros((n, 2, 6))
    dt[0, 0, 2] = np.nan
    aw, asd = [a.cpu().numpy() for a in P.apply(L, _dev(dp), _dev(dt), _dev(ds))]
    assert np.isnan(aw[0, 0]).any() and (aw[:, 1] == 0).all() and (aw[1:] == 0).all() and (asd[1:] == 0).all()
    P.close()


def test_tangent_stiffness_against_central_differences(pfc):
    """local_jacobian_tangent on a smooth regularized item against central differences of pfc_eval along exp-map pose
    perturbations and twist perturbations (fd_check's tolerance, 2e-5)."""
    w = pfc.configs.c2_box_on_plane(4, montecarlo=True)
    m = pfc.configs.build_scenario(w)
    wr, _, L, counts = m.local_jacobian(w.pose, w.twist, w.s, w.ins_ids)
    Lt = pfc.scenario.local_jacobian_tangent(L, w.pose)
    h = 1e-6
    for k in range(w.n_items):
        assert counts[k, 3] > 0
        R0 = w.pose[k][:9].reshape(3, 3, order="F"); t0 = w.pose[k][9:12]
        poses, twists = [], []
        for j in range(12):
            for sg in (1, -1):
                e = np.zeros(12); e[j] = sg * h
                poses.append(pose_of(R0, t0, e[:6])); twists.append(w.twist[k] + e[6:])
        ids = np.full(24, w.ins_ids[k], dtype=np.int32)
        fw, _, _ = m.force_all_elastic_intersections(np.array(poses), np.array(twists), np.zeros((24, 6)), ids)
        for j in range(12):
            fd = (fw[2 * j] - fw[2 * j + 1]) / (2 * h)
            assert np.linalg.norm(Lt[k, :6, j] - fd) <= 2e-5 * np.linalg.norm(fd) + 1e-9 * np.linalg.norm(wr[k]), (k, j)
        assert np.abs(Lt[k, :6, :6]).max() > 0
    m.close()


@pytest.mark.parametrize("scene", ["bristle", "regularized"])
def test_items_without_contact(pfc, scene):
    w = (pfc.configs.c3_blob_tool(3, seed=3, n_div_blob=5, n_div_tool=4) if scene == "bristle"
         else pfc.configs.c2_box_on_plane(3, montecarlo=True))
    _with_state(w, 6)
    R0 = w.pose[0][:9].reshape(3, 3, order="F")
    w.pose[0] = pose_of(R0, w.pose[0][9:12] + 50.0, np.zeros(6))      # item 0 far away
    m = pfc.configs.build_scenario(w)
    _, _, L, counts = m.local_jacobian(w.pose, w.twist, w.s, w.ins_ids)
    m.close()
    assert counts[0, 1] == 0 and counts[1:, 3].max() > 0
    assert (L[0, :6] == 0).all() and (L[0, 6:, :30] == 0).all()
    c = w.instructions[int(w.ins_ids[0])]
    expect = -np.eye(6) / c.tau if scene == "bristle" else np.zeros((6, 6))
    np.testing.assert_allclose(L[0, 6:, 30:], expect, rtol=1e-14, atol=0)
    assert np.abs(L[1:, :6]).max() > 0


def test_apply_outlives_evaluations_options_and_streams(pfc):
    torch = _torch()
    w = _with_state(SMALL["c3"](pfc.configs), 7)
    n, nd = w.n_items, 6
    P = Point(pfc, w)
    L = P.L()
    rng = np.random.default_rng(7)
    t = [_dev(rng.standard_normal((n, nd, 24)) * 1e-2), _dev(rng.standard_normal((n, nd, 6)) * 0.1),
         _dev(rng.standard_normal((n, nd, 6)) * 1e-3)]
    mw, _ = P.more(*t)
    a0 = [a.cpu().numpy() for a in P.apply(L, *t)]
    # the scatter of apply's partials against the scatter of _more's, as a chunk of the Jacobian would run them
    x = np.zeros((n, 12))
    for k in range(n):
        x[k, :9] = pfc.configs.random_rotation(rng).reshape(-1, order="F"); x[k, 9:] = rng.standard_normal(3)
    nv = 12
    jac = rng.standard_normal((2 * n, nv, 6))
    t_x, t_j = _dev(x), _dev(jac)
    t_b1, t_b2 = _dev(np.arange(n), torch.int32), _dev(np.arange(n) + n, torch.int32)
    dws = _dev(a0[0])
    outs = []
    for dw in (mw, dws):
        f, df = _z(1, nv), _z(1, nd, nv)
        P.m.scatter_generalized_dual_device(n, nd, P.o_w.data_ptr(), dw.data_ptr(), t_x.data_ptr(), 0, t_b1.data_ptr(), t_b2.data_ptr(),
                                            0, 1, nv, t_j.data_ptr(), 0, f.data_ptr(), df.data_ptr(), False, P.st)
        torch.cuda.synchronize()
        outs.append(df.cpu().numpy())
    assert np.abs(outs[0]).max() > 0
    assert np.abs(outs[1] - outs[0]).max() <= 1e-9 * np.abs(outs[0]).max()
    # L is caller data: another evaluation, an option change and another stream leave apply's bytes alone
    P.m.force_all_elastic_intersections(w.pose[:2], w.twist[:2], w.s[:2], w.ins_ids[:2])
    assert all(_same(a, b) for a, b in zip(a0, [a.cpu().numpy() for a in P.apply(L, *t)]))
    P.m.set_option("fixed_order", 1)
    assert all(_same(a, b) for a, b in zip(a0, [a.cpu().numpy() for a in P.apply(L, *t)]))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(a0, [a.cpu().numpy() for a in P.apply(L, *t, stream=s.cuda_stream)]))
    # and the host forms give the same bytes
    hw, hsd = P.m.apply_local_jacobian(L.cpu().numpy(), *[a.cpu().numpy() for a in t])
    assert _same(hw, a0[0]) and _same(hsd, a0[1])
    P.close()


def test_bad_arguments(pfc):
    lib, E = pfc._lib.lib(), pfc._lib
    w = _with_state(SMALL["c3"](pfc.configs), 8)
    n = w.n_items
    L = _z(n + 1, 12, 36)
    seeds = [_z(n, 16, 24), _z(n, 16, 6), _z(n, 16, 6)]
    out = [_z(n, 16, 6), _z(n, 16, 6)]
    m = pfc.configs.build_scenario(w)
    assert lib.pfc_local_jacobian_device(m._h, L.data_ptr(), None) == E.ERR_STATE      # no Dual evaluation yet
    m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    assert lib.pfc_local_jacobian_device(m._h, L.data_ptr(), None) == E.ERR_STATE      # a value evaluation is no point to extend
    m.close()
    P = Point(pfc, w)
    h = P.m._h
    assert lib.pfc_local_jacobian_device(h, None, None) == E.ERR_BAD_ARG
    ap = lambda n_items=n, nd=4, dL=L.data_ptr(), dp=seeds[0].data_ptr(), dt=seeds[1].data_ptr(), dw=out[0].data_ptr(), dsd=out[1].data_ptr(): \
        lib.pfc_apply_local_jacobian_device(h, n_items, nd, dL, dp, dt, None, dw, dsd, None)
    for kw in (dict(nd=0), dict(nd=17), dict(n_items=-1), dict(dL=None), dict(dp=None), dict(dt=None), dict(dw=None), dict(dsd=None),
               dict(dL=L.data_ptr() + 8)):
        assert ap(**kw) == E.ERR_BAD_ARG, kw
    assert ap(n_items=0) == E.OK
    P_ = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))
    Lh, wr, sd = np.zeros((n, 12, 36)), np.zeros((n, 6)), np.zeros((n, 6))
    ids = np.ascontiguousarray(w.ins_ids, dtype=np.int32)
    assert lib.pfc_local_jacobian(h, n, P_(ids, C.c_int), P_(w.pose), P_(w.twist), P_(w.s), P_(wr), P_(sd), None, None) == E.ERR_BAD_ARG
    assert lib.pfc_local_jacobian(h, n, P_(ids, C.c_int), P_(w.pose), P_(w.twist), None, P_(wr), P_(sd), P_(Lh), None) == E.ERR_BAD_ARG
    assert lib.pfc_local_jacobian(h, -1, None, None, None, None, None, None, None, None) == E.ERR_BAD_ARG
    assert lib.pfc_apply_local_jacobian(h, n, 17, P_(Lh), P_(np.zeros((n, 17, 24))), P_(np.zeros((n, 17, 6))), None,
                                        P_(np.zeros((n, 17, 6))), P_(np.zeros((n, 17, 6)))) == E.ERR_BAD_ARG
    with pytest.raises(ValueError):
        P.m.apply_local_jacobian(Lh, np.zeros((n, 2, 24)), np.zeros((n, 3, 6)))
    with pytest.raises(ValueError):
        P.m.local_jacobian(w.pose, w.twist[:2], w.s, w.ins_ids)
    # the handle is still usable
    _, _, L2, _ = P.m.local_jacobian(w.pose, w.twist, w.s, w.ins_ids)
    assert np.abs(L2).max() > 0
    P.close()


@pytest.mark.parametrize("fixed", [0, 1])
def test_multi_device_handle_gives_the_single_handle_L(pfc, fixed):
    """A {0, 0} handle: L within the apply tolerances of the single handle's (the shards' sums are grouped differently: C5's ṡ
    rows at 1e-6, as above); under fixed_order the same bytes on two fresh multi handles and the bytes of the multi handle's _more
    with unit seeds, the guarantees option fixed_order gives multi-device evaluations (tests/test_gpu_fixed_order.py)."""
    C5 = pfc.configs
    w = C5.c5_pile(n_side=3) if fixed else C5.c3_blob_tool(16, seed=9, n_div_blob=6, n_div_tool=4)
    _with_state(w, 9)
    opts = {"fixed_order": 1} if fixed else None
    sd_tol = 1e-6 if fixed else 1e-7
    P1 = Point(pfc, w, options=opts)
    a = P1.L().cpu().numpy()
    P2 = Point(pfc, w, options=opts, devices=[0, 0])
    L2 = P2.L()
    b = L2.cpu().numpy()
    assert P2.m.last_shards() == 2
    assert np.abs(a).max() > 0

    def near(x):
        return (np.abs(x[:, :6] - a[:, :6]).max() <= 1e-9 * np.abs(a[:, :6]).max() and
                np.abs(x[:, 6:] - a[:, 6:]).max() <= sd_tol * np.abs(a[:, 6:]).max())

    assert near(b)
    if fixed:
        P3 = Point(pfc, w, options=opts, devices=[0, 0])
        assert _same(P3.L().cpu().numpy(), b)
        P3.close()
        assert _same(L_from_more(P2), b)
    # _more still extends the multi handle's point, and apply on it (first device) agrees with it
    rng = np.random.default_rng(9)
    t = [_dev(rng.standard_normal((w.n_items, 6, 24)) * 1e-2), _dev(rng.standard_normal((w.n_items, 6, 6)) * 0.1), None]
    mw, _ = P2.more(*t)
    aw, _ = P2.apply(L2, *t)
    mw, aw = mw.cpu().numpy(), aw.cpu().numpy()
    assert np.abs(aw - mw).max() <= 1e-9 * np.abs(mw).max()
    # the host one-shot on the multi handle
    _, _, Lh, _ = P2.m.local_jacobian(w.pose, w.twist, w.s, w.ins_ids)
    assert near(Lh)
    P1.close()
    P2.close()
