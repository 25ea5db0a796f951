"""pfc_contact_surface_fric on the device: the friction half of the contact surface (per-point T_c and branch, per-item friction
wrench, total wrench, ṡ, K / K̄^{-1/2} / S⁻¹ / Δ²) against the CPU oracle, a numpy restatement of traction(), an analytic case,
its reproducibility across options and handles, the capacity protocol, and that it leaves the handle's evaluations alone."""
import ctypes as C

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

SCENES = ["c1", "c2", "c3", "vv_reg", "vv_bristle", "c5", "spoon"]
TOL_TIGHT = 1e-9       # test_gpu_parity.py's tolerances
TOL_WRENCH = 1e-6


def _workload(pfc, name, seed=11):
    Cf = pfc.configs
    w = {"c1": lambda: Cf.c1_boxes(), "c2": lambda: Cf.c2_box_on_plane(3), "c3": lambda: Cf.c3_blob_tool(4, n_div_blob=8, n_div_tool=6),
         "vv_reg": lambda: Cf.vol_vol(6, n_div=5), "vv_bristle": lambda: Cf.vol_vol(6, n_div=5, model="bristle"),
         "c5": lambda: Cf.c5_pile(n_side=3), "spoon": lambda: Cf.spoon_pencil_pads(6)}[name]()
    # non-zero twists and bristle states throughout
    rng = np.random.default_rng(seed)
    n = w.n_items
    w.twist = np.ascontiguousarray(w.twist + np.concatenate([rng.uniform(-0.5, 0.5, (n, 3)), rng.uniform(-0.05, 0.05, (n, 3))], axis=1))
    w.s = np.ascontiguousarray(rng.standard_normal((n, 6)) * 1e-4)
    return w


def _model(w, k):
    return w.instructions[int(w.ins_ids[k])].model


def _ins_params(pfc, w, k):
    c = w.instructions[int(w.ins_ids[k])]
    mu_s, mu_d = pfc.scenario.determine_mu_s_mu_d(c.mu_s, c.mu_d)
    return c, mu_s, mu_d


def _arrays(F):
    S = F.surface
    return [S.poly_off, S.poly_idx, S.poly_xyz, S.poly_trac, S.trac, S.summary, S.counts, F.fric, F.fric_summary, F.stiff]


def _same_bytes(F1, F2):
    for a, b in zip(_arrays(F1), _arrays(F2)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_surface(S1, S2):
    for a, b in zip([S1.poly_off, S1.poly_idx, S1.poly_xyz, S1.poly_trac, S1.trac, S1.summary, S1.counts],
                    [S2.poly_off, S2.poly_idx, S2.poly_xyz, S2.poly_trac, S2.trac, S2.summary, S2.counts]):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _close(a, b, tol):
    if np.linalg.norm(b) == 0.0:
        return np.linalg.norm(a) == 0.0
    return H.rel_err(a, b) < tol


def _oracle_traction_fns(O):
    L = O.lib()
    dp = C.POINTER(C.c_double)
    reg = C.CFUNCTYPE(None, C.c_double, C.c_double, C.c_double, dp, C.c_double, dp)(("pfo_traction_regularized", L))
    bri = C.CFUNCTYPE(None, C.c_double, C.c_double, dp, C.c_double, dp)(("pfo_traction_bristle", L))
    return reg, bri, dp


def _branch_input(pfc, w, F, k):
    """Per point of item k: the vector traction() takes (vel_t or T̄s), p dA, the threshold of the first branch -- from the surface's
    own trac rows, the twist, the call's cop (summary) and Δ² (stiff)."""
    it = F.item(k)
    c, mu_s, mu_d = _ins_params(pfc, w, k)
    bristle = c.model == "bristle"
    v, pdA, thr = H.friction_branch_input(c, mu_s, it["trac"], w.twist[k], it["Delta"] if bristle else None,
                                          it["cop"] if bristle else None)
    return c, mu_s, mu_d, v, pdA, thr


def _check_points(pfc, O, w, F, k):
    reg, bri, dp = _oracle_traction_fns(O)
    it = F.item(k)
    c, mu_s, mu_d, v, pdA, thr = _branch_input(pfc, w, F, k)
    fr = it["fric"]
    out = np.zeros(3)
    for j in range(v.shape[0]):
        vj = np.ascontiguousarray(v[j])
        if c.model == "regularized":
            reg(mu_s, mu_d, c.v_tol, vj.ctypes.data_as(dp), float(pdA[j]), out.ctypes.data_as(dp))
        else:
            bri(mu_s, mu_d, vj.ctypes.data_as(dp), float(pdA[j]), out.ctypes.data_as(dp))
        assert np.all(np.abs(fr[j, 0:3] - out) <= 1e-12 * mu_s * pdA[j] + 1e-300), (k, j, fr[j], out)
    m2 = np.sum(v * v, axis=1)
    flag = np.where(m2 < thr * thr, 0.0, 1.0)
    near = np.abs(m2 - thr * thr) <= 1e-12 * thr * thr
    assert np.all((fr[:, 3] == flag) | near), k
    assert set(np.unique(fr[:, 3])) <= {0.0, 1.0}


def _check_consistency(F, k):
    it = F.item(k)
    T, fr = it["trac"], it["fric"]
    Tc = fr[:, 0:3]
    lin = Tc.sum(axis=0)
    ang = np.cross(T[:, 3:6], Tc).sum(axis=0)
    ref = np.concatenate([ang, lin])
    assert _close(it["fric_wrench"], ref, 1e-12), (k, it["fric_wrench"], ref)
    assert it["total_wrench"].tobytes() == (F.surface.summary[k, 0:6] + F.fric_summary[k, 6:12]).tobytes()
    first = fr[:, 3] == 0.0
    assert it["n_first"] == int(first.sum())
    pdA = T[:, 6] * T[:, 7]
    assert _close([it["first_p_dA"]], [pdA[first].sum()], 1e-12)


def _kis_tolerances(r, eK):
    """Tolerances of K̄^{-1/2} and Δ² against the oracle: test_gpu_parity's 1e-8 and TOL_TIGHT, or the first-order perturbation
    bound where K̄ = S⁻¹ K S⁻¹ is so ill-conditioned that the bound is larger: K is summed in another order than the oracle's
    (rel. difference eK, asserted < TOL_TIGHT by the caller), and a relative change
    e of K̄ moves the smallest eigenvalue by up to e cond(K̄) of itself, so λ_min^{-1/2} -- the largest entry of K̄^{-1/2} --
    by half that; the factor 8 covers the Jacobi rotations' own rounding (a few eps cond).  Some C5 contacts (a box edge on a
    face) reach cond ~ 1e10; for those ṡ is held to the north-star tolerance, as the library's own C5 evaluation is."""
    Kb = r.Sinv[:, None] * r.K * r.Sinv[None, :]
    lam = np.linalg.eigvalsh(0.5 * (Kb + Kb.T))
    cond = lam[-1] / max(lam[0], lam[-1] * 1e-16)
    bound = 8.0 * cond * (eK + 1e-16)
    return max(1e-8, bound), max(TOL_TIGHT, bound)


def _check_against_oracle(w, F, items, ref):
    for k, r in zip(items, ref):
        it = F.item(k)
        assert np.array_equal(F.surface.counts[k], r.counts)
        assert _close(it["total_wrench"], r.wrench, TOL_TIGHT), (k, it["total_wrench"], r.wrench)
        tol_sdot = TOL_TIGHT
        if _model(w, k) == "bristle" and r.has_K:
            eK = H.rel_err(it["K"], r.K)
            assert eK < TOL_TIGHT, k
            assert H.rel_err(it["Sinv"], r.Sinv) < TOL_TIGHT, k
            tol_kis, tol_delta = _kis_tolerances(r, eK)
            if tol_kis > 1e-8:
                tol_sdot = TOL_WRENCH      # as test_gpu_scale.py::test_c5_pile_all_pairs: ṡ carries the clamped direction's noise
            assert H.rel_err(it["Kbar_inv_sqrt"], r.Kbar_inv_sqrt) < tol_kis, (k, H.rel_err(it["Kbar_inv_sqrt"], r.Kbar_inv_sqrt), tol_kis)
            assert H.rel_err(it["Delta"], r.Delta) < tol_delta, (k, H.rel_err(it["Delta"], r.Delta), tol_delta)
        else:
            assert np.all(F.stiff[k] == 0.0), k
        assert _close(it["sdot"], r.sdot, tol_sdot), (k, it["sdot"], r.sdot, tol_sdot)
        if _model(w, k) == "regularized":
            assert np.all(it["sdot"] == 0.0), k


@pytest.mark.parametrize("name", SCENES)
def test_friction_surface_against_oracle_and_surface(pfc, O, name):
    w = _workload(pfc, name)
    m = pfc.configs.build_scenario(w)
    F = m.contact_surface_fric(w.pose, w.twist, w.s, w.ins_ids)
    assert F.surface.trac.shape[0] > 0
    # 1. the surface's outputs, byte for byte
    _same_surface(F.surface, m.contact_surface(w.pose, w.twist, w.ins_ids))
    # 2. the oracle
    ref = H.oracle_run(pfc, w)
    _check_against_oracle(w, F, range(w.n_items), ref)
    for k in range(w.n_items):
        _check_points(pfc, O, w, F, k)     # 3.
        _check_consistency(F, k)            # 4.
    # 6. two calls, and handles with other options, return the same bytes
    _same_bytes(F, m.contact_surface_fric(w.pose, w.twist, w.s, w.ins_ids))
    for opt in ({"fused": 0}, {"team": 0}, {"fixed_order": 1}, {"split_min": 1}, {"debug": 1}):
        m2 = pfc.configs.build_scenario(w)
        for key, v in opt.items():
            m2.set_option(key, v)
        m2.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
        _same_bytes(F, m2.contact_surface_fric(w.pose, w.twist, w.s, w.ins_ids))
        m2.close()
    m.close()


def test_regularized_sliding_box_is_analytic(pfc):
    """C2 box on the plane sliding at 5 cm/s (above v_μd = 3 v_c = 3 cm/s): every point takes the second branch and Σ T_c =
    -μd F_n v̂."""
    w = pfc.configs.c2_box_on_plane(3)
    v = np.array([0.03, -0.04, 0.0])
    w.twist = np.tile(np.concatenate([np.zeros(3), v]), (w.n_items, 1))
    m = pfc.configs.build_scenario(w)
    F = m.contact_surface_fric(w.pose, w.twist, None, w.ins_ids)
    _, mu_s, mu_d = _ins_params(pfc, w, 0)
    for k in range(w.n_items):
        it = F.item(k)
        assert it["trac"].shape[0] > 0
        assert np.all(it["fric"][:, 3] == 1.0) and it["n_first"] == 0 and it["first_p_dA"] == 0.0
        Fn = np.linalg.norm(it["wrench"][3:6])
        expect = -mu_d * Fn * v / np.linalg.norm(v)
        assert H.rel_err(it["fric_wrench"][3:6], expect) < 1e-12, (k, it["fric_wrench"], expect)
        assert np.all(it["sdot"] == 0.0)
    m.close()


def test_bristle_at_rest_has_no_friction(pfc):
    w = pfc.configs.c3_blob_tool(3, n_div_blob=8, n_div_tool=6)
    w.twist = np.zeros_like(w.twist)
    m = pfc.configs.build_scenario(w)
    F = m.contact_surface_fric(w.pose, w.twist, np.zeros((w.n_items, 6)), w.ins_ids)
    assert F.fric.shape[0] > 0
    assert np.all(F.fric[:, 0:3] == 0.0) and np.all(F.fric[:, 3] == 0.0)
    assert np.all(F.fric_summary[:, 6:18] == 0.0)
    assert F.fric_summary[:, 0:6].tobytes() == (F.surface.summary[:, 0:6] + 0.0).tobytes()
    m.close()


def test_s_of_regularized_items_and_bristle_items_without_contact(pfc):
    rng = np.random.default_rng(3)
    w = _workload(pfc, "c2")
    m = pfc.configs.build_scenario(w)
    A = m.contact_surface_fric(w.pose, w.twist, None, w.ins_ids)
    B = m.contact_surface_fric(w.pose, w.twist, rng.standard_normal((w.n_items, 6)), w.ins_ids)
    _same_bytes(A, B)
    m.close()
    w = pfc.configs.c3_blob_tool(3, n_div_blob=6, n_div_tool=5, distance=0.25)     # separated: no traction point
    w.s = rng.standard_normal((w.n_items, 6)) * 1e-3
    m = pfc.configs.build_scenario(w)
    F = m.contact_surface_fric(w.pose, w.twist, w.s, w.ins_ids)
    _, sdot, _ = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    assert F.fric.shape[0] == 0
    assert F.fric_summary[:, 12:18].tobytes() == sdot.tobytes()
    assert np.all(F.fric_summary[:, 12:18] != 0.0)
    assert np.all(F.fric_summary[:, 0:12] == 0.0) and np.all(F.fric_summary[:, 18:] == 0.0) and np.all(F.stiff == 0.0)
    m.close()


def test_multi_device_handle_and_device_form(pfc):
    import torch
    w = _workload(pfc, "c3")
    m = pfc.configs.build_scenario(w)
    F = m.contact_surface_fric(w.pose, w.twist, w.s, w.ins_ids)
    mm = pfc.configs.build_scenario(w, devices=[0, 0])
    _same_bytes(F, mm.contact_surface_fric(w.pose, w.twist, w.s, w.ins_ids))
    mm.close()
    dev = torch.device("cuda:0")
    n, P, T = w.n_items, F.surface.poly_idx.shape[0], F.fric.shape[0]
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    ids, pose, twist, s = t(w.ins_ids, torch.int32), t(w.pose), t(w.twist), t(w.s)
    full = lambda sh, v, dt=torch.float64: torch.full(sh, v, dtype=dt, device=dev)
    o = dict(off=full((n + 1,), -5, torch.int64), idx=full((P, 3), -5, torch.int32), xyz=full((P, 8, 3), np.nan),
             ptr=full((P + 1,), -5, torch.int64), trac=full((T, 8), np.nan), fric=full((T, 4), np.nan), sm=full((n, 11), np.nan),
             fs=full((n, 20), np.nan), st=full((n, 84), np.nan), cnt=full((n, 4), -5, torch.int32), tot=full((2,), 0, torch.int64))
    strm = torch.cuda.Stream()
    with torch.cuda.stream(strm):
        for _ in range(4):
            m.contact_surface_fric_device(n, ids.data_ptr(), pose.data_ptr(), twist.data_ptr(), s.data_ptr(), P, T, o["off"].data_ptr(),
                                          o["idx"].data_ptr(), o["xyz"].data_ptr(), o["ptr"].data_ptr(), o["trac"].data_ptr(),
                                          o["fric"].data_ptr(), o["sm"].data_ptr(), o["fs"].data_ptr(), o["st"].data_ptr(),
                                          o["cnt"].data_ptr(), o["tot"].data_ptr(), strm.cuda_stream)
            if m.check() == pfc._lib.OK:
                break
        else:
            pytest.fail("the device form did not settle")
    torch.cuda.synchronize()
    c = lambda key: o[key].cpu().numpy()
    D = pfc.FrictionSurface(pfc.ContactSurface(c("off"), c("idx"), c("xyz"), c("ptr"), c("trac"), c("sm"), c("cnt")), c("fric"), c("fs"),
                            c("st"))
    _same_bytes(F, D)
    assert list(c("tot")) == [P, T]
    m.close()


def _raw(pfc, m, w, cap_p, cap_t):
    n = w.n_items
    b = dict(off=np.full(n + 1, -7, np.int64), idx=np.full((max(cap_p, 1), 3), -7, np.int32), xyz=np.full((max(cap_p, 1), 8, 3), -7.0),
             ptr=np.full(cap_p + 1, -7, np.int64), trac=np.full((max(cap_t, 1), 8), -7.0), fric=np.full((max(cap_t, 1), 4), -7.0),
             sm=np.full((n, 11), -7.0), fs=np.full((n, 20), -7.0), st=np.full((n, 84), -7.0), cnt=np.full((n, 4), -7, np.int32),
             tot=np.full(2, -7, np.int64))
    ids = np.ascontiguousarray(w.ins_ids, np.int32); pose = np.ascontiguousarray(w.pose); tw = np.ascontiguousarray(w.twist)
    s = np.ascontiguousarray(w.s)
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    rc = pfc._lib.lib().pfc_contact_surface_fric(m._h, n, ids.ctypes.data_as(ip), pose.ctypes.data_as(dp), tw.ctypes.data_as(dp),
                                                 s.ctypes.data_as(dp), cap_p, cap_t, b["off"].ctypes.data_as(lp), b["idx"].ctypes.data_as(ip),
                                                 b["xyz"].ctypes.data_as(dp), b["ptr"].ctypes.data_as(lp), b["trac"].ctypes.data_as(dp),
                                                 b["fric"].ctypes.data_as(dp), b["sm"].ctypes.data_as(dp), b["fs"].ctypes.data_as(dp),
                                                 b["st"].ctypes.data_as(dp), b["cnt"].ctypes.data_as(ip), b["tot"].ctypes.data_as(lp))
    return rc, b


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_capacity_protocol(pfc, name):
    w = _workload(pfc, name)
    m = pfc.configs.build_scenario(w)
    F = m.contact_surface_fric(w.pose, w.twist, w.s, w.ins_ids)
    P, T = F.surface.poly_idx.shape[0], F.fric.shape[0]
    assert P > 1 and T > 1
    for cp, ct in ((P - 1, T - 1), (P - 1, T), (P, T - 1), (0, 0)):
        rc, b = _raw(pfc, m, w, cp, ct)
        assert rc == pfc._lib.ERR_OVERFLOW, (cp, ct, rc)
        assert list(b["tot"]) == [P, T]
        assert np.array_equal(b["off"], F.surface.poly_off) and b["sm"].tobytes() == F.surface.summary.tobytes()
        assert np.array_equal(b["cnt"], F.surface.counts)
        assert b["fs"].tobytes() == F.fric_summary.tobytes() and b["st"].tobytes() == F.stiff.tobytes()
        for key in ("idx", "xyz", "ptr", "trac", "fric"):
            assert np.all(b[key] == -7), key
    rc, b = _raw(pfc, m, w, P, T)
    assert rc == pfc._lib.OK
    D = pfc.FrictionSurface(pfc.ContactSurface(b["off"], b["idx"][:P], b["xyz"][:P], b["ptr"], b["trac"][:T], b["sm"], b["cnt"]),
                            b["fric"][:T], b["fs"], b["st"])
    _same_bytes(F, D)
    m.close()


def test_no_interference_with_fixed_order_evaluations(pfc):
    w = _workload(pfc, "c5")
    m = pfc.configs.build_scenario(w)
    m.set_option("fixed_order", 1)
    a = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    m.contact_surface_fric(w.pose, w.twist, w.s, w.ins_ids)
    b = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    m.close()


def test_friction_surface_ends_dual_reuse(pfc):
    import torch
    w = _workload(pfc, "c3")
    m = pfc.configs.build_scenario(w)
    dev = torch.device("cuda:0")
    n, nd = w.n_items, 2
    rng = np.random.default_rng(5)
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    T = dict(ids=t(w.ins_ids, torch.int32), pose=t(w.pose), twist=t(w.twist), s=t(w.s), dp=t(rng.standard_normal((n, nd, 24)) * 1e-3),
             dt=t(rng.standard_normal((n, nd, 6))), ds=t(np.zeros((n, nd, 6))))
    z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=dev)
    o = dict(w=z(n, 6), sd=z(n, 6), dw=z(n, nd, 6), dsd=z(n, nd, 6), c=torch.zeros((n, 4), dtype=torch.int32, device=dev))
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(6):
        m.eval_dual_device(n, nd, T["ids"].data_ptr(), T["pose"].data_ptr(), T["twist"].data_ptr(), T["s"].data_ptr(), T["dp"].data_ptr(),
                           T["dt"].data_ptr(), T["ds"].data_ptr(), o["w"].data_ptr(), o["sd"].data_ptr(), o["dw"].data_ptr(),
                           o["dsd"].data_ptr(), o["c"].data_ptr(), st)
        if m.check() == pfc._lib.OK:
            break
    else:
        pytest.fail("the Dual evaluation did not settle")
    m.contact_surface_fric(w.pose, w.twist, w.s, w.ins_ids)
    with pytest.raises(pfc._lib.PFCError) as e:
        m.eval_dual_device_more(nd, T["dp"].data_ptr(), T["dt"].data_ptr(), T["ds"].data_ptr(), o["dw"].data_ptr(), o["dsd"].data_ptr(), st)
    assert e.value.status == pfc._lib.ERR_STATE
    m.close()


def test_scale_full_size_c3(pfc):
    w = pfc.configs.c3_blob_tool(64)
    m = pfc.configs.build_scenario(w)
    F = m.contact_surface_fric(w.pose, w.twist, w.s, w.ins_ids)
    _, _, counts = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    assert np.array_equal(F.surface.counts, counts) and F.fric.shape[0] == int(counts[:, 3].sum())
    items = [0, 21, 42, 63]
    _check_against_oracle(w, F, items, H.oracle_run(pfc, w, items=items))
    for k in items:
        _check_consistency(F, k)
    m.close()
