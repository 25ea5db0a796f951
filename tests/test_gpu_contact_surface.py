"""pfc_contact_surface on the device: the contact surface (polygons, TractionCache, normal wrench / cop) against the CPU oracle,
its geometry, its canonical order and reproducibility across options and handles, the capacity protocol, and that it leaves the
handle's evaluations alone."""
import ctypes as C

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

SCENES = ["c1", "c2", "c3", "c3_full", "vv_reg", "vv_bristle", "c5", "spoon"]


def _workload(pfc, name):
    Cf = pfc.configs
    return {"c1": lambda: Cf.c1_boxes(), "c2": lambda: Cf.c2_box_on_plane(3), "c3": lambda: Cf.c3_blob_tool(4, n_div_blob=8, n_div_tool=6),
            "c3_full": lambda: Cf.c3_blob_tool(2), "vv_reg": lambda: Cf.vol_vol(6, n_div=5),
            "vv_bristle": lambda: Cf.vol_vol(6, n_div=5, model="bristle"), "c5": lambda: Cf.c5_pile(n_side=3),
            "spoon": lambda: Cf.spoon_pencil_pads(6)}[name]()


def _arrays(S):
    return [S.poly_off, S.poly_idx, S.poly_xyz, S.poly_trac, S.trac, S.summary, S.counts]


def _same_bytes(S1, S2):
    for a, b in zip(_arrays(S1), _arrays(S2)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _lib_meshes(w, k):
    """(mesh_1, mesh_2) of item k as the library holds them (add_friction! puts the triangle mesh first)."""
    c = w.instructions[int(w.ins_ids[k])]
    m1, m2 = w.meshes[c.id_1].mesh, w.meshes[c.id_2].mesh
    if m1.tri is None and m2.tri is not None:
        m1, m2 = m2, m1
    return m1, m2, c


def _multiset(t):
    return t[np.lexsort(tuple(t[:, c] for c in range(7, -1, -1)))]


def _close(a, b, tol=1e-12):
    if np.linalg.norm(b) == 0.0:
        return np.linalg.norm(a) == 0.0
    return H.rel_err(a, b) < tol


def _check_against_oracle(pfc, w, S, items, ref):
    for k, r in zip(items, ref):
        it = S.item(k)
        assert np.array_equal(S.counts[k], r.counts), (k, S.counts[k], r.counts)
        pairs, clip_n = H.sorted_pairs(r.pairs, r.clip_n)
        keep = clip_n >= 3
        assert np.array_equal(it["keys"], pairs[keep]), f"item {k}: polygon keys differ"
        assert np.array_equal(it["n_vert"], clip_n[keep]), f"item {k}: vertex counts differ"
        assert it["trac"].shape == r.trac.shape and it["trac"].shape[0] == S.counts[k, 3]
        assert np.array_equal(_multiset(it["trac"]), _multiset(r.trac)), f"item {k}: traction points are not bit-identical"
        # summary against the oracle's points
        nw = H.normal_wrench_from_tractions(r.trac)
        assert _close(it["wrench"], nw), (k, it["wrench"], nw)
        pdA = r.trac[:, 6] * r.trac[:, 7]
        assert _close([it["sum_p_dA"]], [pdA.sum()]) and _close([it["area"]], [r.trac[:, 6].sum()]), k
        if r.trac.shape[0]:
            assert _close(it["cop"], (pdA[:, None] * r.trac[:, 3:6]).sum(axis=0) / pdA.sum()), k
        else:
            assert np.all(S.summary[k] == 0.0)
        if w.instructions[int(w.ins_ids[k])].model == "bristle" and r.trac.shape[0]:
            assert _close(it["wrench"], r.wrench_normal), (k, it["wrench"], r.wrench_normal)
            assert _close(it["cop"], r.cop), (k, it["cop"], r.cop)


def _check_geometry(w, S):
    for k in range(S.n_items):
        it = S.item(k)
        m1, m2, c = _lib_meshes(w, k)
        nq = 1 if c.n_quad_rule == 1 else 3
        R21 = w.pose[k, 0:9].reshape(3, 3, order="F"); t21 = w.pose[k, 9:12]
        scale = max(1e-300, float(np.abs(m2.point).max()))
        tol = 1e-12 * scale
        keys = it["keys"].astype(np.int64)
        assert np.all(np.diff(keys[:, 0] * (1 << 32) + keys[:, 1]) > 0), f"item {k}: keys not strictly increasing"
        for j in range(it["keys"].shape[0]):
            nv = int(it["n_vert"][j])
            assert 3 <= nv <= 8
            V = it["xyz"][j, :nv]
            assert np.all(it["xyz"][j, nv:] == 0.0)
            t0, t1 = int(it["poly_trac"][j]), int(it["poly_trac"][j + 1])
            T = it["trac"][t0:t1]
            if m1.tri is not None:      # tri-tet: on the plane of triangle e1 (moved into r2), inside tet e2
                tri = m1.point[m1.tri[it["keys"][j, 0]]] @ R21.T + t21
                nrm = np.cross(tri[1] - tri[0], tri[2] - tri[0]); nrm /= np.linalg.norm(nrm)
                assert np.all(np.abs((V - tri[0]) @ nrm) <= tol), (k, j)
            tet = m2.point[m2.tet[it["keys"][j, 1]]]
            A = np.vstack([tet.T, np.ones(4)])
            zeta = np.linalg.solve(A, np.vstack([V.T, np.ones(nv)]))
            assert np.all(zeta >= -1e-12), (k, j, zeta.min())
            # the fan area about vertex 0 (in coordinates relative to it: the polygon can be tiny next to its distance from the
            # origin); slack: the rounding of areas formed from edges of length h is ~1e-16 h^2
            D = V - V[0]
            area_vec = 0.5 * sum(np.cross(D[i], D[i + 1]) for i in range(1, nv - 1))
            area = float(np.linalg.norm(area_vec))
            slack = 1e-12 * area + 1e-14 * float(np.max(np.sum(D * D, axis=1)))
            if T.shape[0]:
                n = T[0, 0:3]
                assert np.all(T[:, 0:3] == n)
                assert np.all(np.abs((V - V[0]) @ n) <= tol), (k, j)            # planar, normal = the points' n
                assert area_vec @ n > 0.0
                for i in range(nv):                                              # every point inside the polygon
                    e = V[(i + 1) % nv] - V[i]
                    assert np.all(np.cross(e, T[:, 3:6] - V[i]) @ n >= -tol * scale), (k, j, i)
                sdA = T[:, 6].sum()
                assert sdA <= area + slack, (k, j, sdA, area)
                if T.shape[0] == nv * nq:
                    assert abs(sdA - area) <= slack, (k, j, sdA, area)


@pytest.mark.parametrize("name", SCENES)
def test_surface_matches_oracle_and_geometry(pfc, name):
    w = _workload(pfc, name)
    m = pfc.configs.build_scenario(w)
    S = m.contact_surface(w.pose, w.twist, w.ins_ids)
    _, _, counts = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    assert np.array_equal(S.counts, counts)
    assert int(S.poly_off[-1]) == int(counts[:, 2].sum()) and S.trac.shape[0] == int(counts[:, 3].sum())
    assert S.trac.shape[0] > 0
    ref = H.oracle_run(pfc, w)
    _check_against_oracle(pfc, w, S, range(w.n_items), ref)
    _check_geometry(w, S)
    # two calls, and handles with other options, return the same bytes
    _same_bytes(S, m.contact_surface(w.pose, w.twist, w.ins_ids))
    for opt in ({"fused": 0}, {"team": 0}, {"fixed_order": 1}, {"split_min": 1}, {"debug": 1}):
        m2 = pfc.configs.build_scenario(w)
        for key, v in opt.items():
            m2.set_option(key, v)
        m2.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
        _same_bytes(S, m2.contact_surface(w.pose, w.twist, w.ins_ids))
        m2.close()
    m.close()


def test_multi_device_handle_and_device_form(pfc):
    import torch
    w = _workload(pfc, "c3")
    m = pfc.configs.build_scenario(w)
    S = m.contact_surface(w.pose, w.twist, w.ins_ids)
    mm = pfc.configs.build_scenario(w, devices=[0, 0])
    _same_bytes(S, mm.contact_surface(w.pose, w.twist, w.ins_ids))
    mm.close()
    dev = torch.device("cuda:0")
    n, P, T = w.n_items, S.poly_idx.shape[0], S.trac.shape[0]
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    ids, pose, twist = t(w.ins_ids, torch.int32), t(w.pose), t(w.twist)
    o = dict(off=torch.full((n + 1,), -5, dtype=torch.int64, device=dev), idx=torch.full((P, 3), -5, dtype=torch.int32, device=dev),
             xyz=torch.full((P, 8, 3), np.nan, dtype=torch.float64, device=dev), ptr=torch.full((P + 1,), -5, dtype=torch.int64, device=dev),
             trac=torch.full((T, 8), np.nan, dtype=torch.float64, device=dev), sm=torch.full((n, 11), np.nan, dtype=torch.float64, device=dev),
             cnt=torch.full((n, 4), -5, dtype=torch.int32, device=dev), tot=torch.zeros(2, dtype=torch.int64, device=dev))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(4):
            m.contact_surface_device(n, ids.data_ptr(), pose.data_ptr(), twist.data_ptr(), P, T, o["off"].data_ptr(), o["idx"].data_ptr(),
                                     o["xyz"].data_ptr(), o["ptr"].data_ptr(), o["trac"].data_ptr(), o["sm"].data_ptr(),
                                     o["cnt"].data_ptr(), o["tot"].data_ptr(), s.cuda_stream)
            if m.check() == pfc._lib.OK:
                break
        else:
            pytest.fail("the device form did not settle")
    torch.cuda.synchronize()
    D = pfc.ContactSurface(o["off"].cpu().numpy(), o["idx"].cpu().numpy(), o["xyz"].cpu().numpy(), o["ptr"].cpu().numpy(),
                           o["trac"].cpu().numpy(), o["sm"].cpu().numpy(), o["cnt"].cpu().numpy())
    _same_bytes(S, D)
    assert list(o["tot"].cpu().numpy()) == [P, T]
    m.close()


def _raw(pfc, m, w, cap_p, cap_t, fill=True):
    n = w.n_items
    b = dict(off=np.full(n + 1, -7, np.int64), idx=np.full((max(cap_p, 1), 3), -7, np.int32), xyz=np.full((max(cap_p, 1), 8, 3), -7.0),
             ptr=np.full(cap_p + 1, -7, np.int64), trac=np.full((max(cap_t, 1), 8), -7.0), sm=np.full((n, 11), -7.0),
             cnt=np.full((n, 4), -7, np.int32), tot=np.full(2, -7, np.int64))
    ids = np.ascontiguousarray(w.ins_ids, np.int32); pose = np.ascontiguousarray(w.pose); tw = np.ascontiguousarray(w.twist)
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    rc = pfc._lib.lib().pfc_contact_surface(m._h, n, ids.ctypes.data_as(ip), pose.ctypes.data_as(dp), tw.ctypes.data_as(dp), cap_p, cap_t,
                                            b["off"].ctypes.data_as(lp), b["idx"].ctypes.data_as(ip), b["xyz"].ctypes.data_as(dp),
                                            b["ptr"].ctypes.data_as(lp), b["trac"].ctypes.data_as(dp), b["sm"].ctypes.data_as(dp),
                                            b["cnt"].ctypes.data_as(ip), b["tot"].ctypes.data_as(lp))
    return rc, b


def test_capacity_protocol(pfc):
    w = _workload(pfc, "c2")
    m = pfc.configs.build_scenario(w)
    S = m.contact_surface(w.pose, w.twist, w.ins_ids)
    P, T = S.poly_idx.shape[0], S.trac.shape[0]
    assert P > 1 and T > 1
    for cp, ct in ((P - 1, T), (P, T - 1), (0, 0)):
        rc, b = _raw(pfc, m, w, cp, ct)
        assert rc == pfc._lib.ERR_OVERFLOW, (cp, ct, rc)
        assert list(b["tot"]) == [P, T]
        assert np.array_equal(b["off"], S.poly_off) and b["sm"].tobytes() == S.summary.tobytes() and np.array_equal(b["cnt"], S.counts)
        for key in ("idx", "xyz", "ptr", "trac"):
            assert np.all(b[key] == -7), key
    rc, b = _raw(pfc, m, w, P, T)
    assert rc == pfc._lib.OK
    _same_bytes(S, pfc.ContactSurface(b["off"], b["idx"][:P], b["xyz"][:P], b["ptr"], b["trac"][:T], b["sm"], b["cnt"]))
    m.close()


def test_empty_and_separated(pfc):
    w = pfc.configs.c3_blob_tool(3, n_div_blob=6, n_div_tool=5, distance=0.25)
    m = pfc.configs.build_scenario(w)
    S = m.contact_surface(w.pose, w.twist, w.ins_ids)
    assert np.all(S.poly_off == 0) and S.poly_idx.shape[0] == 0 and S.trac.shape[0] == 0 and np.all(S.summary == 0.0)
    assert np.all(S.counts[:, 2:] == 0)
    E = m.contact_surface(np.zeros((0, 24)), np.zeros((0, 6)), np.zeros(0, dtype=np.int32))
    assert E.n_items == 0 and E.poly_off.tolist() == [0] and E.trac.shape == (0, 8)
    m.close()


def test_no_interference_with_fixed_order_evaluations(pfc):
    w = _workload(pfc, "c5")
    m = pfc.configs.build_scenario(w)
    m.set_option("fixed_order", 1)
    a = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    m.contact_surface(w.pose, w.twist, w.ins_ids)
    b = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    c = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    m.close()


def test_surface_ends_dual_reuse(pfc):
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

    def dual():
        for _ in range(6):
            m.eval_dual_device(n, nd, T["ids"].data_ptr(), T["pose"].data_ptr(), T["twist"].data_ptr(), T["s"].data_ptr(), T["dp"].data_ptr(),
                               T["dt"].data_ptr(), T["ds"].data_ptr(), o["w"].data_ptr(), o["sd"].data_ptr(), o["dw"].data_ptr(),
                               o["dsd"].data_ptr(), o["c"].data_ptr(), st)
            if m.check() == pfc._lib.OK:
                return
        pytest.fail("the Dual evaluation did not settle")

    more = lambda: m.eval_dual_device_more(nd, T["dp"].data_ptr(), T["dt"].data_ptr(), T["ds"].data_ptr(), o["dw"].data_ptr(),
                                           o["dsd"].data_ptr(), st)
    dual()
    more()                                  # allowed right after a checked Dual evaluation
    assert m.check() == pfc._lib.OK
    dual()
    m.contact_surface(w.pose, w.twist, w.ins_ids)
    with pytest.raises(pfc._lib.PFCError) as e:
        more()
    assert e.value.status == pfc._lib.ERR_STATE
    m.close()


def test_scale_full_size_c3(pfc):
    w = pfc.configs.c3_blob_tool(64)
    m = pfc.configs.build_scenario(w)
    S = m.contact_surface(w.pose, w.twist, w.ins_ids)
    _, _, counts = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    assert S.trac.shape[0] == int(counts[:, 3].sum()) and S.poly_idx.shape[0] == int(counts[:, 2].sum())
    assert np.array_equal(S.counts, counts)
    items = [0, 21, 42, 63]
    _check_against_oracle(pfc, w, S, items, H.oracle_run(pfc, w, items=items))
    m.close()
