"""Shared test helpers: run a configs.Workload through the CPU oracle."""
import numpy as np

from oracle import oracle as O


def oracle_meshes(w):
    return [O.OracleMesh(ms.mesh, ms.tree, ms.Ebar or 0.0) for ms in w.meshes]


def oracle_ins(pfc, c):
    mu_s, mu_d = pfc.scenario.determine_mu_s_mu_d(c.mu_s, c.mu_d)
    if c.model == "regularized":
        return O.make_ins(c.chi, c.n_quad_rule, O.REGULARIZED, mu_s, mu_d, v_c=c.v_tol)
    return O.make_ins(c.chi, c.n_quad_rule, O.BRISTLE, mu_s, mu_d, tau=c.tau, k_bar=c.k_bar, magic=c.magic)


def oracle_run(pfc, w, items=None, debug=True):
    """Per-item oracle evaluation (force_single_elastic_intersection!).  Returns a list of EvalResult."""
    om = oracle_meshes(w)
    oi = [oracle_ins(pfc, c) for c in w.instructions]
    out = []
    for k in (range(w.n_items) if items is None else items):
        c = w.instructions[int(w.ins_ids[k])]
        out.append(O.evaluate(om[c.id_1], om[c.id_2], oi[int(w.ins_ids[k])], w.pose[k], w.twist[k], w.s[k],
                              debug=debug))
    return out


def sorted_pairs(pairs, clip_n):
    """Canonical order for comparing candidate sets: sort by (i_1, i_2)."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    clip_n = np.asarray(clip_n).reshape(-1)
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    return pairs[order], clip_n[order]


def sdot_tolerance(r):
    """The project's parity bound for ṡ of one item against its oracle debug result r (tests/test_gpu_scale.py, bench.py's
    validation): 1e-6, and 1e-3 for a bristle patch whose scaled stiffness K̄ has two or more eigenvalues below 1e-12 σ_max
    (slivers, edge and single-triangle contacts), where the reference's own ṡ moves by more than 1e-6 under a rounding-level
    change of K̄ (tests/test_sdot_sensitivity.py)."""
    if r.has_K:
        Kb = np.diag(r.Sinv) @ r.K @ np.diag(r.Sinv)
        ev = np.linalg.eigvalsh((Kb + Kb.T) / 2)
        if np.sum(ev < 1e-12 * ev[-1]) >= 2:
            return 1e-3
    return 1e-6


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    scale = max(np.linalg.norm(b), 1e-300)
    return float(np.linalg.norm(a - b) / scale)


# ----------------------------------------------------------------------------------------------------------------
# One (mesh_1, mesh_2, instruction, pose) scene through either backend: "oracle" (CPU restatement) or "hip" (the
# library, through the C ABI, debug views on).  The reference's scene-level tests read m.float.bodyBodyCache after
# one calcXd (test/test_normal.jl:31-41, test/test_friction.jl:228-236,251-256); both backends return the same view.
# ----------------------------------------------------------------------------------------------------------------
class SceneResult:
    __slots__ = ("status", "wrench", "sdot", "counts", "trac", "has_K", "K", "Kbar_inv_sqrt", "Sinv", "cop", "pairs", "clip_n")


def normal_wrench_from_tractions(trac):
    """normal_wrench(b) (src/contact_algorithms_normal.jl:2-15) over a TractionCache dump (n 3, r 3, dA, p)."""
    pdA = trac[:, 6] * trac[:, 7]
    lin = (pdA[:, None] * trac[:, 0:3]).sum(axis=0)
    ang = np.cross(trac[:, 3:6], pdA[:, None] * trac[:, 0:3]).sum(axis=0)
    return np.concatenate([ang, lin])


def eval_scene(backend, pfc, mesh_1, Ebar_1, mesh_2, Ebar_2, ins, pose, twist, s=None, trees=None, options=None,
               want_pairs=False):
    """ins: dict(model="regularized"|"bristle", chi, n_quad, mu_s, mu_d, v_c | tau, k_bar, magic).
    trees: optional (OBBTree, OBBTree) supplied by the host instead of the library's builder."""
    G = pfc.geometry
    t1, t2 = trees if trees is not None else (G.build_tree(mesh_1), G.build_tree(mesh_2))
    r = SceneResult()
    if backend == "oracle":
        m1, m2 = O.OracleMesh(mesh_1, t1, Ebar_1 or 0.0), O.OracleMesh(mesh_2, t2, Ebar_2 or 0.0)
        if ins["model"] == "regularized":
            oi = O.make_ins(ins["chi"], ins["n_quad"], O.REGULARIZED, ins["mu_s"], ins["mu_d"], v_c=ins["v_c"])
        else:
            oi = O.make_ins(ins["chi"], ins["n_quad"], O.BRISTLE, ins["mu_s"], ins["mu_d"], tau=ins["tau"],
                            k_bar=ins["k_bar"], magic=ins["magic"])
        e = O.evaluate(m1, m2, oi, pose, twist, s)
        r.status, r.wrench, r.sdot, r.counts, r.trac = e.status, e.wrench, e.sdot, e.counts, e.trac
        r.has_K, r.K, r.Kbar_inv_sqrt, r.Sinv, r.cop = e.has_K, e.K, e.Kbar_inv_sqrt, e.Sinv, e.cop
        r.pairs, r.clip_n = e.pairs, e.clip_n
        return r
    assert backend == "hip"
    S = pfc.scenario
    m = S.MechanismScenario()
    i1 = m.add_contact("mesh_1", mesh_1, c_prop=None if mesh_1.tri is not None else S.ContactProperties(Ebar_1), tree=t1)
    i2 = m.add_contact("mesh_2", mesh_2, c_prop=S.ContactProperties(Ebar_2), tree=t2)
    if ins["model"] == "regularized":
        m.add_friction_regularize(i1, i2, mu_s=ins["mu_s"], mu_d=ins["mu_d"], chi=ins["chi"], v_tol=ins["v_c"],
                                  n_quad_rule=ins["n_quad"])
    else:
        m.add_friction_bristle(i1, i2, tau=ins["tau"], k_bar=ins["k_bar"], mu_s=ins["mu_s"], mu_d=ins["mu_d"],
                               chi=ins["chi"], n_quad_rule=ins["n_quad"], magic=ins["magic"])
    m.finalize()
    m.set_option("debug", 1)
    for k, v in (options or {}).items():
        m.set_option(k, v)
    pose = np.asarray(pose, dtype=np.float64).reshape(1, 24)
    twist = np.asarray(twist, dtype=np.float64).reshape(1, 6)
    s_in = np.zeros((1, 6)) if s is None else np.asarray(s, dtype=np.float64).reshape(1, 6)
    wrench, sdot, counts = m.force_all_elastic_intersections(pose, twist, s_in)
    r.status, r.wrench, r.sdot, r.counts = 0, wrench[0], sdot[0], counts[0]
    r.trac = m.debug_tractions(0)
    r.pairs, r.clip_n = m.debug_pairs(0) if want_pairs else (None, None)
    st = m.debug_stiffness(0) if ins["model"] == "bristle" else None
    r.has_K = st is not None
    r.K, r.Kbar_inv_sqrt, r.Sinv, r.cop = st if st is not None else (None, None, None, None)
    m.close()
    return r


def fuzz_workload(pfc, rng, n_items, degenerate, tet_tet=False):
    """Random small meshes in random relative poses: a box surface (12 triangles), a sphere surface and a tet box /
    tet sphere with random scales; poses put the surfaces at random depths through the tets.  degenerate: poses
    snapped to axis-aligned rotations and lattice offsets, so that triangle vertices and edges land exactly on tet
    faces (the strict / non-strict inside tests of static_clip.jl:140-188 and the zero ties of the trivial reject)."""
    G, Cf = pfc.geometry, pfc.configs
    box_tet = G.as_tet_emesh(G.emesh_box_div(np.array([0.5, 0.5, 0.5]), 2))
    sph_tet = G.as_tet_emesh(G.emesh_sphere(0.5, 3))
    box_tri = G.as_tri_emesh(G.emesh_box(np.array([0.25, 0.25, 0.25])))
    sph_tri = G.as_tri_emesh(G.emesh_sphere(0.3, 2))
    meshes = [Cf._mesh("box_tri", box_tri), Cf._mesh("sph_tri", sph_tri), Cf._mesh("box_tet", box_tet, 1.0e6),
              Cf._mesh("sph_tet", sph_tet, 2.0e6)]
    ins = [Cf.InsSpec(0, 2, "regularized", chi=0.5, mu_d=0.3, v_tol=1e-2), Cf.InsSpec(1, 2, "bristle", chi=0.3, mu_d=0.4),
           Cf.InsSpec(0, 3, "bristle", chi=0.5, mu_d=0.3, n_quad_rule=1), Cf.InsSpec(1, 3, "regularized", chi=0.1, mu_d=0.2, v_tol=1e-3)]
    if tet_tet:    # volume-volume instructions in the same scenario: the TT kernel variants serve all six
        ins += [Cf.InsSpec(2, 3, "regularized", chi=0.5, mu_d=0.3, v_tol=1e-2), Cf.InsSpec(3, 2, "bristle", chi=0.4, mu_d=0.3)]
    ids = rng.integers(0, len(ins), n_items).astype(np.int32)
    pose, twist, s = [], [], []
    quarter = [np.eye(3), np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]]), np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]]),
               np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0.0]])]
    for k in range(n_items):
        if degenerate:
            R = quarter[rng.integers(0, 4)] @ quarter[rng.integers(0, 4)]
            t = rng.integers(-3, 4, 3) * 0.125
        else:
            R = Cf.random_rotation(rng)
            t = rng.uniform(-0.6, 0.6, 3)
        pose.append(pfc.scenario.relative_pose(R, t, np.eye(3), np.zeros(3)))
        twist.append(rng.standard_normal(6) * np.array([1, 1, 1, 0.1, 0.1, 0.1]))
        s.append(rng.standard_normal(6) * 1e-3)
    return Cf.Workload("fuzz", meshes, ins, ids, np.array(pose), np.array(twist), np.array(s))


# ----------------------------------------------------------------------------------------------------------------
# The four regimes of traction() (friction.jl): x = |v_t| / v_c (regularized) or |T̄s| / mu_s (bristle); stick x < 1,
# plateau at mu_s 1 <= x < 2, ramp to mu_d 2 <= x < 3, slide x >= 3.  Scenes with mu_s > mu_d whose points populate all
# four, and the classifier that counts them from the oracle's debug result.
# ----------------------------------------------------------------------------------------------------------------
REGIME_MU_S = 0.6
REGIME_EDGES = (1.0, 2.0, 3.0)
REGIME_NAMES = ("stick", "plateau", "ramp", "slide")


def friction_branch_input(c, mu_s, trac, twist, Delta=None, cop=None):
    """Per traction point (rows n 3, r 3, dA, p) of one item: the vector traction() takes (vel_t, regularized, or T̄s,
    bristle: from the item's Delta and cop), projected off n̂; p dA; and the threshold of the first branch."""
    n, r, pdA = trac[:, 0:3], trac[:, 3:6], trac[:, 6] * trac[:, 7]
    ang, lin = twist[0:3], twist[3:6]
    rdot = lin + np.cross(ang, r)
    if c.model == "regularized":
        v = rdot
        thr = c.v_tol
    else:
        x = r - cop
        v = -c.k_bar * ((Delta[3:6] + np.cross(Delta[0:3], x)) + c.tau * rdot)
        thr = mu_s
    v = v - np.sum(v * n, axis=1)[:, None] * n      # vec_sub_vec_proj
    return v, pdA, thr


def friction_regime_scenes(pfc):
    """{name: Workload}: R1 (regularized tri-tet), B1 (bristle tri-tet), V_reg / V_bri (tet-tet), every instruction with
    mu_s = 0.6 > mu_d = 0.3, twists and bristle states scaled so that every regime holds traction points."""
    Cf = pfc.configs
    r1 = Cf.c2_box_on_plane(4, n_div=3)
    r1.twist = np.array([[0.0, 0.0, 0.6, 0.005 * k, 0.0, 0.0] for k in range(r1.n_items)])
    b1 = Cf.c3_blob_tool(4, n_div_blob=6, n_div_tool=4)
    b1.twist = b1.twist * 0.04
    b1.s = np.random.default_rng(5).standard_normal((4, 6)) * 1e-4
    v_reg = Cf.vol_vol(4, n_div=3, model="regularized")
    v_reg.twist = v_reg.twist * 0.3
    v_bri = Cf.vol_vol(4, n_div=3, model="bristle")
    v_bri.twist = v_bri.twist * 0.04
    v_bri.s = np.random.default_rng(5).standard_normal((8, 6)) * 1e-4
    scenes = {"R1": r1, "B1": b1, "V_reg": v_reg, "V_bri": v_bri}
    for w in scenes.values():
        for c in w.instructions:
            c.mu_s = REGIME_MU_S
        w.twist = np.ascontiguousarray(w.twist); w.s = np.ascontiguousarray(w.s)
    return scenes


def friction_regimes(pfc, w, k, ref):
    """Regimes of item k's traction points from its oracle debug result ref: (counts of stick, plateau, ramp, slide;
    the smallest |x - e| over the points and the edges e = 1, 2, 3 -- inf without points)."""
    c = w.instructions[int(w.ins_ids[k])]
    mu_s, _ = pfc.scenario.determine_mu_s_mu_d(c.mu_s, c.mu_d)
    if ref.trac is None or ref.trac.shape[0] == 0:
        return np.zeros(4, dtype=int), np.inf
    v, _, thr = friction_branch_input(c, mu_s, ref.trac, w.twist[k], ref.Delta, ref.cop)
    x = np.linalg.norm(v, axis=1) / thr
    counts = np.bincount(np.searchsorted(np.array(REGIME_EDGES), x, side="right"), minlength=4)
    return counts, float(np.abs(x[:, None] - np.array(REGIME_EDGES)[None, :]).min())


# ----------------------------------------------------------------------------------------------------------------
# The host-pointer forms that stage through the context's block (csrc/pfc_hip.hip, Stage): a small scene and raw calls
# with any optional pointer null.
# ----------------------------------------------------------------------------------------------------------------
import ctypes as C


def random_body_states(pfc, rng, n_scene, n_body):
    """World states of n_scene x n_body bodies: x (R column-major, then t) and twist."""
    x = np.zeros((n_scene, n_body, 12)); tw = rng.standard_normal((n_scene, n_body, 6))
    for s in range(n_scene):
        for b in range(n_body):
            x[s, b, :9] = pfc.configs.random_rotation(rng).reshape(-1, order="F")
            x[s, b, 9:] = rng.uniform(-1, 1, 3) * rng.uniform(0, 10)
    return x, tw


HOST_FORMS_ORDER = ("surface_fric", "items", "local_jacobian", "scatter", "seeds", "apply", "scatter_dual", "surface")   # staging need large -> small -> large
N_SCENE, N_BODY, NV = 2, 3, 5
BIND = [(-1, 0), (1, 2), (0, 2), (2, -1)]
LJAC = ("local_jacobian", "local_jacobian3", "local_jacobian_c1")
_CT = {np.dtype(np.float64): C.c_double, np.dtype(np.int32): C.c_int, np.dtype(np.int64): C.c_longlong}


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(_CT[a.dtype]))


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class HostFormsCase:
    """The inputs of every host-pointer form that stages through the context's block, made once, and one call of a form through the C
    ABI (tests/test_gpu_host_staging.py, scripts/host_forms_rate.py)."""

    def __init__(self, pfc):
        rng = np.random.default_rng(3)
        self.w = w = fuzz_workload(pfc, rng, 5, False)
        w.ins_ids[:3] = np.arange(3)       # a null ins_ids of three items names these
        self.c1 = pfc.configs.c1_boxes()   # regularized instructions only: s may be null
        self.x, self.tw = random_body_states(pfc, rng, N_SCENE, N_BODY)
        self.scene = _i32([0, 1, 1, 0, 1])
        self.dx, self.dtw = rng.standard_normal((N_SCENE, N_BODY, 3, 12)), rng.standard_normal((N_SCENE, N_BODY, 3, 6))
        self.L = rng.standard_normal((3, 12, 36))
        self.seed = [rng.standard_normal((3, 1, 24)), rng.standard_normal((3, 1, 6)), rng.standard_normal((3, 1, 6))]
        xr = np.zeros((5, 12))
        for k in range(5):
            xr[k, :9] = pfc.configs.random_rotation(rng).reshape(-1, order="F"); xr[k, 9:] = rng.standard_normal(3)
        self.sc = dict(wrench=rng.standard_normal((5, 6)), d_wrench=rng.standard_normal((5, 3, 6)), x_w_r2=xr,
                       d_x_w_r2=rng.standard_normal((5, 3, 12)), body_1=_i32([-1, 0, 2, 1, 0]), body_2=_i32([1, 2, -1, 0, 2]),
                       jac=rng.standard_normal((N_BODY, NV, 6)), d_jac=rng.standard_normal((N_BODY, 3, NV, 6)))

    def handle(self, pfc, devices=None, c1=False, **options):
        m = pfc.configs.build_scenario(self.c1 if c1 else self.w, devices=devices)
        for k, v in options.items():
            m.set_option(k, v)
        for k, (b1, b2) in enumerate(BIND):
            m.set_instruction_bodies(k, b1, b2)
        return m

    # Every form: (inputs that may be null or replaced, outputs); drop names the arguments passed as NULL.
    def args(self, form):
        w, s, z = self.w, self.sc, np.zeros
        if form == "items":
            return dict(ins_ids=_i32(w.ins_ids[:3]), scene=self.scene[:3].copy()), dict(
                pose=z((3, 24)), twist=z((3, 6)), x_w_r2=z((3, 12)), body_1=z(3, np.int32), body_2=z(3, np.int32))
        if form == "seeds":
            return dict(d_x_w_b=self.dx, d_twist_w_b=self.dtw), dict(d_pose=z((5, 3, 24)), d_twist=z((5, 3, 6)), d_x_w_r2=z((5, 3, 12)))
        if form in LJAC:      # five items; three, instructions 0 .. 2; three of C1's, on a handle of C1
            n = 5 if form == "local_jacobian" else 3
            w = self.c1 if form == "local_jacobian_c1" else w
            return dict(ins_ids=_i32(w.ins_ids[:n]), s=np.ascontiguousarray(w.s[:n])), dict(
                wrench=z((n, 6)), sdot=z((n, 6)), L=z((n, 12, 36)), counts=z((n, 4), np.int32))
        if form == "apply":
            return dict(d_s=self.seed[2]), dict(d_wrench=z((3, 1, 6)), d_sdot=z((3, 1, 6)))
        if form == "scatter":
            return dict(scene=self.scene), dict(f=z((N_SCENE, NV)))
        if form == "scatter_dual":
            return dict(d_x_w_r2=s["d_x_w_r2"], d_jac=s["d_jac"], scene=self.scene), dict(f=z((N_SCENE, NV)), d_f=z((N_SCENE, 3, NV)))
        raise KeyError(form)

    def run(self, pfc, m, form, drop=(), **over):
        """One call of a form through the C ABI; returns {output name: array} of the outputs asked for."""
        if form in ("surface", "surface_fric"):
            return self.surface(pfc, m, form == "surface_fric", drop)
        L, w, s = pfc._lib.lib(), self.w, self.sc
        a, o = self.args(form)
        a.update(over)
        for k in drop:
            (a if k in a else o)[k] = None
        h, out = m._h, [_ptr(v) for v in o.values()]
        if form == "items":
            rc = L.pfc_items_from_bodies(h, 3, _ptr(a["ins_ids"]), _ptr(a["scene"]), N_SCENE, N_BODY, _ptr(self.x), _ptr(self.tw), *out)
        elif form == "seeds":
            rc = L.pfc_dual_seeds_from_bodies(h, 5, 3, _ptr(_i32(w.ins_ids)), _ptr(self.scene), N_SCENE, N_BODY, _ptr(self.x), _ptr(self.tw),
                                              _ptr(a["d_x_w_b"]), _ptr(a["d_twist_w_b"]), *out)
        elif form in LJAC:
            n, w = o["wrench"].shape[0], self.c1 if form == "local_jacobian_c1" else w
            rc = L.pfc_local_jacobian(h, n, _ptr(a["ins_ids"]), _ptr(np.ascontiguousarray(w.pose[:n])), _ptr(np.ascontiguousarray(w.twist[:n])),
                                      _ptr(a["s"]), *out)
        elif form == "apply":
            rc = L.pfc_apply_local_jacobian(h, 3, 1, _ptr(self.L), _ptr(self.seed[0]), _ptr(self.seed[1]), _ptr(a["d_s"]), *out)
        elif form == "scatter":
            rc = L.pfc_scatter_generalized(h, 5, _ptr(s["wrench"]), _ptr(s["x_w_r2"]), _ptr(s["body_1"]), _ptr(s["body_2"]), _ptr(a["scene"]),
                                           N_SCENE, N_BODY, NV, _ptr(s["jac"]), *out)
        else:
            rc = L.pfc_scatter_generalized_dual(h, 5, 3, _ptr(s["wrench"]), _ptr(s["d_wrench"]), _ptr(s["x_w_r2"]), _ptr(a["d_x_w_r2"]),
                                                _ptr(s["body_1"]), _ptr(s["body_2"]), _ptr(a["scene"]), N_SCENE, N_BODY, NV, _ptr(s["jac"]),
                                                _ptr(a["d_jac"]), *out)
        m._check(rc)
        return {k: v for k, v in o.items() if v is not None}

    def surface(self, pfc, m, fric, drop=(), caps=(64, 512)):
        """pfc_contact_surface[_fric] with the caller's half of the capacity protocol (grow to the totals, call again); the lists cut
        to the totals."""
        L, w, z = pfc._lib.lib(), self.w, np.zeros
        n = w.n_items
        ids, pose, twist, s = _i32(w.ins_ids), np.ascontiguousarray(w.pose), np.ascontiguousarray(w.twist), np.ascontiguousarray(w.s)
        cp, ct = caps
        for attempt in range(2):
            o = dict(poly_off=z(n + 1, np.int64), poly_idx=z((cp, 3), np.int32), poly_xyz=z((cp, 8, 3)), poly_trac=z(cp + 1, np.int64),
                     trac=z((ct, 8)), fric=z((ct, 4)), summary=z((n, 11)), fric_summary=z((n, 20)), stiff=z((n, 84)),
                     counts=z((n, 4), np.int32), totals=z(2, np.int64))
            if not fric:
                for k in ("fric", "fric_summary", "stiff"):
                    del o[k]
            for k in drop:
                o[k] = None
            rc = (L.pfc_contact_surface_fric(m._h, n, _ptr(ids), _ptr(pose), _ptr(twist), _ptr(s), cp, ct, *[_ptr(v) for v in o.values()]) if fric
                  else L.pfc_contact_surface(m._h, n, _ptr(ids), _ptr(pose), _ptr(twist), cp, ct, *[_ptr(v) for v in o.values()]))
            if rc == pfc._lib.ERR_OVERFLOW and attempt == 0:
                cp, ct = max(cp, int(o["totals"][0])), max(ct, int(o["totals"][1]))
                continue
            m._check(rc)
            break
        P, T = int(o["totals"][0]), int(o["totals"][1])
        assert P > 0 and T > 0      # the scene has contact
        cut = dict(poly_idx=P, poly_xyz=P, poly_trac=P + 1, trac=T, fric=T)
        return {k: (v[:cut[k]] if k in cut else v) for k, v in o.items() if v is not None}


# ----------------------------------------------------------------------------------------------------------------
# Host-supplied OBB trees that the library's builders never make (pfc_add_mesh takes any flattened tree, include/pfc.h):
# rotated, dishonest (shrunk) and mixed internal boxes, random and degenerate topologies.  Every generator returns a
# tree of the same container type over the same leaf set, nodes in preorder (node 0 = root, parents before children).
# ----------------------------------------------------------------------------------------------------------------
def _node_axes(tree, k):
    return np.asarray(tree.R[k], dtype=np.float64).reshape(3, 3, order="F")


def _is_internal(tree):
    return np.asarray(tree.child)[:, 0] >= 0


def _random_rotation(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def tree_rotated(tree, rng, fraction=1.0, scale=1.0):
    """Internal nodes (a random `fraction` of them) get a random rotation Q and the extents of the box with those axes
    that encloses the node's own box (same centre): R = Q, e = |Q' A| e for a box with axes A; then e *= scale."""
    c, e, R = tree.c.copy(), tree.e.copy(), tree.R.copy()
    for k in np.nonzero(_is_internal(tree))[0]:
        Q = _random_rotation(rng)               # drawn for every node: the stream does not depend on `fraction`
        if rng.random() >= fraction:
            continue
        e[k] = (np.abs(Q.T @ _node_axes(tree, k)) @ tree.e[k]) * scale
        R[k] = Q.reshape(-1, order="F")
    return type(tree)(c, e, R, tree.child.copy(), tree.leaf.copy())


def tree_shrunk(tree, rng):
    """tree_rotated with the internal extents x 0.7: boxes that do not contain their children.  A pair is tested iff its
    parent pair hit, on the device as in the reference."""
    return tree_rotated(tree, rng, scale=0.7)


def tree_mixed(tree, rng):
    """A random half of the internal nodes rotated, the rest left as they are: waves hold both kinds."""
    return tree_rotated(tree, rng, fraction=0.5)


def tree_identity_twin(tree):
    """The same centres and extents with R := I on every internal node (what a kernel that ignores R on internal
    nodes would see)."""
    R = tree.R.copy()
    R[_is_internal(tree)] = np.eye(3).reshape(-1)
    return type(tree)(tree.c.copy(), tree.e.copy(), R, tree.child.copy(), tree.leaf.copy())


def _leaf_boxes(tree):
    """[(c, e, R9, element)] of the leaves, and their axis-aligned bounds (lo, hi)."""
    out = []
    for k in np.nonzero(~_is_internal(tree))[0]:
        h = np.abs(_node_axes(tree, k)) @ tree.e[k]
        out.append(((tree.c[k].copy(), tree.e[k].copy(), tree.R[k].copy(), int(tree.leaf[k])), tree.c[k] - h, tree.c[k] + h))
    return out


def _flatten(tree, root, internal_code):
    """root: nested (leaf_box, None, None, lo, hi) / (None, left, right, lo, hi) -> preorder arrays (iterative: a chain of
    a hundred levels is a legitimate input)."""
    C_, E_, R_, CH, LF = [], [], [], [], []
    stack = [(root, -1, 0)]
    I9 = np.eye(3).reshape(-1)
    while stack:
        t, parent, side = stack.pop()
        k = len(C_)
        if parent >= 0:
            CH[parent][side] = k
        if t[0] is not None:
            c, e, R9, elem = t[0]
            C_.append(c); E_.append(e); R_.append(R9); CH.append([-1, -1]); LF.append(elem)
        else:
            lo, hi = t[3], t[4]
            C_.append((hi + lo) * 0.5); E_.append((hi - lo) * 0.5); R_.append(I9); CH.append([-1, -1]); LF.append(internal_code)
            stack.append((t[2], k, 1))
            stack.append((t[1], k, 0))
    return type(tree)(np.array(C_), np.array(E_), np.array(R_), np.array(CH, dtype=np.int32), np.array(LF, dtype=np.int32))


def _internal_code(tree):
    ii = np.nonzero(_is_internal(tree))[0]
    return int(tree.leaf[ii[0]]) if ii.size else -9999


def _join(a, b):
    return (None, a, b, np.minimum(a[3], b[3]), np.maximum(a[4], b[4]))


def tree_random_topology(tree, rng):
    """A random binary tree over the leaves of `tree` (their tight boxes kept): two random subtrees are joined until one
    is left; an internal box is the axis-aligned union of its children."""
    forest = [(lb, None, None, lo, hi) for lb, lo, hi in _leaf_boxes(tree)]
    while len(forest) > 1:
        i, j = rng.choice(len(forest), 2, replace=False)
        a, b = forest[i], forest[j]
        forest = [t for k, t in enumerate(forest) if k != i and k != j] + [_join(a, b)]
    return _flatten(tree, forest[0], _internal_code(tree))


def tree_caterpillar(tree, rng):
    """Every internal node has one leaf child (randomly the first or the second) and the rest of the chain as the other:
    depth n_leaf - 1, long runs of leaf x internal descent (tree_types.jl:97-103)."""
    leaves = [(lb, None, None, lo, hi) for lb, lo, hi in _leaf_boxes(tree)]
    order = rng.permutation(len(leaves))
    t = leaves[order[0]]
    for k in order[1:]:
        t = _join(leaves[k], t) if rng.random() < 0.5 else _join(t, leaves[k])
    return _flatten(tree, t, _internal_code(tree))


def single_leaf_mesh(mesh, rng):
    """(mesh of one random element of `mesh`, its one-node tree): the leaf's box is the element's axis-aligned box, as
    the reference leaves it for a single element (blob_types.jl:139-146)."""
    tri = mesh.tri is not None
    elem = mesh.tri if tri else mesh.tet
    idx = elem[int(rng.integers(0, elem.shape[0]))]
    pts = mesh.point[idx]
    one = np.arange(idx.size, dtype=elem.dtype).reshape(1, -1)
    m1 = type(mesh)(pts.copy(), tri=one) if tri else type(mesh)(pts.copy(), tet=one, eps=mesh.eps[idx].copy())
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    return m1, ((hi + lo) * 0.5).reshape(1, 3), ((hi - lo) * 0.5).reshape(1, 3)


HOST_TREE_GENERATORS = {"rotated": tree_rotated, "shrunk": tree_shrunk, "mixed": tree_mixed,
                        "random_topology": tree_random_topology, "caterpillar": tree_caterpillar}
HOST_TREE_SCENES = tuple(HOST_TREE_GENERATORS) + ("single_leaf",)


def host_tree_meshes(pfc, fine=False):
    """The 80-triangle sphere (r 0.3) and the 48-tet box (half-width 0.5) with their built trees; fine: 320 triangles and
    192 tets (512 leaves: a team of four workgroups per item)."""
    G = pfc.geometry
    import tree_reference
    sph = G.as_tri_emesh(G.emesh_sphere(0.3, 4 if fine else 2))
    box = G.as_tet_emesh(G.emesh_box_div(np.array([0.5, 0.5, 0.5]), 4 if fine else 2))
    return sph, tree_reference.build_tree_py(G, sph), box, tree_reference.build_tree_py(G, box)


def host_tree_poses(pfc, rng, n, span):
    """n random relative poses (translations uniform in +-span), twists and bristle states, all non-zero."""
    pose = np.array([pfc.scenario.relative_pose(pfc.configs.random_rotation(rng), rng.uniform(-span, span, 3), np.eye(3), np.zeros(3))
                     for _ in range(n)])
    twist = rng.standard_normal((n, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1])
    return pose, twist, rng.standard_normal((n, 6)) * 1e-3


# translations: the shares of items with and without candidates are asserted by the tests
HOST_TREE_SPAN = {"single_leaf": 0.7}


def host_tree_workload(pfc, scene, n_items, seed=7, fine=False, span=None):
    """One scenario of tests/test_gpu_host_trees.py: the sphere / box pair under the generated trees of `scene`
    ("built": the builder's own), a regularized and a bristle instruction, items alternating between them."""
    G, Cf = pfc.geometry, pfc.configs
    span = HOST_TREE_SPAN.get(scene, 1.0) if span is None else span
    rng = np.random.default_rng([seed, sorted(HOST_TREE_SCENES + ("built",)).index(scene)])
    sph, t1, box, t2 = host_tree_meshes(pfc, fine)
    if scene == "single_leaf":
        # one tet of the box under the whole sphere (a one-triangle mesh would make every bristle patch planar: a stiffness of
        # rank 3, whose sdot is rounding noise in the reference itself, tests/test_sdot_sensitivity.py)
        box, c, e = single_leaf_mesh(box, rng)
        t2 = G.OBBTree(c, e, np.eye(3).reshape(1, 9), np.full((1, 2), -1, dtype=np.int32), np.zeros(1, dtype=np.int32))
        t1 = tree_caterpillar(t1, rng)
    elif scene != "built":
        gen = HOST_TREE_GENERATORS[scene]
        t1, t2 = gen(t1, rng), gen(t2, rng)
    meshes = [Cf.MeshSpec("sphere", sph, t1, None), Cf.MeshSpec("box", box, t2, 1.0e6)]
    ins = [Cf.InsSpec(0, 1, "regularized", chi=0.5, mu_d=0.3, v_tol=1e-2), Cf.InsSpec(0, 1, "bristle", chi=0.3, mu_d=0.4)]
    pose, twist, s = host_tree_poses(pfc, np.random.default_rng(seed), n_items, span)     # the same poses for every scene
    ids = (np.arange(n_items) % 2).astype(np.int32)
    return Cf.Workload("host trees: " + scene, meshes, ins, ids, pose, twist, s)


# ---- the host Dual routes (tests/test_gpu_dual.py::test_host_dual_routes, scripts/dual_routes_dump.py) -------------------------
DUAL_ROUTE_BATCH = 516      # items of the large batch: beyond the one-graph route's 512


def dual_route_scenes(pfc):
    """{name: (Workload, k)}: "boxes" (C1's four regularized items) and "blob" (two bristle poses of a reduced C3), each tiled to
    DUAL_ROUTE_BATCH items with one instruction PER ITEM, so that a call may leave ins_ids out (item i is instruction i) at
    every size.  Item i repeats item i % k: an oracle result of the k distinct items checks the whole batch."""
    Cf = pfc.configs
    out = {}
    for name, base in (("boxes", Cf.c1_boxes()), ("blob", Cf.c3_blob_tool(2, seed=3, n_div_blob=6, n_div_tool=4))):
        k = base.n_items
        reps = DUAL_ROUTE_BATCH // k
        ins = [base.instructions[int(i)] for i in base.ins_ids] * reps
        out[name] = (Cf.Workload(name, base.meshes, ins, np.arange(k * reps, dtype=np.int32), np.tile(base.pose, (reps, 1)),
                                 np.tile(base.twist, (reps, 1)), np.tile(base.s, (reps, 1))), k)
    return out


def dual_route_seeds(w, k, n_dir, seed):
    """(d_pose, d_twist, d_s) of the batch: random seeds of the k distinct items (d_pose tangent to the pose), tiled like the items."""
    from test_oracle_dual import tangents
    rng = np.random.default_rng(seed)
    dq = rng.standard_normal((k, n_dir, 6)) * np.array([1, 1, 1, 0.05, 0.05, 0.05])
    d_pose = np.array([tangents(w.pose[i][:9].reshape(3, 3, order="F"), w.pose[i][9:12], dq[i]) for i in range(k)])
    d_twist = rng.standard_normal((k, n_dir, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1])
    d_s = rng.standard_normal((k, n_dir, 6)) * 1e-3
    reps = w.n_items // k
    return tuple(np.ascontiguousarray(np.tile(a, (reps, 1, 1))) for a in (d_pose, d_twist, d_s))


def dual_route_steps(m, w, seeds, ids_given, s_given):
    """One handle through every host Dual route it can take.  seeds: {"A", "B": 6 directions; "C", "D": 2 directions}
    (dual_route_seeds).  Yields (label, n_items, seed name, result of force_all_elastic_intersections_dual, (pfc_last_parts,
    pfc_last_team, pfc_last_dual_reused)).  The value evaluation in front ends whatever an earlier sequence on the handle kept."""
    import os

    def call(n, name):
        sd = seeds[name]
        out = m.force_all_elastic_intersections_dual(w.pose[:n], w.twist[:n], w.s[:n] if s_given else None, sd[0][:n], sd[1][:n],
                                                     sd[2][:n] if s_given else None, w.ins_ids[:n] if ids_given else None)
        return n, name, out, (m.last_parts(), m.last_team(), int(m.last_dual_reused()))

    m.force_all_elastic_intersections(w.pose[:2], w.twist[:2], w.s[:2] if s_given else None, w.ins_ids[:2] if ids_given else None)
    big = w.n_items
    try:
        yield ("first",) + call(2, "A")
        yield ("repeat",) + call(2, "B")
        yield ("chunk",) + call(2, "A")
        os.environ["PFC_NO_HYBRID"] = "1"
        yield ("one-graph",) + call(2, "B")
        yield ("one-graph chunk",) + call(2, "A")
        os.environ.pop("PFC_NO_HYBRID")
        yield ("one-sync",) + call(big, "C")
        yield ("one-sync chunk",) + call(big, "D")
        os.environ["PFC_DUAL_TWO_STAGE"] = "1"
        yield ("two-stage",) + call(big, "C")
        yield ("two-stage again",) + call(big, "D")
    finally:
        os.environ.pop("PFC_NO_HYBRID", None)
        os.environ.pop("PFC_DUAL_TWO_STAGE", None)
