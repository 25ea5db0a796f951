"""Host-side mirror of the reference's scenario API for the contact hot path.

Same names, argument meaning, defaults and error behaviour as the reference's Julia API (snake_case instead of
the trailing ``!``), restricted to what the hot path needs:

  MechanismScenario()                      src/mechanism_scenario.jl:166-199
  add_contact(name, e_mesh, c_prop=)       :298-314      -> MeshCache (src/structs.jl:33-45)
  add_friction_regularize(id_1, id_2, ..)  :365-377      -> ContactInstructions (:36-49) with Regularized (:22-34)
  add_friction_bristle(id_1, id_2, ..)     :384-399      -> ContactInstructions with Bristle (:5-20)
  finalize()                               :206-231      -> uploads meshes/trees/instructions (pfc_finalize)
  force_all_elastic_intersections(...)     src/contact_algorithms_non_friction.jl:60-84 -> pfc_eval
  contact_surface(pose, twist, ins_ids=)   TractionCache + normal_wrench_cop per item     -> pfc_contact_surface
  contact_surface_fric(pose, twist, s=, ins_ids=)  ... + per-point friction, ṡ, K       -> pfc_contact_surface_fric
  local_jacobian(pose, twist, s=, ins_ids=)        per-item contact Jacobian L (12 x 36)  -> pfc_local_jacobian
  apply_local_jacobian(L, d_pose, d_twist, d_s=)   partials of further seed chunks from L -> pfc_apply_local_jacobian

The rigid-body side of calcXd! (RigidBodyDynamics: poses, twists, Jacobians, mass matrix, third-law scatter)
stays with the host integrator; this class takes the per-instruction relative pose / twist / bristle state that
refreshBodyBodyTransform! / refreshBodyBodyCache! (:103-134) produce and returns the per-instruction wrench, ṡ and
counters.  All compute runs in libpfc_hip (HIP, gfx950); nothing here has a CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np

from . import _lib
from .geometry import EMesh, OBBTree, build_tree

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_llp = C.POINTER(C.c_longlong)


def default_chi() -> float:
    return 0.5          # src/mechanism_scenario.jl:347


def default_mu() -> float:
    return 0.3          # :348


def determine_mu_s_mu_d(mu_s: Optional[float], mu_d: Optional[float]):
    """src/mechanism_scenario.jl:350-356 (the (nothing, nothing) case returns default_χ twice, sic)."""
    if mu_s is None and mu_d is None:
        return default_chi(), default_chi()
    if mu_d is None:
        raise ValueError("need to specify μd")
    if mu_s is None:
        return float(mu_d), float(mu_d)
    if not (mu_d <= mu_s):
        raise ValueError("something is wrong")
    return float(mu_s), float(mu_d)


@dataclass(frozen=True)
class ContactProperties:
    """src/structs.jl:9-15."""
    Ebar: float

    def __post_init__(self):
        if not (1.0e4 <= self.Ebar <= 3.0e11):
            raise ValueError("E_effective in unexpected range.")


@dataclass(frozen=True)
class Regularized:
    """src/mechanism_scenario.jl:22-34."""
    v_c: float
    mu_s: float
    mu_d: float

    @property
    def v_mu_s(self): return 2 * self.v_c
    @property
    def v_mu_d(self): return 3 * self.v_c


@dataclass(frozen=True)
class Bristle:
    """src/mechanism_scenario.jl:5-20."""
    bristle_id: int
    tau: float
    k_bar: float
    mu_s: float
    mu_d: float
    magic: float

    @property
    def Ts_mu_s(self): return 2 * self.mu_s
    @property
    def Ts_mu_d(self): return 3 * self.mu_s


@dataclass
class MeshCache:
    """src/structs.jl:33-45 (BodyID / FrameID stay with the host mechanism)."""
    name: str
    mesh: EMesh
    tree: OBBTree
    c_prop: Optional[ContactProperties]

    @property
    def is_tri(self): return self.mesh.tri is not None
    @property
    def is_tet(self): return self.mesh.tet is not None


@dataclass(frozen=True)
class ContactInstructions:
    """src/mechanism_scenario.jl:36-49."""
    id_1: int
    id_2: int
    chi: float
    friction_model: Union[Regularized, Bristle]
    n_quad_rule: int


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def _i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_ip)


_addressof, _char_from_buffer = C.addressof, C.c_char.from_buffer


def _addr(a):
    """address of a C-contiguous array's first element: through the buffer protocol (0.35 us) where the array is writable,
    through ndarray.ctypes (0.95 us: it builds a helper object per call) where it is not -- seven of these per evaluation
    were two thirds of the general entry point's overhead over BoundEvaluation"""
    try:
        return _addressof(_char_from_buffer(a))
    except (TypeError, ValueError):      # read-only or empty
        return a.ctypes.data


def _da(a):
    """float64 C-contiguous view (no copy when it already is one) and its address"""
    if not (type(a) is np.ndarray and a.dtype == np.float64 and a.flags.c_contiguous):
        a = np.ascontiguousarray(a, dtype=np.float64)
    return a, _addr(a)


def _ia(a):
    if not (type(a) is np.ndarray and a.dtype == np.int32 and a.flags.c_contiguous):
        a = np.ascontiguousarray(a, dtype=np.int32)
    return a, _addr(a)


class BoundEvaluation:
    """force_all_elastic_intersections on buffers that live as long as this object: the inputs are copied once into
    `pose` (n,24), `twist` (n,6), `s` (n,6 or None) -- change them IN PLACE between calls -- and every call overwrites
    `wrench` (n,6), `sdot` (n,6), `counts` (n,4) and returns them.  One foreign call per evaluation with prebuilt
    arguments: the ~10 us of array checks and allocations of the general entry point (a quarter of a one-box scene's
    40 us) are paid once here."""

    def __init__(self, scenario: "MechanismScenario", pose, twist, s=None, ins_ids=None):
        self._m = scenario
        self.pose = np.array(pose, dtype=np.float64, order="C").reshape(-1, 24)
        n = self.pose.shape[0]
        self.twist = np.array(twist, dtype=np.float64, order="C").reshape(-1, 6)
        if self.twist.shape[0] != n:
            raise ValueError("twist must have 6 entries per item")
        self.s = None
        if s is not None:
            self.s = np.array(s, dtype=np.float64, order="C").reshape(-1, 6)
            if self.s.shape[0] != n:
                raise ValueError("s must have 6 entries per item")
        self.ins_ids = None
        if ins_ids is not None:
            self.ins_ids = np.array(ins_ids, dtype=np.int32, order="C").reshape(-1)
            if self.ins_ids.size != n:
                raise ValueError("ins_ids must have one entry per item")
        self.wrench = np.zeros((n, 6)); self.sdot = np.zeros((n, 6)); self.counts = np.zeros((n, 4), dtype=np.int32)
        self._fn = _lib.lib().pfc_eval_addr
        # (the handle is NOT captured: after MechanismScenario.close() a call must raise, not hand a freed handle to the library)
        self._args = (n, None if self.ins_ids is None else self.ins_ids.ctypes.data, self.pose.ctypes.data,
                      self.twist.ctypes.data, None if self.s is None else self.s.ctypes.data, self.wrench.ctypes.data,
                      self.sdot.ctypes.data, self.counts.ctypes.data)

    def __call__(self):
        h = self._m._h
        if h is None:
            raise RuntimeError("the scenario of this BoundEvaluation has been closed")
        rc = self._fn(h, *self._args)
        if rc != 0:
            self._m._check(rc)
        return self.wrench, self.sdot, self.counts


@dataclass(eq=False)
class ContactSurface:
    """The contact surface of n items (pfc_contact_surface), frame r2 of every item:

    poly_off  (n+1,)    int64    the polygons of item i are poly_off[i] : poly_off[i+1]
    poly_idx  (P, 3)    int32    element of mesh_1, element of mesh_2, vertex count (3..8); ascending pairs within an item
    poly_xyz  (P, 8, 3) float64  vertices, unused slots 0
    poly_trac (P+1,)    int64    the traction points of polygon k are poly_trac[k] : poly_trac[k+1]
    trac      (T, 8)    float64  TractionCache entries n̂ (3), r (3), dA, p -- in the reference's fan and quadrature order
    summary   (n, 11)   float64  normal wrench [ang 3; lin 3] about the r2 origin, cop (3), sum p dA, sum dA; zeros without points
    counts    (n, 4)    int32    as force_all_elastic_intersections'
    """

    poly_off: np.ndarray
    poly_idx: np.ndarray
    poly_xyz: np.ndarray
    poly_trac: np.ndarray
    trac: np.ndarray
    summary: np.ndarray
    counts: np.ndarray

    def __post_init__(self):
        for f in ("poly_off", "poly_idx", "poly_xyz", "poly_trac", "trac", "summary", "counts"):
            setattr(self, f, np.asarray(getattr(self, f)))
        n = self.poly_off.shape[0] - 1 if self.poly_off.ndim == 1 else -1
        P, T = self.poly_idx.shape[0] if self.poly_idx.ndim == 2 else -1, self.trac.shape[0] if self.trac.ndim == 2 else -1
        if n < 0:
            raise ValueError("poly_off must be a vector of n_items + 1 offsets")
        if self.poly_idx.shape != (P, 3) or P < 0:
            raise ValueError("poly_idx must be (P, 3)")
        if self.poly_xyz.shape != (P, 8, 3):
            raise ValueError("poly_xyz must be (P, 8, 3)")
        if self.poly_trac.shape != (P + 1,):
            raise ValueError("poly_trac must have P + 1 offsets")
        if self.trac.shape != (T, 8) or T < 0:
            raise ValueError("trac must be (T, 8)")
        if self.summary.shape != (n, 11):
            raise ValueError("summary must be (n_items, 11)")
        if self.counts.shape != (n, 4):
            raise ValueError("counts must be (n_items, 4)")
        if int(self.poly_off[0]) != 0 or int(self.poly_off[-1]) != P or int(self.poly_trac[0]) != 0 or int(self.poly_trac[-1]) != T:
            raise ValueError("offsets do not cover the polygon and traction arrays")

    @property
    def n_items(self) -> int:
        return self.poly_off.shape[0] - 1

    def item(self, i: int) -> dict:
        """Views of item i: keys (m, 2) element pairs, n_vert (m,), xyz (m, 8, 3), poly_trac (m + 1,) offsets into its own trac,
        trac (t, 8), wrench (6,), cop (3,), sum_p_dA, area, counts (4,)."""
        if not 0 <= i < self.n_items:
            raise IndexError(i)
        p0, p1 = int(self.poly_off[i]), int(self.poly_off[i + 1])
        t0, t1 = int(self.poly_trac[p0]), int(self.poly_trac[p1])
        s = self.summary[i]
        return dict(keys=self.poly_idx[p0:p1, :2], n_vert=self.poly_idx[p0:p1, 2], xyz=self.poly_xyz[p0:p1],
                    poly_trac=self.poly_trac[p0:p1 + 1] - t0, trac=self.trac[t0:t1], wrench=s[0:6], cop=s[6:9],
                    sum_p_dA=float(s[9]), area=float(s[10]), counts=self.counts[i])


@dataclass(eq=False)
class FrictionSurface:
    """The contact surface with its friction half (pfc_contact_surface_fric), frame r2 of every item:

    surface       ContactSurface           what contact_surface returns for the same inputs, byte for byte
    fric          (T, 4)   float64  per traction point (surface.trac order): T_c (3) = traction() times p dA, branch (0.0 the first)
    fric_summary  (n, 20)  float64  total wrench [ang 3; lin 3] about the r2 origin (= summary[0:6] + friction wrench), friction
                                    wrench (6), ṡ (6), first-branch sum p dA, first-branch count
    stiff         (n, 84)  float64  K (36, column-major), K̄^{-1/2} (36), diag S⁻¹ (6), Δ² (6); zeros unless bristle with points
    """

    surface: ContactSurface
    fric: np.ndarray
    fric_summary: np.ndarray
    stiff: np.ndarray

    def __post_init__(self):
        if not isinstance(self.surface, ContactSurface):
            raise ValueError("surface must be a ContactSurface")
        for f in ("fric", "fric_summary", "stiff"):
            setattr(self, f, np.asarray(getattr(self, f)))
        n, T = self.surface.n_items, self.surface.trac.shape[0]
        if self.fric.shape != (T, 4):
            raise ValueError("fric must be (T, 4): one row per traction point")
        if self.fric_summary.shape != (n, 20):
            raise ValueError("fric_summary must be (n_items, 20)")
        if self.stiff.shape != (n, 84):
            raise ValueError("stiff must be (n_items, 84)")

    @property
    def n_items(self) -> int:
        return self.surface.n_items

    def item(self, i: int) -> dict:
        """ContactSurface.item(i), and: fric (t, 4), total_wrench (6,), fric_wrench (6,), sdot (6,), first_p_dA, n_first,
        K (6, 6), Kbar_inv_sqrt (6, 6), Sinv (6,), Delta (6,)."""
        d = self.surface.item(i)
        S = self.surface
        p0, p1 = int(S.poly_off[i]), int(S.poly_off[i + 1])
        t0, t1 = int(S.poly_trac[p0]), int(S.poly_trac[p1])
        f, k = self.fric_summary[i], self.stiff[i]
        d.update(fric=self.fric[t0:t1], total_wrench=f[0:6], fric_wrench=f[6:12], sdot=f[12:18], first_p_dA=float(f[18]),
                 n_first=int(f[19]), K=k[0:36].reshape(6, 6, order="F"), Kbar_inv_sqrt=k[36:72].reshape(6, 6, order="F"),
                 Sinv=k[72:78], Delta=k[78:84])
        return d


@dataclass(eq=False)
class BodyItems:
    """What MechanismScenario.items_from_bodies returns: the per-item inputs of the evaluation and of the third-law scatter."""
    pose: np.ndarray        # (n,24) x_r2_r1 then x_r1_r2
    twist: np.ndarray       # (n,6) twist_r2_r1_r2
    x_w_r2: np.ndarray      # (n,12) x_rw_r2
    body_1: np.ndarray      # (n,) int32: body of mesh_1 (-1: the world), offset by scene * n_body when scenes are given
    body_2: np.ndarray


@dataclass(eq=False)
class BodySeeds:
    """What MechanismScenario.dual_seeds_from_bodies returns: the partials of BodyItems' pose, twist and x_w_r2 per seed direction."""
    d_pose: np.ndarray      # (n,n_dir,24) partials of x_r2_r1 then x_r1_r2
    d_twist: np.ndarray     # (n,n_dir,6) partials of twist_r2_r1_r2
    d_x_w_r2: np.ndarray    # (n,n_dir,12) partials of x_rw_r2

    def __iter__(self):
        return iter((self.d_pose, self.d_twist, self.d_x_w_r2))


class MechanismScenario:
    """Contact part of MechanismScenario{T} (src/mechanism_scenario.jl:166-199), backed by a pfc_handle."""

    def __init__(self, device: int = 0, devices: Optional[Sequence[int]] = None):
        """device: the HIP device of the scenario; devices: a list of HIP devices instead (pfc_create_multi: the one host
        process uses them all, items are cut into ranges per device inside the library)."""
        self.MeshCache: List[MeshCache] = []
        self.ContactInstructions: List[ContactInstructions] = []
        self.n_bristle = 0
        self.device = device
        self.devices = None if devices is None else [int(d) for d in devices]
        self._h = None
        self._finalized = False
        self._ins_bodies = {}        # bindings made before finalize(): the handle does not exist yet
        self._mechanism = None       # set_mechanism's tables, likewise
        self._inertia = None         # set_inertia's, likewise (dropped by a later set_mechanism, as the library drops them)

    # ---- scenario construction ---------------------------------------------------------------------------------
    def add_contact(self, name: str, e_mesh: EMesh, c_prop: Optional[ContactProperties] = None,
                    tree: Optional[OBBTree] = None) -> int:
        """add_contact! (:298-314).  Returns the mesh id (0-based)."""
        if self._finalized:
            raise RuntimeError("add_contact after finalize")
        # verify_eMesh_ContactProperties (:301-306)
        if e_mesh.tri is not None and e_mesh.tet is not None:
            raise ValueError("eMesh has triangles and tets. Use as_tri_eMesh or as_tet_eMesh to convert eMesh.")
        if e_mesh.tri is not None and c_prop is not None:
            raise ValueError("Using ContactProperties for triangular eMesh")
        if e_mesh.tet is not None and c_prop is None:
            raise ValueError("Using nothing as ContactProperties for tet eMesh")
        if tree is None:
            tree = build_tree(e_mesh)           # eMesh_to_tree (:309)
        self.MeshCache.append(MeshCache(name, e_mesh, tree, c_prop))
        return len(self.MeshCache) - 1

    def find_mesh_id(self, name: str) -> int:
        """src/utility.jl:22-33."""
        ids = [k for k, m in enumerate(self.MeshCache) if m.name == name]
        if len(ids) > 1:
            raise KeyError("multiple")
        if not ids:
            raise KeyError(f"no mesh found by name: {name}")
        return ids[0]

    def _add_friction(self, id_1: int, id_2: int, model, chi: float, n_quad_rule: int) -> ContactInstructions:
        """add_friction! (:402-416): id_1 becomes the triangle mesh (or a tet mesh), id_2 is always a tet mesh."""
        m_1, m_2 = self.MeshCache[id_1], self.MeshCache[id_2]
        if m_1.is_tet and m_2.is_tri:
            id_1, id_2 = id_2, id_1
            m_1, m_2 = m_2, m_1
        if not m_2.is_tet:
            raise TypeError("no method matching add_friction!(tri, tri): one mesh must be a tet mesh")
        if not (1 <= n_quad_rule <= 2):
            raise ValueError("only quadrature rules 1 (first order) and 2 (second? order) are currently implemented")
        c = ContactInstructions(id_1, id_2, float(chi), model, int(n_quad_rule))
        self.ContactInstructions.append(c)
        return c

    def add_friction_regularize(self, mesh_id_1: int, mesh_id_2: int, mu_s=None, mu_d=None, chi: float = None,
                                v_tol: float = 0.01, n_quad_rule: int = 2) -> ContactInstructions:
        """add_friction_regularize! (:365-377)."""
        if self._finalized:
            raise RuntimeError("add_friction after finalize")
        chi = default_chi() if chi is None else chi
        mu_s, mu_d = determine_mu_s_mu_d(mu_s, mu_d)
        return self._add_friction(mesh_id_1, mesh_id_2, Regularized(float(v_tol), mu_s, mu_d), chi, n_quad_rule)

    def add_friction_bristle(self, mesh_id_1: int, mesh_id_c: int, tau: float = 0.05, k_bar: float = 1.0e4,
                             mu_s=None, mu_d=None, chi: float = None, n_quad_rule: int = 2,
                             magic: float = 1.0e-3) -> ContactInstructions:
        """add_friction_bristle! (:384-399)."""
        if self._finalized:
            raise RuntimeError("add_friction after finalize")
        chi = default_chi() if chi is None else chi
        mu_s, mu_d = determine_mu_s_mu_d(mu_s, mu_d)
        if not (0 < mu_d):
            raise ValueError("μd cannot be 0 for bristle friction")
        b = Bristle(self.n_bristle, float(tau), float(k_bar), mu_s, mu_d, float(magic))
        c = self._add_friction(mesh_id_1, mesh_id_c, b, chi, n_quad_rule)
        self.n_bristle += 1
        return c

    # ---- device ------------------------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != _lib.OK:
            msg = _lib.lib().pfc_last_error(self._h).decode() if self._h else ""
            raise _lib.PFCError(rc, msg)

    def _id(self, rc: int) -> int:
        if rc < 0:
            self._check(-rc)
        return rc

    def finalize(self):
        """finalize! (:206-231): upload every MeshCache and ContactInstructions, build device tables."""
        if self._finalized:
            raise RuntimeError("finalize called twice")
        L = _lib.lib()
        h = C.c_void_p()
        if self.devices is not None:
            dv = (C.c_int * len(self.devices))(*self.devices)
            rc = L.pfc_create_multi(dv, len(self.devices), C.byref(h))
        else:
            rc = L.pfc_create(self.device, C.byref(h))
        if rc != _lib.OK:
            raise _lib.PFCError(rc, "pfc_create failed: no usable HIP device (there is no CPU fallback)")
        self._h = h
        for m in self.MeshCache:
            keep = []
            p, pp = _d(m.mesh.point); keep.append(p)
            tri_p = tet_p = eps_p = None
            n_tri = n_tet = 0
            if m.is_tri:
                a, tri_p = _i(m.mesh.tri); keep.append(a); n_tri = m.mesh.n_tri
            else:
                a, tet_p = _i(m.mesh.tet); keep.append(a); n_tet = m.mesh.n_tet
                a, eps_p = _d(m.mesh.eps); keep.append(a)
            t = m.tree
            c, cp = _d(t.c); e, ep = _d(t.e); R, Rp = _d(t.R); ch, chp = _i(t.child); lf, lfp = _i(t.leaf)
            self._id(L.pfc_add_mesh(h, m.mesh.n_point, pp, n_tri, tri_p, n_tet, tet_p, eps_p,
                                    m.c_prop.Ebar if m.c_prop else 0.0, t.n_node, cp, ep, Rp, chp, lfp))
        for c in self.ContactInstructions:
            f = c.friction_model
            if isinstance(f, Regularized):
                par, model = [f.mu_s, f.mu_d, f.v_c, 0, 0, 0, 0, 0], _lib.REGULARIZED
            else:
                par, model = [f.mu_s, f.mu_d, f.tau, f.k_bar, f.magic, 0, 0, 0], _lib.BRISTLE
            a, ap = _d(par)
            self._id(L.pfc_add_instruction(h, c.id_1, c.id_2, c.chi, c.n_quad_rule, model, ap))
        self._check(L.pfc_finalize(h))
        self._finalized = True
        for ins, (b1, b2) in self._ins_bodies.items():
            self._check(L.pfc_set_instruction_bodies(h, ins, b1, b2))
        if self._mechanism is not None:
            self._send_mechanism()
            if self._inertia is not None:
                self._send_inertia()

    def set_mechanism(self, parent, joint_type, x_p_j, axis=None):
        """pfc_set_mechanism: the tree the kinematics calls below evaluate.  Body b is the successor of joint b; parent (n_body,) in
        [-1, b), -1 the world; joint_type (n_body,) of _lib.JOINT_FIXED / JOINT_REVOLUTE / JOINT_PRISMATIC / JOINT_FLOATING_MRP;
        x_p_j (n_body,12) the joint_pose, R column-major then t; axis (n_body,3) in the joint frame (None: no revolute or prismatic
        joint).  Before or after finalize(); a second call replaces the first."""
        parent = np.ascontiguousarray(parent, dtype=np.int32).reshape(-1)
        n_body = parent.size
        joint_type = np.ascontiguousarray(joint_type, dtype=np.int32).reshape(-1)
        x_p_j = np.ascontiguousarray(x_p_j, dtype=np.float64).reshape(-1)
        axis = np.zeros(3 * n_body) if axis is None else np.ascontiguousarray(axis, dtype=np.float64).reshape(-1)
        if joint_type.size != n_body or x_p_j.size != 12 * n_body or axis.size != 3 * n_body:
            raise ValueError("set_mechanism: one parent, joint type, joint_pose (12) and axis (3) per body")
        mech = (n_body, parent, joint_type, x_p_j, axis)
        self._inertia = None
        if not self._finalized:
            self._mechanism = mech      # sent by finalize(): the library validates it there
            return
        self._send_mechanism(mech)

    def _send_mechanism(self, mech=None):
        n_body, parent, joint_type, x_p_j, axis = mech or self._mechanism
        L = _lib.lib()
        self._check(L.pfc_set_mechanism(self._h, n_body, parent.ctypes.data_as(_ip), joint_type.ctypes.data_as(_ip),
                                        x_p_j.ctypes.data_as(_dp), axis.ctypes.data_as(_dp)))
        self._mechanism = mech or self._mechanism

    def set_inertia(self, inertia, gravity=(0.0, 0.0, -9.81)):
        """pfc_set_inertia: the bodies' spatial inertias in their own frames, (n_body,13) = moment (9, column-major, about the frame
        origin), cross_part = m com (3), mass (1) -- geometry.mesh_inertia's record -- and gravity (3) in world.  After
        set_mechanism; a later set_mechanism drops them."""
        if self._mechanism is None:
            raise RuntimeError("set_mechanism first")
        inertia = np.ascontiguousarray(inertia, dtype=np.float64).reshape(-1)
        gravity = np.ascontiguousarray(gravity, dtype=np.float64).reshape(-1)
        if inertia.size % 13 or gravity.size != 3:
            raise ValueError("set_inertia: 13 doubles per body and a gravity vector")
        self._inertia = (inertia.size // 13, inertia, gravity)
        if self._finalized:
            self._send_inertia()

    def _send_inertia(self):
        n_body, inertia, gravity = self._inertia
        self._check(_lib.lib().pfc_set_inertia(self._h, n_body, inertia.ctypes.data_as(_dp), gravity.ctypes.data_as(_dp)))

    def mechanism_sizes(self):
        """pfc_mechanism_sizes: (n_body, nq, nv) of the mechanism the library holds."""
        if not self._finalized:
            raise RuntimeError("finalize the scenario first")
        nb, nq, nv = C.c_int(), C.c_int(), C.c_int()
        self._check(_lib.lib().pfc_mechanism_sizes(self._h, C.byref(nb), C.byref(nq), C.byref(nv)))
        return nb.value, nq.value, nv.value

    def set_instruction_bodies(self, ins: int, body_1: int, body_2: int):
        """pfc_set_instruction_bodies: instruction `ins` (0-based, the order of the add_friction_* calls) acts between body_1 (of
        its mesh_1) and body_2 (of its mesh_2); -1 is the world.  Before or after finalize(); a second call overwrites."""
        ins, body_1, body_2 = int(ins), int(body_1), int(body_2)
        if not (0 <= ins < len(self.ContactInstructions)) or body_1 < -1 or body_2 < -1:
            raise ValueError("set_instruction_bodies: an instruction of the scenario and body ids >= -1")
        self._ins_bodies[ins] = (body_1, body_2)
        if self._finalized:
            self._check(_lib.lib().pfc_set_instruction_bodies(self._h, ins, body_1, body_2))

    def close(self):
        if self._h is not None:
            _lib.lib().pfc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name: str, value: int):
        self._check(_lib.lib().pfc_set_option(self._h, name.encode(), int(value)))

    # ---- evaluation --------------------------------------------------------------------------------------------
    def force_all_elastic_intersections(self, pose, twist, s=None, ins_ids: Optional[Sequence[int]] = None):
        """forceAllElasticIntersections! without the RigidBodyDynamics parts (host buffers, synchronous).

        pose (n,24), twist (n,6), s (n,6) or None, ins_ids (n,) or None (item i = instruction i).
        Returns (wrench (n,6), sdot (n,6), counts (n,4))."""
        if not self._finalized:
            raise RuntimeError("finalize the scenario first")
        pose_a, pose_p = _da(pose)
        n = pose_a.size // 24
        tw_a, tw_p = _da(twist)
        if tw_a.size != 6 * n:
            raise ValueError("twist must have 6 entries per item")
        s_p = None
        if s is not None:
            s_a, s_p = _da(s)
            if s_a.size != 6 * n:
                raise ValueError("s must have 6 entries per item")
        id_p = None
        if ins_ids is not None:
            id_a, id_p = _ia(ins_ids)
            if id_a.size != n:
                raise ValueError("ins_ids must have one entry per item")
        wrench = np.zeros((n, 6)); sdot = np.zeros((n, 6)); counts = np.zeros((n, 4), dtype=np.int32)
        rc = _lib.lib().pfc_eval_addr(self._h, n, id_p, pose_p, tw_p, s_p, _addr(wrench), _addr(sdot), _addr(counts))
        if rc != 0:
            self._check(rc)
        return wrench, sdot, counts

    def bind(self, pose, twist, s=None, ins_ids: Optional[Sequence[int]] = None) -> "BoundEvaluation":
        """Persistent buffers for a scene that is evaluated again and again (what TypedElasticBodyBodyCache's preallocated
        arrays are to calcXd!, src/mechanism_scenario.jl:78-97): see BoundEvaluation."""
        if not self._finalized:
            raise RuntimeError("finalize the scenario first")
        return BoundEvaluation(self, pose, twist, s, ins_ids)

    def force_all_elastic_intersections_dual(self, pose, twist, s, d_pose, d_twist, d_s=None,
                                             ins_ids: Optional[Sequence[int]] = None, bp_pose=None):
        """The evaluation on Dual numbers (MechanismScenario.dual, src/mechanism_scenario.jl:187): values plus, for
        each of n_dir seed directions, the partials.  d_pose (n, n_dir, 24), d_twist (n, n_dir, 6), d_s (n, n_dir, 6)
        or None.  bp_pose (n, 24) or None: the pose the broadphase culls with -- the reference takes m.float's
        (calcTriTetIntersections!, src/contact_algorithms_non_friction.jl:94-101), i.e. the pose of the last Float64
        evaluation; None = pose.  Returns (wrench, sdot, d_wrench (n, n_dir, 6), d_sdot (n, n_dir, 6), counts)."""
        if not self._finalized:
            raise RuntimeError("finalize the scenario first")
        pose_a, pose_p = _da(pose)
        n = pose_a.size // 24
        tw_a, tw_p = _da(twist)
        dp_a, dp_p = _da(d_pose)
        if n == 0 or dp_a.size % (24 * n) != 0:
            raise ValueError("d_pose must be (n, n_dir, 24)")
        n_dir = dp_a.size // (24 * n)
        dt_a, dt_p = _da(d_twist)
        if tw_a.size != 6 * n or dt_a.size != 6 * n * n_dir:
            raise ValueError("twist must be (n, 6) and d_twist (n, n_dir, 6)")
        s_p = ds_p = id_p = None
        if s is not None:
            s_a, s_p = _da(s)
            if s_a.size != 6 * n:
                raise ValueError("s must have 6 entries per item")
        if d_s is not None:
            ds_a, ds_p = _da(d_s)
            if ds_a.size != 6 * n * n_dir:
                raise ValueError("d_s must be (n, n_dir, 6)")
        if ins_ids is not None:
            id_a, id_p = _ia(ins_ids)
            if id_a.size != n:
                raise ValueError("ins_ids must have one entry per item")
        wrench = np.zeros((n, 6)); sdot = np.zeros((n, 6)); counts = np.zeros((n, 4), dtype=np.int32)
        dw = np.zeros((n, n_dir, 6)); dsd = np.zeros((n, n_dir, 6))
        if bp_pose is not None:
            bp_a, bp_p = _da(bp_pose)
            if bp_a.size != 24 * n:
                raise ValueError("bp_pose must have 24 entries per item")
            rc = _lib.lib().pfc_eval_dual_bp_addr(self._h, n, n_dir, id_p, pose_p, bp_p, tw_p, s_p, dp_p, dt_p, ds_p, _addr(wrench),
                                                  _addr(sdot), _addr(dw), _addr(dsd), _addr(counts))
        else:
            rc = _lib.lib().pfc_eval_dual_addr(self._h, n, n_dir, id_p, pose_p, tw_p, s_p, dp_p, dt_p, ds_p, _addr(wrench),
                                               _addr(sdot), _addr(dw), _addr(dsd), _addr(counts))
        if rc != 0:
            self._check(rc)
        return wrench, sdot, dw, dsd, counts

    def scatter_generalized(self, wrench, x_w_r2, body_1, body_2, jac, scene=None, n_scene: int = 1):
        """addGeneralizedForcesThirdLaw! for all items (non_friction.jl:267-286) on the device.
        wrench (n,6); x_w_r2 (n,12) = R col-major + t; body_1/body_2 (n,) body ids (-1: no Jacobian);
        jac (n_body, nv, 6): per body and velocity coordinate [angular 3; linear 3]; returns f (n_scene, nv)."""
        w_a, w_p = _d(wrench); x_a, x_p = _d(x_w_r2)
        b1_a, b1_p = _i(body_1); b2_a, b2_p = _i(body_2)
        j_a, j_p = _d(jac)
        n = w_a.size // 6
        n_body, nv = (int(np.shape(jac)[0]), int(np.shape(jac)[1])) if np.ndim(jac) == 3 else (0, 0)
        sc_p = None
        if scene is not None:
            sc_a, sc_p = _i(scene)
        f = np.zeros((n_scene, nv))
        self._check(_lib.lib().pfc_scatter_generalized(self._h, n, w_p, x_p, b1_p, b2_p, sc_p, n_scene, n_body, nv, j_p,
                                                       f.ctypes.data_as(_dp)))
        return f

    def scatter_generalized_device(self, n_items: int, d_wrench: int, d_x_w_r2: int, d_body_1: int, d_body_2: int, d_scene: int,
                                   n_scene: int, nv: int, d_jac: int, d_f: int, accumulate: bool = False, stream: int = 0):
        """pfc_scatter_generalized_device: raw device addresses, asynchronous on `stream`; f_generalized stays in HBM."""
        self._check(_lib.lib().pfc_scatter_generalized_device(self._h, int(n_items), d_wrench, d_x_w_r2, d_body_1, d_body_2,
                                                              d_scene or None, int(n_scene), int(nv), d_jac, d_f,
                                                              1 if accumulate else 0, stream or None))

    def scatter_generalized_dual(self, wrench, d_wrench, x_w_r2, d_x_w_r2, body_1, body_2, jac, d_jac, scene=None,
                                 n_scene: int = 1):
        """addGeneralizedForcesThirdLaw! on Dual numbers (pfc_scatter_generalized_dual): arguments as scatter_generalized, plus
        d_wrench (n, n_dir, 6), d_x_w_r2 (n, n_dir, 12) or None, d_jac (n_body, n_dir, nv, 6) or None (None: constant).
        Sums run over each scene's items in item order, so the result is the same bytes on every call.
        Returns (f (n_scene, nv), d_f (n_scene, n_dir, nv))."""
        w_a, w_p = _d(wrench); x_a, x_p = _d(x_w_r2)
        n = w_a.size // 6
        dw_a, dw_p = _d(d_wrench)
        if n == 0:
            n_dir = int(np.shape(d_wrench)[1]) if np.ndim(d_wrench) == 3 else 0
        elif dw_a.size % (6 * n) != 0:
            raise ValueError("d_wrench must be (n, n_dir, 6)")
        else:
            n_dir = dw_a.size // (6 * n)
        if w_a.size != 6 * n or x_a.size != 12 * n:
            raise ValueError("wrench must be (n, 6) and x_w_r2 (n, 12)")
        b1_a, b1_p = _i(body_1); b2_a, b2_p = _i(body_2)
        if b1_a.size != n or b2_a.size != n:
            raise ValueError("body_1 and body_2 must have one entry per item")
        j_a, j_p = _d(jac)
        if j_a.ndim != 3 or j_a.shape[2] != 6:
            raise ValueError("jac must be (n_body, nv, 6)")
        n_body, nv = j_a.shape[0], j_a.shape[1]
        dx_p = dj_p = sc_p = None
        if d_x_w_r2 is not None:
            dx_a, dx_p = _d(d_x_w_r2)
            if dx_a.size != 12 * n * n_dir:
                raise ValueError("d_x_w_r2 must be (n, n_dir, 12)")
        if d_jac is not None:
            dj_a, dj_p = _d(d_jac)
            if dj_a.size != n_body * n_dir * nv * 6:
                raise ValueError("d_jac must be (n_body, n_dir, nv, 6)")
        if scene is not None:
            sc_a, sc_p = _i(scene)
            if sc_a.size != n:
                raise ValueError("scene must have one entry per item")
        f = np.zeros((n_scene, nv)); d_f = np.zeros((n_scene, n_dir, nv))
        self._check(_lib.lib().pfc_scatter_generalized_dual(self._h, n, n_dir, w_p, dw_p, x_p, dx_p, b1_p, b2_p, sc_p, n_scene, n_body,
                                                            nv, j_p, dj_p, f.ctypes.data_as(_dp), d_f.ctypes.data_as(_dp)))
        return f, d_f

    def scatter_generalized_dual_device(self, n_items: int, n_dir: int, d_wrench: int, d_dwrench: int, d_x_w_r2: int,
                                        d_dx_w_r2: int, d_body_1: int, d_body_2: int, d_scene: int, n_scene: int, nv: int, d_jac: int,
                                        d_djac: int, d_f: int, d_df: int, accumulate: bool = False, stream: int = 0):
        """pfc_scatter_generalized_dual_device: raw device addresses (0: NULL for d_dx_w_r2, d_scene, d_djac, d_f), asynchronous
        on `stream`; f_generalized and its partials stay in HBM."""
        self._check(_lib.lib().pfc_scatter_generalized_dual_device(
            self._h, int(n_items), int(n_dir), d_wrench, d_dwrench, d_x_w_r2, d_dx_w_r2 or None, d_body_1, d_body_2, d_scene or None,
            int(n_scene), int(nv), d_jac, d_djac or None, d_f or None, d_df, 1 if accumulate else 0, stream or None))

    def eval_device(self, n_items: int, d_ins_ids: int, d_pose: int, d_twist: int, d_s: int, d_wrench: int,
                    d_sdot: int, d_counts: int, stream: int = 0):
        """pfc_eval_device: raw device addresses (e.g. torch.Tensor.data_ptr()); asynchronous."""
        self._check(_lib.lib().pfc_eval_device(self._h, int(n_items), d_ins_ids or None, d_pose, d_twist,
                                               d_s or None, d_wrench, d_sdot, d_counts or None, stream or None))

    def eval_dual_device(self, n_items: int, n_dir: int, d_ins_ids: int, d_pose: int, d_twist: int, d_s: int, d_dpose: int,
                         d_dtwist: int, d_ds: int, d_wrench: int, d_sdot: int, d_dwrench: int, d_dsdot: int, d_counts: int,
                         stream: int = 0, d_bp_pose: int = 0):
        """pfc_eval_dual_device[_bp]: raw device addresses; asynchronous; follow with check() (re-issue on ERR_OVERFLOW)."""
        self._check(_lib.lib().pfc_eval_dual_device_bp(self._h, int(n_items), int(n_dir), d_ins_ids or None, d_pose, d_bp_pose or None,
                                                       d_twist, d_s or None, d_dpose, d_dtwist, d_ds or None, d_wrench, d_sdot,
                                                       d_dwrench, d_dsdot, d_counts or None, stream or None))

    def eval_dual_device_more(self, n_dir: int, d_dpose: int, d_dtwist: int, d_ds: int, d_dwrench: int, d_dsdot: int,
                              stream: int = 0):
        """pfc_eval_dual_device_more: further seed directions at the point of the previous eval_dual_device evaluation
        (the chunks of one Jacobian); only the Dual passes run.  Follow with check()."""
        self._check(_lib.lib().pfc_eval_dual_device_more(self._h, int(n_dir), d_dpose, d_dtwist, d_ds or None, d_dwrench,
                                                         d_dsdot, stream or None))

    def local_jacobian(self, pose, twist, s=None, ins_ids: Optional[Sequence[int]] = None):
        """The contact Jacobian of every item at (pose, twist, s) (pfc_local_jacobian): [d_wrench; d_sdot] = L . [d_pose; d_twist; d_s]
        for any seeds at this point.  Returns (wrench (n,6), sdot (n,6), L (n,12,36), counts (n,4)); L's rows are the wrench
        [ang; lin] then ṡ, its columns the 24 pose numbers (pose packing), twist 6 and s 6.  The handle may then extend this point
        with eval_dual_device_more / local_jacobian_device."""
        if not self._finalized:
            raise RuntimeError("finalize the scenario first")
        pose_a, pose_p = _da(pose)
        n = pose_a.size // 24
        if pose_a.size != 24 * n:
            raise ValueError("pose must have 24 entries per item")
        tw_a, tw_p = _da(twist)
        if tw_a.size != 6 * n:
            raise ValueError("twist must have 6 entries per item")
        s_p = id_p = None
        if s is not None:
            s_a, s_p = _d(s)
            if s_a.size != 6 * n:
                raise ValueError("s must have 6 entries per item")
        if ins_ids is not None:
            id_a, id_p = _i(ins_ids)
            if id_a.size != n:
                raise ValueError("ins_ids must have one entry per item")
        wrench = np.zeros((n, 6)); sdot = np.zeros((n, 6)); L = np.zeros((n, 12, 36)); counts = np.zeros((n, 4), dtype=np.int32)
        self._check(_lib.lib().pfc_local_jacobian(self._h, n, id_p, pose_a.ctypes.data_as(_dp), tw_a.ctypes.data_as(_dp), s_p,
                                                  wrench.ctypes.data_as(_dp), sdot.ctypes.data_as(_dp), L.ctypes.data_as(_dp),
                                                  counts.ctypes.data_as(_ip)))
        return wrench, sdot, L, counts

    def apply_local_jacobian(self, L, d_pose, d_twist, d_s=None):
        """Partials of a seed chunk from the contact Jacobians L (n,12,36) (pfc_apply_local_jacobian): d_pose (n,n_dir,24),
        d_twist (n,n_dir,6), d_s (n,n_dir,6) or None.  Returns (d_wrench (n,n_dir,6), d_sdot (n,n_dir,6)), what
        force_all_elastic_intersections_dual returns for these seeds at L's point.  Keys with all-zero seeds get exact zeros."""
        L_a, L_p = _d(L)
        n = L_a.size // 432
        if L_a.size != 432 * n:
            raise ValueError("L must be (n, 12, 36)")
        dp_a, dp_p = _d(d_pose)
        if n == 0:
            n_dir = int(np.shape(d_pose)[1]) if np.ndim(d_pose) == 3 else 1
        elif dp_a.size % (24 * n) != 0:
            raise ValueError("d_pose must be (n, n_dir, 24)")
        else:
            n_dir = dp_a.size // (24 * n)
        dt_a, dt_p = _d(d_twist)
        if dt_a.size != 6 * n * n_dir:
            raise ValueError("d_twist must be (n, n_dir, 6)")
        ds_p = None
        if d_s is not None:
            ds_a, ds_p = _d(d_s)
            if ds_a.size != 6 * n * n_dir:
                raise ValueError("d_s must be (n, n_dir, 6)")
        dw = np.zeros((n, n_dir, 6)); dsd = np.zeros((n, n_dir, 6))
        self._check(_lib.lib().pfc_apply_local_jacobian(self._h, n, n_dir, L_p, dp_p, dt_p, ds_p, dw.ctypes.data_as(_dp),
                                                        dsd.ctypes.data_as(_dp)))
        return dw, dsd

    def local_jacobian_device(self, d_L: int, stream: int = 0):
        """pfc_local_jacobian_device: L (n_items x 12 x 36 doubles at raw device address d_L) at the point of the previous
        eval_dual_device evaluation; asynchronous.  Follow with check()."""
        self._check(_lib.lib().pfc_local_jacobian_device(self._h, d_L, stream or None))

    def apply_local_jacobian_device(self, n_items: int, n_dir: int, d_L: int, d_dpose: int, d_dtwist: int, d_ds: int, d_dwrench: int,
                                    d_dsdot: int, stream: int = 0):
        """pfc_apply_local_jacobian_device: raw device addresses (d_ds 0: zeros), the layouts of eval_dual_device_more; asynchronous on
        `stream`, no check() needed."""
        self._check(_lib.lib().pfc_apply_local_jacobian_device(self._h, int(n_items), int(n_dir), d_L, d_dpose, d_dtwist, d_ds or None,
                                                               d_dwrench, d_dsdot, stream or None))

    def _bodies_call(self, x_w_b, twist_w_b, ins_ids, scene):
        """Shared argument handling of the host-buffer *_bodies calls: (n, leading ctypes arguments, empty BodyItems, its pointers)."""
        if not self._finalized:
            raise RuntimeError("finalize the scenario first")
        x_a = np.ascontiguousarray(x_w_b, dtype=np.float64)
        if x_a.ndim == 2:
            x_a = x_a[None]
        if x_a.ndim != 3 or x_a.shape[2] != 12:
            raise ValueError("x_w_b must be (n_body, 12) or (n_scene, n_body, 12)")
        n_scene, n_body = x_a.shape[0], x_a.shape[1]
        tw_a = np.ascontiguousarray(twist_w_b, dtype=np.float64).reshape(n_scene, n_body, 6)
        id_a = sc_a = id_p = sc_p = None
        n = len(self.ContactInstructions)
        if ins_ids is not None:
            id_a, id_p = _i(ins_ids)
            n = id_a.size
        if scene is not None:
            sc_a, sc_p = _i(scene)
            if ins_ids is None:
                n = sc_a.size
            elif sc_a.size != n:
                raise ValueError("scene must have one entry per item")
        it = BodyItems(np.zeros((n, 24)), np.zeros((n, 6)), np.zeros((n, 12)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
        head = (self._h, n, id_p, sc_p, n_scene, n_body, x_a.ctypes.data_as(_dp), tw_a.ctypes.data_as(_dp))
        outs = (it.pose.ctypes.data_as(_dp), it.twist.ctypes.data_as(_dp), it.x_w_r2.ctypes.data_as(_dp), it.body_1.ctypes.data_as(_ip),
                it.body_2.ctypes.data_as(_ip))
        return n, head, it, outs, (x_a, tw_a, id_a, sc_a)

    def items_from_bodies(self, x_w_b, twist_w_b, ins_ids: Optional[Sequence[int]] = None, scene=None) -> BodyItems:
        """The items of refreshBodyBodyTransform! / refreshBodyBodyCache! from the bodies' world states (pfc_items_from_bodies, host
        buffers, synchronous).  x_w_b (n_body,12) or (n_scene,n_body,12): R column-major then t; twist_w_b likewise with 6:
        [angular; linear] in world about the world origin.  ins_ids (n,) or None (item i = instruction i); scene (n,) or None
        (scene 0).  Every instruction used must have been given its bodies (set_instruction_bodies)."""
        n, head, it, outs, keep = self._bodies_call(x_w_b, twist_w_b, ins_ids, scene)
        self._check(_lib.lib().pfc_items_from_bodies(*head, *outs))
        return it

    def force_all_elastic_intersections_bodies(self, x_w_b, twist_w_b, s=None, ins_ids: Optional[Sequence[int]] = None, scene=None):
        """force_all_elastic_intersections on the items of items_from_bodies (pfc_eval_bodies, host buffers, synchronous).
        Returns (wrench (n,6), sdot (n,6), counts (n,4), items: BodyItems)."""
        n, head, it, outs, keep = self._bodies_call(x_w_b, twist_w_b, ins_ids, scene)
        s_p = None
        if s is not None:
            s_a, s_p = _d(s)
            if s_a.size != 6 * n:
                raise ValueError("s must have 6 entries per item")
        wrench = np.zeros((n, 6)); sdot = np.zeros((n, 6)); counts = np.zeros((n, 4), dtype=np.int32)
        self._check(_lib.lib().pfc_eval_bodies(*head, s_p, *outs, wrench.ctypes.data_as(_dp), sdot.ctypes.data_as(_dp),
                                               counts.ctypes.data_as(_ip)))
        return wrench, sdot, counts, it

    def items_from_bodies_device(self, n_items: int, d_ins_ids: int, d_scene: int, n_scene: int, n_body: int, d_x_w_b: int,
                                 d_twist_w_b: int, d_pose: int, d_twist: int, d_x_w_r2: int, d_body_1: int, d_body_2: int, stream: int = 0):
        """pfc_items_from_bodies_device: raw device addresses (0: NULL for d_ins_ids, d_scene and any output not wanted); asynchronous
        on `stream`, not an evaluation, no check() needed."""
        self._check(_lib.lib().pfc_items_from_bodies_device(self._h, int(n_items), d_ins_ids or None, d_scene or None, int(n_scene),
                                                            int(n_body), d_x_w_b or None, d_twist_w_b or None, d_pose or None, d_twist or None,
                                                            d_x_w_r2 or None, d_body_1 or None, d_body_2 or None, stream or None))

    def eval_bodies_device(self, n_items: int, d_ins_ids: int, d_scene: int, n_scene: int, n_body: int, d_x_w_b: int, d_twist_w_b: int,
                           d_s: int, d_pose: int, d_twist: int, d_x_w_r2: int, d_body_1: int, d_body_2: int, d_wrench: int, d_sdot: int,
                           d_counts: int, stream: int = 0):
        """pfc_eval_bodies_device: items_from_bodies_device then eval_device on the d_pose / d_twist it wrote, on one stream;
        asynchronous, follow with check() (re-issue on ERR_OVERFLOW)."""
        self._check(_lib.lib().pfc_eval_bodies_device(self._h, int(n_items), d_ins_ids or None, d_scene or None, int(n_scene), int(n_body),
                                                      d_x_w_b or None, d_twist_w_b or None, d_s or None, d_pose, d_twist, d_x_w_r2 or None,
                                                      d_body_1 or None, d_body_2 or None, d_wrench, d_sdot, d_counts or None, stream or None))

    def _state_arrays(self, q, v):
        """(n_scene, n_body, nv, q (n_scene,nq), v (n_scene,nv)) for the mechanism the library holds."""
        n_body, nq, nv = self.mechanism_sizes()
        q_a = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, nq) if nq else np.zeros((np.shape(q)[0] if np.ndim(q) == 2 else 1, 0))
        v_a = np.ascontiguousarray(v, dtype=np.float64).reshape(q_a.shape[0], nv)
        return q_a.shape[0], n_body, nv, q_a, v_a

    def kinematics(self, q, v, want_jac: bool = True):
        """The bodies' world poses, twists and geometric Jacobians from the joint state (pfc_kinematics, host buffers, synchronous).
        q (nq,) or (n_scene,nq), v likewise with nv, in the coordinate order of set_mechanism's bodies.  Returns x_w_b
        (n_scene,n_body,12), twist_w_b (n_scene,n_body,6) and jac (n_scene n_body, nv, 6) (None without want_jac): the inputs of
        items_from_bodies and of scatter_generalized."""
        n_scene, n_body, nv, q_a, v_a = self._state_arrays(q, v)
        x = np.zeros((n_scene, n_body, 12)); tw = np.zeros((n_scene, n_body, 6))
        jac = np.zeros((n_scene * n_body, nv, 6)) if want_jac else None
        self._check(_lib.lib().pfc_kinematics(self._h, n_scene, q_a.ctypes.data_as(_dp), v_a.ctypes.data_as(_dp), x.ctypes.data_as(_dp),
                                              tw.ctypes.data_as(_dp), jac.ctypes.data_as(_dp) if want_jac else None))
        return x, tw, jac

    def kinematics_device(self, n_scene: int, d_q: int, d_v: int, d_x_w_b: int, d_twist_w_b: int, d_jac: int, stream: int = 0):
        """pfc_kinematics_device: raw device addresses (0: NULL for any output not wanted); asynchronous on `stream`, not an
        evaluation, no check() needed."""
        self._check(_lib.lib().pfc_kinematics_device(self._h, int(n_scene), d_q or None, d_v or None, d_x_w_b or None, d_twist_w_b or None,
                                                     d_jac or None, stream or None))

    def force_all_elastic_intersections_state(self, q, v, s=None, ins_ids: Optional[Sequence[int]] = None, scene=None):
        """kinematics, force_all_elastic_intersections_bodies and scatter_generalized in one call (pfc_eval_state, host buffers,
        synchronous): from the joint state to f_generalized.  q, v as kinematics; s, ins_ids, scene as
        force_all_elastic_intersections_bodies.  Returns (wrench (n,6), sdot (n,6), counts (n,4), f (n_scene,nv), items: BodyItems,
        (x_w_b, twist_w_b, jac))."""
        n_scene, n_body, nv, q_a, v_a = self._state_arrays(q, v)
        x = np.zeros((n_scene, n_body, 12)); tw = np.zeros((n_scene, n_body, 6)); jac = np.zeros((n_scene * n_body, nv, 6))
        n, head, it, outs, keep = self._bodies_call(x, tw, ins_ids, scene)
        s_p = None
        if s is not None:
            s_a, s_p = _d(s)
            if s_a.size != 6 * n:
                raise ValueError("s must have 6 entries per item")
        wrench = np.zeros((n, 6)); sdot = np.zeros((n, 6)); counts = np.zeros((n, 4), dtype=np.int32); f = np.zeros((n_scene, nv))
        self._check(_lib.lib().pfc_eval_state(self._h, n, head[2], head[3], n_scene, q_a.ctypes.data_as(_dp), v_a.ctypes.data_as(_dp), s_p,
                                              x.ctypes.data_as(_dp), tw.ctypes.data_as(_dp), jac.ctypes.data_as(_dp), *outs,
                                              wrench.ctypes.data_as(_dp), sdot.ctypes.data_as(_dp), counts.ctypes.data_as(_ip),
                                              f.ctypes.data_as(_dp)))
        return wrench, sdot, counts, f, it, (x, tw, jac)

    def eval_state_device(self, n_items: int, d_ins_ids: int, d_scene: int, n_scene: int, d_q: int, d_v: int, d_s: int, d_x_w_b: int,
                          d_twist_w_b: int, d_jac: int, d_pose: int, d_twist: int, d_x_w_r2: int, d_body_1: int, d_body_2: int,
                          d_wrench: int, d_sdot: int, d_counts: int, d_f: int, stream: int = 0):
        """pfc_eval_state_device: kinematics_device, eval_bodies_device and scatter_generalized_device (d_f 0: no scatter) on one
        stream; asynchronous, follow with check() (re-issue on ERR_OVERFLOW)."""
        self._check(_lib.lib().pfc_eval_state_device(self._h, int(n_items), d_ins_ids or None, d_scene or None, int(n_scene), d_q or None,
                                                     d_v or None, d_s or None, d_x_w_b or None, d_twist_w_b or None, d_jac or None,
                                                     d_pose or None, d_twist or None, d_x_w_r2 or None, d_body_1 or None, d_body_2 or None,
                                                     d_wrench or None, d_sdot or None, d_counts or None, d_f or None, stream or None))

    def dynamics(self, q, v, x_w_b=None, twist_w_b=None):
        """qdot, the mass matrix and the bias from the joint state (pfc_dynamics, host buffers, synchronous).  q, v as kinematics;
        x_w_b, twist_w_b its outputs for the same state (None: computed here).  Returns qdot (n_scene,nq), H (n_scene,nv,nv),
        c (n_scene,nv): H vdot + c = tau + f."""
        n_scene, n_body, nv, q_a, v_a = self._state_arrays(q, v)
        if x_w_b is None or twist_w_b is None:
            x_w_b, twist_w_b, _ = self.kinematics(q_a, v_a, want_jac=False)
        x = np.ascontiguousarray(x_w_b, dtype=np.float64).reshape(n_scene, n_body, 12)
        tw = np.ascontiguousarray(twist_w_b, dtype=np.float64).reshape(n_scene, n_body, 6)
        qd = np.zeros((n_scene, nv)); H = np.zeros((n_scene, nv, nv)); c = np.zeros((n_scene, nv))
        self._check(_lib.lib().pfc_dynamics(self._h, n_scene, q_a.ctypes.data_as(_dp), v_a.ctypes.data_as(_dp), x.ctypes.data_as(_dp),
                                            tw.ctypes.data_as(_dp), qd.ctypes.data_as(_dp), H.ctypes.data_as(_dp), c.ctypes.data_as(_dp)))
        return qd, H, c

    def dynamics_device(self, n_scene: int, d_q: int, d_v: int, d_x_w_b: int, d_twist_w_b: int, d_qdot: int, d_H: int, d_c: int,
                        stream: int = 0):
        """pfc_dynamics_device: raw device addresses (0: NULL for any output not wanted); asynchronous on `stream`, not an
        evaluation, no check() needed."""
        self._check(_lib.lib().pfc_dynamics_device(self._h, int(n_scene), d_q or None, d_v or None, d_x_w_b or None, d_twist_w_b or None,
                                                   d_qdot or None, d_H or None, d_c or None, stream or None))

    def accelerations(self, H, c, f, tau=None):
        """vdot = H^-1 ((f - c) + tau) by Cholesky (pfc_accelerations, host buffers, synchronous).  H (n_scene,nv,nv), c, f and tau
        (None: zeros) (n_scene,nv).  Returns vdot (n_scene,nv) and info (n_scene,): 0, or the 1-based index of the pivot that was
        not > 0 (that scene's vdot is NaN)."""
        _, _, nv = self.mechanism_sizes()
        c_a = np.ascontiguousarray(c, dtype=np.float64).reshape(-1, nv)
        n_scene = c_a.shape[0]
        H_a = np.ascontiguousarray(H, dtype=np.float64).reshape(n_scene, nv, nv)
        f_a = np.ascontiguousarray(f, dtype=np.float64).reshape(n_scene, nv)
        t_a = None if tau is None else np.ascontiguousarray(tau, dtype=np.float64).reshape(n_scene, nv)
        vdot = np.zeros((n_scene, nv)); info = np.zeros(n_scene, dtype=np.int32)
        self._check(_lib.lib().pfc_accelerations(self._h, n_scene, H_a.ctypes.data_as(_dp), c_a.ctypes.data_as(_dp), f_a.ctypes.data_as(_dp),
                                                 None if t_a is None else t_a.ctypes.data_as(_dp), vdot.ctypes.data_as(_dp),
                                                 info.ctypes.data_as(_ip)))
        return vdot, info

    def accelerations_device(self, n_scene: int, d_H: int, d_c: int, d_f: int, d_tau: int, d_vdot: int, d_info: int, stream: int = 0):
        """pfc_accelerations_device: raw device addresses (d_tau 0: zeros; d_info 0: not wanted); asynchronous on `stream`."""
        self._check(_lib.lib().pfc_accelerations_device(self._h, int(n_scene), d_H or None, d_c or None, d_f or None, d_tau or None,
                                                        d_vdot or None, d_info or None, stream or None))

    def state_derivative(self, q, v, s=None, tau=None, ins_ids: Optional[Sequence[int]] = None, scene=None):
        """From x = [q; v; s] to qdot, vdot and sdot in one call (pfc_state_derivative, host buffers, synchronous):
        force_all_elastic_intersections_state, dynamics and accelerations.  Arguments as force_all_elastic_intersections_state; tau
        (n_scene,nv) or None.  Returns (qdot (n_scene,nq), vdot (n_scene,nv), sdot (n,6), info (n_scene,), f (n_scene,nv),
        (H, c), (wrench, counts))."""
        n_scene, n_body, nv, q_a, v_a = self._state_arrays(q, v)
        x = np.zeros((n_scene, n_body, 12)); tw = np.zeros((n_scene, n_body, 6))
        n, head, it, outs, keep = self._bodies_call(x, tw, ins_ids, scene)
        s_p = None
        if s is not None:
            s_a, s_p = _d(s)
            if s_a.size != 6 * n:
                raise ValueError("s must have 6 entries per item")
        t_a = None if tau is None else np.ascontiguousarray(tau, dtype=np.float64).reshape(n_scene, nv)
        wrench = np.zeros((n, 6)); sdot = np.zeros((n, 6)); counts = np.zeros((n, 4), dtype=np.int32); f = np.zeros((n_scene, nv))
        qd = np.zeros((n_scene, nv)); H = np.zeros((n_scene, nv, nv)); c = np.zeros((n_scene, nv)); vdot = np.zeros((n_scene, nv))
        info = np.zeros(n_scene, dtype=np.int32)
        self._check(_lib.lib().pfc_state_derivative(
            self._h, n, head[2], head[3], n_scene, q_a.ctypes.data_as(_dp), v_a.ctypes.data_as(_dp), s_p,
            None if t_a is None else t_a.ctypes.data_as(_dp), x.ctypes.data_as(_dp), tw.ctypes.data_as(_dp), None, *outs,
            wrench.ctypes.data_as(_dp), sdot.ctypes.data_as(_dp), counts.ctypes.data_as(_ip), f.ctypes.data_as(_dp),
            qd.ctypes.data_as(_dp), H.ctypes.data_as(_dp), c.ctypes.data_as(_dp), vdot.ctypes.data_as(_dp), info.ctypes.data_as(_ip)))
        return qd, vdot, sdot, info, f, (H, c), (wrench, counts)

    def state_derivative_device(self, n_items: int, d_ins_ids: int, d_scene: int, n_scene: int, d_q: int, d_v: int, d_s: int, d_tau: int,
                                d_x_w_b: int, d_twist_w_b: int, d_jac: int, d_pose: int, d_twist: int, d_x_w_r2: int, d_body_1: int,
                                d_body_2: int, d_wrench: int, d_sdot: int, d_counts: int, d_f: int, d_qdot: int, d_H: int, d_c: int,
                                d_vdot: int, d_info: int, stream: int = 0):
        """pfc_state_derivative_device: eval_state_device (d_f required), dynamics_device and accelerations_device on one stream;
        asynchronous, follow with check() (re-issue on ERR_OVERFLOW)."""
        a = [d_ins_ids, d_scene]
        b = [d_q, d_v, d_s, d_tau, d_x_w_b, d_twist_w_b, d_jac, d_pose, d_twist, d_x_w_r2, d_body_1, d_body_2, d_wrench, d_sdot, d_counts, d_f,
             d_qdot, d_H, d_c, d_vdot, d_info, stream]
        self._check(_lib.lib().pfc_state_derivative_device(self._h, int(n_items), *[p or None for p in a], int(n_scene),
                                                           *[p or None for p in b]))

    def _seed_arrays(self, n_scene, nq, nv, dq, dv):
        """(n_dir, dq (n_scene,n_dir,nq) or None, dv (n_scene,n_dir,nv) or None): the seed directions of a Jacobian chunk."""
        if dq is None and dv is None:
            raise ValueError("one of dq and dv must be given: they carry n_dir")
        out, n_dir = [], None
        for a, w, name in ((dq, nq, "dq"), (dv, nv, "dv")):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.ndim == 2:
                    a = a[None]
                if a.ndim != 3 or a.shape[0] != n_scene or a.shape[2] != w or n_dir not in (None, a.shape[1]):
                    raise ValueError(f"{name} must be (n_dir, {w}) or (n_scene, n_dir, {w})")
                n_dir = a.shape[1]
            out.append(a)
        return n_dir, out[0], out[1]

    def kinematics_dual(self, q, v, dq, dv, want_jac: bool = True):
        """The partials of kinematics' three outputs for the seed directions of a Jacobian chunk (pfc_kinematics_dual, host buffers,
        synchronous).  q, v as kinematics; dq (n_dir,nq) or (n_scene,n_dir,nq) and dv likewise with nv: the partials of the state,
        either may be None (zeros), not both (n_dir comes from them).  Returns d_x_w_b (n_scene,n_body,n_dir,12), d_twist_w_b
        (n_scene,n_body,n_dir,6) and d_jac (n_scene n_body, n_dir, nv, 6) (None without want_jac): the inputs of
        dual_seeds_from_bodies and of scatter_generalized_dual."""
        n_scene, n_body, nv, q_a, v_a = self._state_arrays(q, v)
        n_dir, dq_a, dv_a = self._seed_arrays(n_scene, q_a.shape[1], nv, dq, dv)
        dx = np.zeros((n_scene, n_body, n_dir, 12)); dtw = np.zeros((n_scene, n_body, n_dir, 6))
        djac = np.zeros((n_scene * n_body, n_dir, nv, 6)) if want_jac else None
        self._check(_lib.lib().pfc_kinematics_dual(
            self._h, n_scene, n_dir, q_a.ctypes.data_as(_dp), v_a.ctypes.data_as(_dp),
            dq_a.ctypes.data_as(_dp) if dq_a is not None else None, dv_a.ctypes.data_as(_dp) if dv_a is not None else None,
            dx.ctypes.data_as(_dp), dtw.ctypes.data_as(_dp), djac.ctypes.data_as(_dp) if want_jac else None))
        return dx, dtw, djac

    def kinematics_dual_device(self, n_scene: int, n_dir: int, d_q: int, d_v: int, d_dq: int, d_dv: int, d_dx_w_b: int,
                               d_dtwist_w_b: int, d_djac: int, stream: int = 0):
        """pfc_kinematics_dual_device: raw device addresses (0: NULL for either seed array and any output not wanted); asynchronous on
        `stream`, not an evaluation, no check() needed."""
        self._check(_lib.lib().pfc_kinematics_dual_device(self._h, int(n_scene), int(n_dir), d_q or None, d_v or None, d_dq or None,
                                                          d_dv or None, d_dx_w_b or None, d_dtwist_w_b or None, d_djac or None,
                                                          stream or None))

    def eval_dual_state_device(self, n_items: int, n_dir: int, d_ins_ids: int, d_scene: int, n_scene: int, d_q: int, d_v: int,
                               d_dq: int, d_dv: int, d_s: int, d_ds: int, d_x_w_b: int, d_twist_w_b: int, d_jac: int, d_dx_w_b: int,
                               d_dtwist_w_b: int, d_djac: int, d_pose: int, d_twist: int, d_x_w_r2: int, d_body_1: int, d_body_2: int,
                               d_dpose: int, d_dtwist: int, d_dx_w_r2: int, d_wrench: int, d_sdot: int, d_dwrench: int, d_dsdot: int,
                               d_counts: int, d_f: int, d_df: int, stream: int = 0):
        """pfc_eval_dual_state_device: kinematics_device, kinematics_dual_device, eval_dual_bodies_device and
        scatter_generalized_dual_device (d_df 0: no scatter) on one stream; asynchronous, follow with check() (re-issue on
        ERR_OVERFLOW)."""
        p = lambda a: a or None
        self._check(_lib.lib().pfc_eval_dual_state_device(
            self._h, int(n_items), int(n_dir), p(d_ins_ids), p(d_scene), int(n_scene), p(d_q), p(d_v), p(d_dq), p(d_dv), p(d_s), p(d_ds),
            p(d_x_w_b), p(d_twist_w_b), p(d_jac), p(d_dx_w_b), p(d_dtwist_w_b), p(d_djac), p(d_pose), p(d_twist), p(d_x_w_r2),
            p(d_body_1), p(d_body_2), p(d_dpose), p(d_dtwist), p(d_dx_w_r2), p(d_wrench), p(d_sdot), p(d_dwrench), p(d_dsdot),
            p(d_counts), p(d_f), p(d_df), stream or None))

    def eval_dual_state_device_more(self, n_items: int, n_dir: int, d_ins_ids: int, d_scene: int, n_scene: int, d_q: int, d_v: int,
                                    d_dq: int, d_dv: int, d_ds: int, d_x_w_b: int, d_twist_w_b: int, d_jac: int, d_dx_w_b: int,
                                    d_dtwist_w_b: int, d_djac: int, d_x_w_r2: int, d_body_1: int, d_body_2: int, d_wrench: int,
                                    d_dpose: int, d_dtwist: int, d_dx_w_r2: int, d_dwrench: int, d_dsdot: int, d_df: int,
                                    stream: int = 0):
        """pfc_eval_dual_state_device_more: kinematics_dual_device, eval_dual_bodies_device_more and the Dual scatter into d_df (0: no
        scatter) for a later chunk of the Jacobian at the kept point; reads the value buffers the first chunk left, writes only
        partials; asynchronous, follow with check()."""
        p = lambda a: a or None
        self._check(_lib.lib().pfc_eval_dual_state_device_more(
            self._h, int(n_items), int(n_dir), p(d_ins_ids), p(d_scene), int(n_scene), p(d_q), p(d_v), p(d_dq), p(d_dv), p(d_ds),
            p(d_x_w_b), p(d_twist_w_b), p(d_jac), p(d_dx_w_b), p(d_dtwist_w_b), p(d_djac), p(d_x_w_r2), p(d_body_1), p(d_body_2),
            p(d_wrench), p(d_dpose), p(d_dtwist), p(d_dx_w_r2), p(d_dwrench), p(d_dsdot), p(d_df), stream or None))

    def force_all_elastic_intersections_dual_state(self, q, v, s, dq, dv, ds=None, ins_ids: Optional[Sequence[int]] = None, scene=None):
        """From the joint state and its seed directions to f_generalized and its partials (host arrays, synchronous; composed here
        from kinematics, kinematics_dual, force_all_elastic_intersections_dual_bodies and scatter_generalized_dual, the calls
        pfc_eval_dual_state_device chains on the device).  q, v, dq, dv as kinematics_dual; s, ds, ins_ids, scene as
        force_all_elastic_intersections_dual_bodies.  Returns (wrench, sdot, d_wrench, d_sdot, counts, f (n_scene,nv),
        d_f (n_scene,n_dir,nv), items: BodyItems, seeds: BodySeeds, (x_w_b, twist_w_b, jac), (d_x_w_b, d_twist_w_b, d_jac))."""
        x, tw, jac = self.kinematics(q, v)
        dx, dtw, djac = self.kinematics_dual(q, v, dq, dv)
        wrench, sdot, dw, dsd, counts, it, sd = self.force_all_elastic_intersections_dual_bodies(x, tw, s, dx, dtw, ds, ins_ids, scene)
        f, d_f = self.scatter_generalized_dual(wrench, dw, it.x_w_r2, sd.d_x_w_r2, it.body_1, it.body_2, jac, djac, scene, x.shape[0])
        return wrench, sdot, dw, dsd, counts, f, d_f, it, sd, (x, tw, jac), (dx, dtw, djac)

    def dynamics_dual(self, q, v, dq, dv, x_w_b=None, twist_w_b=None, d_x_w_b=None, d_twist_w_b=None):
        """The partials of dynamics' three outputs for the seed directions of a Jacobian chunk (pfc_dynamics_dual, host buffers,
        synchronous).  q, v, dq, dv as kinematics_dual; x_w_b, twist_w_b and d_x_w_b, d_twist_w_b the outputs of kinematics and
        kinematics_dual for them (None: computed here).  Returns d_qdot (n_scene,n_dir,nq), d_H (n_scene,n_dir,nv,nv) and d_c
        (n_scene,n_dir,nv)."""
        n_scene, n_body, nv, q_a, v_a = self._state_arrays(q, v)
        nq = q_a.shape[1]
        n_dir, dq_a, dv_a = self._seed_arrays(n_scene, nq, nv, dq, dv)
        if x_w_b is None or twist_w_b is None:
            x_w_b, twist_w_b, _ = self.kinematics(q_a, v_a, want_jac=False)
        if d_x_w_b is None or d_twist_w_b is None:
            d_x_w_b, d_twist_w_b, _ = self.kinematics_dual(q_a, v_a, dq_a, dv_a, want_jac=False)
        x = np.ascontiguousarray(x_w_b, dtype=np.float64).reshape(n_scene, n_body, 12)
        tw = np.ascontiguousarray(twist_w_b, dtype=np.float64).reshape(n_scene, n_body, 6)
        dx = np.ascontiguousarray(d_x_w_b, dtype=np.float64).reshape(n_scene, n_body, n_dir, 12)
        dtw = np.ascontiguousarray(d_twist_w_b, dtype=np.float64).reshape(n_scene, n_body, n_dir, 6)
        dqd = np.zeros((n_scene, n_dir, nq)); dH = np.zeros((n_scene, n_dir, nv, nv)); dc = np.zeros((n_scene, n_dir, nv))
        p = lambda a: None if a is None else a.ctypes.data_as(_dp)
        self._check(_lib.lib().pfc_dynamics_dual(self._h, n_scene, n_dir, p(q_a), p(v_a), p(dq_a), p(dv_a), p(x), p(tw), p(dx), p(dtw),
                                                 p(dqd), p(dH), p(dc)))
        return dqd, dH, dc

    def dynamics_dual_device(self, n_scene: int, n_dir: int, d_q: int, d_v: int, d_dq: int, d_dv: int, d_x_w_b: int, d_twist_w_b: int,
                             d_dx_w_b: int, d_dtwist_w_b: int, d_dqdot: int, d_dH: int, d_dc: int, stream: int = 0):
        """pfc_dynamics_dual_device: raw device addresses (0: NULL for either seed array and any output not wanted); asynchronous on
        `stream`, not an evaluation, no check() needed."""
        a = [d_q, d_v, d_dq, d_dv, d_x_w_b, d_twist_w_b, d_dx_w_b, d_dtwist_w_b, d_dqdot, d_dH, d_dc, stream]
        self._check(_lib.lib().pfc_dynamics_dual_device(self._h, int(n_scene), int(n_dir), *[p or None for p in a]))

    def accelerations_dual(self, H, c, f, dH, dc, df, tau=None, dtau=None):
        """vdot and its partials dvdot = H^-1 (((df - dc) + dtau) - dH vdot) with the value factor (pfc_accelerations_dual, host
        buffers, synchronous).  H, c, f, tau as accelerations; dH (n_scene,n_dir,nv,nv), dc, df and dtau (None: zeros)
        (n_scene,n_dir,nv).  Returns vdot (n_scene,nv), dvdot (n_scene,n_dir,nv) and info (n_scene,)."""
        _, _, nv = self.mechanism_sizes()
        c_a = np.ascontiguousarray(c, dtype=np.float64).reshape(-1, nv)
        n_scene = c_a.shape[0]
        dc_a = np.ascontiguousarray(dc, dtype=np.float64).reshape(n_scene, -1, nv)
        n_dir = dc_a.shape[1]
        arr = lambda a, *shape: None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(*shape)
        H_a, f_a, t_a = arr(H, n_scene, nv, nv), arr(f, n_scene, nv), arr(tau, n_scene, nv)
        dH_a, df_a, dt_a = arr(dH, n_scene, n_dir, nv, nv), arr(df, n_scene, n_dir, nv), arr(dtau, n_scene, n_dir, nv)
        vdot = np.zeros((n_scene, nv)); dvdot = np.zeros((n_scene, n_dir, nv)); info = np.zeros(n_scene, dtype=np.int32)
        p = lambda a: None if a is None else a.ctypes.data_as(_dp)
        self._check(_lib.lib().pfc_accelerations_dual(self._h, n_scene, n_dir, p(H_a), p(c_a), p(f_a), p(t_a), p(dH_a), p(dc_a), p(df_a),
                                                      p(dt_a), p(vdot), p(dvdot), info.ctypes.data_as(_ip)))
        return vdot, dvdot, info

    def accelerations_dual_device(self, n_scene: int, n_dir: int, d_H: int, d_c: int, d_f: int, d_tau: int, d_dH: int, d_dc: int,
                                  d_df: int, d_dtau: int, d_vdot: int, d_dvdot: int, d_info: int, stream: int = 0):
        """pfc_accelerations_dual_device: raw device addresses (d_tau, d_dtau 0: zeros; d_vdot, d_info 0: not wanted); asynchronous on
        `stream`."""
        a = [d_H, d_c, d_f, d_tau, d_dH, d_dc, d_df, d_dtau, d_vdot, d_dvdot, d_info, stream]
        self._check(_lib.lib().pfc_accelerations_dual_device(self._h, int(n_scene), int(n_dir), *[p or None for p in a]))

    def state_derivative_dual_device(self, n_items: int, n_dir: int, d_ins_ids: int, d_scene: int, n_scene: int, d_q: int, d_v: int,
                                     d_dq: int, d_dv: int, d_s: int, d_ds: int, d_tau: int, d_dtau: int, d_x_w_b: int, d_twist_w_b: int,
                                     d_jac: int, d_dx_w_b: int, d_dtwist_w_b: int, d_djac: int, d_pose: int, d_twist: int,
                                     d_x_w_r2: int, d_body_1: int, d_body_2: int, d_dpose: int, d_dtwist: int, d_dx_w_r2: int,
                                     d_wrench: int, d_sdot: int, d_dwrench: int, d_dsdot: int, d_counts: int, d_f: int, d_df: int,
                                     d_qdot: int, d_H: int, d_c: int, d_vdot: int, d_info: int, d_dqdot: int, d_dH: int, d_dc: int,
                                     d_dvdot: int, stream: int = 0):
        """pfc_state_derivative_dual_device: eval_dual_state_device (d_f, d_df required), dynamics_device, dynamics_dual_device and
        accelerations_dual_device on one stream; asynchronous, follow with check() (re-issue on ERR_OVERFLOW)."""
        a = [d_q, d_v, d_dq, d_dv, d_s, d_ds, d_tau, d_dtau, d_x_w_b, d_twist_w_b, d_jac, d_dx_w_b, d_dtwist_w_b, d_djac, d_pose, d_twist,
             d_x_w_r2, d_body_1, d_body_2, d_dpose, d_dtwist, d_dx_w_r2, d_wrench, d_sdot, d_dwrench, d_dsdot, d_counts, d_f, d_df,
             d_qdot, d_H, d_c, d_vdot, d_info, d_dqdot, d_dH, d_dc, d_dvdot, stream]
        self._check(_lib.lib().pfc_state_derivative_dual_device(self._h, int(n_items), int(n_dir), d_ins_ids or None, d_scene or None,
                                                                int(n_scene), *[p or None for p in a]))

    def state_derivative_dual_device_more(self, n_items: int, n_dir: int, d_ins_ids: int, d_scene: int, n_scene: int, d_q: int, d_v: int,
                                          d_dq: int, d_dv: int, d_ds: int, d_tau: int, d_dtau: int, d_x_w_b: int, d_twist_w_b: int,
                                          d_jac: int, d_dx_w_b: int, d_dtwist_w_b: int, d_djac: int, d_x_w_r2: int, d_body_1: int,
                                          d_body_2: int, d_wrench: int, d_dpose: int, d_dtwist: int, d_dx_w_r2: int, d_dwrench: int,
                                          d_dsdot: int, d_df: int, d_H: int, d_c: int, d_f: int, d_dqdot: int, d_dH: int, d_dc: int,
                                          d_dvdot: int, stream: int = 0):
        """pfc_state_derivative_dual_device_more: eval_dual_state_device_more (d_df required), dynamics_dual_device and
        accelerations_dual_device (no vdot) for a later chunk at the kept point; reads d_H, d_c, d_f and d_tau as the first chunk
        left them, writes only partials; asynchronous, follow with check()."""
        a = [d_q, d_v, d_dq, d_dv, d_ds, d_tau, d_dtau, d_x_w_b, d_twist_w_b, d_jac, d_dx_w_b, d_dtwist_w_b, d_djac, d_x_w_r2, d_body_1,
             d_body_2, d_wrench, d_dpose, d_dtwist, d_dx_w_r2, d_dwrench, d_dsdot, d_df, d_H, d_c, d_f, d_dqdot, d_dH, d_dc, d_dvdot, stream]
        self._check(_lib.lib().pfc_state_derivative_dual_device_more(self._h, int(n_items), int(n_dir), d_ins_ids or None, d_scene or None,
                                                                     int(n_scene), *[p or None for p in a]))

    def state_derivative_dual(self, q, v, s, dq, dv, ds=None, tau=None, dtau=None, ins_ids: Optional[Sequence[int]] = None, scene=None):
        """From x = [q; v; s] and the seed directions of a Jacobian chunk to [qdot; vdot; sdot] and a column block of its Jacobian
        (host arrays, synchronous; composed here from force_all_elastic_intersections_dual_state, dynamics, dynamics_dual and
        accelerations_dual, the calls pfc_state_derivative_dual_device chains on the device).  Arguments as
        force_all_elastic_intersections_dual_state; tau (n_scene,nv) and dtau (n_scene,n_dir,nv) or None.  Returns (qdot, vdot, sdot,
        d_qdot (n_scene,n_dir,nq), d_vdot (n_scene,n_dir,nv), d_sdot, info, (f, d_f), (H, c), (d_H, d_c), (wrench, d_wrench, counts))."""
        wrench, sdot, dw, dsd, counts, f, d_f, _, _, (x, tw, _), (dx, dtw, _) = self.force_all_elastic_intersections_dual_state(
            q, v, s, dq, dv, ds, ins_ids, scene)
        qd, H, c = self.dynamics(q, v, x, tw)
        dqd, dH, dc = self.dynamics_dual(q, v, dq, dv, x, tw, dx, dtw)
        vdot, dvdot, info = self.accelerations_dual(H, c, f, dH, dc, d_f, tau, dtau)
        return qd, vdot, sdot, dqd, dvdot, dsd, info, (f, d_f), (H, c), (dH, dc), (wrench, dw, counts)

    # ---- the Radau IIA step on the device (include/pfc.h; mirrors integrate_scenario_radau, src/example_integrator.jl) -----------
    def radau_configure(self, n_scene: int, ins_ids: Sequence[int], h0: float = 1e-4, tol_a: float = 1e-4, tol_r: float = 1e-4,
                        tol_newton: float = 1e-16, h_max: float = 0.01, h_min: float = 1e-8, k_iter_max: int = 15, max_rule: int = 2,
                        n_chunk: int = 6, cooldown: int = 10):
        """pfc_radau_configure: a batch of n_scene scenes of the mechanism, each with the items ins_ids; the reference's defaults.
        Returns NX = nq + nv + 6 (bristle items per scene)."""
        ids = np.ascontiguousarray(ins_ids, dtype=np.int32).reshape(-1)
        par = np.array([h0, tol_a, tol_r, tol_newton, h_max, h_min], dtype=np.float64)
        self._check(_lib.lib().pfc_radau_configure(self._h, int(n_scene), int(ids.size), ids.ctypes.data_as(_ip), par.ctypes.data_as(_dp),
                                                   int(k_iter_max), int(max_rule), int(n_chunk), int(cooldown)))
        self._radau_n_scene = int(n_scene)
        return self.radau_sizes()[0]

    def radau_sizes(self):
        """(NX, item indices of the bristle items of a scene)."""
        nx, nb = C.c_int(0), C.c_int(0)
        items = np.zeros(16, dtype=np.int32)
        self._check(_lib.lib().pfc_radau_sizes(self._h, C.byref(nx), C.byref(nb), items.ctypes.data_as(_ip)))
        return nx.value, items[:nb.value].copy()

    def radau_set_state(self, x, t=None):
        """x (n_scene, NX) = [q; v; s of the bristle items] and t (n_scene,) or None (zeros); resets h, rule, cooldown and the norms."""
        nx = self.radau_sizes()[0]
        x_a = np.ascontiguousarray(x, dtype=np.float64).reshape(self._radau_n_scene, nx)
        t_a = None if t is None else np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.float64), (self._radau_n_scene,)))
        self._check(_lib.lib().pfc_radau_set_state(self._h, x_a.ctypes.data_as(_dp), None if t_a is None else t_a.ctypes.data_as(_dp)))

    def radau_set_rule_state(self, h=None, rule=None, cooldown=None):
        """pfc_radau_set_rule_state: per-scene step size, rule and cooldown (each (n_scene,) or a scalar, or None: unchanged) in
        place of what radau_set_state reset them to."""
        n = self._radau_n_scene
        arr = lambda a, dt: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=dt), (n,)))
        h_a, r_a, c_a = arr(h, np.float64), arr(rule, np.int32), arr(cooldown, np.int32)
        self._check(_lib.lib().pfc_radau_set_rule_state(self._h, None if h_a is None else h_a.ctypes.data_as(_dp),
                                                        None if r_a is None else r_a.ctypes.data_as(_ip),
                                                        None if c_a is None else c_a.ctypes.data_as(_ip)))

    def radau_get_state(self):
        """(x (n_scene, NX), t (n_scene,))."""
        nx = self.radau_sizes()[0]
        x = np.zeros((self._radau_n_scene, nx)); t = np.zeros(self._radau_n_scene)
        self._check(_lib.lib().pfc_radau_get_state(self._h, x.ctypes.data_as(_dp), t.ctypes.data_as(_dp)))
        return x, t

    def radau_set_tau(self, tau=None):
        """tau (n_scene, nv) held constant over the steps that follow, or None (zeros)."""
        t_a = None if tau is None else np.ascontiguousarray(tau, dtype=np.float64).reshape(self._radau_n_scene, -1)
        self._check(_lib.lib().pfc_radau_set_tau(self._h, None if t_a is None else t_a.ctypes.data_as(_dp)))

    def radau_get_tau(self):
        """pfc_radau_get_tau: the tau the step reads, (3, n_scene, nv): radau_set_tau's, overwritten by the controller's fires."""
        n, nv = self._radau_n_scene, self.mechanism_sizes()[2]
        tau = np.zeros((3, n, nv))
        self._check(_lib.lib().pfc_radau_get_tau(self._h, tau.ctypes.data_as(_dp)))
        return tau

    def radau_rule_state(self):
        """Per scene: dict of h, rule, cooldown, theta, psi_k, x_err_norm, x_err_norm_next (arrays of n_scene)."""
        out = np.zeros((self._radau_n_scene, 7))
        self._check(_lib.lib().pfc_radau_rule_state(self._h, out.ctypes.data_as(_dp)))
        return dict(h=out[:, 0].copy(), rule=out[:, 1].astype(np.int32), cooldown=out[:, 2].astype(np.int32), theta=out[:, 3].copy(),
                    psi_k=out[:, 4].copy(), x_err_norm=out[:, 5].copy(), x_err_norm_next=out[:, 6].copy())

    def radau_step(self):
        """pfc_radau_step: one step of every scene.  Returns dict(h_taken, flags, iters, attempts) and raises PFCError("time step is
        too small, something is wrong") naming the scenes whose exit flag is 5, as the reference's solveRadau_inner throws."""
        n = getattr(self, "_radau_n_scene", 0)      # 0: not configured, the library says so
        h = np.zeros(n); fl = np.zeros(n, dtype=np.int32); it = np.zeros(n, dtype=np.int32); at = np.zeros(n, dtype=np.int32)
        self._check(_lib.lib().pfc_radau_step(self._h, h.ctypes.data_as(_dp), fl.ctypes.data_as(_ip), it.ctypes.data_as(_ip),
                                              at.ctypes.data_as(_ip)))
        if (fl == 5).any():
            raise _lib.PFCError(_lib.ERR_STATE, "time step is too small, something is wrong (scenes %s)" % np.flatnonzero(fl == 5).tolist())
        return dict(h_taken=h, flags=fl, iters=it, attempts=at)

    def integrate_radau(self, t_final: float, max_steps: int = 100000):
        """Steps until every scene's t >= t_final or max_steps steps were taken (integrate_scenario_radau steps while t < t_final
        and does not shorten the last step).  A scene that has arrived is still stepped with the others.  Returns (x, t, steps)."""
        steps = 0
        x, t = self.radau_get_state()
        while (t < t_final).any() and steps < max_steps:
            self.radau_step()
            steps += 1
            x, t = self.radau_get_state()
        return x, t, steps

    def radau_set_end(self, t_final=None, max_rows: int = 0):
        """pfc_radau_set_end: an end time per scene ((n_scene,) or a scalar; None: +inf) and the rows each scene may record (0:
        none, else >= 2).  Row 0 of every trajectory is the state now; a scene parks at the commit that leaves t_final < t or fills its
        last row, and radau_step reports flag 6 for it afterwards."""
        n = getattr(self, "_radau_n_scene", 0)      # 0: not configured, the library says so
        t_a = None if t_final is None else np.ascontiguousarray(np.broadcast_to(np.asarray(t_final, dtype=np.float64), (n,)))
        self._check(_lib.lib().pfc_radau_set_end(self._h, None if t_a is None else t_a.ctypes.data_as(_dp), int(max_rows)))

    def radau_integrate(self, max_steps: int):
        """pfc_radau_integrate: batch steps until no scene is live or max_steps were taken, the trajectory recorded on the device and
        nothing but counts read back per step.  Returns (steps_done, n_live)."""
        steps, live = C.c_int(0), C.c_int(0)
        self._check(_lib.lib().pfc_radau_integrate(self._h, int(max_steps), C.byref(steps), C.byref(live)))
        return steps.value, live.value

    def radau_trajectory_rows(self):
        """The rows recorded per scene since radau_set_end ((n_scene,) int32)."""
        rows = np.zeros(getattr(self, "_radau_n_scene", 0), dtype=np.int32)
        self._check(_lib.lib().pfc_radau_trajectory_rows(self._h, rows.ctypes.data_as(_ip)))
        return rows

    def radau_trajectory(self, scene: int, rows: Optional[int] = None):
        """(data_time (rows,), data_state (rows, NX)) of a scene: row 0 is the state at radau_set_end, then one row per committed step.
        rows: the scene's entry of radau_trajectory_rows() where the caller has it already."""
        if rows is None:
            rows = self.radau_trajectory_rows()[int(scene)] if 0 <= int(scene) < getattr(self, "_radau_n_scene", 0) else 0
        n = int(rows)
        nx = self.radau_sizes()[0]
        t = np.zeros(n); x = np.zeros((n, nx))
        self._check(_lib.lib().pfc_radau_trajectory(self._h, int(scene), 0, n, t.ctypes.data_as(_dp), x.ctypes.data_as(_dp)))
        return t, x

    def radau_set_controller(self, act, kp, kd, dt: float, seg_t, seg_q, seg_ff=None, a_max=None, t_last0=None):
        """pfc_radau_set_controller: a zero-order-hold computed-torque PD controller that fires on the device at the top of every
        batch step of radau_step / radau_integrate (the law: computed_torque_pd below, the clock: discrete_clock).  act (n_act,)
        the actuated coordinates, strictly increasing, each owned by a revolute or prismatic joint; kp, kd, a_max (n_act,) or scalars
        (a_max None: no clamp); dt the controller's period; seg_t (n_scene, n_seg) or (n_seg,) the segments' start times (entry 0 is
        not read), seg_q (n_scene, n_seg, n_act) or (n_seg, n_act) the setpoints, seg_ff (n_scene, n_seg, nv) or (n_seg, nv) a
        feed-forward torque (None: zeros); t_last0 (n_scene,) or a scalar (None: every scene's current t; the reference's constructor
        gives 0.0).  Once it has fired for a scene, radau_set_tau's value for that scene is overwritten."""
        n = getattr(self, "_radau_n_scene", 0)
        nv = self.mechanism_sizes()[2]
        act_a = np.ascontiguousarray(act, dtype=np.int32).reshape(-1)
        na = act_a.size
        vec = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (na,)))
        kp_a, kd_a = vec(kp), vec(kd)
        am_a = None if a_max is None else vec(a_max)
        st = np.asarray(seg_t, dtype=np.float64)
        n_seg = st.shape[-1] if st.ndim else 1
        st_a = np.ascontiguousarray(np.broadcast_to(st.reshape(-1, n_seg), (n, n_seg)))
        sq_a = np.zeros((n, n_seg, 0)) if na == 0 else \
            np.ascontiguousarray(np.broadcast_to(np.asarray(seg_q, dtype=np.float64).reshape((-1, n_seg, na)), (n, n_seg, na)))
        ff_a = None if seg_ff is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(seg_ff, dtype=np.float64).reshape((-1, n_seg, nv)), (n, n_seg, nv)))
        t0_a = None if t_last0 is None else np.ascontiguousarray(np.broadcast_to(np.asarray(t_last0, dtype=np.float64), (n,)))
        p = lambda a: None if a is None else a.ctypes.data_as(_dp)
        self._check(_lib.lib().pfc_radau_set_controller(self._h, int(na), act_a.ctypes.data_as(_ip), p(kp_a), p(kd_a), p(am_a), float(dt),
                                                        p(t0_a), int(n_seg), p(st_a), p(sq_a), p(ff_a)))
        self._radau_n_act = int(na)

    def radau_clear_controller(self):
        """pfc_radau_clear_controller: the step is the step without a controller again."""
        self._check(_lib.lib().pfc_radau_clear_controller(self._h))

    def radau_controller_state(self):
        """(t_last (n_scene,), fires (n_scene,) int32) of the device controller: its clock and the additions counted per scene."""
        n = getattr(self, "_radau_n_scene", 0)
        t_last = np.zeros(n); fires = np.zeros(n, dtype=np.int32)
        self._check(_lib.lib().pfc_radau_controller_state(self._h, t_last.ctypes.data_as(_dp), fires.ctypes.data_as(_ip)))
        return t_last, fires

    def radau_control_device(self, n_scene: int, nq: int, nv: int, n_act: int, n_seg: int, dt: float, d_act: int, d_kp: int, d_kd: int,
                             d_a_max: int, d_seg_t: int, d_seg_q: int, d_seg_ff: int, d_t: int, d_q: int, d_v: int, d_H: int, d_c: int,
                             d_istate: int, d_t_last: int, d_fires: int, d_tau: int, stream: int = 0):
        """pfc_radau_control_device: the controller's part on raw device addresses (0: NULL for d_seg_ff and d_istate); asynchronous
        on `stream`."""
        a = [d_act, d_kp, d_kd, d_a_max, d_seg_t, d_seg_q, d_seg_ff, d_t, d_q, d_v, d_H, d_c, d_istate, d_t_last, d_fires, d_tau, stream]
        self._check(_lib.lib().pfc_radau_control_device(self._h, int(n_scene), int(nq), int(nv), int(n_act), int(n_seg), float(dt),
                                                        *[x or None for x in a]))

    def computed_torque_pd_fn(self, act, kp, kd, seg_t, seg_q, seg_ff=None, a_max=None):
        """fn(x, t, scene) -> tau for integrate_scenario_radau(discrete_controller=(fn, dt)): computed_torque_pd on H and c of the
        host form `dynamics` at the scene's (q, v).  The arrays are radau_set_controller's; a leading scene axis is indexed by
        `scene`."""
        _, nq, nv = self.mechanism_sizes()
        act_l = [int(a) for a in np.asarray(act).reshape(-1)]
        na = len(act_l)
        vec = lambda a: [float(e) for e in np.broadcast_to(np.asarray(a, dtype=np.float64), (na,))]
        kp_l, kd_l = vec(kp), vec(kd)
        am_l = None if a_max is None else vec(a_max)
        st = np.asarray(seg_t, dtype=np.float64)
        n_seg = st.shape[-1] if st.ndim else 1
        st = st.reshape(-1, n_seg)
        sq = np.zeros((1, n_seg, 0)) if na == 0 else np.asarray(seg_q, dtype=np.float64).reshape(-1, n_seg, na)
        ff = None if seg_ff is None else np.asarray(seg_ff, dtype=np.float64).reshape(-1, n_seg, nv)
        row = lambda a, s: a[s if a.shape[0] > 1 else 0]

        def fn(x, t, scene):
            q, v = np.asarray(x[:nq], dtype=np.float64), np.asarray(x[nq:nq + nv], dtype=np.float64)
            _, H, c = self.dynamics(q, v)
            return computed_torque_pd(q.tolist(), v.tolist(), H[0].tolist(), c[0].tolist(), float(t), act_l, kp_l, kd_l,
                                      row(st, scene).tolist(), row(sq, scene).tolist(), None if ff is None else row(ff, scene).tolist(), am_l)
        return fn

    def radau_host_controller_state(self):
        """(t_last, fires) of the host route's clock after integrate_scenario_radau(discrete_controller=...)."""
        t_last, fires = self._radau_host_ctl
        return t_last.copy(), fires.copy()

    # ---- continuous feedback (include/pfc.h, pfc_radau_set_feedback; the scalar statements: feedback_pd, feedback_pd_partials) ---
    def radau_set_feedback(self, act, kp, kd, seg_t, seg_q, seg_ff=None, a_max=None):
        """pfc_radau_set_feedback: radau_set_controller's computed-torque PD law evaluated inside the differential equation -- at
        every stage evaluation with that stage's time, and with its partials in every Jacobian chunk -- and added to the held tau
        (radau_set_tau, the discrete controller).  The arrays are radau_set_controller's, without dt and t_last0."""
        n = getattr(self, "_radau_n_scene", 0)
        nv = self.mechanism_sizes()[2]
        act_a = np.ascontiguousarray(act, dtype=np.int32).reshape(-1)
        na = act_a.size
        vec = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (na,)))
        kp_a, kd_a = vec(kp), vec(kd)
        am_a = None if a_max is None else vec(a_max)
        st = np.asarray(seg_t, dtype=np.float64)
        n_seg = st.shape[-1] if st.ndim else 1
        st_a = np.ascontiguousarray(np.broadcast_to(st.reshape(-1, n_seg), (n, n_seg)))
        sq_a = np.zeros((n, n_seg, 0)) if na == 0 else \
            np.ascontiguousarray(np.broadcast_to(np.asarray(seg_q, dtype=np.float64).reshape((-1, n_seg, na)), (n, n_seg, na)))
        ff_a = None if seg_ff is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(seg_ff, dtype=np.float64).reshape((-1, n_seg, nv)), (n, n_seg, nv)))
        p = lambda a: None if a is None else a.ctypes.data_as(_dp)
        self._check(_lib.lib().pfc_radau_set_feedback(self._h, int(na), act_a.ctypes.data_as(_ip), p(kp_a), p(kd_a), p(am_a), int(n_seg),
                                                      p(st_a), p(sq_a), p(ff_a)))

    def radau_clear_feedback(self):
        """pfc_radau_clear_feedback: the step is the step without a continuous law again."""
        self._check(_lib.lib().pfc_radau_clear_feedback(self._h))

    def radau_stage_times(self):
        """pfc_radau_stage_times: (3, n_scene), the times at which the last attempt evaluated the continuous law: row s of scene i
        is (c_s h_i) + t_i for s < NS(rule_i) and t_i otherwise.  With a law or body wrenches set (the library says so otherwise)."""
        out = np.zeros((3, getattr(self, "_radau_n_scene", 0)))
        self._check(_lib.lib().pfc_radau_stage_times(self._h, out.ctypes.data_as(_dp)))
        return out

    def feedback_device(self, n_rows: int, n_scene: int, nv: int, n_act: int, n_seg: int, d_act: int, d_kp: int, d_kd: int, d_a_max: int,
                        d_seg_t: int, d_seg_q: int, d_seg_ff: int, d_t: int, d_q: int, d_v: int, d_H: int, d_c: int, d_tau_in: int,
                        d_tau_out: int, stream: int = 0):
        """pfc_feedback_device: the law's value on raw device addresses (0: NULL for d_a_max, d_seg_ff, d_tau_in and, with one
        segment, d_seg_t); asynchronous on `stream`."""
        a = [d_act, d_kp, d_kd, d_a_max, d_seg_t, d_seg_q, d_seg_ff, d_t, d_q, d_v, d_H, d_c, d_tau_in, d_tau_out, stream]
        self._check(_lib.lib().pfc_feedback_device(self._h, int(n_rows), int(n_scene), int(nv), int(n_act), int(n_seg), *[x or None for x in a]))

    def feedback_dual_device(self, n_rows: int, n_dir: int, n_scene: int, nv: int, n_act: int, n_seg: int, d_act: int, d_kp: int,
                             d_kd: int, d_a_max: int, d_seg_t: int, d_seg_q: int, d_t: int, d_q: int, d_v: int, d_H: int, d_dq: int,
                             d_dv: int, d_dH: int, d_dc: int, d_dtau: int, stream: int = 0):
        """pfc_feedback_dual_device: the law's partials along n_dir directions on raw device addresses (0: NULL for d_a_max, d_dq,
        d_dv); asynchronous on `stream`."""
        a = [d_act, d_kp, d_kd, d_a_max, d_seg_t, d_seg_q, d_t, d_q, d_v, d_H, d_dq, d_dv, d_dH, d_dc, d_dtau, stream]
        self._check(_lib.lib().pfc_feedback_dual_device(self._h, int(n_rows), int(n_dir), int(n_scene), int(nv), int(n_act), int(n_seg),
                                                        *[x or None for x in a]))

    # ---- applied body wrenches (include/pfc.h, pfc_radau_set_body_wrenches; the scalar statements: body_wrench_tau[_partials]) ----
    def radau_set_body_wrenches(self, body, frame, point, seg_t, seg_w):
        """pfc_radau_set_body_wrenches: n_w wrenches -- body (n_w,), frame (n_w,; 0 world axes, 1 body axes), point (n_w, 3) in the
        body frame -- with loads seg_w (n_scene, n_seg, n_w, 6) = [moment; force] on the schedule seg_t (n_scene, n_seg); leading
        scene axes broadcast.  Projected into tau on the device inside the differential equation, behind the continuous law, with
        their partials in every Jacobian chunk."""
        n = getattr(self, "_radau_n_scene", 0)
        body_a = np.ascontiguousarray(body, dtype=np.int32).reshape(-1)
        nw = body_a.size
        frame_a = np.ascontiguousarray(np.broadcast_to(np.asarray(frame, dtype=np.int32), (nw,)))
        point_a = np.ascontiguousarray(np.broadcast_to(np.asarray(point, dtype=np.float64).reshape(-1, 3), (nw, 3)))
        st = np.asarray(seg_t, dtype=np.float64)
        n_seg = st.shape[-1] if st.ndim else 1
        st_a = np.ascontiguousarray(np.broadcast_to(st.reshape(-1, n_seg), (n, n_seg)))
        sw_a = np.ascontiguousarray(np.broadcast_to(np.asarray(seg_w, dtype=np.float64).reshape((-1, n_seg, nw, 6)), (n, n_seg, nw, 6)))
        self._check(_lib.lib().pfc_radau_set_body_wrenches(self._h, int(nw), body_a.ctypes.data_as(_ip), frame_a.ctypes.data_as(_ip),
                                                           point_a.ctypes.data_as(_dp), int(n_seg), st_a.ctypes.data_as(_dp),
                                                           sw_a.ctypes.data_as(_dp)))

    def radau_clear_body_wrenches(self):
        """pfc_radau_clear_body_wrenches: the step is the step without wrenches again."""
        self._check(_lib.lib().pfc_radau_clear_body_wrenches(self._h))

    def body_wrench_device(self, n_rows: int, n_scene: int, n_body: int, nv: int, n_w: int, n_seg: int, d_body: int, d_frame: int,
                           d_point: int, d_seg_t: int, d_seg_w: int, d_t: int, d_x_w_b: int, d_jac: int, d_tau_in: int, d_tau_out: int,
                           stream: int = 0):
        """pfc_body_wrench_device: the wrenches' torques added to d_tau_in on raw device addresses (0: NULL for d_tau_in and, with
        one segment, d_seg_t); asynchronous on `stream`."""
        a = [d_body, d_frame, d_point, d_seg_t, d_seg_w, d_t, d_x_w_b, d_jac, d_tau_in, d_tau_out, stream]
        self._check(_lib.lib().pfc_body_wrench_device(self._h, int(n_rows), int(n_scene), int(n_body), int(nv), int(n_w), int(n_seg),
                                                      *[x or None for x in a]))

    def body_wrench_dual_device(self, n_rows: int, n_dir: int, n_scene: int, n_body: int, nv: int, n_w: int, n_seg: int, d_body: int,
                                d_frame: int, d_point: int, d_seg_t: int, d_seg_w: int, d_t: int, d_x_w_b: int, d_jac: int, d_dx_w_b: int,
                                d_djac: int, d_dtau_in: int, d_dtau: int, stream: int = 0):
        """pfc_body_wrench_dual_device: the partials of the wrenches' torques along n_dir directions, added to d_dtau_in (0: NULL),
        on raw device addresses; asynchronous on `stream`."""
        a = [d_body, d_frame, d_point, d_seg_t, d_seg_w, d_t, d_x_w_b, d_jac, d_dx_w_b, d_djac, d_dtau_in, d_dtau, stream]
        self._check(_lib.lib().pfc_body_wrench_dual_device(self._h, int(n_rows), int(n_dir), int(n_scene), int(n_body), int(nv), int(n_w),
                                                           int(n_seg), *[x or None for x in a]))

    # ---- the gripper program (include/pfc.h, pfc_radau_set_program; the scalar statement: gripper_program_step below) -----------
    def _program_arrays(self, prog_dt, prog_q, prog_slip):
        """(n_ins, prog_dt (n_scene, n_ins), prog_q (n_scene, n_ins, n_act), prog_slip (n_scene, n_ins)): leading scene axes broadcast;
        n_act is prog_q's last axis."""
        n_act = np.shape(prog_q)[-1] if np.ndim(prog_q) >= 2 else 0
        dt = np.asarray(prog_dt, dtype=np.float64)
        n_ins = dt.shape[-1] if dt.ndim else 1
        n = getattr(self, "_radau_n_scene", 0) or dt.size // n_ins      # 0: not configured, the library says so
        dt_a = np.ascontiguousarray(np.broadcast_to(dt.reshape(-1, n_ins), (n, n_ins)))
        sl_a = np.ascontiguousarray(np.broadcast_to(np.asarray(prog_slip, dtype=np.float64).reshape(-1, n_ins), (n, n_ins)))
        q_a = np.zeros((n, n_ins, 0)) if n_act == 0 else \
            np.ascontiguousarray(np.broadcast_to(np.asarray(prog_q, dtype=np.float64).reshape((-1, n_ins, n_act)), (n, n_ins, n_act)))
        return n_ins, dt_a, q_a, sl_a

    def radau_set_program(self, body: int, grip, tau_soft: float, tau_hard: float, prog_dt, prog_q, prog_slip):
        """pfc_radau_set_program: a gripper program in front of the controller of radau_set_controller (one segment, with seg_ff).
        body the watched body; grip the grip coordinates (each one of the controller's act);
        prog_dt (n_scene, n_ins) or (n_ins,) the durations, prog_q (n_scene, n_ins, n_act) or (n_ins, n_act) the setpoints, prog_slip
        like prog_dt: -inf no grip, 0 tau_hard, +inf tau_soft, finite: tau_soft until the body has turned by that angle since the
        instruction began, then tau_hard."""
        n_ins, dt_a, q_a, sl_a = self._program_arrays(prog_dt, prog_q, prog_slip)
        if q_a.shape[2] != getattr(self, "_radau_n_act", q_a.shape[2]):
            raise ValueError("radau_set_program: prog_q has %d setpoints per instruction, the controller %d actuated coordinates"
                             % (q_a.shape[2], self._radau_n_act))
        g_a = np.ascontiguousarray(grip, dtype=np.int32).reshape(-1)
        self._check(_lib.lib().pfc_radau_set_program(self._h, int(body), int(g_a.size), g_a.ctypes.data_as(_ip), float(tau_soft),
                                                     float(tau_hard), int(n_ins), dt_a.ctypes.data_as(_dp), q_a.ctypes.data_as(_dp),
                                                     sl_a.ctypes.data_as(_dp)))

    def radau_clear_program(self):
        """pfc_radau_clear_program: the controller is the controller of radau_set_controller again."""
        self._check(_lib.lib().pfc_radau_clear_program(self._h))

    def radau_program_state(self):
        """The records of the device program: dict of cursor, pops (int32) and t0, rot_0, angle, tau_grip, arrays of n_scene."""
        n = getattr(self, "_radau_n_scene", 0)
        cur, pops = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        d = [np.zeros(n) for _ in range(4)]
        self._check(_lib.lib().pfc_radau_program_state(self._h, cur.ctypes.data_as(_ip), pops.ctypes.data_as(_ip),
                                                       *[a.ctypes.data_as(_dp) for a in d]))
        return dict(cursor=cur, pops=pops, t0=d[0], rot_0=d[1], angle=d[2], tau_grip=d[3])

    def radau_program_device(self, n_scene: int, n_body: int, nv: int, n_act: int, n_ins: int, body: int, n_grip: int, d_grip: int,
                             tau_soft: float, tau_hard: float, d_prog_dt: int, d_prog_q: int, d_prog_slip: int, d_t: int, d_t_last: int,
                             d_x_w_b: int, d_istate: int, d_cursor: int, d_pstate: int, d_seg_q: int, d_seg_ff: int, stream: int = 0):
        """pfc_radau_program_device: the program's part on raw device addresses (0: NULL); asynchronous on `stream`."""
        a = [d_prog_dt, d_prog_q, d_prog_slip, d_t, d_t_last, d_x_w_b, d_istate, d_cursor, d_pstate, d_seg_q, d_seg_ff, stream]
        self._check(_lib.lib().pfc_radau_program_device(self._h, int(n_scene), int(n_body), int(nv), int(n_act), int(n_ins), int(body),
                                                        int(n_grip), d_grip or None, float(tau_soft), float(tau_hard),
                                                        *[x or None for x in a]))

    def gripper_program_fn(self, act, kp, kd, seg_ff, body: int, grip, tau_soft: float, tau_hard: float, prog_dt, prog_q, prog_slip,
                           a_max=None):
        """fn(x, t, scene) -> tau for integrate_scenario_radau(discrete_controller=(fn, dt, t_last0)): the program and the law of
        radau_set_program + radau_set_controller on the host, with a record per scene -- the angle from the host form `kinematics`
        (math.atan2), gripper_program_step, then computed_torque_pd on `dynamics`' H and c with the segment the program wrote.
        seg_ff (n_scene, nv) or (nv,): the feed-forward of the one segment; the arrays as radau_set_program's.  fn.records is the list
        of the scenes' records."""
        n = self._radau_n_scene
        _, nq, nv = self.mechanism_sizes()
        act_l = [int(a) for a in np.asarray(act).reshape(-1)]
        na = len(act_l)
        vec = lambda a: [float(e) for e in np.broadcast_to(np.asarray(a, dtype=np.float64), (na,))]
        kp_l, kd_l = vec(kp), vec(kd)
        am_l = None if a_max is None else vec(a_max)
        grip_l = [int(g) for g in np.asarray(grip).reshape(-1)]
        _, dt_a, q_a, sl_a = self._program_arrays(prog_dt, prog_q, prog_slip)
        ff = np.array(np.broadcast_to(np.asarray(seg_ff, dtype=np.float64).reshape(-1, nv), (n, nv)))      # written by the program
        records = [dict(PROGRAM_RECORD0) for _ in range(n)]
        body = int(body)

        def fn(x, t, scene):
            q, v = np.asarray(x[:nq], dtype=np.float64), np.asarray(x[nq:nq + nv], dtype=np.float64)
            x_w_b, tw, _ = self.kinematics(q, v, want_jac=False)
            angle = rotation_angle(x_w_b[0, body, :9])
            records[scene], seg_q, tau_grip = gripper_program_step(records[scene], t, angle, dt_a[scene].tolist(), q_a[scene].tolist(),
                                                                   sl_a[scene].tolist(), tau_soft, tau_hard)
            for g in grip_l:
                ff[scene, g] = tau_grip
            _, H, c = self.dynamics(q, v, x_w_b, tw)
            return computed_torque_pd(q.tolist(), v.tolist(), H[0].tolist(), c[0].tolist(), float(t), act_l, kp_l, kd_l, [0.0], [seg_q],
                                      [ff[scene].tolist()], am_l)
        fn.records = records
        return fn

    def radau_host_tau(self):
        """tau (n_scene, nv) as the host route last set it (integrate_scenario_radau(discrete_controller=...))."""
        return self._radau_host_tau.copy()

    def _integrate_with_callback(self, tf, max_steps: int, discrete_controller):
        """The host route: the reference's loop (src/example_integrator.jl:25-30) per live scene before every batch step -- t_last by
        repeated addition, fn called at every addition -- then radau_set_tau and one radau_step."""
        fn, dt = discrete_controller[0], float(discrete_controller[1])
        n, nv = self._radau_n_scene, self.mechanism_sizes()[2]
        if not (dt > 0.0 and np.isfinite(dt)):
            raise ValueError("discrete_controller: dt must be finite and > 0")
        max_rows = int(max_steps) + 1
        x, t = self.radau_get_state()
        t_last = t.copy() if len(discrete_controller) < 3 or discrete_controller[2] is None else \
            np.array(np.broadcast_to(np.asarray(discrete_controller[2], dtype=np.float64), (n,)))
        fires = np.zeros(n, dtype=np.int32)
        tau = np.zeros((n, nv))
        live = np.ones(n, dtype=bool)
        fl = np.zeros(n, dtype=np.int32)
        steps = 0
        while live.any() and steps < int(max_steps):
            for s in np.flatnonzero(live):
                k = 0
                while t_last[s] <= t[s] and k < RADAU_MAX_FIRES:
                    t_last[s] = t_last[s] + dt
                    k += 1
                    tau[s] = np.asarray(fn(x[s].copy(), float(t[s]), int(s)), dtype=np.float64).reshape(nv)
                fires[s] += k
            self.radau_set_tau(tau)
            self._check(_lib.lib().pfc_radau_step(self._h, None, fl.ctypes.data_as(_ip), None, None))
            steps += 1
            x, t = self.radau_get_state()
            rows = self.radau_trajectory_rows()
            live = (fl == 0) & ~(tf < t) & (rows < max_rows)      # neither retired (5) nor parked (6, or by this commit)
        self._radau_host_ctl = (t_last, fires)
        self._radau_host_tau = tau

    def integrate_scenario_radau(self, t_final, max_steps: int = 1000, discrete_controller=None, continuous_controller=None):
        """The reference's integrate_scenario_radau for every scene of the batch: from the state as it is, each scene steps while
        t_final < t is false (t_final a scalar or (n_scene,); the last step is not shortened) and for at most max_steps steps.  Returns
        per scene (data_time, data_state), the reference's return value: the start and every step.  A scene whose step size fell
        below h_min raises the reference's "time step is too small, something is wrong" (the other scenes were integrated to their
        ends first).
        A controller given with radau_set_controller runs on the device inside the loop.  discrete_controller = (fn, dt) or (fn, dt,
        t_last0) is the reference's general DiscreteControl instead, on the host: before every batch step, for every live scene,
        `while t_last <= t: t_last += dt; tau[scene] = fn(x, t, scene)` (at most RADAU_MAX_FIRES additions per step), then
        radau_set_tau and one radau_step -- any Python law, one batch step at a time, x downloaded and tau uploaded per step.  tau
        starts from zeros; t_last0 None is every scene's t now.  Not to be combined with radau_set_controller.
        continuous_controller: the reference's continuous slot, here the tables of radau_set_feedback as a dict (act, kp, kd, seg_t,
        seg_q and optionally seg_ff, a_max): the law is set for this run -- evaluated on the device inside the differential
        equation, with either kind of discrete controller beside it -- and cleared when the run ends."""
        n = self._radau_n_scene
        tf = np.ascontiguousarray(np.broadcast_to(np.asarray(t_final, dtype=np.float64), (n,)))
        if continuous_controller is not None:
            self.radau_set_feedback(**continuous_controller)
        try:
            self.radau_set_end(tf, int(max_steps) + 1)
            if discrete_controller is None:
                self.radau_integrate(int(max_steps))
            else:
                self._integrate_with_callback(tf, int(max_steps), discrete_controller)
        finally:
            if continuous_controller is not None:
                self.radau_clear_feedback()
        rows = self.radau_trajectory_rows()
        out = [self.radau_trajectory(s, rows[s]) for s in range(n)]
        # a scene stops by parking -- past its end, or its rows full -- or by retiring with exit flag 5
        small = [s for s in range(n) if out[s][0].size < int(max_steps) + 1 and not tf[s] < out[s][0][-1]]
        if small:
            raise _lib.PFCError(_lib.ERR_STATE, "time step is too small, something is wrong (scenes %s)" % small)
        return out

    # ---- parts of the Radau IIA step (include/pfc.h, csrc/pfc_radau.h): raw device addresses, asynchronous on `stream` ----------
    # layout = (n_scene, nx, nq, nv, n_ips, br_items): x = [q; v; 6 states per bristle item], br_items the bristle items of a scene.
    @staticmethod
    def _radau_layout(layout):
        n_scene, nx, nq, nv, n_ips, br = layout
        br_a = np.ascontiguousarray(br, dtype=np.int32).reshape(-1)
        return [int(n_scene), int(nx), int(nq), int(nv), int(n_ips), int(br_a.size), br_a.ctypes.data_as(_ip)], br_a

    def radau_seed_device(self, layout, chunk: int, n_chunk: int, d_dq: int, d_dv: int, d_ds: int, stream: int = 0):
        """pfc_radau_seed_device: the unit seeds of a Jacobian chunk in state_derivative_dual_device's seed layouts."""
        head, keep = self._radau_layout(layout)
        self._check(_lib.lib().pfc_radau_seed_device(self._h, *head, int(chunk), int(n_chunk), d_dq or None, d_dv or None, d_ds or None,
                                                     stream or None))

    def radau_jacobian_device(self, layout, chunk: int, n_chunk: int, d_dqdot: int, d_dvdot: int, d_dsdot: int, d_qdot: int, d_vdot: int,
                              d_sdot: int, d_neg_J: int, d_xdot0: int, d_nstate: int = 0, d_istate: int = 0, stream: int = 0):
        """pfc_radau_jacobian_device: a chunk's partials into columns of -J; chunk 0 also writes xdot0 and arms the scenes."""
        head, keep = self._radau_layout(layout)
        a = [d_dqdot, d_dvdot, d_dsdot, d_qdot, d_vdot, d_sdot, d_neg_J, d_xdot0, d_nstate, d_istate, stream]
        self._check(_lib.lib().pfc_radau_jacobian_device(self._h, *head, int(chunk), int(n_chunk), *[p or None for p in a]))

    def radau_factor_device(self, n_scene: int, nx: int, d_neg_J: int, d_h: int, d_rule: int, d_active: int, d_lu0: int, d_lu1: int,
                            d_perm: int, d_info: int, stream: int = 0):
        """pfc_radau_factor_device: the LU factors of -J + (lam / h) I per scene, real and (rule 2) complex."""
        a = [d_neg_J, d_h, d_rule, d_active, d_lu0, d_lu1, d_perm, d_info, stream]
        self._check(_lib.lib().pfc_radau_factor_device(self._h, int(n_scene), int(nx), *[p or None for p in a]))

    def radau_unpack_device(self, layout, d_x0: int, d_rule: int, d_istate: int, d_X: int, d_q: int, d_v: int, d_s: int, stream: int = 0):
        """pfc_radau_unpack_device: the stage states into (q, v, s) of the 3 n_scene stage-scenes."""
        head, keep = self._radau_layout(layout)
        a = [d_x0, d_rule, d_istate, d_X, d_q, d_v, d_s, stream]
        self._check(_lib.lib().pfc_radau_unpack_device(self._h, *head, *[p or None for p in a]))

    def radau_newton_device(self, layout, d_qdot: int, d_vdot: int, d_sdot: int, d_x0: int, d_h: int, d_rule: int, d_lu0: int, d_lu1: int,
                            d_perm: int, d_info: int, tol_newton: float, k_iter_max: int, d_X: int, d_F_save: int, d_nstate: int,
                            d_istate: int, d_count: int, stream: int = 0):
        """pfc_radau_newton_device: one iteration of simple_newton! for every iterating scene (d_F_save 0: F is not kept)."""
        head, keep = self._radau_layout(layout)
        a = [d_qdot, d_vdot, d_sdot, d_x0, d_h, d_rule, d_lu0, d_lu1, d_perm, d_info]
        b = [d_X, d_F_save, d_nstate, d_istate, d_count, stream]
        self._check(_lib.lib().pfc_radau_newton_device(self._h, *head, *[p or None for p in a], float(tol_newton), int(k_iter_max),
                                                       *[p or None for p in b]))

    def radau_finish_device(self, layout, mrp_off, params, k_iter_max: int, max_rule: int, cooldown: int, d_F: int, d_xdot0: int, d_X: int, d_lu0: int, d_perm: int, d_x: int, d_t: int, d_h: int, d_rule: int,
                            d_cool: int, d_enorm: int, d_nstate: int, d_istate: int, d_count: int, stream: int = 0):
        """pfc_radau_finish_device: the end of an attempt -- error norm, new h and rule, the commit or the re-arming.  mrp_off: the
        offsets in q of the floating joints' MRPs; params = (tol_a, tol_r, h_max, h_min)."""
        head, keep = self._radau_layout(layout)
        m_a = np.ascontiguousarray(mrp_off, dtype=np.int32).reshape(-1)
        p_a = np.ascontiguousarray(params, dtype=np.float64).reshape(4)
        a = [d_F, d_xdot0, d_X, d_lu0, d_perm, d_x, d_t, d_h, d_rule, d_cool, d_enorm, d_nstate, d_istate, d_count, stream]
        self._check(_lib.lib().pfc_radau_finish_device(self._h, *head, int(m_a.size), m_a.ctypes.data_as(_ip), p_a.ctypes.data_as(_dp),
                                                       int(k_iter_max), int(max_rule), int(cooldown), *[p or None for p in a]))

    def radau_finish_end_device(self, layout, mrp_off, params, k_iter_max: int, max_rule: int, cooldown: int, d_F: int, d_xdot0: int,
                                d_X: int, d_lu0: int, d_perm: int, d_x: int, d_t: int, d_h: int, d_rule: int, d_cool: int, d_enorm: int,
                                d_nstate: int, d_istate: int, d_count: int, d_t_final: int, d_traj: int, d_rows: int, max_rows: int,
                                d_live: int, stream: int = 0):
        """pfc_radau_finish_end_device: radau_finish_device with ends -- a commit appends the row (t, x) to the scene's trajectory,
        parks the scene past d_t_final (0: +inf) or on its last row, and counts the scenes that go on in *d_live (not zeroed)."""
        head, keep = self._radau_layout(layout)
        m_a = np.ascontiguousarray(mrp_off, dtype=np.int32).reshape(-1)
        p_a = np.ascontiguousarray(params, dtype=np.float64).reshape(4)
        a = [d_F, d_xdot0, d_X, d_lu0, d_perm, d_x, d_t, d_h, d_rule, d_cool, d_enorm, d_nstate, d_istate, d_count, d_t_final, d_traj, d_rows]
        self._check(_lib.lib().pfc_radau_finish_end_device(self._h, *head, int(m_a.size), m_a.ctypes.data_as(_ip), p_a.ctypes.data_as(_dp),
                                                           int(k_iter_max), int(max_rule), int(cooldown), *[p or None for p in a],
                                                           int(max_rows), d_live or None, stream or None))

    def dual_seeds_from_bodies(self, x_w_b, twist_w_b, d_x_w_b, d_twist_w_b, ins_ids: Optional[Sequence[int]] = None,
                               scene=None) -> BodySeeds:
        """The Dual seeds of items_from_bodies' items from the partials of the bodies' world states (pfc_dual_seeds_from_bodies, host
        buffers, synchronous).  x_w_b, twist_w_b, ins_ids, scene as items_from_bodies; d_x_w_b (n_body,n_dir,12) or
        (n_scene,n_body,n_dir,12) and d_twist_w_b likewise with 6, either may be None (zeros), not both (n_dir comes from them)."""
        n, head, it, outs, keep = self._bodies_call(x_w_b, twist_w_b, ins_ids, scene)
        n_scene, n_body = head[4], head[5]
        if d_x_w_b is None and d_twist_w_b is None:
            raise ValueError("one of d_x_w_b and d_twist_w_b must be given: they carry n_dir")
        dx_a = dtw_a = dx_p = dtw_p = None
        n_dir = None
        for a, width, name in ((d_x_w_b, 12, "d_x_w_b"), (d_twist_w_b, 6, "d_twist_w_b")):
            if a is None:
                continue
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.ndim == 3:
                a = a[None]
            if a.ndim != 4 or a.shape[0] != n_scene or a.shape[1] != n_body or a.shape[3] != width or (n_dir not in (None, a.shape[2])):
                raise ValueError(f"{name} must be (n_body, n_dir, {width}) or (n_scene, n_body, n_dir, {width})")
            n_dir = a.shape[2]
            if width == 12:
                dx_a, dx_p = a, a.ctypes.data_as(_dp)
            else:
                dtw_a, dtw_p = a, a.ctypes.data_as(_dp)
        sd = BodySeeds(np.zeros((n, n_dir, 24)), np.zeros((n, n_dir, 6)), np.zeros((n, n_dir, 12)))
        self._check(_lib.lib().pfc_dual_seeds_from_bodies(head[0], n, n_dir, *head[2:], dx_p, dtw_p, sd.d_pose.ctypes.data_as(_dp),
                                                          sd.d_twist.ctypes.data_as(_dp), sd.d_x_w_r2.ctypes.data_as(_dp)))
        return sd

    def force_all_elastic_intersections_dual_bodies(self, x_w_b, twist_w_b, s, d_x_w_b, d_twist_w_b, d_s=None,
                                                    ins_ids: Optional[Sequence[int]] = None, scene=None):
        """force_all_elastic_intersections_dual on the items of items_from_bodies and the seeds of dual_seeds_from_bodies (host
        buffers, synchronous; three calls composed here).  Returns (wrench, sdot, d_wrench, d_sdot, counts, items: BodyItems,
        seeds: BodySeeds)."""
        it = self.items_from_bodies(x_w_b, twist_w_b, ins_ids, scene)
        sd = self.dual_seeds_from_bodies(x_w_b, twist_w_b, d_x_w_b, d_twist_w_b, ins_ids, scene)
        out = self.force_all_elastic_intersections_dual(it.pose, it.twist, s, sd.d_pose, sd.d_twist, d_s, ins_ids)
        return (*out, it, sd)

    def dual_seeds_from_bodies_device(self, n_items: int, n_dir: int, d_ins_ids: int, d_scene: int, n_scene: int, n_body: int,
                                      d_x_w_b: int, d_twist_w_b: int, d_dx_w_b: int, d_dtwist_w_b: int, d_dpose: int, d_dtwist: int,
                                      d_dx_w_r2: int, stream: int = 0):
        """pfc_dual_seeds_from_bodies_device: raw device addresses (0: NULL for d_ins_ids, d_scene, either partial array and any output
        not wanted); asynchronous on `stream`, not an evaluation, no check() needed."""
        self._check(_lib.lib().pfc_dual_seeds_from_bodies_device(
            self._h, int(n_items), int(n_dir), d_ins_ids or None, d_scene or None, int(n_scene), int(n_body), d_x_w_b or None,
            d_twist_w_b or None, d_dx_w_b or None, d_dtwist_w_b or None, d_dpose or None, d_dtwist or None, d_dx_w_r2 or None,
            stream or None))

    def eval_dual_bodies_device(self, n_items: int, n_dir: int, d_ins_ids: int, d_scene: int, n_scene: int, n_body: int, d_x_w_b: int,
                                d_twist_w_b: int, d_dx_w_b: int, d_dtwist_w_b: int, d_s: int, d_ds: int, d_pose: int, d_twist: int,
                                d_x_w_r2: int, d_body_1: int, d_body_2: int, d_dpose: int, d_dtwist: int, d_dx_w_r2: int, d_wrench: int,
                                d_sdot: int, d_dwrench: int, d_dsdot: int, d_counts: int, stream: int = 0):
        """pfc_eval_dual_bodies_device: items_from_bodies_device, dual_seeds_from_bodies_device, then eval_dual_device on the buffers
        they wrote, on one stream; asynchronous, follow with check() (re-issue on ERR_OVERFLOW)."""
        self._check(_lib.lib().pfc_eval_dual_bodies_device(
            self._h, int(n_items), int(n_dir), d_ins_ids or None, d_scene or None, int(n_scene), int(n_body), d_x_w_b or None,
            d_twist_w_b or None, d_dx_w_b or None, d_dtwist_w_b or None, d_s or None, d_ds or None, d_pose, d_twist, d_x_w_r2 or None,
            d_body_1 or None, d_body_2 or None, d_dpose, d_dtwist, d_dx_w_r2 or None, d_wrench, d_sdot, d_dwrench, d_dsdot,
            d_counts or None, stream or None))

    def eval_dual_bodies_device_more(self, n_items: int, n_dir: int, d_ins_ids: int, d_scene: int, n_scene: int, n_body: int,
                                     d_x_w_b: int, d_twist_w_b: int, d_dx_w_b: int, d_dtwist_w_b: int, d_ds: int, d_dpose: int,
                                     d_dtwist: int, d_dx_w_r2: int, d_dwrench: int, d_dsdot: int, stream: int = 0):
        """pfc_eval_dual_bodies_device_more: dual_seeds_from_bodies_device, then eval_dual_device_more on the seeds it wrote (a later
        chunk of the Jacobian at the kept point); asynchronous, follow with check()."""
        self._check(_lib.lib().pfc_eval_dual_bodies_device_more(
            self._h, int(n_items), int(n_dir), d_ins_ids or None, d_scene or None, int(n_scene), int(n_body), d_x_w_b or None,
            d_twist_w_b or None, d_dx_w_b or None, d_dtwist_w_b or None, d_ds or None, d_dpose, d_dtwist, d_dx_w_r2 or None, d_dwrench,
            d_dsdot, stream or None))

    def contact_surface(self, pose, twist, ins_ids: Optional[Sequence[int]] = None) -> ContactSurface:
        """The contact surface of every item (pfc_contact_surface): clipped polygons, traction points and normal wrench / cop in
        one canonical order (see ContactSurface).  pose (n,24), twist (n,6), ins_ids (n,) or None.  The buffers start at the
        size of the previous call's surface; if the surface is bigger they are grown to its totals and the call is issued again."""
        if not self._finalized:
            raise RuntimeError("finalize the scenario first")
        pose_a, pose_p = _da(pose)
        n = pose_a.size // 24
        if pose_a.size != 24 * n:
            raise ValueError("pose must have 24 entries per item")
        tw_a, tw_p = _da(twist)
        if tw_a.size != 6 * n:
            raise ValueError("twist must have 6 entries per item")
        id_p = None
        if ins_ids is not None:
            id_a, id_p = _ia(ins_ids)
            if id_a.size != n:
                raise ValueError("ins_ids must have one entry per item")
        cap_p, cap_t = getattr(self, "_surf_caps", (max(64, 8 * n), max(512, 64 * n)))
        L = _lib.lib()
        for attempt in range(2):
            poly_off = np.zeros(n + 1, dtype=np.int64); poly_idx = np.zeros((cap_p, 3), dtype=np.int32)
            poly_xyz = np.zeros((cap_p, 8, 3)); poly_trac = np.zeros(cap_p + 1, dtype=np.int64); trac = np.zeros((cap_t, 8))
            summary = np.zeros((n, 11)); counts = np.zeros((n, 4), dtype=np.int32); totals = np.zeros(2, dtype=np.int64)
            rc = L.pfc_contact_surface(self._h, n, None if id_p is None else C.cast(id_p, _ip), C.cast(pose_p, _dp), C.cast(tw_p, _dp),
                                       cap_p, cap_t, poly_off.ctypes.data_as(_llp), poly_idx.ctypes.data_as(_ip),
                                       poly_xyz.ctypes.data_as(_dp), poly_trac.ctypes.data_as(_llp), trac.ctypes.data_as(_dp),
                                       summary.ctypes.data_as(_dp), counts.ctypes.data_as(_ip), totals.ctypes.data_as(_llp))
            if rc == _lib.ERR_OVERFLOW and attempt == 0:
                cap_p, cap_t = max(cap_p, int(totals[0])), max(cap_t, int(totals[1]))
                continue
            self._check(rc)
            break
        self._surf_caps = (cap_p, cap_t)
        P, T = int(totals[0]), int(totals[1])
        return ContactSurface(poly_off, poly_idx[:P], poly_xyz[:P], poly_trac[:P + 1], trac[:T], summary, counts)

    def contact_surface_fric(self, pose, twist, s=None, ins_ids: Optional[Sequence[int]] = None) -> FrictionSurface:
        """The contact surface with its friction half (pfc_contact_surface_fric; see FrictionSurface).  pose (n,24), twist (n,6),
        s (n,6) or None (zeros), ins_ids (n,) or None.  Buffers grow and the call is re-issued as in contact_surface."""
        if not self._finalized:
            raise RuntimeError("finalize the scenario first")
        pose_a, pose_p = _da(pose)
        n = pose_a.size // 24
        if pose_a.size != 24 * n:
            raise ValueError("pose must have 24 entries per item")
        tw_a, tw_p = _da(twist)
        if tw_a.size != 6 * n:
            raise ValueError("twist must have 6 entries per item")
        s_p = None
        if s is not None:
            s_a, s_p = _da(s)
            if s_a.size != 6 * n:
                raise ValueError("s must have 6 entries per item")
        id_p = None
        if ins_ids is not None:
            id_a, id_p = _ia(ins_ids)
            if id_a.size != n:
                raise ValueError("ins_ids must have one entry per item")
        cap_p, cap_t = getattr(self, "_surf_caps", (max(64, 8 * n), max(512, 64 * n)))
        L = _lib.lib()
        for attempt in range(2):
            poly_off = np.zeros(n + 1, dtype=np.int64); poly_idx = np.zeros((cap_p, 3), dtype=np.int32)
            poly_xyz = np.zeros((cap_p, 8, 3)); poly_trac = np.zeros(cap_p + 1, dtype=np.int64); trac = np.zeros((cap_t, 8))
            fric = np.zeros((cap_t, 4)); summary = np.zeros((n, 11)); fric_summary = np.zeros((n, 20)); stiff = np.zeros((n, 84))
            counts = np.zeros((n, 4), dtype=np.int32); totals = np.zeros(2, dtype=np.int64)
            rc = L.pfc_contact_surface_fric(self._h, n, None if id_p is None else C.cast(id_p, _ip), C.cast(pose_p, _dp), C.cast(tw_p, _dp),
                                            None if s_p is None else C.cast(s_p, _dp), cap_p, cap_t, poly_off.ctypes.data_as(_llp),
                                            poly_idx.ctypes.data_as(_ip), poly_xyz.ctypes.data_as(_dp), poly_trac.ctypes.data_as(_llp),
                                            trac.ctypes.data_as(_dp), fric.ctypes.data_as(_dp), summary.ctypes.data_as(_dp),
                                            fric_summary.ctypes.data_as(_dp), stiff.ctypes.data_as(_dp), counts.ctypes.data_as(_ip),
                                            totals.ctypes.data_as(_llp))
            if rc == _lib.ERR_OVERFLOW and attempt == 0:
                cap_p, cap_t = max(cap_p, int(totals[0])), max(cap_t, int(totals[1]))
                continue
            self._check(rc)
            break
        self._surf_caps = (cap_p, cap_t)
        P, T = int(totals[0]), int(totals[1])
        surface = ContactSurface(poly_off, poly_idx[:P], poly_xyz[:P], poly_trac[:P + 1], trac[:T], summary, counts)
        return FrictionSurface(surface, fric[:T], fric_summary, stiff)

    def contact_surface_device(self, n_items: int, d_ins_ids: int, d_pose: int, d_twist: int, cap_poly: int, cap_trac: int,
                               d_poly_off: int, d_poly_idx: int, d_poly_xyz: int, d_poly_trac: int, d_trac: int, d_summary: int,
                               d_counts: int, d_totals: int, stream: int = 0):
        """pfc_contact_surface_device: raw device addresses; asynchronous; follow with check() (ERR_OVERFLOW: re-issue, after
        growing the buffers if the totals exceed a capacity)."""
        self._check(_lib.lib().pfc_contact_surface_device(self._h, int(n_items), d_ins_ids or None, d_pose, d_twist, int(cap_poly),
                                                          int(cap_trac), d_poly_off, d_poly_idx or None, d_poly_xyz or None, d_poly_trac,
                                                          d_trac or None, d_summary or None, d_counts or None, d_totals,
                                                          stream or None))

    def contact_surface_fric_device(self, n_items: int, d_ins_ids: int, d_pose: int, d_twist: int, d_s: int, cap_poly: int,
                                    cap_trac: int, d_poly_off: int, d_poly_idx: int, d_poly_xyz: int, d_poly_trac: int, d_trac: int,
                                    d_fric: int, d_summary: int, d_fric_summary: int, d_stiff: int, d_counts: int, d_totals: int,
                                    stream: int = 0):
        """pfc_contact_surface_fric_device: raw device addresses (d_s, d_stiff, d_counts may be 0); asynchronous; follow with
        check(), as after contact_surface_device."""
        self._check(_lib.lib().pfc_contact_surface_fric_device(self._h, int(n_items), d_ins_ids or None, d_pose, d_twist, d_s or None,
                                                               int(cap_poly), int(cap_trac), d_poly_off, d_poly_idx or None,
                                                               d_poly_xyz or None, d_poly_trac, d_trac or None, d_fric or None,
                                                               d_summary or None, d_fric_summary or None, d_stiff or None,
                                                               d_counts or None, d_totals, stream or None))

    def check(self) -> int:
        """pfc_check: synchronise; returns the status (PFC_ERR_OVERFLOW means: re-issue, buffers were grown)."""
        rc = _lib.lib().pfc_check(self._h)
        if rc not in (_lib.OK, _lib.ERR_OVERFLOW):
            self._check(rc)
        return rc

    def stats(self) -> dict:
        out = (C.c_longlong * 8)()
        self._check(_lib.lib().pfc_get_stats(self._h, out))
        k = ("node_tests", "candidates", "nonempty", "tractions", "levels", "frontier_peak", "status", "n_items")
        return dict(zip(k, [int(v) for v in out]))

    def last_parts(self) -> int:
        """1, or 2 if the last checked evaluation ran as two concurrent halves (option split_min); 0 if it ran as the
        single fused small-scene kernel (option fused)."""
        return int(_lib.lib().pfc_last_parts(self._h))

    def last_shards(self) -> int:
        """Devices that took part in the last evaluation (1 for a single-device scenario)."""
        return int(_lib.lib().pfc_last_shards(self._h))

    def last_shard_bounds(self) -> list:
        """Debug view of the last partition: [b_0 = 0, b_1, ..., b_used = n_items]; device k evaluated items [b_k, b_k+1).
        [0, n_items] for a single-device scenario."""
        L = _lib.lib()
        out = (C.c_int * (max(L.pfc_last_shards(self._h), 1) + 1))()
        n = L.pfc_last_shard_bounds(self._h, out, len(out))
        if n < 0:
            self._check(-n)
        return [int(v) for v in out[:n + 1]]

    def last_team(self) -> int:
        """Workgroups per item of the last checked evaluation if it ran as one fused kernel (> 1: a team per item), else 0."""
        return int(_lib.lib().pfc_last_team(self._h))

    def last_dual_reused(self) -> bool:
        """True if the last Dual evaluation ran only its Dual passes on the previous one's value pass."""
        return bool(_lib.lib().pfc_last_dual_reused(self._h))

    def stage_ms(self) -> dict:
        out = (C.c_float * 6)()
        self._check(_lib.lib().pfc_get_stage_ms(self._h, out))
        k = ("setup", "broadphase", "narrowphase", "bristle", "final", "total")
        return dict(zip(k, [float(v) for v in out]))

    # ---- debug views (m.float.bodyBodyCache of the reference's tests) -------------------------------------------
    def debug_pairs(self, item: int):
        L = _lib.lib()
        n = self._id(L.pfc_debug_pairs(self._h, item, None, None, 0))
        pairs = np.zeros((max(n, 1), 2), dtype=np.int32); clip_n = np.zeros(max(n, 1), dtype=np.int32)
        self._id(L.pfc_debug_pairs(self._h, item, pairs.ctypes.data_as(_ip), clip_n.ctypes.data_as(_ip), n))
        return pairs[:n], clip_n[:n]

    def debug_tractions(self, item: int) -> np.ndarray:
        L = _lib.lib()
        n = self._id(L.pfc_debug_tractions(self._h, item, None, 0))
        buf = np.zeros((max(n, 1), 8))
        self._id(L.pfc_debug_tractions(self._h, item, buf.ctypes.data_as(_dp), n))
        return buf[:n]

    def debug_stiffness(self, item: int):
        K = np.zeros(36); Kis = np.zeros(36); Sinv = np.zeros(6); cop = np.zeros(3)
        n = self._id(_lib.lib().pfc_debug_stiffness(self._h, item, K.ctypes.data_as(_dp), Kis.ctypes.data_as(_dp),
                                                    Sinv.ctypes.data_as(_dp), cop.ctypes.data_as(_dp)))
        if n == 0:
            return None
        return K.reshape(6, 6, order="F"), Kis.reshape(6, 6, order="F"), Sinv, cop


# ---- host helpers standing in for the RigidBodyDynamics calls of refreshBodyBodyTransform!/Cache! -----------------
def radau_table(rule: int) -> dict:
    """The Radau IIA constants compiled into the library (pfc_radau_table; generated by scripts/radau_tables.py): rule 1 (one stage) or
    2 (three stages).  c (s,), A (s,s), lam (s,) complex, T and Tinv (s,s) complex with A^-1 T = T diag(lam), bhat0, bhat (s,)."""
    ns = C.c_int(0)
    c = np.zeros(3); A = np.zeros(9); lam = np.zeros(6); T = np.zeros(18); Ti = np.zeros(18); bh = np.zeros(4)
    rc = _lib.lib().pfc_radau_table(int(rule), C.byref(ns), *[a.ctypes.data_as(_dp) for a in (c, A, lam, T, Ti, bh)])
    if rc != _lib.OK:
        raise _lib.PFCError(rc, "pfc_radau_table: rules 1 and 2 only")
    s = ns.value
    cx = lambda a, shape: (a[:2 * int(np.prod(shape))].reshape(-1, 2) @ np.array([1.0, 1.0j])).reshape(shape)
    return dict(c=c[:s].copy(), A=A[:s * s].reshape(s, s).copy(), lam=cx(lam, (s,)), T=cx(T, (s, s)), Tinv=cx(Ti, (s, s)),
                bhat0=float(bh[0]), bhat=bh[1:1 + s].copy())


# ---- the discrete controller: the scalar statement of include/pfc.h (pfc_radau_control_device) in Python floats ---------------------
RADAU_MAX_FIRES = 4096      # PFC_RADAU_MAX_FIRES


def discrete_clock(t_last: float, t: float, dt: float):
    """The reference's `while ctrl.t_last <= t: ctrl.t_last += ctrl.dt` by repeated addition, at most RADAU_MAX_FIRES times.
    Returns (t_last, fires)."""
    t_last, t, dt, fires = float(t_last), float(t), float(dt), 0
    while t_last <= t and fires < RADAU_MAX_FIRES:
        t_last = t_last + dt
        fires += 1
    return t_last, fires


def computed_torque_pd(q, v, H, c, t, act, kp, kd, seg_t, seg_q, seg_ff=None, a_max=None):
    """The law of one scene at one firing, in the written order: q, v (nv) the state; H (nv x nv, rows) and c (nv) the mass matrix and
    bias at it; act the actuated coordinates, increasing; kp, kd, a_max (None: no clamp) per actuated coordinate; seg_t (n_seg; entry
    0 is not read), seg_q (n_seg x n_act), seg_ff (n_seg x nv, or None: zeros) the schedule.  Returns tau (nv floats):
    k = #{j >= 1: seg_t[j] <= t};  acc_a = (-(kd_a v_a)) - kp_a (q_a - seg_q[k][a]), clamped to [-a_max_a, a_max_a];
    tau_a = ((..(0 + H[a][b0] acc_b0) + ..) + c_a) + ff[k][a];  tau_i = ff[k][i] elsewhere."""
    t = float(t)
    nv = len(c)
    k = sum(1 for j in range(1, len(seg_t)) if float(seg_t[j]) <= t)
    acc = []
    for a, co in enumerate(act):
        e = float(q[co]) - float(seg_q[k][a])
        x = (-(float(kd[a]) * float(v[co]))) - float(kp[a]) * e
        if a_max is not None:
            am = float(a_max[a])
            if x < -am:
                x = -am
            if x > am:
                x = am
        acc.append(x)
    ff = [0.0] * nv if seg_ff is None else [float(e) for e in seg_ff[k]]
    tau = list(ff)
    for co in act:
        s = 0.0
        for b, cb in enumerate(act):
            s = s + float(H[co][cb]) * acc[b]
        tau[co] = (s + float(c[co])) + ff[co]
    return tau


# ---- continuous feedback: the scalar statements of include/pfc.h (pfc_feedback_device, pfc_feedback_dual_device) in Python floats ----
def feedback_pd(q, v, H, c, t, tau_in, act, kp, kd, seg_t, seg_q, seg_ff=None, a_max=None):
    """The continuous law of one row: computed_torque_pd at (q, v, H, c, t) plus tau_in (nv floats, or None).  An actuated
    coordinate: law_a + tau_in_a; any other: ff[k][i] + tau_in_i with seg_ff given, tau_in_i copied (a signed zero survives) without;
    tau_in None: the law alone, +0.0 where there is none."""
    law = computed_torque_pd(q, v, H, c, t, act, kp, kd, seg_t, seg_q, seg_ff, a_max)
    if tau_in is None:
        return law
    actuated = set(int(co) for co in act)
    return [law[i] + float(tau_in[i]) if (i in actuated or seg_ff is not None) else float(tau_in[i]) for i in range(len(law))]


def feedback_pd_partials(q, v, H, t, dq, dv, dH, dc, act, kp, kd, seg_t, seg_q, a_max=None):
    """The partials of feedback_pd along one direction: dq, dv (nv, or None: zeros) the seeds, dH (nv x nv) and dc (nv) the partials
    of H and c.  The value statement on (value, partial) numbers with the product rule d(a b) = da b + a db; t, the tables and
    tau_in are constants.  dacc_a = (-(kd_a dv_a)) - kp_a dq_a, 0.0 where the value's clamp engaged; dtau_a = ((0 + (dH[a][b0]
    acc_b0 + H[a][b0] dacc_b0)) + ..) + dc_a; 0.0 for a coordinate that is not actuated.  Returns dtau (nv floats)."""
    t = float(t)
    nv = len(dc)
    k = sum(1 for j in range(1, len(seg_t)) if float(seg_t[j]) <= t)
    acc, dacc = [], []
    for a, co in enumerate(act):
        e = float(q[co]) - float(seg_q[k][a])
        x = (-(float(kd[a]) * float(v[co]))) - float(kp[a]) * e
        dqa = 0.0 if dq is None else float(dq[co])
        dva = 0.0 if dv is None else float(dv[co])
        dx = (-(float(kd[a]) * dva)) - float(kp[a]) * dqa
        if a_max is not None:
            am = float(a_max[a])
            if x < -am:
                x, dx = -am, 0.0
            if x > am:
                x, dx = am, 0.0
        acc.append(x)
        dacc.append(dx)
    dtau = [0.0] * nv
    for co in act:
        s = 0.0
        for b, cb in enumerate(act):
            s = s + (float(dH[co][cb]) * acc[b] + float(H[co][cb]) * dacc[b])
        dtau[co] = s + float(dc[co])
    return dtau


# ---- applied body wrenches: the scalar statements of include/pfc.h (pfc_body_wrench_device, pfc_body_wrench_dual_device) ------------
class _Dual:
    """ScatDual (csrc/pfc_scatter.h) in Python floats: a value and one partial; sums componentwise, d(a b) = da b + a db."""
    __slots__ = ("v", "d")

    def __init__(self, v, d=0.0):
        self.v, self.d = float(v), float(d)

    def __add__(self, o):
        return _Dual(self.v + o.v, self.d + o.d)

    def __sub__(self, o):
        return _Dual(self.v - o.v, self.d - o.d)

    def __mul__(self, o):
        return _Dual(self.v * o.v, self.d * o.v + self.v * o.d)


def _body_wrench_world(frame, x, p, l, lit):
    """W = [M + r x F; F] of the load l = [m; f] at point p of the body with pose x = (R column-major, t), on floats or _Dual
    numbers (lit lifts a constant): the one statement both body_wrench_tau and body_wrench_tau_partials run."""
    p0, p1, p2 = lit(p[0]), lit(p[1]), lit(p[2])
    w = [lit(e) for e in l]
    r = [((x[i] * p0 + x[3 + i] * p1) + x[6 + i] * p2) + x[9 + i] for i in range(3)]
    if frame == 1:
        F = [(x[i] * w[3] + x[3 + i] * w[4]) + x[6 + i] * w[5] for i in range(3)]
        M = [(x[i] * w[0] + x[3 + i] * w[1]) + x[6 + i] * w[2] for i in range(3)]
    else:
        F, M = w[3:], w[:3]
    cr = [r[1] * F[2] - r[2] * F[1], r[2] * F[0] - r[0] * F[2], r[0] * F[1] - r[1] * F[0]]
    return [M[i] + cr[i] for i in range(3)] + F


def _body_wrench_segment(seg_t, t):
    return sum(1 for j in range(1, len(seg_t)) if float(seg_t[j]) <= float(t))


def body_wrench_tau(x_w_b, jac, t, tau_in, body, frame, point, seg_t, seg_w):
    """The applied body wrenches of one row: x_w_b (n_body x 12) and jac (n_body x nv x 6) of pfc_kinematics, the row's time t,
    tau_in (nv floats, or None: the sum starts from +0.0), body, frame (n_w), point (n_w x 3), the scene's schedule seg_t (n_seg)
    and seg_w (n_seg x n_w x 6, [moment; force]).  Per wrench, k ascending: the application point r = ((R[:,0] p0 + R[:,1] p1) +
    R[:,2] p2) + t_b; frame 1: F = R f, M = R m, frame 0: copies; W = [M + r x F; F]; tau_k,j = ((J0 W0 + J1 W1) + J2 W2) + ((J3 W3
    + J4 W4) + J5 W5); tau_out_j = (..(tau_in_j + tau_0,j) + ..).  Returns tau_out (nv floats)."""
    nv = len(jac[0])
    seg = _body_wrench_segment(seg_t, t)
    out = [0.0 if tau_in is None else float(tau_in[j]) for j in range(nv)]
    for k, b in enumerate(body):
        x = [float(e) for e in x_w_b[b]]
        W = _body_wrench_world(int(frame[k]), x, point[k], seg_w[seg][k], float)
        for j in range(nv):
            J = [float(e) for e in jac[b][j]]
            out[j] = out[j] + (((J[0] * W[0] + J[1] * W[1]) + J[2] * W[2]) + ((J[3] * W[3] + J[4] * W[4]) + J[5] * W[5]))
    return out


def body_wrench_tau_partials(x_w_b, jac, dx_w_b, djac, t, dtau_in, body, frame, point, seg_t, seg_w):
    """The partials of body_wrench_tau along one direction: dx_w_b (n_body x 12) and djac (n_body x nv x 6) of pfc_kinematics_dual
    for that direction.  The value statement on (value, partial) numbers with ScatDual's rules (_Dual); t, the tables, the points and
    the loads are constants {x, 0.0}.  dtau_out_j = (..(dtau_in_j + d tau_0,j) + ..), from +0.0 where dtau_in is None.  Returns
    dtau_out (nv floats)."""
    nv = len(jac[0])
    seg = _body_wrench_segment(seg_t, t)
    out = [0.0 if dtau_in is None else float(dtau_in[j]) for j in range(nv)]
    for k, b in enumerate(body):
        x = [_Dual(x_w_b[b][e], dx_w_b[b][e]) for e in range(12)]
        W = _body_wrench_world(int(frame[k]), x, point[k], seg_w[seg][k], _Dual)
        for j in range(nv):
            J = [_Dual(jac[b][j][e], djac[b][j][e]) for e in range(6)]
            out[j] = out[j] + (((J[0] * W[0] + J[1] * W[1]) + J[2] * W[2]) + ((J[3] * W[3] + J[4] * W[4]) + J[5] * W[5])).d
    return out


# ---- the gripper program: the scalar statement of include/pfc.h (pfc_radau_program_device) in Python floats -------------------------
PROGRAM_RECORD0 = dict(cursor=0, pops=0, t0=float("inf"), rot_0=float("inf"), angle=0.0, tau_grip=0.0)


def rotation_angle(R, atan2=math.atan2) -> float:
    """The angle in [0, pi] of a rotation, in the written order.  R is (3, 3) (R[i][j]) or flat column-major (the first nine of a
    body's x_w_b record): a = R32 - R23, b = R13 - R31, c = R21 - R12; s = sqrt((a a + b b) + c c); w = ((R11 + R22) + R33) - 1;
    atan2(s, w).  atan2: the function to take it with (the tests pass a high-precision one)."""
    A = np.asarray(R, dtype=np.float64)
    x = [float(e) for e in (A.reshape(-1, order="F") if A.ndim == 2 else A.reshape(-1)[:9])]      # x[(i - 1) + 3 (j - 1)] = Rij
    s, w = rotation_angle_terms(x)
    return float(atan2(s, w))


def rotation_angle_terms(x):
    """(s, w) of rotation_angle from the nine column-major entries, as Python floats."""
    a, b, c = x[5] - x[7], x[6] - x[2], x[1] - x[3]
    s = math.sqrt((a * a + b * b) + c * c)
    w = ((x[0] + x[4]) + x[8]) - 1.0
    return s, w


def gripper_program_step(record, t, angle, prog_dt, prog_q, prog_slip, tau_soft, tau_hard):
    """One due evaluation of a scene's program (steps 2 - 5 of the statement; the angle of step 1 is given).  record: dict of cursor,
    pops, t0, rot_0, angle, tau_grip (PROGRAM_RECORD0 initially); prog_dt (n_ins), prog_q (n_ins x n_act), prog_slip (n_ins).
    Returns (the new record, the segment's setpoints prog_q[cursor], tau_grip); `record` is not changed."""
    inf = float("inf")
    t, angle = float(t), float(angle)
    cursor, pops, t0, rot_0 = int(record["cursor"]), int(record["pops"]), float(record["t0"]), float(record["rot_0"])
    if t0 == inf:
        t0 = t
    if cursor < len(prog_dt) - 1 and float(prog_dt[cursor]) < (t - t0):
        cursor, pops, t0, rot_0 = cursor + 1, pops + 1, t, angle
    sl = float(prog_slip[cursor])
    if sl == -inf:
        tau_grip = 0.0
    elif sl == 0.0:
        tau_grip = float(tau_hard)
    elif sl == inf:
        tau_grip = float(tau_soft)
    else:
        tau_grip = float(tau_soft) if abs(angle - rot_0) < sl else float(tau_hard)
    new = dict(cursor=cursor, pops=pops, t0=t0, rot_0=rot_0, angle=angle, tau_grip=tau_grip)
    return new, [float(e) for e in prog_q[cursor]], tau_grip


def relative_pose(R_w1, t_w1, R_w2, t_w2) -> np.ndarray:
    """pose[24] for bodies with world poses x_rw_r1 = (R_w1, t_w1), x_rw_r2 = (R_w2, t_w2):
    x_r2_rw = inv(x_rw_r2); x_r2_r1 = x_r2_rw * x_rw_r1; x_r1_r2 = inv(x_r2_r1)
    (src/contact_algorithms_non_friction.jl:109-113; inv(Transform3D) = (R', -R' t))."""
    R_w1 = np.asarray(R_w1, dtype=np.float64).reshape(3, 3); t_w1 = np.asarray(t_w1, dtype=np.float64).reshape(3)
    R_w2 = np.asarray(R_w2, dtype=np.float64).reshape(3, 3); t_w2 = np.asarray(t_w2, dtype=np.float64).reshape(3)
    R_2w = R_w2.T
    t_2w = -(R_2w @ t_w2)
    R21 = R_2w @ R_w1
    t21 = R_2w @ t_w1 + t_2w
    R12 = R21.T
    t12 = -(R12 @ t21)
    return np.concatenate([R21.reshape(-1, order="F"), t21, R12.reshape(-1, order="F"), t12])


def relative_twist(R_w2, t_w2, twist_w1, twist_w2) -> np.ndarray:
    """twist_r2_r1_r2 = transform(-twist_w_r1 + twist_w_r2, x_r2_rw) (:125-128); twists are [angular; linear]
    expressed in world about the world origin (RigidBodyDynamics convention)."""
    R_w2 = np.asarray(R_w2, dtype=np.float64).reshape(3, 3); t_w2 = np.asarray(t_w2, dtype=np.float64).reshape(3)
    tw = np.asarray(twist_w2, dtype=np.float64) - np.asarray(twist_w1, dtype=np.float64)
    R = R_w2.T
    t = -(R @ t_w2)
    ang = R @ tw[:3]
    lin = R @ tw[3:] + np.cross(t, ang)
    return np.concatenate([ang, lin])


def _hat(a) -> np.ndarray:
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def joint_kinematics(parent, joint_type, x_p_j, axis, q, v):
    """World poses, twists and geometric Jacobians of a tree's bodies from its joint state: transform_to_root, twist_wrt_world and
    refreshJacobians! (src/contact_algorithms_non_friction.jl:86-92,109-110,125-126) in NumPy, for one scene -- the matrix
    formulation (4x4 homogeneous products, 6x6 adjoints, Rodrigues' formula), deliberately not the scalar statement of
    pfc_kinematics, which the tests compare with it.  Arguments as MechanismScenario.set_mechanism, q (nq,), v (nv,).
    Returns x_w_b (n_body,12), twist_w_b (n_body,6), jac (n_body,nv,6)."""
    parent = np.asarray(parent, dtype=np.int64).reshape(-1)
    n_body = parent.size
    joint_type = np.asarray(joint_type, dtype=np.int64).reshape(-1)
    x_p_j = np.asarray(x_p_j, dtype=np.float64).reshape(n_body, 12)
    axis = np.zeros((n_body, 3)) if axis is None else np.asarray(axis, dtype=np.float64).reshape(n_body, 3)
    ndof = [{_lib.JOINT_FIXED: 0, _lib.JOINT_REVOLUTE: 1, _lib.JOINT_PRISMATIC: 1, _lib.JOINT_FLOATING_MRP: 6}[int(t)] for t in joint_type]
    off = np.concatenate([[0], np.cumsum(ndof)]).astype(int)
    nv = int(off[-1])
    q = np.asarray(q, dtype=np.float64).reshape(nv); v = np.asarray(v, dtype=np.float64).reshape(nv)
    H, tw, J = [None] * n_body, np.zeros((n_body, 6)), np.zeros((n_body, nv, 6))
    for b in range(n_body):
        qb, vb, a = q[off[b]:off[b + 1]], v[off[b]:off[b + 1]], axis[b]
        Xj, S = np.eye(4), np.zeros((6, ndof[b]))
        if joint_type[b] == _lib.JOINT_REVOLUTE:
            K = _hat(a)
            Xj[:3, :3] = np.eye(3) + np.sin(qb[0]) * K + (1.0 - np.cos(qb[0])) * (K @ K)
            S[:3, 0] = a
        elif joint_type[b] == _lib.JOINT_PRISMATIC:
            Xj[:3, 3] = a * qb[0]
            S[3:, 0] = a
        elif joint_type[b] == _lib.JOINT_FLOATING_MRP:
            p, P = qb[:3], _hat(qb[:3])
            p2 = float(p @ p)
            Xj[:3, :3] = np.eye(3) + (4.0 * (1.0 - p2) * P + 8.0 * (P @ P)) / (1.0 + p2) ** 2
            Xj[:3, 3] = qb[3:]
            S = np.eye(6)
        Xp = np.eye(4)
        Xp[:3, :3] = x_p_j[b, :9].reshape(3, 3, order="F"); Xp[:3, 3] = x_p_j[b, 9:]
        H[b] = (H[parent[b]] if parent[b] >= 0 else np.eye(4)) @ Xp @ Xj
        R, t = H[b][:3, :3], H[b][:3, 3]
        Ad = np.zeros((6, 6))      # a motion vector [angular; linear] of the body frame in world about the world origin
        Ad[:3, :3] = R; Ad[3:, 3:] = R; Ad[3:, :3] = _hat(t) @ R
        Sw = Ad @ S
        tw[b] = (tw[parent[b]] if parent[b] >= 0 else 0.0) + Sw @ vb
        if parent[b] >= 0:
            J[b] = J[parent[b]]
        J[b, off[b]:off[b + 1]] = Sw.T
    x = np.array([np.concatenate([h[:3, :3].reshape(-1, order="F"), h[:3, 3]]) for h in H])
    return x, tw, J


def joint_dynamics(parent, joint_type, x_p_j, axis, inertia, gravity, q, v):
    """qdot, the mass matrix H and the bias c of a tree (H vdot + c = tau + f) for one scene in NumPy -- the matrix formulation
    on joint_kinematics' Jacobians, deliberately not the recursion of pfc_dynamics, which the tests compare with it.  With I_b the
    6x6 spatial inertia of body b in world about the world origin, J_b (6,nv) its geometric Jacobian and tw_b its twist:
        H = sum_b J_b' I_b J_b,      c = sum_b J_b' (I_b (Jdot_b v - [0; g]) + tw_b x* I_b tw_b),
    column k of Jdot_b being tw_body(k) x_m S_k where k's joint lies on b's path.  qdot: v for revolute and prismatic joints;
    (1/4 [(1 - p'p) I + 2 [p]x + 2 p p'] omega, R_j(p) v_lin) for a floating one.  inertia (n_body,13) as
    MechanismScenario.set_inertia, gravity (3) in world.  Returns qdot (nq,), H (nv,nv), c (nv,)."""
    x, tw, J = joint_kinematics(parent, joint_type, x_p_j, axis, q, v)
    parent = np.asarray(parent, dtype=np.int64).reshape(-1)
    joint_type = np.asarray(joint_type, dtype=np.int64).reshape(-1)
    n_body, nv = parent.size, J.shape[1]
    inertia = np.asarray(inertia, dtype=np.float64).reshape(n_body, 13)
    g6 = np.concatenate([np.zeros(3), np.asarray(gravity, dtype=np.float64).reshape(3)])
    ndof = [{_lib.JOINT_FIXED: 0, _lib.JOINT_REVOLUTE: 1, _lib.JOINT_PRISMATIC: 1, _lib.JOINT_FLOATING_MRP: 6}[int(t)] for t in joint_type]
    off = np.concatenate([[0], np.cumsum(ndof)]).astype(int)
    owner = np.repeat(np.arange(n_body), ndof)
    q = np.asarray(q, dtype=np.float64).reshape(nv); v = np.asarray(v, dtype=np.float64).reshape(nv)

    def crm(t):      # the 6x6 matrix of t x_m
        M = np.zeros((6, 6))
        M[:3, :3] = _hat(t[:3]); M[3:, 3:] = _hat(t[:3]); M[3:, :3] = _hat(t[3:])
        return M

    H, c = np.zeros((nv, nv)), np.zeros(nv)
    for b in range(n_body):
        R, t = x[b, :9].reshape(3, 3, order="F"), x[b, 9:]
        M, cp, m = inertia[b, :9].reshape(3, 3, order="F"), inertia[b, 9:12], inertia[b, 12]
        hw = R @ cp + m * t                       # m times the centre of mass, world
        C_, T_ = _hat(R @ cp), _hat(t)
        I6 = np.zeros((6, 6))
        I6[:3, :3] = R @ M @ R.T - m * (T_ @ T_) - (T_ @ C_ + C_ @ T_)      # the moment moved from the frame origin to the world's
        I6[:3, 3:] = _hat(hw); I6[3:, :3] = -_hat(hw); I6[3:, 3:] = m * np.eye(3)
        Jb = J[b].T                               # (6, nv)
        Jd = np.zeros((6, nv))
        for k in range(nv):
            if Jb[:, k].any():
                Jd[:, k] = crm(tw[owner[k]]) @ Jb[:, k]
        H += Jb.T @ I6 @ Jb
        c += Jb.T @ (I6 @ (Jd @ v - g6) - crm(tw[b]).T @ (I6 @ tw[b]))
    qd = v.copy()
    for b in range(n_body):
        if joint_type[b] == _lib.JOINT_FLOATING_MRP:
            p, w, u = q[off[b]:off[b] + 3], v[off[b]:off[b] + 3], v[off[b] + 3:off[b] + 6]
            P = _hat(p)
            p2 = float(p @ p)
            qd[off[b]:off[b] + 3] = 0.25 * (((1.0 - p2) * np.eye(3) + 2.0 * P + 2.0 * np.outer(p, p)) @ w)
            qd[off[b] + 3:off[b] + 6] = (np.eye(3) + (4.0 * (1.0 - p2) * P + 8.0 * (P @ P)) / (1.0 + p2) ** 2) @ u
    return qd, H, c


def joint_kinematics_partials(parent, joint_type, x_p_j, axis, q, v, dq, dv):
    """The directional derivatives of joint_kinematics' three outputs along the seed directions of a Jacobian chunk, for one scene and
    all directions at once: the matrix form of the derivative in joint_kinematics' formulation (derivatives of Rodrigues' formula and
    of the MRP rotation, the product rule on the 4x4 homogeneous products and the 6x6 adjoints), deliberately not the scalar Dual
    statement of pfc_kinematics_dual, which the tests compare with it.  Arguments as joint_kinematics, plus dq (n_dir,nq) and dv
    (n_dir,nv), the partials of the state (None: zeros; not both).  Returns d_x_w_b (n_body,n_dir,12), d_twist_w_b (n_body,n_dir,6),
    d_jac (n_body,n_dir,nv,6)."""
    parent = np.asarray(parent, dtype=np.int64).reshape(-1)
    n_body = parent.size
    joint_type = np.asarray(joint_type, dtype=np.int64).reshape(-1)
    x_p_j = np.asarray(x_p_j, dtype=np.float64).reshape(n_body, 12)
    axis = np.zeros((n_body, 3)) if axis is None else np.asarray(axis, dtype=np.float64).reshape(n_body, 3)
    ndof = [{_lib.JOINT_FIXED: 0, _lib.JOINT_REVOLUTE: 1, _lib.JOINT_PRISMATIC: 1, _lib.JOINT_FLOATING_MRP: 6}[int(t)] for t in joint_type]
    off = np.concatenate([[0], np.cumsum(ndof)]).astype(int)
    nv = int(off[-1])
    q = np.asarray(q, dtype=np.float64).reshape(nv); v = np.asarray(v, dtype=np.float64).reshape(nv)
    if dq is None and dv is None:
        raise ValueError("one of dq and dv must be given: they carry n_dir")
    dq = None if dq is None else np.asarray(dq, dtype=np.float64).reshape(-1, nv)
    dv = None if dv is None else np.asarray(dv, dtype=np.float64).reshape(-1, nv)
    n_dir = (dq if dq is not None else dv).shape[0]
    dq = np.zeros((n_dir, nv)) if dq is None else dq
    dv = np.zeros((n_dir, nv)) if dv is None else dv
    hat_all = lambda A: np.stack([_hat(a) for a in A])      # (n_dir,3) -> (n_dir,3,3)
    H, dH = [None] * n_body, [None] * n_body
    tw, dtw, dJ = np.zeros((n_body, 6)), np.zeros((n_body, n_dir, 6)), np.zeros((n_body, n_dir, nv, 6))
    for b in range(n_body):
        sl = slice(off[b], off[b + 1])
        qb, vb, dqb, dvb, a = q[sl], v[sl], dq[:, sl], dv[:, sl], axis[b]
        Xj, dXj, S = np.eye(4), np.zeros((n_dir, 4, 4)), np.zeros((6, ndof[b]))
        if joint_type[b] == _lib.JOINT_REVOLUTE:
            K = _hat(a)
            Xj[:3, :3] = np.eye(3) + np.sin(qb[0]) * K + (1.0 - np.cos(qb[0])) * (K @ K)
            dXj[:, :3, :3] = dqb[:, 0, None, None] * (np.cos(qb[0]) * K + np.sin(qb[0]) * (K @ K))
            S[:3, 0] = a
        elif joint_type[b] == _lib.JOINT_PRISMATIC:
            Xj[:3, 3] = a * qb[0]
            dXj[:, :3, 3] = dqb[:, 0, None] * a
            S[3:, 0] = a
        elif joint_type[b] == _lib.JOINT_FLOATING_MRP:
            p, P = qb[:3], _hat(qb[:3])
            p2 = float(p @ p)
            N, den = 4.0 * (1.0 - p2) * P + 8.0 * (P @ P), 1.0 + p2
            Xj[:3, :3] = np.eye(3) + N / den ** 2
            Xj[:3, 3] = qb[3:]
            dP = hat_all(dqb[:, :3])
            dp2 = 2.0 * (dqb[:, :3] @ p)
            dN = 4.0 * (1.0 - p2) * dP - 4.0 * dp2[:, None, None] * P + 8.0 * (dP @ P + P @ dP)
            dXj[:, :3, :3] = dN / den ** 2 - (2.0 * dp2 / den ** 3)[:, None, None] * N
            dXj[:, :3, 3] = dqb[:, 3:]
            S = np.eye(6)
        Xp = np.eye(4)
        Xp[:3, :3] = x_p_j[b, :9].reshape(3, 3, order="F"); Xp[:3, 3] = x_p_j[b, 9:]
        Hp = H[parent[b]] if parent[b] >= 0 else np.eye(4)
        dHp = dH[parent[b]] if parent[b] >= 0 else np.zeros((n_dir, 4, 4))
        B = Hp @ Xp
        H[b] = B @ Xj
        dH[b] = (dHp @ Xp) @ Xj + B @ dXj
        R, t, dR, dt = H[b][:3, :3], H[b][:3, 3], dH[b][:, :3, :3], dH[b][:, :3, 3]
        Ad, dAd = np.zeros((6, 6)), np.zeros((n_dir, 6, 6))
        Ad[:3, :3] = R; Ad[3:, 3:] = R; Ad[3:, :3] = _hat(t) @ R
        dAd[:, :3, :3] = dR; dAd[:, 3:, 3:] = dR; dAd[:, 3:, :3] = hat_all(dt) @ R + _hat(t) @ dR
        Sw, dSw = Ad @ S, dAd @ S
        tw[b] = (tw[parent[b]] if parent[b] >= 0 else 0.0) + Sw @ vb
        dtw[b] = (dtw[parent[b]] if parent[b] >= 0 else 0.0) + dSw @ vb + dvb @ Sw.T
        if parent[b] >= 0:
            dJ[b] = dJ[parent[b]]
        dJ[b, :, sl] = dSw.transpose(0, 2, 1)
    dx = np.array([np.concatenate([d[:, :3, :3].transpose(0, 2, 1).reshape(n_dir, 9), d[:, :3, 3]], axis=1) for d in dH])
    return dx, dtw, dJ


def local_jacobian_tangent(L, pose) -> np.ndarray:
    """The contact Jacobians L (n,12,36) of MechanismScenario.local_jacobian on the 18 tangent coordinates of the state:
    (δθ 3, δt 3, twist 6, s 6).  The pose columns are contracted with the consistent seeds of the perturbation
    x_r2_r1 = (exp(δθ) R0, t0 + δt), pose (n,24) giving (R0, t0) -- the convention of tests/test_oracle_dual.py's tangents():
    δθ is a rotation of body 1 relative to body 2 expressed in frame r2 (left perturbation of R_r2_r1), δt the displacement of
    frame r1's origin in frame r2.  Returns (n,12,18): columns 0..5 are the contact stiffness on (δθ, δt), 6..11 the damping,
    12..17 the bristle-state columns."""
    L = np.asarray(L, dtype=np.float64)
    pose = np.asarray(pose, dtype=np.float64).reshape(-1, 24)
    one = L.ndim == 2
    L = L.reshape(-1, 12, 36)
    if L.shape[0] != pose.shape[0]:
        raise ValueError("L and pose must have the same number of items")
    out = np.zeros((L.shape[0], 12, 18))
    for k in range(L.shape[0]):
        R0 = pose[k, :9].reshape(3, 3, order="F"); t0 = pose[k, 9:12]
        T = np.zeros((24, 6))
        for j in range(3):
            e = np.eye(3)[j]
            E = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
            dR = E @ R0
            T[:9, j] = dR.reshape(-1, order="F")
            T[12:21, j] = dR.T.reshape(-1, order="F")
            T[21:24, j] = R0.T @ np.cross(e, t0)
            T[9:12, 3 + j] = e
            T[21:24, 3 + j] = -R0.T @ e
        out[k, :, :6] = L[k, :, :24] @ T
        out[k, :, 6:] = L[k, :, 24:]
    return out[0] if one else out
