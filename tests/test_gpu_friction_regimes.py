"""Every regime of traction() (friction.jl: stick, plateau at mu_s, ramp from mu_s to mu_d, slide at mu_d) on every device
copy of the law, with mu_s = 0.6 > mu_d = 0.3 -- with mu_s == mu_d the slope of the ramp is exactly 0, both clamps are no-ops
and the derivative of mu through |v_t| / |T̄s| is multiplied by zero.

Scenes: helpers.friction_regime_scenes (R1, B1, V_reg, V_bri); tests/test_oracle_dual.py asserts on the CPU that each of them
holds >= 30 traction points in every regime and none within 1e-4 thresholds of an edge, and pins the Dual oracle on them by
central differences.  Here: the value paths, the friction surface and the Dual paths against the oracles, and a box in pure
translation against the closed form (value and d/d|v|), which does not go through any oracle."""
import numpy as np
import pytest

import helpers as H
from helpers import oracle_ins, oracle_meshes
from test_gpu_contact_friction import _branch_input, _check_against_oracle, _check_consistency, _check_points
from test_gpu_dual import run_case
from test_gpu_parity import TOL_TIGHT, _assert_item_parity
from test_oracle_dual import tangents

pytestmark = pytest.mark.gpu

SCENES = ["R1", "B1", "V_reg", "V_bri"]
BRISTLE = {"B1", "V_bri"}

# name: (options, last_parts() expected: 0 the one-launch kernel k_fused, 1 the batched launch sequence, 2 two halves)
#   fused          k_fused, a team of workgroups per item where the pair has >= 512 leaves (B1), else one workgroup
#   fused_wg       k_fused<.., false>: one workgroup per item
#   one_kernel     k_narrow<., 0> (regularized law inside) + k_fric<true>
#   clip_integ     k_narrow<., 2> + k_integ (regularized law) + k_fric<true> (bristle, per-corner fields)
#   clip_point     ... + k_fric<false> (bristle, per point); the option changes nothing for regularized items
#   fixed          k_integ_fixed + k_fric_fixed<true>
#   halves         two concurrent halves, each k_narrow<., 0> + k_fric<true>.  Option split_min alone leaves scenes of this size
#                  on k_fused (the one-launch kernel is tried first), so the path switches it off to reach the split.
#   debug          k_narrow<., 1> + k_fric<false>: the handle whose candidate pairs every other path is compared with
PATHS = {
    "fused": ({}, 0),
    "fused_wg": ({"team": 0}, 0),
    "one_kernel": ({"fused": 0, "clip_min": 0}, 1),
    "clip_integ": ({"fused": 0, "clip_min": 1}, 1),
    "clip_point": ({"fused": 0, "clip_min": 1, "vertex_fields": 0}, 1),
    "fixed": ({"fused": 0, "fixed_order": 1}, 1),
    "halves": ({"fused": 0, "split_min": 1}, 2),
    "debug": ({"debug": 1}, 1),
}
# workgroups per item of the default path: one per 128 leaves of the pair, teams from 4 on (B1: 720 tets + 320 triangles)
TEAM = {"R1": 1, "B1": 8, "V_reg": 1, "V_bri": 1}
CASES = [(s, p) for s in SCENES for p in PATHS if p != "clip_point" or s in BRISTLE]


@pytest.fixture(scope="module")
def scenes(pfc):
    return H.friction_regime_scenes(pfc)


@pytest.fixture(scope="module")
def refs(pfc, O, scenes):
    """The oracle's debug results per scene, computed once and left unchanged."""
    return {name: H.oracle_run(pfc, w) for name, w in scenes.items()}


class _Pairs:
    """The candidate pairs of a debug handle's evaluation, in the shape _assert_item_parity asks a handle for: the other
    paths keep no per-item pair list (their counts, wrench and ṡ are their own)."""

    def __init__(self, m, n_items):
        self._pairs = [m.debug_pairs(k) for k in range(n_items)]

    def debug_pairs(self, k):
        return self._pairs[k]


@pytest.fixture(scope="module")
def pairs(pfc, scenes):
    out = {}
    for name, w in scenes.items():
        m = pfc.configs.build_scenario(w, debug=True)
        m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
        out[name] = _Pairs(m, w.n_items)
        m.close()
    return out


def _handle(pfc, w, options):
    m = pfc.configs.build_scenario(w)
    for key, v in options.items():
        m.set_option(key, v)
    return m


# ---- 3. value paths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,path", CASES)
def test_value_paths_against_the_oracle(pfc, scenes, refs, pairs, scene, path):
    w, ref = scenes[scene], refs[scene]
    options, parts = PATHS[path]
    m = _handle(pfc, w, options)
    wrench, sdot, counts = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    assert m.last_parts() == parts, (scene, path, m.last_parts())
    if parts == 0:
        assert m.last_team() == (1 if path == "fused_wg" else TEAM[scene]), (scene, path, m.last_team())
    view = m if path == "debug" else pairs[scene]
    n_K = 0
    for k, r in enumerate(ref):
        assert r.counts[3] > 0
        _assert_item_parity(view, k, r, wrench, sdot, counts, TOL_TIGHT)
        if scene in BRISTLE and parts == 1 and r.has_K:      # (k_fused keeps K in LDS; a half keeps its own items')
            K, Kis, Sinv, cop = m.debug_stiffness(k)
            assert H.rel_err(K, r.K) < TOL_TIGHT, (k, H.rel_err(K, r.K))
            assert H.rel_err(Sinv, r.Sinv) < TOL_TIGHT, (k, H.rel_err(Sinv, r.Sinv))
            assert H.rel_err(cop, r.cop) < TOL_TIGHT, (k, H.rel_err(cop, r.cop))
            assert H.rel_err(Kis, r.Kbar_inv_sqrt) < 1e-8, (k, H.rel_err(Kis, r.Kbar_inv_sqrt))
            n_K += 1
    if scene in BRISTLE and parts == 1:
        assert n_K > 0
    m.close()


# ---- 4. friction surface per point ----------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", SCENES)
def test_friction_surface_points_in_every_regime(pfc, O, scenes, refs, scene):
    w, ref = scenes[scene], refs[scene]
    m = pfc.configs.build_scenario(w)
    F = m.contact_surface_fric(w.pose, w.twist, w.s, w.ins_ids)
    m.close()
    _check_against_oracle(w, F, range(w.n_items), ref)
    total = np.zeros(4, dtype=int)
    for k in range(w.n_items):
        _check_points(pfc, O, w, F, k)         # every T_c within 1e-12 mu_s p dA of pfo_traction_*
        _check_consistency(F, k)
        it = F.item(k)
        _, _, _, v, _, thr = _branch_input(pfc, w, F, k)
        x = np.linalg.norm(v, axis=1) / thr
        assert np.array_equal(it["fric"][:, 3], np.where(x >= 1.0, 1.0, 0.0)), k
        regimes, _ = H.friction_regimes(pfc, w, k, ref[k])
        assert int(np.sum(it["fric"][:, 3] == 0.0)) == regimes[0] == it["n_first"], (k, regimes, it["n_first"])
        total += regimes
    assert np.all(total >= 30), total


# ---- 5. analytic sliding box ----------------------------------------------------------------------------------------
MU_S, MU_D, V_C = 0.6, 0.3, 0.01
V_HAT = np.array([0.6, -0.8, 0.0])
# u = |v| / v_c: (mu_eff, d mu_eff / d|v|) of stick, plateau, ramp, slide
SLIDING = {0.5: (MU_S * 0.5, MU_S / V_C), 1.5: (MU_S, 0.0), 2.5: (MU_S + 0.5 * (MU_D - MU_S), (MU_D - MU_S) / V_C), 5.0: (MU_D, 0.0)}


def _sliding_box(pfc, u):
    w = pfc.configs.c2_box_on_plane(3)
    c = w.instructions[0]
    c.mu_s = MU_S
    assert c.mu_d == MU_D and c.v_tol == V_C and c.model == "regularized"
    w.twist = np.ascontiguousarray(np.tile(np.concatenate([np.zeros(3), u * V_C * V_HAT]), (w.n_items, 1)))
    return w


def _assert_tangential(force, mu_eff, label):
    """force: the force rows (n, 3) of wrenches about frame r2 (z the ground normal): tangential part -mu_eff F_n v̂, 1e-11
    relative -- every point's traction points along -v̂, nothing cancels."""
    for k, f in enumerate(force):
        Fn = abs(f[2])
        assert Fn > 0
        expect = -mu_eff * Fn * V_HAT[:2]
        err = np.linalg.norm(f[:2] - expect) / np.linalg.norm(expect)
        assert err < 1e-11, (label, k, f, expect, err)


@pytest.mark.parametrize("u", sorted(SLIDING))
def test_sliding_box_value_is_analytic(pfc, u):
    w = _sliding_box(pfc, u)
    mu_eff, _ = SLIDING[u]
    m = pfc.configs.build_scenario(w)
    F = m.contact_surface_fric(w.pose, w.twist, None, w.ins_ids)
    m.close()
    for k in range(w.n_items):
        it = F.item(k)
        assert it["trac"].shape[0] > 0
        assert np.all(it["fric"][:, 3] == (0.0 if u < 1 else 1.0)), k      # every point in one regime
        Fn = np.linalg.norm(it["wrench"][3:6])
        expect = -mu_eff * Fn * V_HAT
        assert H.rel_err(it["fric_wrench"][3:6], expect) < 1e-11, (k, it["fric_wrench"], expect)
    for label, options, parts in (("fused", {"fused": 1}, 0), ("one_kernel", {"fused": 0, "clip_min": 0}, 1),
                                  ("clip_integ", {"fused": 0, "clip_min": 1}, 1)):
        m = _handle(pfc, w, options)
        wrench, _, counts = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
        assert m.last_parts() == parts, (label, m.last_parts())
        m.close()
        assert np.all(counts[:, 3] > 0)
        _assert_tangential(wrench[:, 3:6], mu_eff, label)


@pytest.mark.parametrize("u", sorted(SLIDING))
def test_sliding_box_dual_is_analytic(pfc, u):
    """A seed of the twist along v̂ changes |v| only, not p (the normal velocity stays 0): d(force)/d|v| = -F_n v̂ dmu_eff/d|v|,
    to 1e-9 of mu_s F_n / v_c."""
    w = _sliding_box(pfc, u)
    mu_eff, dmu = SLIDING[u]
    n = w.n_items
    d_pose, d_twist = np.zeros((n, 1, 24)), np.zeros((n, 1, 6))
    d_twist[:, 0, 3:6] = V_HAT
    m = pfc.configs.build_scenario(w)
    wrench, _, dw, _, counts = m.force_all_elastic_intersections_dual(w.pose, w.twist, w.s, d_pose, d_twist, None, w.ins_ids)
    m.close()
    assert np.all(counts[:, 3] > 0)
    _assert_tangential(wrench[:, 3:6], mu_eff, "dual value")
    for k in range(n):
        Fn = abs(wrench[k, 5])
        expect = -Fn * V_HAT * dmu
        scale = MU_S * Fn / V_C
        assert np.abs(dw[k, 0, 3:6] - expect).max() <= 1e-9 * scale, (k, dw[k, 0, 3:6], expect, scale)


# ---- 6. Dual paths against the Dual oracle --------------------------------------------------------------------------
@pytest.mark.parametrize("options", [None, {"fused": 0}], ids=["default", "batched"])
@pytest.mark.parametrize("scene", SCENES)
def test_dual_paths_against_the_dual_oracle(pfc, O, scenes, scene, options):
    w = scenes[scene]
    s0 = w.s.copy()
    assert run_case(pfc, O, w, 6, 7, zero_s=True, options=options) == w.n_items      # 1e-6 wrench, 1e-5 ṡ partials
    assert np.array_equal(w.s, s0)


def test_fused_dual_kernel_against_the_dual_oracle(pfc, O, scenes):
    """The Dual passes inside k_fused (all-regularized tri-tet scenes, from a handle's second Dual evaluation on; a fresh
    handle, as in run_case, takes the two-stage path): R1 against the Dual oracle at run_case's tolerance."""
    w = scenes["R1"]
    n, nd = w.n_items, 6
    rng = np.random.default_rng(9)
    dq = rng.standard_normal((n, nd, 6)) * np.array([1, 1, 1, 0.05, 0.05, 0.05])
    d_twist = rng.standard_normal((n, nd, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1])
    d_pose = np.stack([tangents(w.pose[k][:9].reshape(3, 3, order="F"), w.pose[k][9:12], dq[k]) for k in range(n)])
    m = pfc.configs.build_scenario(w)
    for _ in range(2):
        _, _, dw, dsd, counts = m.force_all_elastic_intersections_dual(w.pose, w.twist, w.s, d_pose, d_twist, None, w.ins_ids)
    assert m.last_parts() == 0, "the Dual passes of the fused kernel did not run"
    m.close()
    assert np.all(dsd == 0.0)
    om = oracle_meshes(w)
    for k in range(n):
        assert counts[k, 3] > 0
        c = w.instructions[int(w.ins_ids[k])]
        st, _, _, rdw, _ = O.evaluate_dual(om[c.id_1], om[c.id_2], oracle_ins(pfc, c), w.pose[k], w.twist[k], w.s[k], d_pose[k],
                                           d_twist[k], np.zeros((nd, 6)))
        assert st == 0
        sw = np.abs(rdw).max()
        assert np.abs(dw[k] - rdw).max() <= 1e-6 * sw, (k, np.abs(dw[k] - rdw).max() / sw)


def test_local_jacobian_tangent_against_the_dual_oracle(pfc, O, scenes):
    """L of B1 on the 18 tangent coordinates, applied to 6 directions, against the Dual oracle seeded with the same
    directions: the tolerances of tests/test_gpu_local_jacobian.py::test_L_against_the_dual_oracle."""
    w = scenes["B1"]
    n, nd = w.n_items, 6
    rng = np.random.default_rng(8)
    dq = rng.standard_normal((n, nd, 6)) * np.array([1, 1, 1, 0.05, 0.05, 0.05])
    d_twist = rng.standard_normal((n, nd, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1])
    d_s = rng.standard_normal((n, nd, 6)) * 1e-3
    m = pfc.configs.build_scenario(w)
    _, _, L, counts = m.local_jacobian(w.pose, w.twist, w.s, w.ins_ids)
    m.close()
    Lt = pfc.scenario.local_jacobian_tangent(L, w.pose)
    om = oracle_meshes(w)
    for k in range(n):
        assert counts[k, 3] > 0
        c = w.instructions[int(w.ins_ids[k])]
        d_pose = tangents(w.pose[k][:9].reshape(3, 3, order="F"), w.pose[k][9:12], dq[k])
        st, _, _, rdw, rdsd = O.evaluate_dual(om[c.id_1], om[c.id_2], oracle_ins(pfc, c), w.pose[k], w.twist[k], w.s[k],
                                              d_pose, d_twist[k], d_s[k])
        assert st == 0
        got = np.concatenate([dq[k], d_twist[k], d_s[k]], axis=1) @ Lt[k].T      # (nd, 12)
        sw, ss = np.abs(rdw).max(), np.abs(rdsd).max()
        assert np.abs(got[:, :6] - rdw).max() <= 1e-6 * sw, (k, np.abs(got[:, :6] - rdw).max() / sw)
        assert np.abs(got[:, 6:] - rdsd).max() <= 1e-5 * ss, (k, np.abs(got[:, 6:] - rdsd).max() / ss)
