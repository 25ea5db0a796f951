"""Every broadphase descent kernel on host-supplied OBB trees that the library's builders never make (tests/helpers.py:
rotated, shrunk and mixed internal boxes, random and caterpillar topologies, a one-node tree against a deep one), against the
CPU oracle, whose tree_tree_intersect / BB_BB_intersect use whatever the tree holds like the reference's
(src/obb/tree_types.jl:88-111, src/obb/bb_intersection.jl:2-74).  tests/test_host_trees_oracle.py shows on the CPU that these
trees discriminate: ignoring R on internal nodes changes the counters of nearly every pose.

Paths: k_bp_dfs32 (Float32 filter + cooperative exact settle), k_bp_dfs (all Float64, option no_filter), k_bp_expand (seed
levels), k_fused with and without its filter, the team form of k_fused (a 512-leaf pair), k_bp_dfs32<128> (two halves of 3 072
items) and a Dual evaluation.  All four counters bit-equal to the oracle's for every item, candidate sets equal on the paths
with debug views, wrench 1e-9 and sdot 1e-6 relative (exact zero where the oracle's is zero), every path equal to every other.
(sdot: the project's parity rule, H.sdot_tolerance -- 1e-3 for the patches whose stiffness has two or more eigenvalues at its
rounding level, where the reference's own sdot is no better than that: of these scenes' 1 800 items one, in the shrunk scene, a
single pair left by the pruning -- device 2.3e-6, the oracle's own sdot moves by 3.5e-6 under a rounding-level change of K.)
"""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H
from oracle import oracle as Orc

pytestmark = pytest.mark.gpu

N_ITEMS = 300
PATHS = {"dfs32": dict(debug=1, no_filter=0, bfs_levels=0), "dfs64": dict(debug=1, no_filter=1, bfs_levels=0),
         "expand": dict(debug=1, no_filter=0, bfs_levels=1), "expand5": dict(debug=1, no_filter=0, bfs_levels=5),
         "fused": dict(), "fused_exact": dict(fused_f32=0)}


@functools.lru_cache(maxsize=None)
def _scene(pfc, scene):
    """(workload, oracle results with pair lists) of one scenario: computed once, shared by every path."""
    w = H.host_tree_workload(pfc, scene, N_ITEMS)
    ref = H.oracle_run(pfc, w, debug=True)
    assert all(r.status == 0 for r in ref)
    return w, ref


def _against(ref, wrench, sdot, counts, tag):
    """ref: oracle debug results (they carry the patch stiffness the sdot bound looks at, H.sdot_tolerance)."""
    for k, r in enumerate(ref):
        assert np.array_equal(counts[k], r.counts), (tag, k, counts[k], r.counts)
        for name, a, b, tol in (("wrench", wrench[k], r.wrench, 1e-9), ("sdot", sdot[k], r.sdot, H.sdot_tolerance(r))):
            if np.linalg.norm(b) == 0.0:
                assert np.linalg.norm(a) == 0.0, (tag, name, k, a)
            else:
                assert H.rel_err(a, b) < tol, (tag, name, k, a, b)


@functools.lru_cache(maxsize=None)
def _run(pfc, scene, path):
    """One path over the scenario's items, checked against the oracle; returns its counters."""
    w, ref = _scene(pfc, scene)
    m = pfc.configs.build_scenario(w)
    for k, v in PATHS[path].items():
        m.set_option(k, v)
    try:
        if path.startswith("fused"):
            out = []
            for lo in range(0, N_ITEMS, 150):       # the one-launch kernel takes evaluations of <= 256 items
                sl = slice(lo, lo + 150)
                out.append(m.force_all_elastic_intersections(w.pose[sl], w.twist[sl], w.s[sl], w.ins_ids[sl]))
                assert m.last_parts() == 0, "the fused kernel did not run"
            wrench, sdot, counts = (np.concatenate([o[j] for o in out]) for j in range(3))
        else:
            wrench, sdot, counts = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
            assert m.last_parts() == 1
        _against(ref, wrench, sdot, counts, (scene, path))
        if not path.startswith("fused"):
            for k, r in enumerate(ref):
                pairs, clip_n = H.sorted_pairs(*m.debug_pairs(k))
                rp, rc = H.sorted_pairs(r.pairs, r.clip_n)
                assert np.array_equal(pairs, rp) and np.array_equal(clip_n, rc), (scene, path, k)
    finally:
        m.close()
    return counts


@pytest.mark.parametrize("scene", H.HOST_TREE_SCENES)
def test_items_with_and_without_candidates(pfc, scene):
    """By the oracle alone: at least a quarter of the items have candidates, at least a tenth have none."""
    _, ref = _scene(pfc, scene)
    has = np.array([r.counts[1] > 0 for r in ref])
    assert has.mean() >= 0.25 and (~has).mean() >= 0.1, has.mean()
    assert sum(r.counts[3] > 0 for r in ref) >= N_ITEMS // 10


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("scene", H.HOST_TREE_SCENES)
def test_path_equals_oracle(pfc, scene, path):
    _run(pfc, scene, path)


@pytest.mark.parametrize("scene", H.HOST_TREE_SCENES)
def test_paths_agree(pfc, scene):
    counts = [_run(pfc, scene, path) for path in PATHS]
    for c in counts[1:]:
        assert np.array_equal(c, counts[0])


@pytest.mark.parametrize("scene", ["rotated", "shrunk", "mixed", "random_topology"])
def test_team_of_workgroups(pfc, scene):
    """A 320-triangle sphere against a 192-tet box (512 leaves): four workgroups per item, the top of the descent level
    by level."""
    w = H.host_tree_workload(pfc, scene, 6, fine=True, span=0.7)
    ref = H.oracle_run(pfc, w, debug=True)
    assert sum(r.counts[1] > 0 for r in ref) >= 3
    m = pfc.configs.build_scenario(w)
    wrench, sdot, counts = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    assert m.last_parts() == 0 and m.last_team() >= 4, (m.last_parts(), m.last_team())
    _against(ref, wrench, sdot, counts, (scene, "team"))
    m.set_option("team", 0)                     # without teams (a workgroup per item, or the batched path for an item with
    _, _, c1 = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)     # more than 4 096 candidates): the same integers
    assert m.last_team() <= 1 and np.array_equal(c1, counts)
    m.close()


def test_big_batch_in_128_thread_workgroups(pfc):
    """6 144 items: two halves of 3 072, each through k_bp_dfs32<128>."""
    n = 6144
    w = H.host_tree_workload(pfc, "rotated", n)
    om = H.oracle_meshes(w)
    oi = [H.oracle_ins(pfc, c) for c in w.instructions]
    st, rw, rs, rc = Orc.evaluate_batch(om, oi, [c.id_1 for c in w.instructions], [c.id_2 for c in w.instructions], w.ins_ids,
                                        w.pose, w.twist, w.s, n_threads=16)
    assert st == 0
    m = pfc.configs.build_scenario(w)
    wrench, sdot, counts = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    assert m.last_parts() == 2
    m.close()
    assert np.array_equal(counts, rc), np.nonzero(np.any(counts != rc, axis=1))[0][:8]
    live = np.linalg.norm(rw, axis=1) > 0
    assert np.all(wrench[~live] == 0.0) and live.sum() > n // 10
    err = np.linalg.norm(wrench[live] - rw[live], axis=1) / np.linalg.norm(rw[live], axis=1)
    assert err.max() < 1e-9, err.max()
    sl = np.linalg.norm(rs, axis=1) > 0
    assert np.all(sdot[~sl] == 0.0)
    err = np.zeros(n)
    err[sl] = np.linalg.norm(sdot[sl] - rs[sl], axis=1) / np.linalg.norm(rs[sl], axis=1)
    loose = np.nonzero(err >= 1e-6)[0]          # the batch call returns no stiffness: the few items beyond 1e-6 are evaluated again
    assert loose.size <= n // 100, loose.size
    for k, r in zip(loose, H.oracle_run(pfc, w, items=loose, debug=True)):
        assert err[k] < H.sdot_tolerance(r), (k, err[k])


@pytest.mark.parametrize("fused", [1, 0])
def test_dual_evaluation(pfc, fused):
    """pfc_eval_dual, three directions: the Dual passes start from the lists of the same descent."""
    from test_gpu_dual import tangents
    n, n_dir = 24, 3
    w, ref = _scene(pfc, "rotated")
    rng = np.random.default_rng(17)
    dq = rng.standard_normal((n, n_dir, 6)) * np.array([1, 1, 1, 0.05, 0.05, 0.05])
    d_twist = rng.standard_normal((n, n_dir, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1])
    d_s = rng.standard_normal((n, n_dir, 6)) * 1e-3
    d_pose = np.array([tangents(w.pose[k][:9].reshape(3, 3, order="F"), w.pose[k][9:12], dq[k]) for k in range(n)])
    m = pfc.configs.build_scenario(w)
    m.set_option("fused", fused)
    wr, sd, dw, dsd, counts = m.force_all_elastic_intersections_dual(w.pose[:n], w.twist[:n], w.s[:n], d_pose, d_twist, d_s, w.ins_ids[:n])
    m.close()
    _against(ref[:n], wr, sd, counts, ("rotated", "dual", fused))
    om = H.oracle_meshes(w)
    n_contact = 0
    for k in range(n):
        c = w.instructions[int(w.ins_ids[k])]
        st, _, _, rdw, rdsd = Orc.evaluate_dual(om[c.id_1], om[c.id_2], H.oracle_ins(pfc, c), w.pose[k], w.twist[k], w.s[k],
                                                d_pose[k], d_twist[k], d_s[k])
        assert st == 0
        n_contact += counts[k, 3] > 0
        # the Dual parity bounds of tests/test_gpu_dual.py
        assert np.abs(dw[k] - rdw).max() <= 1e-6 * max(np.abs(rdw).max(), 1e-300), k
        assert np.abs(dsd[k] - rdsd).max() <= 1e-5 * max(np.abs(rdsd).max(), 1e-300), k
    assert n_contact >= 4


def _internal_pair_tests(w, k):
    """(node tests, internal x internal node tests) of item k, recounted over the workload's trees with the oracle's
    BB_BB_intersect: tree_tree_intersect (tree_types.jl:88-111)."""
    L = Orc.lib()
    dp = C.POINTER(C.c_double)
    P = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(dp)
    ta, tb = w.meshes[0].tree, w.meshes[1].tree
    R12, t12 = P(w.pose[k, 12:21]), P(w.pose[k, 21:24])
    n_test = n_ii = 0
    stack = [(0, 0)]
    while stack:
        a, b = stack.pop()
        la, lb = ta.child[a, 0] < 0, tb.child[b, 0] < 0
        n_test += 1
        n_ii += (not la) and (not lb)
        if not L.pfo_bb_bb_intersect(P(ta.c[a]), P(ta.e[a]), P(ta.R[a]), P(tb.c[b]), P(tb.e[b]), P(tb.R[b]), R12, t12):
            continue
        if la and lb:
            continue
        ca = [a] if la else list(ta.child[a])
        cb = [b] if lb else list(tb.child[b])
        stack += [(x, y) for y in cb for x in ca]
    return n_test, n_ii


def test_rotated_internal_boxes_are_settled_by_the_exact_test(pfc):
    """The filter's 24 u radius for internal x internal pairs is derived for identity quaternions (pfc_bp.h, "Error radius
    E", (5)); pfc_add_mesh marks every other internal node exact-only.  Statistics word [7] (pairs settled exactly) is
    therefore at least the number of internal x internal node tests of the rotated scene, and far lower on built trees."""
    n = 48
    settled, n_ii = {}, 0
    for scene in ("rotated", "built"):
        w = H.host_tree_workload(pfc, scene, n)
        m = pfc.configs.build_scenario(w)
        for k, v in PATHS["dfs32"].items():
            m.set_option(k, v)
        _, _, counts = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
        out = (C.c_longlong * 16)()
        assert pfc._lib.lib().pfc_debug_stamps(m._h, out) == 0
        settled[scene] = int(out[7])
        m.close()
        if scene == "rotated":
            for k in range(n):
                nt, ii = _internal_pair_tests(w, k)
                assert nt == counts[k, 0], (k, nt, counts[k])       # the recount is the descent the device ran
                n_ii += ii
    assert n_ii > 1000
    assert settled["rotated"] >= n_ii, (settled, n_ii)
    assert settled["built"] * 20 < n_ii, (settled, n_ii)


# ---- refusals ------------------------------------------------------------------------------------------------------
def _refused(pfc, tree_a, tree_b=None, n_a=2, n_b=2):
    """finalize() of a dummy pair under the given trees (tree_b: by default a sound three-node tree): the status and
    message of the refusal (None: accepted)."""
    from test_gpu_broadphase import _meshes
    S = pfc.scenario
    if tree_b is None:
        tree_b = _three_nodes(pfc, [[1, 2], [-1, -1], [-1, -1]], [pfc.geometry.INTERNAL, 0, 1])
    tri, _ = _meshes(pfc, n_a)
    _, tet = _meshes(pfc, n_b)
    m = S.MechanismScenario()
    i1 = m.add_contact("a", tri, tree=tree_a)
    i2 = m.add_contact("b", tet, c_prop=S.ContactProperties(1.0e6), tree=tree_b)
    m.add_friction_regularize(i1, i2, mu_d=0.3)
    try:
        m.finalize()
        return None
    except pfc._lib.PFCError as e:
        return e.status, str(e)
    finally:
        m.close()        # a refused handle destroys cleanly


def _three_nodes(pfc, child, leaf):
    G = pfc.geometry
    return G.OBBTree(np.zeros((3, 3)), np.ones((3, 3)), np.tile(np.eye(3).reshape(-1), (3, 1)), np.array(child, dtype=np.int32),
                     np.array(leaf, dtype=np.int32))


def test_tree_refusals(pfc):
    INT, BAD = pfc.geometry.INTERNAL, pfc._lib.ERR_BAD_ARG
    assert _refused(pfc, _three_nodes(pfc, [[1, 2], [-1, -1], [-1, -1]], [INT, 0, 1])) is None           # the control
    st, msg = _refused(pfc, _three_nodes(pfc, [[0, 2], [-1, -1], [-1, -1]], [INT, 0, 1]))
    assert st == BAD and "bad child index" in msg          # the root as a child
    st, msg = _refused(pfc, _three_nodes(pfc, [[1, 3], [-1, -1], [-1, -1]], [INT, 0, 1]))
    assert st == BAD and "bad child index" in msg          # out of range
    st, msg = _refused(pfc, _three_nodes(pfc, [[1, 2], [-1, -1], [-1, -1]], [INT, 0, 2]))
    assert st == BAD and "bad leaf id" in msg
    st, msg = _refused(pfc, _three_nodes(pfc, [[1, 2], [-1, -1], [-1, -1]], [INT, 0, -1]))
    assert st == BAD and "bad leaf id" in msg
    st, msg = _refused(pfc, _three_nodes(pfc, [[1, 1], [-1, -1], [-1, -1]], [INT, 0, 1]))
    assert st == BAD and "not a tree" in msg               # a shared child, a node never reached
    st, msg = _refused(pfc, _three_nodes(pfc, [[1, 2], [2, 1], [-1, -1]], [INT, INT, 0]))
    assert st == BAD and "not a tree" in msg               # a cycle: node 1 is its own child


def test_trees_too_deep_are_refused_at_finalize(pfc):
    """Caterpillars of 150 + 148 leaves have the depth sum 296, the deepest pfc_finalize accepts (3 x 297 + 3 = 894 of the
    896 reservable stack slots); one more leaf is PFC_ERR_BAD_ARG, and the handle destroys cleanly."""
    from test_gpu_broadphase import _meshes
    import tree_reference
    G = pfc.geometry
    rng = np.random.default_rng(5)

    def cat(n, tet):
        mesh = _meshes(pfc, n)[1 if tet else 0]
        return H.tree_caterpillar(tree_reference.build_tree_py(G, mesh), rng)
    ta, tb, tb1 = cat(150, False), cat(148, True), cat(149, True)
    assert ta.depth() + tb.depth() == 296 and ta.depth() + tb1.depth() == 297
    assert _refused(pfc, ta, tb, 150, 148) is None
    st, msg = _refused(pfc, ta, tb1, 150, 149)
    assert st == pfc._lib.ERR_BAD_ARG and "too deep" in msg and "297" in msg
