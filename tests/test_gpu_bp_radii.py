"""The broadphase's Float32 node test with its radius sums as fused multiply-add chains and, in k_bp_dfs32, the seed's pose
as wave-uniform scalars read from the item record (ItemRec.R12f, t12f, q12, bp_eabs, pose_exact): verdicts are the
reference's.  Each scene is evaluated through the one-launch kernel (default options for these sizes), the batched Float32
descent (fused = 0: k_bp_dfs32) and the all-Float64 descent (fused = 0, no_filter = 1: k_bp_dfs); the four per-item
counters and the candidate sets must be bit-equal between them and equal to the oracle's.

  * 32 poses of a reduced C3 pair (the sizes of the smoke run), where the share of node tests settled by the exact test must
    stay below 1e-3 (a cap against a filter that decides nothing, not a measurement: about 2e-5 is usual);
  * 8 box-on-plane scenes: every parallel-edge cross axis is exactly degenerate (d = 0 - 0);
  * the touching boxes of tests/test_gpu_broadphase.py (host-supplied one-node and three-node trees) at 1 -/+ {1e-3, 1e-6,
    1e-9, 1e-12}, with items whose pose is not a rotation among them: pose_quat fails, the scalar pose_exact flag sends every
    test of the item to the exact path."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as Orc

pytestmark = pytest.mark.gpu

OPTIONS = {"fused": {}, "dfs32": dict(fused=0), "dfs64": dict(fused=0, no_filter=1)}


def _settled(pfc, m):
    out = (C.c_longlong * 16)()
    assert pfc._lib.lib().pfc_debug_stamps(m._h, out) == 0
    return int(out[7])       # node pairs settled by the exact test in the last evaluation


def _against_oracle(pfc, w):
    """Evaluate w under every option set: counters and candidate sets equal to the oracle's.  Returns (counts, pairs settled
    exactly by k_bp_dfs32)."""
    import helpers as H
    ref = H.oracle_run(pfc, w)
    settled, counts0 = None, None
    for name, opts in OPTIONS.items():
        m = pfc.configs.build_scenario(w, debug=True)
        for k, v in opts.items():
            m.set_option(k, v)
        wrench, sdot, counts = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
        if name == "dfs32":
            settled = _settled(pfc, m)
        for k in range(w.n_items):
            assert np.array_equal(counts[k], ref[k].counts), (name, k, counts[k], ref[k].counts)
            pairs, clip_n = H.sorted_pairs(*m.debug_pairs(k))
            rp, rc = H.sorted_pairs(ref[k].pairs, ref[k].clip_n)
            assert np.array_equal(pairs, rp) and np.array_equal(clip_n, rc), (name, k)
        m.close()
        if counts0 is None:
            counts0 = counts.copy()
        assert np.array_equal(counts, counts0), name
    return counts0, settled


def test_reduced_c3_batch(pfc):
    w = pfc.configs.c3_blob_tool(32, seed=17, n_div_blob=6, n_div_tool=5)
    counts, settled = _against_oracle(pfc, w)
    n_test = int(counts[:, 0].sum())
    print(f"reduced C3, 32 poses: {n_test} node tests, {settled} settled exactly ({settled / n_test:.2e})")
    assert counts[:, 1].sum() > 0 and counts[:, 3].sum() > 0
    assert settled < 1.0e-3 * n_test, (settled, n_test)


def test_box_on_plane_scenes(pfc):
    w = pfc.configs.c2_box_on_plane(8)
    counts, settled = _against_oracle(pfc, w)
    print(f"8 box-on-plane scenes: {int(counts[:, 0].sum())} node tests, {settled} settled exactly")
    assert counts[:, 3].sum() > 0


@pytest.fixture(scope="module")
def touching():
    """(cases, oracle verdict of every case's root pair): the touching configurations, and every 97th of them again with its
    pose scaled by 1 + 1e-3 (not a rotation: pose_exact).  The oracle's BB_BB_intersect takes the matrix as given."""
    from test_gpu_broadphase import EXT, _cases
    cases = _cases()
    cases += [(kind, R * (1.0 + 1.0e-3), t, None, None) for kind, R, t, _, _ in cases[::97]]
    L = Orc.lib()
    dp = C.POINTER(C.c_double)
    P = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(dp)
    z, I = np.zeros(3), np.eye(3).reshape(-1)
    ref = np.array([bool(L.pfo_bb_bb_intersect(P(z), P(EXT[kind][0]), P(I), P(z), P(EXT[kind][1]), P(I), P(R.reshape(-1, order="F")), P(t)))
                    for kind, R, t, _, _ in cases])
    return cases, ref


@pytest.mark.parametrize("internal", [False, True])
def test_touching_boxes(pfc, touching, internal):
    from test_gpu_broadphase import EXT, _meshes, _tree
    cases, ref = touching
    S = pfc.scenario
    tri, tet = _meshes(pfc, 2 if internal else 1)
    n = len(cases)
    ids = np.array([c[0] for c in cases], dtype=np.int32)
    pose = np.zeros((n, 24))
    for k, (kind, R, t, _, _) in enumerate(cases):
        Ri = np.linalg.inv(R)
        pose[k, 12:21] = R.reshape(-1, order="F"); pose[k, 21:24] = t
        pose[k, 0:9] = Ri.reshape(-1, order="F"); pose[k, 9:12] = -(Ri @ t)
    n_exact = sum(1 for c in cases if c[4] is None or c[4] <= 1e-9)     # non-rotations, and offsets inside the radius
    res = {}
    for name, opts in (("dfs32", dict(no_filter=0, bfs_levels=0)), ("dfs64", dict(no_filter=1, bfs_levels=0))):
        m = S.MechanismScenario()
        for k, (ea, eb) in enumerate(EXT):
            i1 = m.add_contact(f"a{k}", tri, tree=_tree(pfc, ea, internal))
            i2 = m.add_contact(f"b{k}", tet, c_prop=S.ContactProperties(1.0e6), tree=_tree(pfc, eb, internal))
            m.add_friction_regularize(i1, i2, mu_d=0.3)
        m.finalize()
        for k, v in opts.items():
            m.set_option(k, v)
        res[name] = m.force_all_elastic_intersections(pose, np.zeros((n, 6)), np.zeros((n, 6)), ids)[2].copy()
        if name == "dfs32":
            assert _settled(pfc, m) >= n_exact, (_settled(pfc, m), n_exact)
        m.close()
    assert np.array_equal(res["dfs32"], res["dfs64"])
    counts = res["dfs32"]
    hit = counts[:, 0] == 5 if internal else counts[:, 1] == 1      # internal: root hit + its 4 child pairs; leaf: one candidate
    assert set(np.unique(counts[:, 0])) <= ({1, 5} if internal else {1})
    assert np.array_equal(hit, ref), np.nonzero(hit != ref)[0][:10]
    for k, (_, _, _, expect, tol) in enumerate(cases):
        if tol is not None and tol >= 1e-9:
            assert bool(hit[k]) == bool(expect), (k, tol)
