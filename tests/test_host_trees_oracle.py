"""The host-supplied OBB trees of tests/helpers.py (rotated, shrunk, mixed, random topology) through the CPU oracle alone:
what tests/test_gpu_host_trees.py may rely on when it runs them on the device.

pfc_add_mesh takes any flattened tree, and the reference's tree_tree_intersect / BB_BB_intersect (src/obb/tree_types.jl:
88-111, src/obb/bb_intersection.jl:2-74; oracle/pfc_oracle.c) use whatever the tree holds.  On the 80-triangle sphere
against the 48-tet box, 200 random poses:
  - trees whose boxes still enclose their children (rotated, mixed, random_topology) find the built tree's non-empty pairs
    and traction points on every pose, and its wrench to 1e-9 (the pairs are summed in another order);
  - the rotation of an internal box matters: against the same boxes with R := I the counters differ on >= 90 % of poses,
    so a kernel that ignores R on internal nodes cannot pass the device test;
  - shrunk boxes (x 0.7) prune: counts[2:] change on >= a quarter of the poses.
"""
import functools

import numpy as np
import pytest

import helpers as H

N_POSE = 200


@functools.lru_cache(maxsize=None)
def _counts(pfc, scene, twin=False):
    w = H.host_tree_workload(pfc, scene, N_POSE, span=0.6)
    if twin:
        for ms in w.meshes:
            ms.tree = H.tree_identity_twin(ms.tree)
    ref = H.oracle_run(pfc, w, debug=False)
    assert all(r.status == 0 for r in ref)
    return np.array([r.counts for r in ref]), np.array([r.wrench for r in ref])


@pytest.mark.parametrize("scene", ["rotated", "mixed", "random_topology"])
def test_enclosing_trees_find_the_built_trees_contact(pfc, scene):
    c0, w0 = _counts(pfc, "built")
    c1, w1 = _counts(pfc, scene)
    assert np.count_nonzero(c0[:, 3]) > N_POSE // 2                 # the poses are in contact
    assert np.array_equal(c1[:, 2:], c0[:, 2:])
    assert not np.array_equal(c1[:, :2], c0[:, :2])                  # ... by another descent
    for k in range(N_POSE):
        if np.linalg.norm(w0[k]) == 0.0:
            assert np.linalg.norm(w1[k]) == 0.0
        else:
            assert H.rel_err(w1[k], w0[k]) < 1e-9, (k, w1[k], w0[k])


def test_rotation_of_internal_boxes_changes_the_descent(pfc):
    c1, _ = _counts(pfc, "rotated")
    c2, _ = _counts(pfc, "rotated", True)
    differ = np.any(c1 != c2, axis=1)
    assert differ.mean() >= 0.9, differ.mean()
    assert np.any(c1[:, 1] != c2[:, 1])                               # candidate sets too, not only node tests


def test_shrunk_boxes_prune(pfc):
    c0, _ = _counts(pfc, "built")
    c1, _ = _counts(pfc, "shrunk")
    changed = np.any(c1[:, 2:] != c0[:, 2:], axis=1)
    assert changed.mean() >= 0.25, changed.mean()


@pytest.mark.parametrize("scene", H.HOST_TREE_SCENES)
def test_generated_trees_are_trees_over_the_same_leaves(pfc, scene):
    G = pfc.geometry
    w = H.host_tree_workload(pfc, scene, 1)
    for ms in w.meshes:
        t = ms.tree
        n_elem = ms.mesh.n_tri if ms.mesh.tri is not None else ms.mesh.n_tet
        internal = t.leaf == G.INTERNAL
        assert t.n_node == 2 * n_elem - 1 and np.array_equal(np.sort(t.leaf[~internal]), np.arange(n_elem))
        kids = t.child[internal].reshape(-1)
        assert np.array_equal(np.sort(kids), np.arange(1, t.n_node))  # every node but the root is the child of one node
        assert np.all(t.child[internal] > np.nonzero(internal)[0][:, None])      # preorder
        assert np.all(t.child[~internal] == -1)
        for k in range(t.n_node):
            R = t.R[k].reshape(3, 3, order="F")
            assert np.allclose(R.T @ R, np.eye(3), atol=1e-14) and np.linalg.det(R) > 0
    t1, t2 = w.meshes[0].tree, w.meshes[1].tree
    if scene == "caterpillar":
        assert t1.depth() == 79 and t2.depth() == 47
    if scene == "single_leaf":
        assert t1.depth() == 79 and t2.n_node == 1
    if scene in ("rotated", "shrunk"):
        assert not np.any(np.all(t1.R[t1.leaf == G.INTERNAL] == np.eye(3).reshape(-1), axis=1))
    if scene == "mixed":
        for t in (t1, t2):
            ident = np.all(t.R[t.leaf == G.INTERNAL] == np.eye(3).reshape(-1), axis=1)
            assert 0.25 < ident.mean() < 0.75
