"""The radius sums of the broadphase's Float32 node test as ONE fused multiply-add chain per axis (sat15_f32_core in
pfc_kernels.h; pfc_bp.h, "Error radius E", (4) and (5)): a NumPy Float32 emulation of that order -- the fma rounds once, as
tests/test_bp_error_bound.py emulates it -- against the Float64 axes of the reference (src/obb/bb_intersection.jl:29-72).

Sampled: seeded random boxes of both kinds (leaf x leaf: quaternion path, radius 320 u S; internal x internal: identity
quaternions, 24 u S), centred at their frame origins and up to 1 000 box sizes away from them, and the touching
configurations of tests/test_gpu_broadphase.py at 1 -/+ {1e-3, 1e-6, 1e-9, 1e-12} for both kinds (the leaf boxes rotated in
their mesh frames).  On EVERY axis |d_float - d_ref| must stay below the radius the kernel uses, E = k S + eabs with the
code's constants; the worst observed multiple of u S is printed.  The bound is derived in pfc_bp.h, not fitted to this.
CPU only."""
import numpy as np
import pytest

from test_bp_error_bound import U, axes, f32, fma, quat_mul32, quat_rot_inv32, quat_to_R32, quat_to_R64

K_LEAF, K_ALIGNED = np.float32(1.92e-5), np.float32(1.44e-6)        # test_pair_f32: >= 320 u, >= 24 u
TOLS = (1.0e-3, 1.0e-6, 1.0e-9, 1.0e-12)


def axes_chain(ea, eb, t, R, aR):
    """sat15_f32_core: per axis, |T.L| minus ONE chain over the radius terms (a face axis seeds it with its own extent)."""
    d = []
    for i in range(3):
        rs = fma(aR[..., i, 2], eb[..., 2], fma(aR[..., i, 1], eb[..., 1], fma(aR[..., i, 0], eb[..., 0], ea[..., i])))
        d.append(np.abs(t[..., i]) - rs)
    for j in range(3):
        tl = np.abs(fma(R[..., 2, j], t[..., 2], fma(R[..., 1, j], t[..., 1], R[..., 0, j] * t[..., 0])))
        rs = fma(aR[..., 2, j], ea[..., 2], fma(aR[..., 1, j], ea[..., 1], fma(aR[..., 0, j], ea[..., 0], eb[..., j])))
        d.append(tl - rs)
    i100, i221 = (1, 0, 0), (2, 2, 1)
    for m, (u, v) in enumerate(((1, 2), (0, 2), (0, 1))):       # rows of the cross block: t[v] R[u] - t[u] R[v]
        for j in range(3):
            tl = np.abs(fma(t[..., v], R[..., u, j], -(t[..., u] * R[..., v, j])))
            if m == 1:      # the middle row is written with the opposite sign (|.| of it is the same value bit for bit)
                tl = np.abs(fma(t[..., u], R[..., v, j], -(t[..., v] * R[..., u, j])))
            rs = fma(eb[..., i100[j]], aR[..., m, i221[j]],
                     fma(eb[..., i221[j]], aR[..., m, i100[j]], fma(ea[..., u], aR[..., v, j], ea[..., v] * aR[..., u, j])))
            d.append(tl - rs)
    return np.stack(d, axis=-1)


def device_and_reference(qa, qb, Rp, tp, ca, cb, ea, eb, leaf):
    """(|d_float - d_ref| per axis, d_float, radius E per pair, S) for box pairs given in Float64: box rotations as unit
    quaternions qa, qb, the pose (Rp, tp), centres and extents.  The device path is test_pair_f32's, operation by operation."""
    Ra, Rb = quat_to_R64(qa), quat_to_R64(qb)
    v64 = np.einsum("nij,nj->ni", Rp, cb) + (tp - ca)
    Rt = np.einsum("nki,nkl,nlj->nij", Ra, Rp, Rb)
    t64 = np.einsum("nki,nk->ni", Ra, v64)
    d_ref = axes(ea, eb, t64, Rt, np.abs(Rt) + 1e-14, lambda a, b, c: a * b + c)
    qaf, qbf, qpf = qa.astype(f32), qb.astype(f32), mat_to_quat(Rp).astype(f32)
    for qf, Rref in ((qaf, Ra), (qbf, Rb), (qpf, Rp)):       # the checks of pfc_add_mesh / pose_quat: who fails is exact-only
        q64 = qf.astype(np.float64)
        assert np.abs(quat_to_R64(q64) - Rref).max() <= 4 * U and np.abs((q64 ** 2).sum(-1) - 1).max() <= 2.25 * U
    eaf, ebf = ea.astype(f32), eb.astype(f32)
    Rpf, caf, cbf, tpf = Rp.astype(f32), ca.astype(f32), cb.astype(f32), tp.astype(f32)
    vf = np.stack([fma(Rpf[:, i, 2], cbf[:, 2], fma(Rpf[:, i, 1], cbf[:, 1], fma(Rpf[:, i, 0], cbf[:, 0], tpf[:, i] - caf[:, i])))
                   for i in range(3)], axis=-1)
    Rf = quat_to_R32(quat_mul32(quat_mul32(qaf, qpf, True), qbf, False))
    tf = quat_rot_inv32(qaf, vf)
    d_f = axes_chain(eaf, ebf, tf, Rf, np.abs(Rf))
    S = ((np.abs(vf[:, 0]) + np.abs(vf[:, 1])) + np.abs(vf[:, 2])) + ((eaf[:, 0] + eaf[:, 1]) + eaf[:, 2]) + ((ebf[:, 0] + ebf[:, 1]) + ebf[:, 2])
    # eabs as k_setup_items forms it (cmax >= |c|_1 of every node: here the one box each)
    babs = np.abs(ca).sum(-1) + np.abs(cb).sum(-1) + np.abs(tp).max(-1)
    eabs = (1.4306e-6 * babs).astype(f32) * f32(1.000001)
    E = fma(np.full_like(S, K_LEAF if leaf else K_ALIGNED), S, eabs)
    err = np.abs(d_f.astype(np.float64) - d_ref)
    return err, d_f, E.astype(np.float64), S.astype(np.float64)


def mat_to_quat(R):
    """unit quaternions (w, x, y, z) of rotation matrices, Float64 (largest-component branch)"""
    n = R.shape[0]
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    cand = np.stack([1 + tr, 1 + 2 * R[:, 0, 0] - tr, 1 + 2 * R[:, 1, 1] - tr, 1 + 2 * R[:, 2, 2] - tr], axis=-1)
    b = np.argmax(cand, axis=-1)
    q = np.empty((n, 4))
    a, x, y = R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]
    s01, s02, s12 = R[:, 1, 0] + R[:, 0, 1], R[:, 0, 2] + R[:, 2, 0], R[:, 2, 1] + R[:, 1, 2]
    rows = [np.stack([cand[:, 0], a, x, y], -1), np.stack([a, cand[:, 1], s01, s02], -1),
            np.stack([x, s01, cand[:, 2], s12], -1), np.stack([y, s02, s12, cand[:, 3]], -1)]
    for k in range(4):
        q[b == k] = rows[k][b == k]
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def random_pairs(n, leaf, seed, far_decades):
    """The sampling of tests/test_bp_error_bound.py::run; far_decades = None puts the boxes at their frame origins."""
    rng = np.random.default_rng(seed)

    def rand_q(k):
        q = rng.standard_normal((k, 4))
        q[: k // 4] *= rng.choice([1.0, 1e-3, 1e-6], size=(k // 4, 4))      # near-axis rotations
        return q / np.linalg.norm(q, axis=-1, keepdims=True)

    ident = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (n, 1))
    qa, qb, qp = (rand_q(n) if leaf else ident), (rand_q(n) if leaf else ident), rand_q(n)
    Rp = quat_to_R64(qp)
    scale = 10.0 ** rng.uniform(-3, 1, (n, 1))
    ea, eb = scale * rng.uniform(0.05, 1.0, (n, 3)), scale * rng.uniform(0.05, 1.0, (n, 3))
    v_goal = scale * rng.standard_normal((n, 3)) * rng.choice([0.3, 1.0, 3.0], size=(n, 1))      # around touching distance
    if far_decades is None:
        ca = cb = np.zeros((n, 3))
    else:
        far = scale * 10.0 ** rng.uniform(-1, far_decades, (n, 1))
        ca, cb = far * rng.standard_normal((n, 3)), far * rng.standard_normal((n, 3))
    tp = v_goal - np.einsum("nij,nj->ni", Rp, cb) + ca
    return qa, qb, Rp, tp, ca, cb, ea, eb


def touching_pairs(leaf, seed):
    """The face-corner and edge-edge touching configurations of tests/test_gpu_broadphase.py at 1 -/+ TOLS.  Leaf boxes are
    rotated in their mesh frames and the pose undoes it (the quaternion path); internal boxes are axis aligned."""
    from test_gpu_broadphase import EXT, _axis_angle, _cases
    rng = np.random.default_rng(seed)
    cases = _cases(TOLS)
    n = len(cases)
    Q = [(_axis_angle(rng.random() * 2 * np.pi, rng.standard_normal(3)), _axis_angle(rng.random() * 2 * np.pi, rng.standard_normal(3)))
         if leaf else (np.eye(3), np.eye(3)) for _ in EXT]
    Rp = np.array([Q[c[0]][0] @ c[1] @ Q[c[0]][1].T for c in cases])
    tp = np.array([Q[c[0]][0] @ c[2] for c in cases])
    qa = mat_to_quat(np.array([Q[c[0]][0] for c in cases]))
    qb = mat_to_quat(np.array([Q[c[0]][1] for c in cases]))
    ea = np.array([EXT[c[0]][0] for c in cases]); eb = np.array([EXT[c[0]][1] for c in cases])
    z = np.zeros((n, 3))
    return (qa, qb, Rp, tp, z, z, ea, eb), np.array([c[3] for c in cases]), np.array([c[4] for c in cases])


def worst(err, E, S):
    return float((err.max(-1) / E).max()), float((err.max(-1) / (U * S)).max())


@pytest.mark.parametrize("leaf", [True, False])
def test_random_boxes_stay_inside_the_radius(leaf):
    k = 320.0 if leaf else 24.0
    err, d_f, E, S = device_and_reference(*random_pairs(200_000, leaf, 41, None), leaf)
    share, mult = worst(err, E, S)
    undecided = np.abs(d_f.max(-1)) <= E
    # generic rotations only: the first quarter of the sample has near-axis poses, whose parallel-edge cross axes are degenerate
    # (d = 0 - 0: an overlapping pair of such boxes is undecided by construction and settled exactly, whatever the radius)
    generic = undecided[undecided.size // 4:]
    print(f"{'leaf' if leaf else 'internal'} pairs at their frame origins: worst |d_float - d_ref| = {mult:.2f} u S "
          f"(radius {k:.0f} u S), = {share:.3f} of E; undecided: {generic.mean():.2e} of the pairs with generic rotations, "
          f"{undecided.mean():.2e} of all")
    assert np.all(err < E[:, None])
    # the cap tests/test_gpu_bp_radii.py puts on the share of node tests settled exactly (1e-3) is not one a sound filter
    # comes near, even on pairs sampled AROUND touching distance (a descent mostly tests pairs far from it)
    assert generic.mean() < 1.0e-3
    err, d_f, E, S = device_and_reference(*random_pairs(200_000, leaf, 42, 3), leaf)
    share, mult = worst(err, E, S)
    print(f"{'leaf' if leaf else 'internal'} pairs up to 1 000 box sizes from their frame origins: worst error = {share:.3f} of E = k S + eabs")
    assert np.all(err < E[:, None])


@pytest.mark.parametrize("leaf", [True, False])
def test_touching_boxes_stay_inside_the_radius(leaf):
    k = 320.0 if leaf else 24.0
    args, expect, tol = touching_pairs(leaf, 43)
    err, d_f, E, S = device_and_reference(*args, leaf)
    share, mult = worst(err, E, S)
    print(f"touching {'leaf' if leaf else 'internal'} boxes: worst |d_float - d_ref| = {mult:.2f} u S (radius {k:.0f} u S), = {share:.3f} of E")
    assert np.all(err < E[:, None])
    # and what follows from it: a verdict the filter gives is the constructed truth; 1e-9 and 1e-12 are inside the radius
    dmax = d_f.max(-1).astype(np.float64)
    sep, hit = dmax > E, dmax < -E
    assert not np.any(sep & (expect == 1)) and not np.any(hit & (expect == 0) & (tol >= 1e-9))
    assert not np.any((sep | hit) & (tol <= 1e-9))
