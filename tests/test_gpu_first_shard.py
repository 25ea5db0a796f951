"""What runs on the first shard of a multi-device handle -- dynamics, accelerations, their Dual forms, the value chain
pfc_state_derivative_device and a Radau step -- against the same calls on a single-device handle, and a refusal whose message has to
travel from the shard to the handle the user holds.

Setup: the C1 boxes mechanism and state of tests/test_gpu_dynamics_dual.py's Rig("C1", fixed_order=1) (3 scenes, 4 items each,
n_dir = 6), once on a single-device handle and once on a handle over the devices [0, 0].

Tolerances: dynamics, accelerations and their Dual forms use no atomics and run on one context on either handle: bytes.  In the value
chain the evaluation is sharded, everything else runs on the first shard: counts and info are equal, the members of that file's EXACT
list that a value call produces are bytes, and wrench, sdot, f and vdot are held to the 1e-9 relative bound that file uses between
two handles.  The Radau step runs entirely on the first shard's context: bytes."""
import numpy as np
import pytest

import helpers as H
import test_dynamics_abi as D
import test_kinematics_abi as K
from test_gpu_dynamics_dual import EXACT, Rig
from test_gpu_items_from_bodies import Guarded, _dev, _torch
from test_gpu_kinematics import _set
from test_gpu_radau import BOX_MASS, BOX_R, _bits, _box_states

pytestmark = pytest.mark.gpu

DEVICES = [0, 0]
CHAIN_VALUES = ("x_w_b", "twist_w_b", "jac", "pose", "twist", "x_w_r2", "body_1", "body_2", "qdot", "H", "c")
assert set(CHAIN_VALUES) <= set(EXACT)


def _sync():
    _torch().cuda.synchronize()


def _c1_handle(pfc, rig, inertia=True, **kw):
    """The scenario of Rig("C1", fixed_order=1) built again, with build_scenario's keywords kw."""
    w = pfc.configs.c1_boxes()
    m = pfc.configs.build_scenario(w, **kw)
    for k, c in enumerate(w.instructions):
        m.set_instruction_bodies(k, c.id_1, c.id_2)
    m.set_option("fixed_order", 1)
    _set(m, rig.mech)
    if inertia:
        m.set_inertia(rig.inertia, D.GRAVITY)
    return m


@pytest.fixture(scope="module")
def pair(pfc):
    """Two rigs with the same inputs (Rig's generators are seeded): A on its single-device handle, B on a handle over DEVICES."""
    A, B = Rig(pfc, "C1", 1), Rig(pfc, "C1", 1)
    B.m.close()
    B.m = _c1_handle(pfc, B, devices=DEVICES)
    yield A, B
    A.m.close(); B.m.close()


def test_dynamics_and_accelerations_return_the_same_bytes_on_both_handles(pair):
    A, B = pair
    ns, nd, nv, nb = A.ns, A.N_DIR, A.nv, A.ns * A.mech["n_body"]
    q, v = A.d_q.data_ptr(), A.d_v.data_ptr()
    dq, dv = (t.data_ptr() for t in A.chunks[0][2:])
    # one set of inputs for both handles: the body states and their partials of the single-device handle, random f and d_f
    kin, dkin = [Guarded(nb, 12), Guarded(nb, 6)], [Guarded(nb * nd, 12), Guarded(nb * nd, 6)]
    _sync()
    A.m.kinematics_device(ns, q, v, kin[0].ptr, kin[1].ptr, 0)
    A.m.kinematics_dual_device(ns, nd, q, v, dq, dv, dkin[0].ptr, dkin[1].ptr, 0)
    rng = np.random.default_rng(83)
    d_f, d_df = _dev(rng.standard_normal((ns, nv))), _dev(rng.standard_normal((ns, nd, nv)))
    tau, dtau = A.d_tau.data_ptr(), A.d_dtau.data_ptr()
    got = []
    for R in (A, B):
        val = [Guarded(ns, nv), Guarded(ns * nv, nv), Guarded(ns, nv)]                          # qdot H c
        par = [Guarded(ns * nd, nv), Guarded(ns * nd * nv, nv), Guarded(ns * nd, nv)]           # dqdot dH dc
        acc = [Guarded(ns, nv), Guarded(ns, 1, True)]                                           # vdot info
        dacc = [Guarded(ns, nv), Guarded(ns * nd, nv), Guarded(ns, 1, True)]                    # vdot dvdot info
        _sync()
        R.m.dynamics_device(ns, q, v, kin[0].ptr, kin[1].ptr, *[o.ptr for o in val])
        R.m.dynamics_dual_device(ns, nd, q, v, dq, dv, kin[0].ptr, kin[1].ptr, dkin[0].ptr, dkin[1].ptr, *[o.ptr for o in par])
        R.m.accelerations_device(ns, val[1].ptr, val[2].ptr, d_f.data_ptr(), tau, *[o.ptr for o in acc])
        R.m.accelerations_dual_device(ns, nd, val[1].ptr, val[2].ptr, d_f.data_ptr(), tau, par[1].ptr, par[2].ptr, d_df.data_ptr(), dtau,
                                      *[o.ptr for o in dacc])
        _sync()
        got.append([o.rows().copy() for o in val + par + acc + dacc])      # rows() checks the guard words
    names = ("qdot", "H", "c", "dqdot", "dH", "dc", "vdot", "info", "vdot (Dual)", "dvdot", "info (Dual)")
    for name, a, b in zip(names, *got):
        assert a.tobytes() == b.tobytes(), name
        assert "info" in name or np.abs(a).max() > 0, name
    assert not got[0][7].any() and not got[0][10].any()


def test_value_chain_on_both_handles(pair):
    A, B = pair
    snaps = []
    for R in (A, B):
        r = [t.data_ptr() for t in R.res]
        R.checked(lambda: R.m.state_derivative_device(
            R.n, R.d_ids.data_ptr(), R.d_sc.data_ptr(), R.ns, R.d_q.data_ptr(), R.d_v.data_ptr(), 0, R.d_tau.data_ptr(), *R._p(R.kin),
            *R._p(R.items), r[0], r[1], r[4], R.f.ptr, *R._p(R.val)))
        snaps.append(R.snapshot())
    a, b = snaps
    ns, n = A.ns, A.n
    assert a["counts"][:, 3].all(), "an item has no contact"
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["info"], b["info"]) and not a["info"].any()
    for k in CHAIN_VALUES:
        assert a[k].tobytes() == b[k].tobytes(), k
    per_item = lambda k: [H.rel_err(a[k].reshape(n, -1)[i], b[k].reshape(n, -1)[i]) for i in range(n) if np.linalg.norm(b[k].reshape(n, -1)[i]) > 0]
    per_scene = lambda k: max(H.rel_err(a[k].reshape(ns, -1)[s], b[k].reshape(ns, -1)[s]) for s in range(ns))
    worst = {k: max(per_item(k) or [0.0]) for k in ("wrench", "sdot")}
    worst.update({k: per_scene(k) for k in ("f", "vdot")})
    print("value chain, one device against [0, 0], largest relative difference: " + ", ".join(f"{k} {e:.2e}" for k, e in worst.items()))
    assert all(np.abs(a[k]).max() > 0 for k in ("wrench", "f", "vdot"))
    assert all(e < 1e-9 for e in worst.values()), worst


def _box(pfc, **kw):
    """tests/test_gpu_radau.py's _box_scenario under fixed_order, with build_scenario's keywords kw."""
    w = pfc.configs.c2_box_on_plane(1, n_div=1)
    w.instructions = [pfc.configs.InsSpec(0, 1, "bristle", chi=0.5, mu_d=0.3)]
    m = pfc.configs.build_scenario(w, **kw)
    m.set_option("fixed_order", 1)
    mech = K.make_mech([-1], [K.FLOATING], [K.WORLD_X], [[0.0, 0.0, 0.0]])
    m.set_mechanism(mech["parent"], mech["joint_type"], mech["x_p_j"], mech["axis"])
    m.set_instruction_bodies(0, -1, 0)
    Ic = np.eye(3) * (2.0 / 3.0) * BOX_MASS * BOX_R * BOX_R
    m.set_inertia(D.make_inertia(BOX_MASS, [0.0, 0.0, 0.0], Ic).reshape(1, 13), D.GRAVITY)
    return m


def test_radau_step_on_both_handles(pfc):
    x0 = _box_states(2, [BOX_R - 1e-3, BOX_R - 2e-3], [0.0, -0.02])
    res = []
    for kw in ({}, {"devices": DEVICES}):
        m = _box(pfc, **kw)
        assert m.radau_configure(2, [0]) == 18
        m.radau_set_state(x0)
        out = m.radau_step()
        res.append((m.radau_get_state(), out))
        m.close()
    ((xa, ta), oa), ((xb, tb), ob) = res
    assert _bits(xa) == _bits(xb) and _bits(ta) == _bits(tb), np.abs(xa - xb).max()
    assert oa["flags"].tolist() == ob["flags"].tolist() == [0, 0]
    assert oa["iters"].tolist() == ob["iters"].tolist() and oa["attempts"].tolist() == ob["attempts"].tolist()
    assert _bits(oa["h_taken"]) == _bits(ob["h_taken"]) and (ta > 0).all() and np.abs(xa - x0).max() > 0


def test_a_refusal_on_the_first_shard_reaches_the_handle(pfc, pair):
    A, _ = pair
    L = pfc._lib
    m = _c1_handle(pfc, A, inertia=False, devices=DEVICES)
    out = [Guarded(A.ns, A.nv), Guarded(A.ns * A.nv, A.nv), Guarded(A.ns, A.nv)]
    _sync()
    with pytest.raises(L.PFCError) as e:
        m.dynamics_device(A.ns, A.d_q.data_ptr(), A.d_v.data_ptr(), A.kin[0].ptr, A.kin[1].ptr, *[o.ptr for o in out])
    _sync()
    assert e.value.status == L.ERR_STATE and "pfc_set_inertia" in str(e.value)
    assert all(o.untouched() for o in out)
    m.close()
