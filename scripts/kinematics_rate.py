"""Cost of the kinematics from joint states on the device (pfc_kinematics_device), of the chain pfc_eval_state_device + pfc_check, and
of the route it replaces: the host's kinematics (scenario.joint_kinematics, NumPy), the upload of body states and Jacobians,
pfc_eval_bodies_device, pfc_scatter_generalized_device and pfc_check.  Shapes warmed up; medians over `reps` blocks of 25 calls, in
microseconds: device events for the kernels alone, a host clock (the blocks end with a synchronise) for the two chains, which alternate
block by block.

  kin     k_kinematics + k_kin_jacobian alone, all three outputs
  state   pfc_eval_state_device + pfc_check: one upload-free call from (q, v) to f_generalized
  parent  joint_kinematics per scene on the host, three host-to-device copies, pfc_eval_bodies_device, the scatter, pfc_check

usage: python scripts/kinematics_rate.py [reps]      (C1: one scene of five bodies, nv = 24; C4: 256 scenes of a rooted ground and a
floating box, nv = 6 each).  PFC_LIB=<variant> PFC_ALLOW_DIAGNOSTIC=1 measures a variant build of the library."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pfc_pkg
import torch

from items_from_bodies_rate import c1_states, median_us

BLOCK = 25
EYE12 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


def mrp_from_rotation(R):
    """Modified Rodrigues parameters p = q_vec / (1 + q_w) of a rotation matrix (rotations well below pi from the identity or not:
    the quaternion with q_w >= 0)."""
    w = 0.5 * np.sqrt(max(1.0 + np.trace(R), 0.0))
    if w > 1e-3:
        vec = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (4.0 * w)
    else:      # a half turn: the axis from the largest diagonal entry
        k = int(np.argmax(np.diag(R)))
        vec = (R[:, k] + np.eye(3)[k]) / np.sqrt(2.0 * (1.0 + R[k, k]))
    return vec / (1.0 + w)


def c1_mechanism(pfc):
    """C1 as a mechanism: the plane fixed on the world, four floating boxes whose joint_poses carry the boxes' turns about z."""
    L = pfc._lib
    w, x, tw, bind, _ = c1_states(pfc.configs)
    x_p_j = np.zeros((5, 12)); x_p_j[:, :9] = x[0, :, :9]
    q, v = np.zeros((1, 24)), np.zeros((1, 24))
    for b in range(1, 5):
        q[0, 6 * (b - 1) + 3:6 * b] = x[0, b, 9:]
        v[0, 6 * (b - 1):6 * (b - 1) + 3] = tw[0, b, :3]
    mech = ([-1] * 5, [L.JOINT_FIXED] + [L.JOINT_FLOATING_MRP] * 4, x_p_j, None)
    return w, mech, q, v, bind, None


def c4_mechanism(pfc, n_scene=256):
    """C4: one scene per item, the ground fixed on the world (body 0) and the box floating (body 1); the joint state reproduces the
    workload's items up to rounding."""
    L = pfc._lib
    w = pfc.configs.c2_box_on_plane(n_scene, montecarlo=True)
    q, v = np.zeros((n_scene, 6)), np.zeros((n_scene, 6))
    assert (w.instructions[0].id_1, w.instructions[0].id_2) == (0, 1)      # mesh_1 the ground, mesh_2 the box
    for k in range(n_scene):      # x_r1_r2 is the box's pose in the ground's frame, twist_r2_r1_r2 its twist in its own frame
        q[k, :3] = mrp_from_rotation(w.pose[k, 12:21].reshape(3, 3, order="F"))
        q[k, 3:] = w.pose[k, 21:24]
        v[k] = w.twist[k]
    mech = ([-1, -1], [L.JOINT_FIXED, L.JOINT_FLOATING_MRP], [EYE12, EYE12], None)
    bind = [(w.instructions[0].id_1, w.instructions[0].id_2)]
    return w, mech, q, v, bind, np.arange(n_scene, dtype=np.int32)


def host_block_us(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(BLOCK):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / BLOCK)
    return out


def run(pfc, name, w, mech, q, v, bind, scene, reps):
    dev = torch.device("cuda:0")
    S = pfc.scenario
    m = pfc.configs.build_scenario(w)
    for k, (a, b) in enumerate(bind):
        m.set_instruction_bodies(k, a, b)
    m.set_mechanism(*mech)
    n_body, nq, nv = m.mechanism_sizes()
    n, n_scene = w.n_items, q.shape[0]
    nb = n_scene * n_body
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    z = lambda *sh, dt=torch.float64: torch.zeros(sh, dtype=dt, device=dev)
    ids, s, dq, dv = t(w.ins_ids, torch.int32), t(w.s), t(q), t(v)
    dsc = t(scene, torch.int32) if scene is not None else None
    sc_p = dsc.data_ptr() if scene is not None else 0
    o_x, o_tw, o_j = z(nb, 12), z(nb, 6), z(nb, nv, 6)
    o_pose, o_twist, o_xr = z(n, 24), z(n, 6), z(n, 12)
    o_b1, o_b2 = z(n, dt=torch.int32), z(n, dt=torch.int32)
    o_w, o_sd, o_ct, o_f = z(n, 6), z(n, 6), z(n, 4, dt=torch.int32), z(n_scene, nv)
    st = torch.cuda.current_stream().cuda_stream
    kin_outs = (o_x.data_ptr(), o_tw.data_ptr(), o_j.data_ptr())
    item_outs = (o_pose.data_ptr(), o_twist.data_ptr(), o_xr.data_ptr(), o_b1.data_ptr(), o_b2.data_ptr())
    eval_outs = (o_w.data_ptr(), o_sd.data_ptr(), o_ct.data_ptr())

    def kin():
        m.kinematics_device(n_scene, dq.data_ptr(), dv.data_ptr(), *kin_outs, st)

    def checked(enqueue):      # the first evaluations of a handle size its lists (ERR_OVERFLOW: issue the same call again)
        def fn():
            for _ in range(40):
                enqueue()
                if m.check() == 0:
                    return
            raise RuntimeError("work lists kept overflowing")
        return fn

    state = checked(lambda: m.eval_state_device(n, ids.data_ptr(), sc_p, n_scene, dq.data_ptr(), dv.data_ptr(), s.data_ptr(), *kin_outs,
                                                *item_outs, *eval_outs, o_f.data_ptr(), st))
    parent_tab = (np.asarray(mech[0]), np.asarray(mech[1]), np.asarray(mech[2], dtype=np.float64), mech[3])

    def parent_enqueue():
        hx, htw, hj = zip(*(S.joint_kinematics(*parent_tab, q[k], v[k]) for k in range(n_scene)))
        ux, utw, uj = (torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (np.array(hx), np.array(htw), np.array(hj)))
        m.eval_bodies_device(n, ids.data_ptr(), sc_p, n_scene, n_body, ux.data_ptr(), utw.data_ptr(), s.data_ptr(), *item_outs, *eval_outs, st)
        m.scatter_generalized_device(n, o_w.data_ptr(), o_xr.data_ptr(), o_b1.data_ptr(), o_b2.data_ptr(), sc_p, n_scene, nv, uj.data_ptr(),
                                     o_f.data_ptr(), stream=st)
        parent_enqueue.keep = (ux, utw, uj)

    parent = checked(parent_enqueue)
    for fn in (state, kin, parent, state, parent):
        fn()
    torch.cuda.synchronize()
    # the measured configuration forms the workload's own items (a check of the set-up, not a test)
    err = float(np.abs(o_pose.cpu().numpy() - w.pose).max()), float(np.abs(o_twist.cpu().numpy() - w.twist).max())
    assert max(err) < 1e-9, err
    contact = int((o_ct.cpu().numpy()[:, 3] > 0).sum())
    f_parent = o_f.cpu().numpy().copy()
    state()
    torch.cuda.synchronize()
    f_err = float(np.abs(o_f.cpu().numpy() - f_parent).max() / max(np.abs(f_parent).max(), 1e-300))
    t_kin = median_us(kin, reps, BLOCK)
    t_state, t_parent = [], []
    for _ in range(reps):      # alternate the two chains block by block
        t_state += host_block_us(state, 1); t_parent += host_block_us(parent, 1)
    up_bytes = 8 * nb * (18 + 6 * nv)
    m.close()
    print(f"{name:>3s}: scenes {n_scene:4d} bodies {n_body} nv {nv:2d} items {n:4d} (in contact {contact:4d}) | kinematics alone {t_kin:7.2f} us | "
          f"eval_state_device+check {float(np.median(t_state)):8.1f} us | host kinematics + upload of {up_bytes} bytes + eval_bodies_device + "
          f"scatter + check {float(np.median(t_parent)):10.1f} us | max |pose - workload| {err[0]:.1e}, f relative {f_err:.1e}", flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    pfc = pfc_pkg.load()
    L = pfc._lib.lib()
    print(f"library {L.pfc_loaded_path} build_info {L.pfc_build_info():#x}", flush=True)
    run(pfc, "C1", *c1_mechanism(pfc), reps)
    run(pfc, "C4", *c4_mechanism(pfc), reps)


if __name__ == "__main__":
    main()
