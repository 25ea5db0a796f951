"""Cost of the forward dynamics on the device: pfc_dynamics_device alone, pfc_accelerations_device alone, and the chain
pfc_state_derivative_device + pfc_check against what a host pays before it can start its own dynamics -- pfc_eval_state_device +
pfc_check + the download of f_generalized.  Shapes warmed up; medians over `reps` blocks of 25 calls, in microseconds: device events
for the kernels alone, a host clock (the blocks end with a synchronise) for the two chains, which alternate block by block.

  dyn     k_dynamics alone, all three outputs (qdot, H, c)
  accel   k_accel alone
  chain   pfc_state_derivative_device + pfc_check: from (q, v, s) to qdot, vdot, sdot, nothing downloaded
  parent  pfc_eval_state_device + pfc_check + f copied to the host (pageable memory, as NumPy gives it)
  eval    pfc_eval_state_device + pfc_check, nothing downloaded (what the chain adds its two launches to)
  parts   pfc_eval_state_device + pfc_check, then pfc_dynamics_device and pfc_accelerations_device enqueued after the check returned
  enqueue the host's time inside pfc_state_derivative_device and inside pfc_eval_state_device alone (an idle stream before, the check
          outside the clock): what the two further launches cost the host

usage: python scripts/dynamics_rate.py [reps] [json]      (C1: one scene of five bodies, nv = 24; C4: 256 scenes of a rooted ground
and a floating box, nv = 6 each; json: a file the figures are also written to)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pfc_pkg
import torch

from items_from_bodies_rate import median_us
from kinematics_rate import BLOCK, c1_mechanism, c4_mechanism, host_block_us


def box_inertias(pfc, w, mech):
    """The inertia of the mesh of the same index at density 400 for every floating body (a tet mesh solid, a tri mesh a shell 0.09
    thick, the reference's test values), zeros for the fixed ones."""
    L = pfc._lib
    out = np.zeros((len(mech[0]), 13))
    for b, t in enumerate(mech[1]):
        if t == L.JOINT_FLOATING_MRP:
            mesh = w.meshes[b].mesh
            out[b] = pfc.geometry.mesh_inertia(mesh, 400.0, None if mesh.tet is not None else 0.09)
    return out


def run(pfc, name, w, mech, q, v, bind, scene, reps):
    dev = torch.device("cuda:0")
    m = pfc.configs.build_scenario(w)
    for k, (a, b) in enumerate(bind):
        m.set_instruction_bodies(k, a, b)
    m.set_mechanism(*mech)
    m.set_inertia(box_inertias(pfc, w, mech))
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
    o_qd, o_H, o_c, o_vd, o_info = z(n_scene, nq), z(n_scene, nv, nv), z(n_scene, nv), z(n_scene, nv), z(n_scene, dt=torch.int32)
    st = torch.cuda.current_stream().cuda_stream
    eval_args = (o_x.data_ptr(), o_tw.data_ptr(), o_j.data_ptr(), o_pose.data_ptr(), o_twist.data_ptr(), o_xr.data_ptr(), o_b1.data_ptr(),
                 o_b2.data_ptr(), o_w.data_ptr(), o_sd.data_ptr(), o_ct.data_ptr(), o_f.data_ptr())
    dyn_outs = (o_qd.data_ptr(), o_H.data_ptr(), o_c.data_ptr())

    def dyn():
        m.dynamics_device(n_scene, dq.data_ptr(), dv.data_ptr(), o_x.data_ptr(), o_tw.data_ptr(), *dyn_outs, st)

    def accel():
        m.accelerations_device(n_scene, o_H.data_ptr(), o_c.data_ptr(), o_f.data_ptr(), 0, o_vd.data_ptr(), o_info.data_ptr(), st)

    def checked(enqueue, after=lambda: None):      # the first evaluations of a handle size its lists (ERR_OVERFLOW: issue the call again)
        def fn():
            for _ in range(40):
                enqueue()
                if m.check() == 0:
                    return after()
            raise RuntimeError("work lists kept overflowing")
        return fn

    enq_chain = lambda: m.state_derivative_device(n, ids.data_ptr(), sc_p, n_scene, dq.data_ptr(), dv.data_ptr(), s.data_ptr(), 0,
                                                  *eval_args, *dyn_outs, o_vd.data_ptr(), o_info.data_ptr(), st)
    enq_eval = lambda: m.eval_state_device(n, ids.data_ptr(), sc_p, n_scene, dq.data_ptr(), dv.data_ptr(), s.data_ptr(), *eval_args, st)
    chain = checked(enq_chain)
    parent = checked(lambda: m.eval_state_device(n, ids.data_ptr(), sc_p, n_scene, dq.data_ptr(), dv.data_ptr(), s.data_ptr(), *eval_args, st),
                     lambda: o_f.cpu())
    bare = checked(lambda: m.eval_state_device(n, ids.data_ptr(), sc_p, n_scene, dq.data_ptr(), dv.data_ptr(), s.data_ptr(), *eval_args, st))
    parts = checked(lambda: m.eval_state_device(n, ids.data_ptr(), sc_p, n_scene, dq.data_ptr(), dv.data_ptr(), s.data_ptr(), *eval_args, st),
                    lambda: (dyn(), accel()))
    for fn in (chain, parent, dyn, accel, chain, parent):
        fn()
    torch.cuda.synchronize()
    chain()
    torch.cuda.synchronize()
    info = o_info.cpu().numpy()
    assert not info.any() and np.isfinite(o_vd.cpu().numpy()).all(), info
    contact = int((o_ct.cpu().numpy()[:, 3] > 0).sum())
    t_dyn, t_accel = median_us(dyn, reps, BLOCK), median_us(accel, reps, BLOCK)
    t_chain, t_parent, t_bare, t_parts = [], [], [], []
    for _ in range(reps):      # alternate the chains block by block
        t_chain += host_block_us(chain, 1); t_parent += host_block_us(parent, 1)
        t_bare += host_block_us(bare, 1); t_parts += host_block_us(parts, 1)

    def enqueue_us(enq):
        out = []
        for _ in range(reps * 5):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); enq(); t1 = time.perf_counter()
            assert m.check() == 0
            out.append((t1 - t0) * 1e6)
        return float(np.median(out))

    e_chain, e_eval = enqueue_us(enq_chain), enqueue_us(enq_eval)
    m.close()
    row = dict(config=name, n_scene=n_scene, n_body=n_body, nv=nv, items=n, in_contact=contact, reps=reps, block=BLOCK,
               dynamics_us=float(t_dyn), accelerations_us=float(t_accel), state_derivative_check_us=float(np.median(t_chain)),
               eval_state_check_download_f_us=float(np.median(t_parent)), eval_state_check_us=float(np.median(t_bare)),
               eval_state_check_then_parts_us=float(np.median(t_parts)), enqueue_state_derivative_us=e_chain, enqueue_eval_state_us=e_eval)
    print(f"{name:>3s}: scenes {n_scene:4d} bodies {n_body} nv {nv:2d} items {n:4d} (in contact {contact:4d}) | dynamics alone {t_dyn:7.2f} us | "
          f"accelerations alone {t_accel:7.2f} us | state_derivative_device+check {row['state_derivative_check_us']:8.1f} us | "
          f"eval_state_device+check+download of f {row['eval_state_check_download_f_us']:8.1f} us | eval_state_device+check "
          f"{row['eval_state_check_us']:8.1f} us | ... then dynamics_device, accelerations_device {row['eval_state_check_then_parts_us']:8.1f} us | "
          f"host time inside the enqueue: state_derivative_device {e_chain:6.1f} us, eval_state_device {e_eval:6.1f} us", flush=True)
    return row


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    pfc = pfc_pkg.load()
    L = pfc._lib.lib()
    print(f"library {L.pfc_loaded_path} build_info {L.pfc_build_info():#x}", flush=True)
    rows = [run(pfc, "C1", *c1_mechanism(pfc), reps), run(pfc, "C4", *c4_mechanism(pfc), reps)]
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
