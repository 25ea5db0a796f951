"""Cost of the Dual forward dynamics on the device: pfc_dynamics_dual_device alone, pfc_accelerations_dual_device alone, and the chains
pfc_state_derivative_dual_device[_more] + pfc_check against what a host pays today before it can start its own Dual dynamics --
pfc_eval_dual_state_device[_more] + pfc_check + the download of f and d_f.  Shapes warmed up; medians over `reps` blocks, in
microseconds: device events for the kernels alone, a host clock (the blocks end with a synchronise) for the chains, the two routes
alternating block by block.

  dyn_dual     k_dynamics_dual alone, all three outputs (dqdot, dH, dc)
  accel_dual   k_accel_dual alone (vdot and dvdot); both also as the host's time from one launch on an idle stream to its completion
  chain        pfc_state_derivative_dual_device + pfc_check: from (q, v, s) and the seeds to [qdot; vdot; sdot] and its partials
  parent       pfc_eval_dual_state_device + pfc_check + f and d_f copied to the host (pageable memory, as NumPy gives it)
  more         pfc_state_derivative_dual_device_more + pfc_check: a later chunk at the kept point
  parent_more  pfc_eval_dual_state_device_more + pfc_check + d_f copied to the host

usage: python scripts/dynamics_dual_rate.py [reps] [json]      (C1: one scene of five bodies, nv = 24; C4: 256 scenes of a rooted ground
and a floating box, nv = 6 each; n_dir 6 and 16; json: a file the figures are also written to)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pfc_pkg
import torch

from dynamics_rate import box_inertias
from items_from_bodies_rate import median_us
from kinematics_dual_rate import host_blocks_us
from kinematics_rate import c1_mechanism, c4_mechanism


def run(pfc, name, w, mech, q, v, bind, scene, n_dir, reps):
    dev = torch.device("cuda:0")
    m = pfc.configs.build_scenario(w)
    for k, (a, b) in enumerate(bind):
        m.set_instruction_bodies(k, a, b)
    m.set_mechanism(*mech)
    m.set_inertia(box_inertias(pfc, w, mech))
    n_body, nq, nv = m.mechanism_sizes()
    n, n_scene = w.n_items, q.shape[0]
    nb = n_scene * n_body
    seeds = []
    for first in (0, nv - n_dir // 2):      # two chunks: configurations first; across the boundary between q and v
        sd = np.zeros((n_scene, n_dir, 2 * nv))
        cols = (first + np.arange(n_dir)) % (2 * nv)
        sd[:, np.arange(n_dir), cols] = 1.0
        seeds.append((np.ascontiguousarray(sd[:, :, :nv]), np.ascontiguousarray(sd[:, :, nv:])))
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    z = lambda *sh, dt=torch.float64: torch.zeros(sh, dtype=dt, device=dev)
    p = lambda a: a.data_ptr()
    P = lambda arrs: [p(a) for a in arrs]
    ids, s, d_q, d_v = t(w.ins_ids, torch.int32), t(w.s), t(q), t(v)
    dsc = t(scene, torch.int32) if scene is not None else None
    d_seeds = [(t(a), t(b)) for a, b in seeds]
    o_kin = [z(nb, 12), z(nb, 6), z(nb, nv, 6)]
    o_dkin = [z(nb, n_dir, 12), z(nb, n_dir, 6), z(nb, n_dir, nv, 6)]
    o_items = [z(n, 24), z(n, 6), z(n, 12), z(n, dt=torch.int32), z(n, dt=torch.int32)]
    o_seeds = [z(n, n_dir, 24), z(n, n_dir, 6), z(n, n_dir, 12)]
    o_res = [z(n, 6), z(n, 6), z(n, n_dir, 6), z(n, n_dir, 6), z(n, 4, dt=torch.int32)]
    o_f, o_df = z(n_scene, nv), z(n_scene, n_dir, nv)
    o_val = [z(n_scene, nq), z(n_scene, nv, nv), z(n_scene, nv), z(n_scene, nv), z(n_scene, dt=torch.int32)]
    o_par = [z(n_scene, n_dir, nq), z(n_scene, n_dir, nv, nv), z(n_scene, n_dir, nv), z(n_scene, n_dir, nv)]
    st = torch.cuda.current_stream().cuda_stream
    head = (n, n_dir, p(ids), p(dsc) if dsc is not None else 0, n_scene, p(d_q), p(d_v))

    def dyn_dual():
        m.dynamics_dual_device(n_scene, n_dir, p(d_q), p(d_v), p(d_seeds[0][0]), p(d_seeds[0][1]), p(o_kin[0]), p(o_kin[1]), p(o_dkin[0]),
                               p(o_dkin[1]), *P(o_par[:3]), st)

    def accel_dual():
        m.accelerations_dual_device(n_scene, n_dir, p(o_val[1]), p(o_val[2]), p(o_f), 0, p(o_par[1]), p(o_par[2]), p(o_df), 0, p(o_val[3]),
                                    p(o_par[3]), p(o_val[4]), st)

    def checked(enqueue, after=lambda: None):      # the first evaluations of a handle size its lists (ERR_OVERFLOW: issue the call again)
        def fn():
            for _ in range(40):
                enqueue()
                if m.check() == 0:
                    return after()
            raise RuntimeError("work lists kept overflowing")
        return fn

    more_tail = (*P(o_kin), *P(o_dkin), p(o_items[2]), p(o_items[3]), p(o_items[4]), p(o_res[0]), *P(o_seeds), p(o_res[2]), p(o_res[3]),
                 p(o_df))
    chain = checked(lambda: m.state_derivative_dual_device(
        *head, p(d_seeds[0][0]), p(d_seeds[0][1]), p(s), 0, 0, 0, *P(o_kin), *P(o_dkin), *P(o_items), *P(o_seeds), *P(o_res), p(o_f), p(o_df),
        *P(o_val), *P(o_par), st))
    parent = checked(lambda: m.eval_dual_state_device(
        *head, p(d_seeds[0][0]), p(d_seeds[0][1]), p(s), 0, *P(o_kin), *P(o_dkin), *P(o_items), *P(o_seeds), *P(o_res), p(o_f), p(o_df), st),
        lambda: (o_f.cpu(), o_df.cpu()))
    more = checked(lambda: m.state_derivative_dual_device_more(
        *head, p(d_seeds[1][0]), p(d_seeds[1][1]), 0, 0, 0, *more_tail, p(o_val[1]), p(o_val[2]), p(o_f), *P(o_par), st))
    parent_more = checked(lambda: m.eval_dual_state_device_more(*head, p(d_seeds[1][0]), p(d_seeds[1][1]), 0, *more_tail, st),
                          lambda: o_df.cpu())
    for fn in (chain, parent, dyn_dual, accel_dual, chain, more, parent_more):
        fn()
    torch.cuda.synchronize()
    chain()
    torch.cuda.synchronize()
    info = o_val[4].cpu().numpy()
    assert not info.any() and all(np.isfinite(a.cpu().numpy()).all() for a in o_par), info
    contact = int((o_res[4].cpu().numpy()[:, 3] > 0).sum())
    t_dyn, t_accel = median_us(dyn_dual, reps, 25), median_us(accel_dual, reps, 25)

    def alone_sync_us(fn):      # one launch on an idle stream until it has completed, host clock
        out = []
        for _ in range(reps * 5):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e6)
        return float(np.median(out))

    s_dyn, s_accel = alone_sync_us(dyn_dual), alone_sync_us(accel_dual)
    block = 10 if n <= 64 else 3
    t_chain, t_parent, t_more, t_pmore = [], [], [], []
    for _ in range(reps):      # alternate the two routes block by block
        t_chain.append(host_blocks_us(chain, block)); t_parent.append(host_blocks_us(parent, block))
    chain()                    # the kept point of the _more pair
    for _ in range(reps):
        t_more.append(host_blocks_us(more, block)); t_pmore.append(host_blocks_us(parent_more, block))
    m.close()
    med = lambda a: float(np.median(a))
    row = dict(config=name, n_dir=n_dir, n_scene=n_scene, n_body=n_body, nv=nv, items=n, in_contact=contact, reps=reps, block=block,
               dynamics_dual_us=float(t_dyn), accelerations_dual_us=float(t_accel), dynamics_dual_launch_to_done_us=s_dyn,
               accelerations_dual_launch_to_done_us=s_accel, state_derivative_dual_check_us=med(t_chain),
               eval_dual_state_check_download_us=med(t_parent), state_derivative_dual_more_check_us=med(t_more),
               eval_dual_state_more_check_download_us=med(t_pmore))
    print(f"{name:>3s} n_dir {n_dir:2d}: scenes {n_scene:4d} bodies {n_body} nv {nv:2d} items {n:4d} (in contact {contact:4d}) | "
          f"dynamics_dual alone {t_dyn:7.2f} us ({s_dyn:.1f} us from launch to done on an idle stream) | accelerations_dual alone "
          f"{t_accel:7.2f} us ({s_accel:.1f} us) | state_derivative_dual_device+check "
          f"{row['state_derivative_dual_check_us']:9.1f} us | eval_dual_state_device+check+download of f, d_f "
          f"{row['eval_dual_state_check_download_us']:9.1f} us | _more+check {row['state_derivative_dual_more_check_us']:9.1f} us | "
          f"eval_dual_state_device_more+check+download of d_f {row['eval_dual_state_more_check_download_us']:9.1f} us", flush=True)
    return row


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    pfc = pfc_pkg.load()
    L = pfc._lib.lib()
    print(f"library {L.pfc_loaded_path} build_info {L.pfc_build_info():#x}", flush=True)
    rows = []
    for name, mk in (("C1", c1_mechanism), ("C4", c4_mechanism)):
        for n_dir in (6, 16):
            rows.append(run(pfc, name, *mk(pfc), n_dir, reps))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
