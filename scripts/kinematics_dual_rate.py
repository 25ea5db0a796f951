"""Cost of the Dual kinematics from joint states on the device (pfc_kinematics_dual_device), of the chained calls
pfc_eval_dual_state_device[_more] + pfc_check, and of the route they replace: the partials of body states and Jacobians formed on the
host (scenario.joint_kinematics_partials, NumPy, all directions at once), three uploads, pfc_eval_dual_bodies_device[_more],
pfc_scatter_generalized_dual_device and pfc_check.  Shapes warmed up; medians over `reps` blocks, in microseconds: device events for
the kernels alone, a host clock (the blocks end with a synchronise) for the chains, the two routes alternating block by block in one run.

  kin_dual     k_kinematics_dual + k_kin_jacobian_dual alone, all three outputs
  state        pfc_eval_dual_state_device + pfc_check: (q, v) and the seeds in, f_generalized and its partials out
  parent       pfc_kinematics_device, joint_kinematics_partials on the host, three host-to-device copies, pfc_eval_dual_bodies_device,
               the Dual scatter, pfc_check
  more         pfc_eval_dual_state_device_more + pfc_check at the kept point
  parent_more  joint_kinematics_partials, three copies, pfc_eval_dual_bodies_device_more, the Dual scatter, pfc_check

usage: python scripts/kinematics_dual_rate.py [reps]      (C1: 4 items, five bodies, nv = 24; C5: 2 016 items, 64 floating bodies,
nv = 384; n_dir 6 and 16, the seeds unit directions over consecutive state variables).  PFC_LIB=<variant> PFC_ALLOW_DIAGNOSTIC=1
measures a variant build of the library."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pfc_pkg
import torch

from items_from_bodies_rate import c5_states, median_us
from kinematics_rate import EYE12, c1_mechanism, mrp_from_rotation


def c5_mechanism(pfc):
    """C5 as a mechanism: 64 floating bodies on the world, the joint state reproducing the body states c5_states draws."""
    L = pfc._lib
    w, x, tw, bind, _ = c5_states(pfc.configs)
    q, v = np.zeros((1, 6 * 64)), np.zeros((1, 6 * 64))
    for b in range(64):
        R, t = x[0, b, :9].reshape(3, 3, order="F"), x[0, b, 9:]
        q[0, 6 * b:6 * b + 3] = mrp_from_rotation(R); q[0, 6 * b + 3:6 * b + 6] = t
        v[0, 6 * b:6 * b + 3] = R.T @ tw[0, b, :3]                                         # [omega; v] in the frame after
        v[0, 6 * b + 3:6 * b + 6] = R.T @ (tw[0, b, 3:] - np.cross(t, tw[0, b, :3]))
    return w, ([-1] * 64, [L.JOINT_FLOATING_MRP] * 64, [EYE12] * 64, None), q, v, bind, None


def host_blocks_us(fn, block):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(block):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / block


def run(pfc, name, w, mech, q, v, bind, n_dir, reps):
    dev = torch.device("cuda:0")
    S = pfc.scenario
    m = pfc.configs.build_scenario(w)
    for k, (a, b) in enumerate(bind):
        m.set_instruction_bodies(k, a, b)
    m.set_mechanism(*mech)
    n_body, nq, nv = m.mechanism_sizes()
    n, n_scene = w.n_items, 1
    nb = n_scene * n_body
    seeds = []
    for first in (0, nv - n_dir // 2):      # two chunks: configurations only; across the boundary between q and v
        sd = np.zeros((1, n_dir, 2 * nv))
        sd[0, np.arange(n_dir), first + np.arange(n_dir)] = 1.0
        seeds.append((np.ascontiguousarray(sd[:, :, :nv]), np.ascontiguousarray(sd[:, :, nv:])))
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    z = lambda *sh, dt=torch.float64: torch.zeros(sh, dtype=dt, device=dev)
    p = lambda a: a.data_ptr()
    ids, s, d_q, d_v = t(w.ins_ids, torch.int32), t(w.s), t(q), t(v)
    d_seeds = [(t(a), t(b)) for a, b in seeds]
    o_kin = [z(nb, 12), z(nb, 6), z(nb, nv, 6)]
    o_dkin = [z(nb, n_dir, 12), z(nb, n_dir, 6), z(nb, n_dir, nv, 6)]
    o_items = [z(n, 24), z(n, 6), z(n, 12), z(n, dt=torch.int32), z(n, dt=torch.int32)]
    o_seeds = [z(n, n_dir, 24), z(n, n_dir, 6), z(n, n_dir, 12)]
    o_res = [z(n, 6), z(n, 6), z(n, n_dir, 6), z(n, n_dir, 6), z(n, 4, dt=torch.int32)]
    o_f, o_df = z(n_scene, nv), z(n_scene, n_dir, nv)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda arrs: [p(a) for a in arrs]
    head = (n, n_dir, p(ids), 0, n_scene)
    tab = (np.asarray(mech[0]), np.asarray(mech[1]), np.asarray(mech[2], dtype=np.float64), mech[3])

    def kin_dual():
        m.kinematics_dual_device(n_scene, n_dir, p(d_q), p(d_v), p(d_seeds[0][0]), p(d_seeds[0][1]), *P(o_dkin), st)

    def checked(enqueue):      # the first evaluations of a handle size its lists (ERR_OVERFLOW: issue the same call again)
        def fn():
            for _ in range(40):
                enqueue()
                if m.check() == 0:
                    return
            raise RuntimeError("work lists kept overflowing")
        return fn

    def scatter(dj, with_f):
        m.scatter_generalized_dual_device(n, n_dir, p(o_res[0]), p(o_res[2]), p(o_items[2]), p(o_seeds[2]), p(o_items[3]), p(o_items[4]), 0,
                                          n_scene, nv, p(o_kin[2]), dj, p(o_f) if with_f else 0, p(o_df), stream=st)

    def host_partials(c):
        dx, dtw, dj = S.joint_kinematics_partials(*tab, q[0], v[0], seeds[c][0][0], seeds[c][1][0])
        up = [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (dx, dtw, dj)]
        host_partials.keep = up
        return up

    state = checked(lambda: m.eval_dual_state_device(*head, p(d_q), p(d_v), p(d_seeds[0][0]), p(d_seeds[0][1]), p(s), 0, *P(o_kin), *P(o_dkin),
                                                     *P(o_items), *P(o_seeds), *P(o_res), p(o_f), p(o_df), st))

    def parent_enqueue():
        m.kinematics_device(n_scene, p(d_q), p(d_v), *P(o_kin), st)
        ux, utw, uj = host_partials(0)
        m.eval_dual_bodies_device(*head, n_body, p(o_kin[0]), p(o_kin[1]), p(ux), p(utw), p(s), 0, *P(o_items), *P(o_seeds), *P(o_res), st)
        scatter(p(uj), True)

    more = checked(lambda: m.eval_dual_state_device_more(*head, p(d_q), p(d_v), p(d_seeds[1][0]), p(d_seeds[1][1]), 0, *P(o_kin), *P(o_dkin),
                                                         p(o_items[2]), p(o_items[3]), p(o_items[4]), p(o_res[0]), *P(o_seeds),
                                                         p(o_res[2]), p(o_res[3]), p(o_df), st))

    def parent_more_enqueue():
        ux, utw, uj = host_partials(1)
        m.eval_dual_bodies_device_more(*head, n_body, p(o_kin[0]), p(o_kin[1]), p(ux), p(utw), 0, *P(o_seeds), p(o_res[2]), p(o_res[3]), st)
        scatter(p(uj), False)

    parent, parent_more = checked(parent_enqueue), checked(parent_more_enqueue)
    for fn in (state, kin_dual, parent, state, parent):
        fn()
    torch.cuda.synchronize()
    # the two routes compute the same thing (a check of the set-up, not a test)
    df_parent = o_df.cpu().numpy().copy()
    contact = int((o_res[4].cpu().numpy()[:, 3] > 0).sum())
    state()
    torch.cuda.synchronize()
    scale = max(np.abs(df_parent).max(), 1e-300)
    err = float(np.abs(o_df.cpu().numpy() - df_parent).max() / scale)
    more(); parent_more(); more()
    torch.cuda.synchronize()
    assert err < 1e-6 and scale > 0, (err, scale)
    t_kin = median_us(kin_dual, reps, 50)
    block = 20 if n <= 64 else 3
    t_state, t_parent, t_more, t_pmore = [], [], [], []
    for _ in range(reps):      # alternate the two routes block by block
        t_state.append(host_blocks_us(state, block)); t_parent.append(host_blocks_us(parent, block))
    state()                    # the kept point of the _more pair
    for _ in range(reps):
        t_more.append(host_blocks_us(more, block)); t_pmore.append(host_blocks_us(parent_more, block))
    up_bytes = 8 * nb * n_dir * (18 + 6 * nv)
    m.close()
    med = lambda a: float(np.median(a))
    print(f"{name:>3s} n_dir {n_dir:2d}: bodies {n_body:2d} nv {nv:3d} items {n:4d} (in contact {contact:4d}) | Dual kinematics alone {t_kin:7.2f} us | "
          f"eval_dual_state_device+check {med(t_state):9.1f} us | parent route (upload of {up_bytes} bytes) {med(t_parent):10.1f} us | "
          f"_more+check {med(t_more):9.1f} us | parent _more route {med(t_pmore):10.1f} us | d_f relative to the parent route's {err:.1e}",
          flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    pfc = pfc_pkg.load()
    L = pfc._lib.lib()
    print(f"library {L.pfc_loaded_path} build_info {L.pfc_build_info():#x}", flush=True)
    for name, mk in (("C1", c1_mechanism), ("C5", c5_mechanism)):
        w, mech, q, v, bind, _ = mk(pfc)
        for n_dir in (6, 16):
            run(pfc, name, w, mech, q, v, bind, n_dir, reps)


if __name__ == "__main__":
    main()
