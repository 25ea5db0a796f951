"""Cost of forming the Dual seeds of the contact items from body states on the device (pfc_dual_seeds_from_bodies_device), of the
chains pfc_eval_dual_bodies_device[_more] + pfc_check next to pfc_eval_dual_device[_more] + pfc_check on the same items and seeds,
and of what the kernel replaces: forming the seeds with NumPy on the host and uploading them.  Device events for the device figures,
a host clock around NumPy + upload + synchronise for the host figure; shapes warmed up, medians over `reps` batches, in microseconds.

  seeds        k_dual_seeds_from_bodies alone, all three outputs
  dual         pfc_eval_dual_device + pfc_check on the items and seeds the kernels wrote
  dual_bodies  pfc_eval_dual_bodies_device + pfc_check (the two alternate batch by batch in one run)
  more         pfc_eval_dual_device_more + pfc_check at the kept point, on the seeds the kernel wrote
  more_bodies  pfc_eval_dual_bodies_device_more + pfc_check (alternating likewise)
  host         the matrix form of the derivative per item in NumPy (all directions at once), three host-to-device copies

usage: python scripts/dual_seeds_from_bodies_rate.py [reps]      (C1: 4 items; C5: 2 016 items, 64 bodies; n_dir 6 and 16).
PFC_LIB=<variant> PFC_ALLOW_DIAGNOSTIC=1 measures a variant build of the library."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pfc_pkg
import torch

from items_from_bodies_rate import c1_states, c5_states, median_us


def host_seeds(w, x, tw, dx, dtw, bind):
    """What a host without the kernel does per chunk: d_pose, d_twist, d_x_w_r2 of every item, the directions as a leading axis."""
    n, n_dir = w.n_items, dx.shape[2]
    d_pose, d_twist, d_xr = np.zeros((n, n_dir, 24)), np.zeros((n, n_dir, 6)), np.zeros((n, n_dir, 12))
    eye, z3, z6 = np.eye(3), np.zeros(3), np.zeros(6)
    zR, zt, zv = np.zeros((n_dir, 3, 3)), np.zeros((n_dir, 3)), np.zeros((n_dir, 6))
    F = lambda a: a[:9].reshape(3, 3, order="F")
    dF = lambda a: a[:, :9].reshape(n_dir, 3, 3).transpose(0, 2, 1)
    for i in range(n):
        p, q = bind[int(w.ins_ids[i])]
        R1, t1, v1, dR1, dt1, dv1 = (F(x[0, p]), x[0, p, 9:], tw[0, p], dF(dx[0, p]), dx[0, p, :, 9:], dtw[0, p]) if p >= 0 else \
            (eye, z3, z6, zR, zt, zv)
        R2, t2, v2, dR2, dt2, dv2 = (F(x[0, q]), x[0, q, 9:], tw[0, q], dF(dx[0, q]), dx[0, q, :, 9:], dtw[0, q]) if q >= 0 else \
            (eye, z3, z6, zR, zt, zv)
        R2w, dR2w = R2.T, dR2.transpose(0, 2, 1)
        t2w = -(R2w @ t2)
        dt2w = -(dR2w @ t2 + dt2 @ R2w.T)
        R21, t21 = R2w @ R1, R2w @ t1 + t2w
        dR21 = dR2w @ R1 + R2w @ dR1
        dt21 = dR2w @ t1 + dt1 @ R2w.T + dt2w
        dt12 = -(np.einsum("kji,j->ki", dR21, t21) + dt21 @ R21)
        v, dv = v2 - v1, dv2 - dv1
        ang = R2w @ v[:3]
        dang = dR2w @ v[:3] + dv[:, :3] @ R2w.T
        dlin = dR2w @ v[3:] + dv[:, 3:] @ R2w.T + np.cross(dt2w, ang) + np.cross(t2w, dang)
        d_pose[i, :, :9] = dR21.transpose(0, 2, 1).reshape(n_dir, 9); d_pose[i, :, 9:12] = dt21
        d_pose[i, :, 12:21] = dR21.reshape(n_dir, 9); d_pose[i, :, 21:] = dt12
        d_twist[i, :, :3] = dang; d_twist[i, :, 3:] = dlin
        if q >= 0:
            d_xr[i] = dx[0, q]
    return d_pose, d_twist, d_xr


def run(pfc, name, w, x, tw, bind, n_dir, reps):
    dev = torch.device("cuda:0")
    n, n_scene, n_body = w.n_items, x.shape[0], x.shape[1]
    m = pfc.configs.build_scenario(w)
    for k, (p, q) in enumerate(bind):
        m.set_instruction_bodies(k, p, q)
    rng = np.random.default_rng(11)
    hdx = rng.standard_normal((1, n_body, n_dir, 12)) * 1e-3
    hdtw = rng.standard_normal((1, n_body, n_dir, 6)) * 1e-2
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    z = lambda *sh, dt=torch.float64: torch.zeros(sh, dtype=dt, device=dev)
    ids, s, d_x, d_tw, d_dx, d_dtw = t(w.ins_ids, torch.int32), t(w.s), t(x), t(tw), t(hdx), t(hdtw)
    o_pose, o_tw, o_xr, o_b1, o_b2 = z(n, 24), z(n, 6), z(n, 12), z(n, dt=torch.int32), z(n, dt=torch.int32)
    o_dp, o_dt, o_dxr = z(n, n_dir, 24), z(n, n_dir, 6), z(n, n_dir, 12)
    o_w, o_sd, o_dw, o_dsd, o_ct = z(n, 6), z(n, 6), z(n, n_dir, 6), z(n, n_dir, 6), z(n, 4, dt=torch.int32)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda q: q.data_ptr()
    head = (n, n_dir, p(ids), 0, n_scene, n_body, p(d_x), p(d_tw), p(d_dx), p(d_dtw))
    torch.cuda.synchronize()

    def seeds():
        m.dual_seeds_from_bodies_device(*head, p(o_dp), p(o_dt), p(o_dxr), st)

    def checked(enqueue):      # the first evaluations of a handle size its lists (ERR_OVERFLOW: issue the same call again)
        def fn():
            for _ in range(40):
                enqueue()
                if m.check() == 0:
                    return
            raise RuntimeError("work lists kept overflowing")
        return fn

    dual = checked(lambda: m.eval_dual_device(n, n_dir, p(ids), p(o_pose), p(o_tw), p(s), p(o_dp), p(o_dt), 0, p(o_w), p(o_sd), p(o_dw),
                                              p(o_dsd), p(o_ct), st))
    dual_bodies = checked(lambda: m.eval_dual_bodies_device(*head, p(s), 0, p(o_pose), p(o_tw), p(o_xr), p(o_b1), p(o_b2), p(o_dp), p(o_dt),
                                                            p(o_dxr), p(o_w), p(o_sd), p(o_dw), p(o_dsd), p(o_ct), st))
    more = checked(lambda: m.eval_dual_device_more(n_dir, p(o_dp), p(o_dt), 0, p(o_dw), p(o_dsd), st))
    more_bodies = checked(lambda: m.eval_dual_bodies_device_more(*head, 0, p(o_dp), p(o_dt), p(o_dxr), p(o_dw), p(o_dsd), st))
    for fn in (dual_bodies, seeds, dual, dual_bodies, dual, dual_bodies):
        fn()
    torch.cuda.synchronize()
    # the measured configuration forms the workload's own items and the seeds of the host form (a check of the set-up, not a test)
    ref = host_seeds(w, x, tw, hdx, hdtw, bind)
    err = max(float(np.abs(a.cpu().numpy() - b).max()) for a, b in zip((o_dp, o_dt, o_dxr), ref))
    assert float(np.abs(o_pose.cpu().numpy() - w.pose).max()) < 1e-12 and err < 1e-12, err
    contact = int((o_ct.cpu().numpy()[:, 3] > 0).sum())
    t_seeds = median_us(seeds, reps, 50)
    batch = 20 if n <= 64 else 5
    t_a, t_b = [], []
    for _ in range(3):      # alternate the two, take the median of the medians
        t_a.append(median_us(dual, reps, batch)); t_b.append(median_us(dual_bodies, reps, batch))
    t_dual, t_dual_b = float(np.median(t_a)), float(np.median(t_b))
    dual()                  # the kept point of the _more pair
    more(); more_bodies()
    t_a, t_b = [], []
    for _ in range(3):
        t_a.append(median_us(more, reps, batch)); t_b.append(median_us(more_bodies, reps, batch))
    t_more, t_more_b = float(np.median(t_a)), float(np.median(t_b))
    host = []
    for _ in range(3 if n > 64 else 20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        arrs = host_seeds(w, x, tw, hdx, hdtw, bind)
        up = [torch.as_tensor(a, device=dev) for a in arrs]
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
    up_bytes = sum(a.nbytes for a in arrs)
    m.close()
    print(f"{name:>3s} n_dir {n_dir:2d}: items {n:5d} (in contact {contact:5d}) | seeds kernel {t_seeds:7.2f} us | "
          f"eval_dual_device+check {t_dual:8.1f} us | eval_dual_bodies_device+check {t_dual_b:8.1f} us (+{t_dual_b - t_dual:6.1f} us) | "
          f"_more+check {t_more:8.1f} us | bodies_more+check {t_more_b:8.1f} us (+{t_more_b - t_more:6.1f} us) | "
          f"host NumPy + upload of {up_bytes} bytes {float(np.median(host)):10.1f} us | max |seeds - host form| {err:.1e}", flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    pfc = pfc_pkg.load()
    L = pfc._lib.lib()
    print(f"library {L.pfc_loaded_path} build_info {L.pfc_build_info():#x}", flush=True)
    C = pfc.configs
    for name, states in (("C1", c1_states), ("C5", c5_states)):
        w, x, tw, bind, _ = states(C)
        for n_dir in (6, 16):
            run(pfc, name, w, x, tw, bind, n_dir, reps)


if __name__ == "__main__":
    main()
