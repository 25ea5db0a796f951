"""Cost of forming the contact items from body states on the device (pfc_items_from_bodies_device), of the chain
pfc_eval_bodies_device + pfc_check next to pfc_eval_device + pfc_check on the same items, and of what they replace: the host loop
over scenario.relative_pose / relative_twist plus the upload of its arrays.  Device events for the device figures, a host clock
around loop + upload + synchronise for the host figure; shapes warmed up, medians over `reps` batches, in microseconds.

  items   k_items_from_bodies alone, all five outputs
  eval    pfc_eval_device + pfc_check on the items the kernel wrote
  bodies  pfc_eval_bodies_device + pfc_check (the two alternate batch by batch in one run)
  host    relative_pose / relative_twist per item, x_rw_r2 and body ids gathered, five host-to-device copies

usage: python scripts/items_from_bodies_rate.py [reps]      (C1: 4 items; C5: 2 016 items, 64 bodies; C3: 8 192 poses, the
flagship batch of bench.py).  PFC_LIB=<variant> PFC_ALLOW_DIAGNOSTIC=1 measures a variant build of the library."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pfc_pkg
import torch


def median_us(fn, reps, batch):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / batch)
    return float(np.median(out))


def pose12(R, t):
    return np.concatenate([np.asarray(R).reshape(-1, order="F"), t])


def c1_states(C):
    r, pen = 0.05, 0.001
    z = [0.0, r - pen, 3 * r - 2 * pen, 5 * r - 3 * pen, 7 * r - 4 * pen]
    x = np.array([[pose12(np.eye(3) if b == 0 else C.rot_z(0.1 * b), np.array([0, 0, z[b]])) for b in range(5)]])
    tw = np.zeros((1, 5, 6)); tw[0, :, 2] = np.arange(5.0)
    w = C.c1_boxes()
    return w, x, tw, [(c.id_1, c.id_2) for c in w.instructions], None


def c5_states(C):
    """The 64 body states configs.c5_pile() draws (the same generator, the same order of draws)."""
    w = C.c5_pile()
    g = C._rng(20260102, 0)
    n_side, r, overlap = 4, 0.05, 0.02
    pitch = 2 * r * (1 - overlap)
    x, tw = np.zeros((1, 64, 12)), np.zeros((1, 64, 6))
    for b in range(64):
        ix, iy, iz = b % n_side, (b // n_side) % n_side, b // (n_side * n_side)
        t = np.array([ix, iy, iz]) * pitch + g.uniform(-0.002, 0.002, size=3)
        R = C.rot_z(g.uniform(-0.05, 0.05)) @ C.rot_y(g.uniform(-0.05, 0.05)) @ C.rot_x(g.uniform(-0.05, 0.05))
        x[0, b] = pose12(R, t)
        tw[0, b] = np.concatenate([g.uniform(-1, 1, size=3), g.uniform(-0.1, 0.1, size=3)])
    return w, x, tw, [(c.id_1 // 2, c.id_2 // 2) for c in w.instructions], None      # meshes b{i}_tri, b{i}_tet per body


def c3_states(C, n):
    """One scene per pose: the tool is its one body, the blob is the world (configs.c3_blob_tool puts it at the identity)."""
    w = C.c3_blob_tool(n)
    x = np.ascontiguousarray(w.pose[:, None, :12])      # x_r2_r1 = x_rw_r1
    tw = np.ascontiguousarray(-w.twist[:, None, :])     # twist_r2_r1_r2 = -twist_w_r1
    return w, x, tw, [(0, -1)], np.arange(n, dtype=np.int32)


def host_items(S, w, x, tw, bind, scene):
    """What a host without the kernel does per step: the loop of configs.py over relative_pose / relative_twist."""
    n, n_body = w.n_items, x.shape[1]
    pose, twist, xr = np.zeros((n, 24)), np.zeros((n, 6)), np.zeros((n, 12))
    b1, b2 = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    eye, zero3, zero6 = np.eye(3), np.zeros(3), np.zeros(6)
    for i in range(n):
        p, q = bind[int(w.ins_ids[i])]
        sc = int(scene[i]) if scene is not None else 0
        R1, t1, v1 = (x[sc, p, :9].reshape(3, 3, order="F"), x[sc, p, 9:], tw[sc, p]) if p >= 0 else (eye, zero3, zero6)
        R2, t2, v2 = (x[sc, q, :9].reshape(3, 3, order="F"), x[sc, q, 9:], tw[sc, q]) if q >= 0 else (eye, zero3, zero6)
        pose[i] = S.relative_pose(R1, t1, R2, t2)
        twist[i] = S.relative_twist(R2, t2, v1, v2)
        xr[i, :9] = R2.reshape(-1, order="F"); xr[i, 9:] = t2
        off = sc * n_body if scene is not None else 0
        b1[i] = p + off if p >= 0 else -1; b2[i] = q + off if q >= 0 else -1
    return pose, twist, xr, b1, b2


def run(pfc, name, w, x, tw, bind, scene, reps):
    dev = torch.device("cuda:0")
    n, n_scene, n_body = w.n_items, x.shape[0], x.shape[1]
    m = pfc.configs.build_scenario(w)
    for k, (p, q) in enumerate(bind):
        m.set_instruction_bodies(k, p, q)
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    z = lambda *sh, dt=torch.float64: torch.zeros(sh, dtype=dt, device=dev)
    ids, s, dx, dtw = t(w.ins_ids, torch.int32), t(w.s), t(x), t(tw)
    dsc = t(scene, torch.int32) if scene is not None else None
    sc_p = dsc.data_ptr() if scene is not None else 0
    o_pose, o_tw, o_xr = z(n, 24), z(n, 6), z(n, 12)
    o_b1, o_b2 = z(n, dt=torch.int32), z(n, dt=torch.int32)
    o_w, o_sd, o_ct = z(n, 6), z(n, 6), z(n, 4, dt=torch.int32)
    st = torch.cuda.current_stream().cuda_stream
    items_args = (n, ids.data_ptr(), sc_p, n_scene, n_body, dx.data_ptr(), dtw.data_ptr())
    item_outs = (o_pose.data_ptr(), o_tw.data_ptr(), o_xr.data_ptr(), o_b1.data_ptr(), o_b2.data_ptr())
    eval_outs = (o_w.data_ptr(), o_sd.data_ptr(), o_ct.data_ptr())

    def items():
        m.items_from_bodies_device(*items_args, *item_outs, st)

    def checked(enqueue):      # the first evaluations of a handle size its lists (ERR_OVERFLOW: issue the same call again)
        def fn():
            for _ in range(40):
                enqueue()
                if m.check() == 0:
                    return
            raise RuntimeError("work lists kept overflowing")
        return fn

    ev = checked(lambda: m.eval_device(n, ids.data_ptr(), o_pose.data_ptr(), o_tw.data_ptr(), s.data_ptr(), *eval_outs, st))
    bodies = checked(lambda: m.eval_bodies_device(*items_args, s.data_ptr(), *item_outs, *eval_outs, st))
    for fn in (bodies, items, ev, bodies, ev, bodies):
        fn()
    torch.cuda.synchronize()
    # the measured configuration forms the workload's own items (a check of the set-up, not a test)
    err = float(np.abs(o_pose.cpu().numpy() - w.pose).max()), float(np.abs(o_tw.cpu().numpy() - w.twist).max())
    assert max(err) < 1e-12, err
    contact = int((o_ct.cpu().numpy()[:, 3] > 0).sum())
    t_items = median_us(items, reps, 50)
    batch = 20 if n <= 64 else 5
    t_ev, t_bod = [], []
    for _ in range(3):      # alternate the two, take the median of the medians
        t_ev.append(median_us(ev, reps, batch)); t_bod.append(median_us(bodies, reps, batch))
    t_ev, t_bod = float(np.median(t_ev)), float(np.median(t_bod))
    host = []
    for _ in range(3 if n > 64 else 20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        arrs = host_items(pfc.scenario, w, x, tw, bind, scene)
        up = [torch.as_tensor(a, device=dev) for a in arrs]
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
    up_bytes = sum(a.nbytes for a in arrs)
    m.close()
    print(f"{name:>3s}: items {n:5d} (in contact {contact:5d}) | items kernel {t_items:7.2f} us | eval_device+check {t_ev:8.1f} us | "
          f"eval_bodies_device+check {t_bod:8.1f} us (+{t_bod - t_ev:6.1f} us) | host loop + upload of {up_bytes} bytes "
          f"{float(np.median(host)):10.1f} us | max |pose - workload| {err[0]:.1e}", flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    pfc = pfc_pkg.load()
    L = pfc._lib.lib()
    print(f"library {L.pfc_loaded_path} build_info {L.pfc_build_info():#x}", flush=True)
    C = pfc.configs
    run(pfc, "C1", *c1_states(C), reps)
    run(pfc, "C5", *c5_states(C), reps)
    run(pfc, "C3", *c3_states(C, 8192), reps)


if __name__ == "__main__":
    main()
