"""Cost of the Dual third-law scatter (pfc_scatter_generalized_dual_device) next to the value scatter
(pfc_scatter_generalized_device) and one Jacobian chunk of the Dual evaluation (pfc_eval_dual_device_more + pfc_check) on the
same scene.  Medians over `reps` batches of device-event-timed calls, in microseconds.

usage: python scripts/scatter_dual_rate.py [reps]      (C5: 2 016 items, 64 bodies, nv 384; C4: 256 scenes, nv 6; Dual(6))"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pfc_pkg
import torch

ND = 6
BATCH = 20


def median_us(fn, reps, batch=BATCH):
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


def settle(m, call):
    for _ in range(40):
        call()
        if m.check() == 0:
            return
    raise RuntimeError("work lists kept overflowing")


def run(pfc, name, w, body_1, body_2, scene, n_scene, n_body, nv, reps):
    dev = torch.device("cuda:0")
    n = w.n_items
    rng = np.random.default_rng(5)
    m = pfc.configs.build_scenario(w)
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=dev)
    ids, pose, twist, s = t(w.ins_ids, torch.int32), t(w.pose), t(w.twist), t(w.s)
    seeds = [t(rng.standard_normal((n, ND, 24)) * 1e-2), t(rng.standard_normal((n, ND, 6)) * 0.1), t(rng.standard_normal((n, ND, 6)) * 1e-3)]
    x = np.zeros((n, 12))
    for k in range(n):
        x[k, :9] = pfc.configs.random_rotation(rng).reshape(-1, order="F"); x[k, 9:] = rng.standard_normal(3)
    tx, tdx = t(x), t(rng.standard_normal((n, ND, 12)))
    tj, tdj = t(rng.standard_normal((n_body, nv, 6))), t(rng.standard_normal((n_body, ND, nv, 6)))
    tb1, tb2 = t(body_1, torch.int32), t(body_2, torch.int32)
    tsc = None if scene is None else t(scene, torch.int32)
    o_w, o_sd, o_dw, o_dsd = z(n, 6), z(n, 6), z(n, ND, 6), z(n, ND, 6)
    o_ct = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    f, df = z(n_scene, nv), z(n_scene, ND, nv)
    st = torch.cuda.current_stream().cuda_stream
    sc = 0 if tsc is None else tsc.data_ptr()
    settle(m, lambda: m.eval_dual_device(n, ND, ids.data_ptr(), pose.data_ptr(), twist.data_ptr(), s.data_ptr(), seeds[0].data_ptr(),
                                         seeds[1].data_ptr(), seeds[2].data_ptr(), o_w.data_ptr(), o_sd.data_ptr(), o_dw.data_ptr(),
                                         o_dsd.data_ptr(), o_ct.data_ptr(), st))

    def chunk():
        m.eval_dual_device_more(ND, seeds[0].data_ptr(), seeds[1].data_ptr(), seeds[2].data_ptr(), o_dw.data_ptr(), o_dsd.data_ptr(), st)
        assert m.check() == 0

    dual = lambda dx, dj: (lambda: m.scatter_generalized_dual_device(n, ND, o_w.data_ptr(), o_dw.data_ptr(), tx.data_ptr(), dx,
                                                                     tb1.data_ptr(), tb2.data_ptr(), sc, n_scene, nv, tj.data_ptr(), dj,
                                                                     f.data_ptr(), df.data_ptr(), False, st))
    full, wrench_only = dual(tdx.data_ptr(), tdj.data_ptr()), dual(0, 0)
    value = lambda: m.scatter_generalized_device(n, o_w.data_ptr(), tx.data_ptr(), tb1.data_ptr(), tb2.data_ptr(), sc, n_scene, nv,
                                                 tj.data_ptr(), f.data_ptr(), False, st)
    for fn in (full, wrench_only, value, chunk):
        fn()
    torch.cuda.synchronize()
    t_full, t_w = median_us(full, reps), median_us(wrench_only, reps)
    t_val = median_us(value, reps)
    t_chunk = median_us(chunk, reps, batch=3)
    m.close()
    print(f"{name:>3s}: items {n:5d} scenes {n_scene:4d} nv {nv:4d} Dual({ND}) | dual scatter {t_full:8.1f} us (d_x_w_r2, d_jac)  "
          f"{t_w:8.1f} us (wrench partials only) | value scatter {t_val:7.1f} us | eval_dual_device_more chunk {t_chunk:8.1f} us | "
          f"dual scatter / chunk {100 * t_full / t_chunk:5.1f} %", flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    pfc = pfc_pkg.load()
    C = pfc.configs
    w = C.c5_pile()
    ids = np.array([[w.instructions[int(k)].id_1, w.instructions[int(k)].id_2] for k in w.ins_ids])
    b1, b2 = (ids[:, 0] // 2).astype(np.int32), (ids[:, 1] // 2).astype(np.int32)      # meshes b{i}_tri, b{i}_tet per body
    run(pfc, "C5", w, b1, b2, None, 1, 64, 384, reps)
    w = C.c2_box_on_plane(256, montecarlo=True)
    n = w.n_items
    run(pfc, "C4", w, np.full(n, -1, np.int32), np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32), n, n, 6, reps)


if __name__ == "__main__":
    main()
