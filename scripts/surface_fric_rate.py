"""Cost of the friction surface (pfc_contact_surface_fric_device) next to the contact surface (pfc_contact_surface_device) and the
evaluation (pfc_eval_device) of the same items.  Device events around `reps` calls after warm-up; every call is followed by its
pfc_check, as bench.py does.

usage: python scripts/surface_fric_rate.py [reps]      (C3 x 256 full-size poses, C5)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pfc_pkg
import torch


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def settle(m, call):
    for _ in range(40):
        call()
        if m.check() == 0:
            return
    raise RuntimeError("work lists kept overflowing")


def run(pfc, name, w, reps):
    dev = torch.device("cuda:0")
    n = w.n_items
    m = pfc.configs.build_scenario(w)
    F = m.contact_surface_fric(w.pose, w.twist, w.s, w.ins_ids)          # sizes the buffers
    P, T = F.surface.poly_idx.shape[0], F.fric.shape[0]
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    ids, pose, twist, s = t(w.ins_ids, torch.int32), t(w.pose), t(w.twist), t(w.s)
    z = lambda sh, dt=torch.float64: torch.zeros(sh, dtype=dt, device=dev)
    o = dict(off=z(n + 1, torch.int64), idx=z((P, 3), torch.int32), xyz=z((P, 8, 3)), ptr=z(P + 1, torch.int64), trac=z((T, 8)),
             fric=z((T, 4)), sm=z((n, 11)), fs=z((n, 20)), st=z((n, 84)), cnt=z((n, 4), torch.int32), tot=z(2, torch.int64),
             w=z((n, 6)), sd=z((n, 6)))
    p = {k: v.data_ptr() for k, v in o.items()}
    st = torch.cuda.current_stream().cuda_stream
    surf = lambda: settle(m, lambda: m.contact_surface_device(n, ids.data_ptr(), pose.data_ptr(), twist.data_ptr(), P, T, p["off"], p["idx"],
                                                              p["xyz"], p["ptr"], p["trac"], p["sm"], p["cnt"], p["tot"], st))
    fric = lambda: settle(m, lambda: m.contact_surface_fric_device(n, ids.data_ptr(), pose.data_ptr(), twist.data_ptr(), s.data_ptr(), P, T,
                                                                   p["off"], p["idx"], p["xyz"], p["ptr"], p["trac"], p["fric"], p["sm"],
                                                                   p["fs"], p["st"], p["cnt"], p["tot"], st))
    ev = lambda: settle(m, lambda: m.eval_device(n, ids.data_ptr(), pose.data_ptr(), twist.data_ptr(), s.data_ptr(), p["w"], p["sd"],
                                                 p["cnt"], st))
    for _ in range(3):
        surf(); fric(); ev()
    assert int(o["tot"][1]) == T
    t_fric = timed(fric, reps)
    t_surf = timed(surf, reps)
    t_eval = timed(ev, reps)
    m.close()
    print(f"{name:>9s}: items {n:5d}  polygons {P:8d}  points {T:9d}  | friction surface {t_fric * 1e3:9.1f} us  surface "
          f"{t_surf * 1e3:9.1f} us  eval {t_eval * 1e3:9.1f} us  | friction / surface {t_fric / t_surf:5.2f}x  friction / eval "
          f"{t_fric / t_eval:5.2f}x", flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    pfc = pfc_pkg.load()
    C = pfc.configs
    run(pfc, "C3 x 256", C.c3_blob_tool(256), reps)
    run(pfc, "C5", C.c5_pile(), reps)


if __name__ == "__main__":
    main()
