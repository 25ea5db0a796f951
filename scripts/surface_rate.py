"""Cost of the contact surface export (pfc_contact_surface_device) next to the evaluation of the same items (pfc_eval_device) and
next to what a caller had before it: option debug, pfc_eval, then pfc_debug_tractions item by item.  Device events around `reps`
calls after warm-up; every call is followed by its pfc_check, as bench.py does.

usage: python scripts/surface_rate.py [reps]      (C3 x 256 and x 2 048 full-size poses, C5)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pfc_pkg
import torch

HBM_GBS = 8000.0      # MI355X peak HBM bandwidth, GB/s (datasheet)


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
    S = m.contact_surface(w.pose, w.twist, w.ins_ids)          # sizes the buffers
    P, T = S.poly_idx.shape[0], S.trac.shape[0]
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    ids, pose, twist, s = t(w.ins_ids, torch.int32), t(w.pose), t(w.twist), t(w.s)
    z = lambda sh, dt=torch.float64: torch.zeros(sh, dtype=dt, device=dev)
    o = dict(off=z(n + 1, torch.int64), idx=z((P, 3), torch.int32), xyz=z((P, 8, 3)), ptr=z(P + 1, torch.int64), trac=z((T, 8)),
             sm=z((n, 11)), cnt=z((n, 4), torch.int32), tot=z(2, torch.int64), w=z((n, 6)), sd=z((n, 6)))
    st = torch.cuda.current_stream().cuda_stream
    surf = lambda: settle(m, lambda: m.contact_surface_device(n, ids.data_ptr(), pose.data_ptr(), twist.data_ptr(), P, T, o["off"].data_ptr(),
                                                              o["idx"].data_ptr(), o["xyz"].data_ptr(), o["ptr"].data_ptr(), o["trac"].data_ptr(),
                                                              o["sm"].data_ptr(), o["cnt"].data_ptr(), o["tot"].data_ptr(), st))
    ev = lambda: settle(m, lambda: m.eval_device(n, ids.data_ptr(), pose.data_ptr(), twist.data_ptr(), s.data_ptr(), o["w"].data_ptr(),
                                                 o["sd"].data_ptr(), o["cnt"].data_ptr(), st))
    for _ in range(3):
        surf(); ev()
    assert int(o["tot"][1]) == T
    t_surf = timed(surf, reps)
    t_eval = timed(ev, reps)
    m.close()
    # the debug route: one evaluation with option debug, then pfc_debug_tractions item by item (each call costs ~0.1 s on a big
    # scene: beyond 32 items the per-item cost of the first 32 is extrapolated to all of them)
    md = pfc.configs.build_scenario(w, debug=True)
    md.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    n_dbg = min(n, 32)
    t_dbg_eval = timed(lambda: md.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids), 1)
    t_dbg_items = timed(lambda: [md.debug_tractions(k) for k in range(n_dbg)], 1)
    t_dbg = t_dbg_eval + t_dbg_items * n / n_dbg
    md.close()
    out_bytes = (n + 1) * 8 + P * (12 + 192 + 8) + 8 + T * 64 + n * (88 + 16) + 16
    gbs = out_bytes / (t_surf * 1e-3) / 1e9
    print(f"{name:>12s}: items {n:5d}  polygons {P:8d}  points {T:9d}  | surface {t_surf * 1e3:9.1f} us  eval {t_eval * 1e3:9.1f} us  "
          f"debug route {t_dbg * 1e3:11.1f} us{' (extrapolated from 32 items)' if n > n_dbg else ''}  (surface {t_dbg / t_surf:6.1f}x faster)  | output {out_bytes / 1e6:7.2f} MB, "
          f"{gbs:7.1f} GB/s = {100 * gbs / HBM_GBS:4.1f} % of HBM peak", flush=True)
    return t_surf, t_dbg


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    pfc = pfc_pkg.load()
    C = pfc.configs
    res = [run(pfc, "C3 x 256", C.c3_blob_tool(256), reps), run(pfc, "C3 x 2048", C.c3_blob_tool(2048), reps),
           run(pfc, "C5", C.c5_pile(), reps)]
    print("bound: the output stream is a few per cent of HBM bandwidth; the surface call is bound like the evaluation -- the clip "
          "and the quadrature, run twice (count, emit), plus the broadphase and the sort of the candidate list")
    assert all(ts < td for ts, td in res), "the surface call must be faster than the debug route"


if __name__ == "__main__":
    main()
