"""Cost of the per-item contact Jacobian L (pfc_local_jacobian_device + pfc_check) and of applying it to a further chunk
(pfc_apply_local_jacobian_device), next to one Jacobian chunk of the Dual evaluation (pfc_eval_dual_device_more + pfc_check) on the
same point.  Device events, shapes warmed up, medians over `reps` batches, in microseconds.

  build       L at the point of the first chunk (three Dual passes with unit seeds + packing)
  chunk       one further Dual(6) chunk by the Dual passes (_more)
  apply       L times Dual(6) seeds: dense seeds (every key live) and one body's seeds (the keys a real chunk has)
  apply+scat  dense apply followed by the Dual third-law scatter (pfc_scatter_generalized_dual_device, wrench partials only)
  break-even  further chunks per Jacobian from which build + k apply < k chunk: build / (chunk - apply dense)

usage: python scripts/local_jacobian_rate.py [reps]      (C5: 2 016 items, 64 bodies; C1: 4 items; C3: a batch of 128 poses)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pfc_pkg
import torch

ND = 6


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


def run(pfc, name, w, one_body, body_1, body_2, n_body, nv, reps):
    dev = torch.device("cuda:0")
    n = w.n_items
    rng = np.random.default_rng(5)
    w.s[:] = rng.standard_normal((n, 6)) * 1e-3
    m = pfc.configs.build_scenario(w)
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=dev)
    ids, pose, twist, s = t(w.ins_ids, torch.int32), t(w.pose), t(w.twist), t(w.s)
    dense = [rng.standard_normal((n, ND, 24)) * 1e-2, rng.standard_normal((n, ND, 6)) * 0.1, rng.standard_normal((n, ND, 6)) * 1e-3]
    sparse = [a * one_body[:, None, None] for a in dense]
    dense, sparse = [t(a) for a in dense], [t(a) for a in sparse]
    o_w, o_sd, o_dw, o_dsd, a_dw, a_dsd = z(n, 6), z(n, 6), z(n, ND, 6), z(n, ND, 6), z(n, ND, 6), z(n, ND, 6)
    o_ct = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    L = z(n, 12, 36)
    x = np.zeros((n, 12))
    for k in range(n):
        x[k, :9] = pfc.configs.random_rotation(rng).reshape(-1, order="F"); x[k, 9:] = rng.standard_normal(3)
    tx, tj = t(x), t(rng.standard_normal((n_body, nv, 6)))
    tb1, tb2 = t(body_1, torch.int32), t(body_2, torch.int32)
    f, df = z(1, nv), z(1, ND, nv)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(40):
        m.eval_dual_device(n, ND, ids.data_ptr(), pose.data_ptr(), twist.data_ptr(), s.data_ptr(), dense[0].data_ptr(), dense[1].data_ptr(),
                           dense[2].data_ptr(), o_w.data_ptr(), o_sd.data_ptr(), o_dw.data_ptr(), o_dsd.data_ptr(), o_ct.data_ptr(), st)
        if m.check() == 0:
            break
    else:
        raise RuntimeError("work lists kept overflowing")

    def build():
        m.local_jacobian_device(L.data_ptr(), st)
        assert m.check() == 0

    def chunk():
        m.eval_dual_device_more(ND, dense[0].data_ptr(), dense[1].data_ptr(), dense[2].data_ptr(), o_dw.data_ptr(), o_dsd.data_ptr(), st)
        assert m.check() == 0

    apply = lambda sd: (lambda: m.apply_local_jacobian_device(n, ND, L.data_ptr(), sd[0].data_ptr(), sd[1].data_ptr(), sd[2].data_ptr(),
                                                              a_dw.data_ptr(), a_dsd.data_ptr(), st))
    scat = lambda: m.scatter_generalized_dual_device(n, ND, o_w.data_ptr(), a_dw.data_ptr(), tx.data_ptr(), 0, tb1.data_ptr(),
                                                     tb2.data_ptr(), 0, 1, nv, tj.data_ptr(), 0, f.data_ptr(), df.data_ptr(), False, st)
    app_dense, app_sparse = apply(dense), apply(sparse)

    def app_scat():
        app_dense()
        scat()

    for fn in (build, chunk, app_dense, app_sparse, app_scat):
        fn()
    torch.cuda.synchronize()
    # the partials apply returns are the chunk's (a check of the measured configuration, not a test)
    chunk(); app_dense(); torch.cuda.synchronize()
    err = float((a_dw - o_dw).abs().max() / o_dw.abs().max().clamp_min(1e-300))
    t_build, t_chunk = median_us(build, reps, 3), median_us(chunk, reps, 3)
    t_dense, t_sparse, t_as = median_us(app_dense, reps, 20), median_us(app_sparse, reps, 20), median_us(app_scat, reps, 20)
    m.close()
    be = t_build / (t_chunk - t_dense) if t_chunk > t_dense else float("inf")
    print(f"{name:>3s}: items {n:5d} (seeded by one body: {int(one_body.sum()):4d}) | build {t_build:8.1f} us | chunk Dual({ND}) "
          f"{t_chunk:8.1f} us | apply dense {t_dense:6.1f} us ({100 * t_dense / t_chunk:4.1f} % of the chunk), one body {t_sparse:6.1f} us | "
          f"apply+scat {t_as:6.1f} us | break-even {be:5.2f} further chunks | max rel diff apply vs chunk {err:.1e}", flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    pfc = pfc_pkg.load()
    C = pfc.configs
    w = C.c5_pile()
    ids = np.array([[w.instructions[int(k)].id_1, w.instructions[int(k)].id_2] for k in w.ins_ids])
    b1, b2 = ids[:, 0] // 2, ids[:, 1] // 2      # meshes b{i}_tri, b{i}_tet per body
    run(pfc, "C5", w, ((b1 == 21) | (b2 == 21)).astype(np.float64), b1, b2, 64, 384, reps)
    for name, w in (("C1", C.c1_boxes()), ("C3", C.c3_blob_tool(128))):
        n = w.n_items
        one = (np.arange(n) == 0).astype(np.float64)
        run(pfc, name, w, one, np.full(n, -1), np.arange(n), n, 6 * n if n <= 64 else 6, reps)


if __name__ == "__main__":
    main()
