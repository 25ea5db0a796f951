#!/usr/bin/env python3
"""Steps per second of the Radau IIA step for one box-on-plane scene and for C4's 256 scenes, by two routes:
  device  MechanismScenario.radau_step (pfc_radau_step)
  host    the same algorithm driven from the host with what existed before the step: the host-form state_derivative /
          state_derivative_dual calls in the step's batch shapes, -J assembled and the three matrices inverted with NumPy, the Newton
          bookkeeping in NumPy.  It is a SIMPLER integrator than the device route and not the same trajectory: one h for the whole
          batch (from the largest error norm), no update_rule! (it stays on rule 1: one real inverse, one stage of three used),
          every scene iterates until the slowest has converged, a failed attempt retries the whole batch at 0.1 h.  The device
          route keeps h per scene and rises to rule 2 after the cooldown.  The ratio is an order of magnitude, not an A/B.
and device-event brackets around pfc_radau_factor_device (both launches) and pfc_radau_newton_device (the memset of the count word
and the launch) at NX = 18 and NX = 64 (synthetic inputs, 64 scenes, rule 2, every repetition from the same X).
Writes profiles/radau_rate_run<N>.json.

  python scripts/radau_rate.py [--steps 20] [--run 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pfc_pkg  # noqa: E402

pfc = pfc_pkg.load()
FLOATING = pfc._lib.JOINT_FLOATING_MRP


def scenario(n_scene, n_div, montecarlo):
    w = pfc.configs.c2_box_on_plane(n_scene, n_div=n_div, montecarlo=montecarlo)
    m = pfc.configs.build_scenario(w)
    m.set_mechanism([-1], [FLOATING], [[1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0]], [[0.0, 0.0, 0.0]])
    m.set_instruction_bodies(0, -1, 0)
    mass, r = 0.8, 0.05
    rec = np.zeros((1, 13))
    rec[0, [0, 4, 8]] = (2.0 / 3.0) * mass * r * r
    rec[0, 12] = mass
    m.set_inertia(rec, (0.0, 0.0, -9.81))
    rng = np.random.default_rng(1)
    x = np.zeros((n_scene, 12))
    x[:, 0:3] = 0.01 * rng.standard_normal((n_scene, 3))
    x[:, 5] = r - rng.uniform(0.5e-3, 2e-3, n_scene)
    x[:, 9:12] = 0.02 * rng.standard_normal((n_scene, 3))
    return m, x


def device_rate(m, x, steps):
    m.radau_configure(x.shape[0], [0])
    m.radau_set_state(x)
    m.radau_step()
    m.radau_set_state(x)
    t0 = time.perf_counter()
    for _ in range(steps):
        m.radau_step()
    return steps / (time.perf_counter() - t0)


def host_rate(m, x, steps, n_chunk=6):
    tb = {r: pfc.scenario.radau_table(r) for r in (1, 2)}
    ns, n = x.shape
    ids, sc1, sc3 = [0] * ns, np.arange(ns, dtype=np.int32), np.arange(3 * ns, dtype=np.int32)
    x = x.copy()
    h, rule = 1e-4, 1

    def de(X):
        qd, vd = m.state_derivative(X[:, :6], X[:, 6:12], None, ins_ids=[0] * X.shape[0], scene=sc3[:X.shape[0]])[:2]
        return np.concatenate([qd, vd], axis=1)

    def one_step(x, h, rule):
        neg_J = np.zeros((ns, n, n))
        for j0 in range(0, n, n_chunk):
            nd = min(n_chunk, n - j0)
            seeds = np.zeros((ns, nd, n))
            seeds[:, np.arange(nd), j0 + np.arange(nd)] = 1.0
            out = m.state_derivative_dual(x[:, :6], x[:, 6:12], None, seeds[:, :, :6], seeds[:, :, 6:12], None, ins_ids=ids, scene=sc1)
            if j0 == 0:
                xdot0 = np.concatenate([out[0], out[1]], axis=1)
            neg_J[:, :, j0:j0 + nd] = -np.concatenate([out[3], out[4]], axis=2).transpose(0, 2, 1)
        while True:
            t = tb[rule]
            NS = t["c"].size
            inv = [np.linalg.inv(neg_J + (t["lam"][i] / h) * np.eye(n)) for i in range(NS)]
            X = np.tile(x[None], (3, 1, 1))
            ok = False
            for k_iter in range(1, 16):
                F = de(X.reshape(3 * ns, n)).reshape(3, ns, n)
                r = [X[i] - x - h * sum(t["A"][i, j] * F[j] for j in range(NS)) for i in range(NS)]
                res = sum((ri * ri).sum(axis=1) for ri in r)
                Ew = [sum(((t["lam"][j] / h) * t["Tinv"][j, i]) * r[i] for i in range(NS)) for j in range(NS)]
                w = [np.einsum("sij,sj->si", inv[i], Ew[i]) for i in range(NS)]
                dZ = [sum(t["T"][j, i] * w[i] for i in range(NS)).real for j in range(NS)]
                if max(np.abs(d).max() for d in dZ) > 10.0 or not np.isfinite(res).all():
                    break
                for j in range(NS):
                    X[j] = X[j] - dZ[j]
                if (res < 1e-16).all():
                    ok = True
                    break
            if not ok:
                h, rule = 0.1 * h, max(rule - 1, 1)
                if h < 1e-8:
                    raise RuntimeError("time step is too small, something is wrong")
                continue
            d = (t["bhat0"] * h) * xdot0 + sum(((t["bhat"][k] - t["A"][NS - 1, k]) * h) * F[k] for k in range(NS))
            e = np.einsum("sij,sj->si", inv[0], d).real
            scl = 1e-4 + np.maximum(np.abs(X[NS - 1]), np.abs(x)) * 1e-4
            err = np.sqrt(((e / scl) ** 2).sum(axis=1) / n).max()
            fac = 0.9 * 31 / (30 + k_iter)
            h_new = min(0.01, 2 * h, fac * h * (1.0 / max(err, 1e-300)) ** (1.0 / (1 + NS)))
            return X[NS - 1].copy(), h_new, rule

    x, h, rule = one_step(x, h, rule)
    t0 = time.perf_counter()
    for _ in range(steps):
        x, h, rule = one_step(x, h, rule)
    return steps / (time.perf_counter() - t0)


def kernel_times(m, nx, n_scene=64, reps=50):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(nx)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nq = nv = (nx - 6 * (nx % 12 // 6)) // 2
    n_br = (nx - nq - nv) // 6
    lay = (n_scene, nx, nq, nv, n_br + 1, [k + 1 for k in range(n_br)])
    J = T(rng.standard_normal((n_scene, nx, nx)) * 20.0)
    h, rule = T(np.full(n_scene, 1e-4)), T(np.full(n_scene, 2, dtype=np.int32))
    lu0, lu1 = torch.zeros(n_scene * nx * nx, dtype=torch.float64, device=dev), torch.zeros(2 * n_scene * nx * nx, dtype=torch.float64, device=dev)
    perm, info = torch.zeros(2 * n_scene * nx, dtype=torch.int32, device=dev), torch.zeros(2 * n_scene, dtype=torch.int32, device=dev)
    qd, vd, sd = T(rng.standard_normal((3 * n_scene, nq))), T(rng.standard_normal((3 * n_scene, nv))), T(rng.standard_normal((3 * n_scene * (n_br + 1), 6)))
    x0 = T(rng.standard_normal((n_scene, nx)))
    X = x0.repeat(3, 1).contiguous()
    Fs = torch.zeros_like(X)
    ist0 = np.zeros((n_scene, 8), dtype=np.int32); ist0[:, 0] = 1; ist0[:, 2] = -1; ist0[:, 3] = 1
    nst0 = np.zeros((n_scene, 8)); nst0[:, 3:5] = np.inf
    ist, nst, cnt = T(ist0), T(nst0), torch.zeros(2, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()
    side = torch.cuda.Stream()      # the kernels and the events that time them go to one stream
    S = side.cuda_stream
    factor = lambda: m.radau_factor_device(n_scene, nx, p(J), p(h), p(rule), 0, p(lu0), p(lu1), p(perm), p(info), S)

    newton = lambda: m.radau_newton_device(lay, p(qd), p(vd), p(sd), p(x0), p(h), p(rule), p(lu0), p(lu1), p(perm), p(info), 1e-16, 15,
                                           p(X), p(Fs), p(nst), p(ist), p(cnt), S)
    out = {}
    for name, call in (("k_radau_factor", factor), ("k_radau_newton", newton)):
        call(); torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            ist.copy_(T(ist0)); nst.copy_(T(nst0)); X.copy_(x0.repeat(3, 1)); torch.cuda.synchronize()      # every scene iterating again, from x0
            with torch.cuda.stream(side):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        out[name + "_us_median"] = float(np.median(ts))
        out[name + "_us_min"] = float(np.min(ts))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--run", type=int, default=1)
    a = ap.parse_args()
    res = {"steps": a.steps}
    for name, ns, n_div, mc in (("box_on_plane_1", 1, 9, False), ("c4_256", 256, 9, True)):
        m, x = scenario(ns, n_div, mc)
        res[name] = {"n_scene": ns, "nx": 12, "device_steps_per_s": device_rate(m, x, a.steps)}
        m.close()
        m, x = scenario(ns, n_div, mc)
        res[name]["host_steps_per_s"] = host_rate(m, x, a.steps)
        m.close()
        print(name, res[name], flush=True)
    m, _ = scenario(1, 1, False)
    for nx in (18, 64):
        res["kernels_nx%d" % nx] = kernel_times(m, nx)
        print(nx, res["kernels_nx%d" % nx], flush=True)
    m.close()
    path = os.path.join(ROOT, "profiles", "radau_rate_run%d.json" % a.run)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
