#!/usr/bin/env python3
"""Batch steps per second of a controlled integration, for one scene and for 256, by two routes on the same build, alternating:
  device  radau_set_controller + integrate_scenario_radau: the clock and the computed-torque PD law run in k_radau_control at the
          top of every batch step; nothing but counts is read back per step
  host    integrate_scenario_radau(discrete_controller=(fn, dt)) with fn = computed_torque_pd_fn: per batch step the states come
          down, every due scene gets a host-form dynamics call and the law in Python floats, tau goes up, one radau_step
The scene is C2's box (972 tets) on the ground with the box on a prismatic z joint (NX = 2), 0.5 .. 2 mm in the ground, a 100 Hz
controller with two setpoint segments.  Both routes give the same trajectory (tests/test_gpu_radau_control.py compares bytes); the
rate is batch steps over wall time, the read-back of the trajectories included.
Writes <out-dir>/radau_control_rate_run<N>.json.

  python scripts/radau_control_rate.py [--steps 20] [--reps 3] [--run 1] [--out-dir profiles]
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
R, MASS, DT = 0.05, 0.8, 0.01


def scenario(n_scene):
    w = pfc.configs.c2_box_on_plane(1, n_div=9)
    m = pfc.configs.build_scenario(w)
    m.set_mechanism([-1], [pfc._lib.JOINT_PRISMATIC], [[1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0]], [[0.0, 0.0, 1.0]])
    m.set_instruction_bodies(0, -1, 0)
    rec = np.zeros((1, 13))
    rec[0, [0, 4, 8]] = (2.0 / 3.0) * MASS * R * R
    rec[0, 12] = MASS
    m.set_inertia(rec, (0.0, 0.0, -9.81))
    rng = np.random.default_rng(1)
    x = np.zeros((n_scene, 2))
    x[:, 0] = R - rng.uniform(0.5e-3, 2e-3, n_scene)
    x[:, 1] = 0.02 * rng.standard_normal(n_scene)
    law = dict(act=[0], kp=[400.0], kd=[40.0], a_max=[5.0],
               seg_t=np.tile([0.0, 0.05], (n_scene, 1)),
               seg_q=(R - rng.uniform(0.5e-3, 2e-3, (n_scene, 2, 1))),
               seg_ff=np.zeros((n_scene, 2, 1)))
    return m, x, law


def device_route(m, x0, law, t_final, max_steps):
    m.radau_set_state(x0)
    m.radau_set_controller(law["act"], law["kp"], law["kd"], DT, law["seg_t"], law["seg_q"], law["seg_ff"], law["a_max"], 0.0)
    t0 = time.perf_counter()
    out = m.integrate_scenario_radau(t_final, max_steps=max_steps)
    dt = time.perf_counter() - t0
    fires = m.radau_controller_state()[1]
    m.radau_clear_controller()
    return max(o[0].size for o in out) - 1, dt, int(fires.sum()), out


def host_route(m, x0, law, t_final, max_steps):
    m.radau_set_state(x0)
    fn = m.computed_torque_pd_fn(law["act"], law["kp"], law["kd"], law["seg_t"], law["seg_q"], law["seg_ff"], law["a_max"])
    t0 = time.perf_counter()
    out = m.integrate_scenario_radau(t_final, max_steps=max_steps, discrete_controller=(fn, DT, 0.0))
    dt = time.perf_counter() - t0
    fires = m.radau_host_controller_state()[1]
    m.radau_set_tau(None)
    return max(o[0].size for o in out) - 1, dt, int(fires.sum()), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--run", type=int, default=1)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    res = {"steps": a.steps, "reps": a.reps, "dt": DT}
    for name, ns in (("slider_1", 1), ("slider_256", 256)):
        m, x0, law = scenario(ns)
        m.radau_configure(ns, [0])
        m.radau_set_state(x0)
        for _ in range(a.steps):      # calibration, and the warm-up of every shape
            m.radau_step()
        t_final = float(np.median(m.radau_get_state()[1]))
        device_route(m, x0, law, t_final, 4 * a.steps)
        host_route(m, x0, law, t_final, 4 * a.steps)
        r = {"n_scene": ns, "nx": 2, "t_final": t_final, "host": [], "device": []}
        for _ in range(a.reps):
            steps, dt, fires, out_h = host_route(m, x0, law, t_final, 4 * a.steps)
            r["host"].append({"batch_steps": steps, "seconds": dt, "steps_per_s": steps / dt, "fires": fires})
            steps, dt, fires, out_d = device_route(m, x0, law, t_final, 4 * a.steps)
            r["device"].append({"batch_steps": steps, "seconds": dt, "steps_per_s": steps / dt, "fires": fires})
        r["rows_equal"] = [o[0].size for o in out_h] == [o[0].size for o in out_d]
        for k in ("host", "device"):
            r[k + "_steps_per_s_median"] = float(np.median([e["steps_per_s"] for e in r[k]]))
        m.close()
        res[name] = r
        print(name, json.dumps(r), flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    path = os.path.join(a.out_dir, "radau_control_rate_run%d.json" % a.run)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
