#!/usr/bin/env python3
"""Batch steps per second of an integration to a common end time, for one box-on-plane scene and for C4's 256 scenes, by two routes
on the same build, alternating:
  loop       what there was before pfc_radau_integrate: radau_step + radau_get_state per step, the rows appended on the host, until
             the slowest scene has arrived (the scenes that arrived earlier are stepped on)
  integrate  MechanismScenario.integrate_scenario_radau: pfc_radau_set_end + pfc_radau_integrate, the trajectory recorded on the
             device and read back once at the end (scenes park as they arrive)
The end time is the median t of the scenes after `--steps` steps of a calibration run, so that both routes take about that many
batch steps.  The rate is batch steps over wall time, the read-back of the trajectories included.
Writes <out-dir>/radau_integrate_rate_run<N>.json.

  python scripts/radau_integrate_rate.py [--steps 20] [--reps 3] [--run 1] [--out-dir profiles]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import radau_rate  # noqa: E402  (the scenarios of the step's own measurement)


def loop_route(m, x0, t_final):
    m.radau_set_state(x0)
    x, t = m.radau_get_state()
    data_t, data_x = [t], [x]
    t0 = time.perf_counter()
    steps = 0
    while (t < t_final).any():
        m.radau_step()
        x, t = m.radau_get_state()
        data_t.append(t); data_x.append(x)
        steps += 1
    return steps, time.perf_counter() - t0


def integrate_route(m, x0, t_final, max_steps):
    m.radau_set_state(x0)
    t0 = time.perf_counter()
    out = m.integrate_scenario_radau(t_final, max_steps=max_steps)
    dt = time.perf_counter() - t0
    return max(o[0].size for o in out) - 1, dt, [int(o[0].size) for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--run", type=int, default=1)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    res = {"steps": a.steps, "reps": a.reps}
    for name, ns, n_div, mc in (("box_on_plane_1", 1, 9, False), ("c4_256", 256, 9, True)):
        m, x0 = radau_rate.scenario(ns, n_div, mc)
        m.radau_configure(ns, [0])
        m.radau_set_state(x0)
        for _ in range(a.steps):      # calibration, and the warm-up of every shape
            m.radau_step()
        t_final = float(np.median(m.radau_get_state()[1]))
        integrate_route(m, x0, t_final, 4 * a.steps)
        r = {"n_scene": ns, "nx": 12, "t_final": t_final, "loop": [], "integrate": []}
        for _ in range(a.reps):
            steps, dt = loop_route(m, x0, t_final)
            r["loop"].append({"batch_steps": steps, "seconds": dt, "steps_per_s": steps / dt})
            steps, dt, rows = integrate_route(m, x0, t_final, 4 * a.steps)
            r["integrate"].append({"batch_steps": steps, "seconds": dt, "steps_per_s": steps / dt})
        r["rows_min_max"] = [min(rows), max(rows)]
        for k in ("loop", "integrate"):
            r[k + "_steps_per_s_median"] = float(np.median([e["steps_per_s"] for e in r[k]]))
        m.close()
        res[name] = r
        print(name, json.dumps(r), flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    path = os.path.join(a.out_dir, "radau_integrate_rate_run%d.json" % a.run)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
