"""The pencil gripper example (configs.pencil_gripper: the reference's test/pencil.jl) through the device route, and the device
route against the host-callback route.  A measurement, not a test: it claims no threshold.

  1. the full example (t_final 18, max_steps 8200) for 1 and 64 scenes with radau_set_controller + radau_set_program: batch steps
     per second, steps taken, final cursors, the time of each pop, the pencil's height at t = 4 s;
  2. 1 scene over the first seconds of simulated time (--host-seconds, default 2) through both routes in the same run, alternating,
     --reps repetitions each (default 3): medians of batch steps per second.

usage: python scripts/pencil_run.py [--scenes 1 64] [--max-steps 8200] [--host-seconds 2.0] [--reps 3] [--out profiles/pencil_run_run1.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pfc_pkg

POLL = 25      # batch steps between two looks at the program's records (an instruction lasts hundreds of steps)


def setup(pfc, d, n_scene):
    m = pfc.configs.build_gripper_scenario(d)
    r = d["radau"]
    m.radau_configure(n_scene, [0, 1, 2, 3], h0=r["h0"], h_max=r["h_max"], h_min=r["h_min"])
    x0 = np.tile(d["x0"], (n_scene, 1))
    x0[:, 0] += 1.0e-4 * np.arange(n_scene)      # the scenes of a batch differ a little: the arm starts 0.1 mm higher per scene
    m.radau_set_state(x0)
    return m


def device_route(pfc, d, n_scene, t_final, max_steps, say):
    c, p = d["controller"], d["program"]
    m = setup(pfc, d, n_scene)
    m.radau_set_controller(c["act"], c["kp"], c["kd"], c["dt"], [0.0], c["seg_q"], c["seg_ff"], c["a_max"], c["t_last0"])
    m.radau_set_program(p["body"], p["grip"], p["tau_soft"], p["tau_hard"], p["prog_dt"], p["prog_q"], p["prog_slip"])
    m.radau_set_end(t_final, max_steps + 1)
    pops, seen = [[] for _ in range(n_scene)], np.zeros(n_scene, dtype=np.int32)
    steps, live, failed = 0, n_scene, None
    t0 = time.perf_counter()
    while live and steps < max_steps:
        try:
            k, live = m.radau_integrate(min(POLL, max_steps - steps))
        except pfc._lib.PFCError as e:
            failed = str(e)
            break
        steps += k
        rec = m.radau_program_state()
        for s in np.flatnonzero(rec["pops"] > seen):
            pops[s].append(float(rec["t0"][s]))      # t0 of the record is the moment of its last pop
            if rec["pops"][s] > seen[s] + 1:
                pops[s].append(None)                 # more than one pop between two looks: the earlier ones were not seen
        seen = rec["pops"].copy()
        if steps % 1000 < POLL:
            say("  %d scenes: %d steps, t = %.4f .. %.4f, cursors %s" % (n_scene, steps, m.radau_get_state()[1].min(), m.radau_get_state()[1].max(),
                                                                       np.bincount(rec["cursor"]).tolist()))
    wall = time.perf_counter() - t0
    x, t = m.radau_get_state()
    rec = m.radau_program_state()
    rows = m.radau_trajectory_rows()
    tt, xx = m.radau_trajectory(0, rows[0])
    at4 = np.flatnonzero(tt >= 4.0)
    out = dict(n_scene=n_scene, batch_steps=steps, wall_s=wall, batch_steps_per_s=steps / wall, scene_steps_per_s=steps * n_scene / wall,
               t_reached=[float(t.min()), float(t.max())], final_cursors=rec["cursor"].tolist(), pops=rec["pops"].tolist(),
               pop_times_scene0=pops[0], tau_grip=rec["tau_grip"].tolist(), arm_z_scene0=float(x[0, 0]), pencil_z_scene0_end=float(x[0, 9]),
               pencil_z_scene0_at_4s=float(xx[at4[0], 9]) if at4.size else None, failed=failed,
               step_sizes_scene0=dict(median=float(np.median(np.diff(tt))), min=float(np.diff(tt).min()), max=float(np.diff(tt).max())))
    m.close()
    return out


def one_route(pfc, d, route, t_final, max_steps):
    c, p = d["controller"], d["program"]
    m = setup(pfc, d, 1)
    t0 = time.perf_counter()
    if route == "device":
        m.radau_set_controller(c["act"], c["kp"], c["kd"], c["dt"], [0.0], c["seg_q"], c["seg_ff"], c["a_max"], c["t_last0"])
        m.radau_set_program(p["body"], p["grip"], p["tau_soft"], p["tau_hard"], p["prog_dt"], p["prog_q"], p["prog_slip"])
        out = m.integrate_scenario_radau(t_final, max_steps)
        cursor = int(m.radau_program_state()["cursor"][0])
    else:
        fn = m.gripper_program_fn(c["act"], c["kp"], c["kd"], c["seg_ff"], p["body"], p["grip"], p["tau_soft"], p["tau_hard"], p["prog_dt"],
                                  p["prog_q"], p["prog_slip"], c["a_max"])
        out = m.integrate_scenario_radau(t_final, max_steps, discrete_controller=(fn, c["dt"], c["t_last0"]))
        cursor = int(fn.records[0]["cursor"])
    wall = time.perf_counter() - t0
    steps = out[0][0].size - 1
    m.close()
    return dict(steps=steps, wall_s=wall, steps_per_s=steps / wall, t_end=float(out[0][0][-1]), cursor=cursor, x_end=out[0][1][-1].tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="*", default=[1, 64])
    ap.add_argument("--max-steps", type=int, default=8200)
    ap.add_argument("--host-seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "pencil_run_run1.json"))
    a = ap.parse_args()
    pfc = pfc_pkg.load()
    d = pfc.configs.pencil_gripper()
    say = lambda s: print(s, flush=True)
    res = dict(example="configs.pencil_gripper()", t_final=d["radau"]["t_final"], max_steps=a.max_steps, full=[], routes={})
    for n in a.scenes:
        say("full example, %d scene(s)" % n)
        res["full"].append(device_route(pfc, d, n, d["radau"]["t_final"], a.max_steps, say))
        say("  " + json.dumps(res["full"][-1]))
    runs = {"device": [], "host": []}
    for rep in range(a.reps):
        for route in ("device", "host"):
            runs[route].append(one_route(pfc, d, route, a.host_seconds, a.max_steps))
            say("%s route, repetition %d: %d steps in %.2f s" % (route, rep, runs[route][-1]["steps"], runs[route][-1]["wall_s"]))
    for route, rr in runs.items():
        if rr:
            res["routes"][route] = dict(t_final=a.host_seconds, steps=[r["steps"] for r in rr], t_end=rr[0]["t_end"], cursor=rr[0]["cursor"],
                                        steps_per_s=[r["steps_per_s"] for r in rr], median_steps_per_s=float(np.median([r["steps_per_s"] for r in rr])))
    if runs["device"] and runs["host"]:
        res["routes"]["same_end_state"] = runs["device"][0]["x_end"] == runs["host"][0]["x_end"]
        res["routes"]["device_over_host"] = res["routes"]["device"]["median_steps_per_s"] / res["routes"]["host"]["median_steps_per_s"]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    say(json.dumps(res["routes"]))


if __name__ == "__main__":
    main()
