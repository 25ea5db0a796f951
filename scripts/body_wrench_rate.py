"""What applied body wrenches cost per batch step.  A measurement, not a test: it claims no threshold.

configs.pencil_gripper() with its controller and program, 1 and 64 scenes, the first --steps batch steps through radau_integrate:
  cleared   no wrenches (the step as it was)
  set       radau_set_body_wrenches with one wrench on the watched body (the pencil), body frame, at an offset point, with a zero
            load: tau_out is the held tau plus zeros and dtau is zero, so the solve reads the cleared run's operands (up to the sign
            of a zero) while every launch of the wrenches is issued -- one more per Newton pass, two per first Jacobian chunk, one
            per later chunk, one per attempt for the stage times.
The two alternate, a fresh process per run, --reps repetitions each, medians of batch steps per second.  --parent ROOT also runs
`cleared` from a checkout of the parent commit (built there) in each repetition: the spread of its single runs is the yardstick
the difference between `set` and `cleared` is read against.  The end states are compared with the first cleared run's (largest
absolute difference per build): this scene's runs differ from process to process in their last bits even between two runs of one
build.

usage: python scripts/body_wrench_rate.py [--scenes 1 64] [--steps 300] [--reps 3] [--parent ROOT] [--out profiles/body_wrench_rate_run1.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(root, mode, n_scene, steps):
    """One run under the package at `root`: batch steps per second, steps done, the end state."""
    sys.path.insert(0, root)
    import numpy as np
    import pfc_pkg
    pfc = pfc_pkg.load()
    d = pfc.configs.pencil_gripper()
    m = pfc.configs.build_gripper_scenario(d, fixed_order=True)
    r, c, p = d["radau"], d["controller"], d["program"]
    m.radau_configure(n_scene, [0, 1, 2, 3], h0=r["h0"], h_max=r["h_max"], h_min=r["h_min"])
    x0 = np.tile(d["x0"], (n_scene, 1))
    x0[:, 0] += 1.0e-4 * np.arange(n_scene)
    m.radau_set_state(x0)
    m.radau_set_controller(c["act"], c["kp"], c["kd"], c["dt"], [0.0], c["seg_q"], c["seg_ff"], c["a_max"], c["t_last0"])
    m.radau_set_program(p["body"], p["grip"], p["tau_soft"], p["tau_hard"], p["prog_dt"], p["prog_q"], p["prog_slip"])
    if mode == "set":
        m.radau_set_body_wrenches([int(p["body"])], [1], [[0.01, 0.0, 0.02]], [0.0], np.zeros((1, 1, 1, 6)))
    m.radau_set_end(float("inf"), 0)
    m.radau_integrate(5)                       # warm-up: work lists, first launches
    t0 = time.perf_counter()
    done, live = m.radau_integrate(steps)
    wall = time.perf_counter() - t0
    x, t = m.radau_get_state()
    m.close()
    return dict(mode=mode, n_scene=n_scene, steps=done, live=live, wall_s=wall, steps_per_s=done / wall, t_end=[float(t.min()), float(t.max())],
                x=x.reshape(-1).tolist())


def child(root, mode, n_scene, steps):
    code = ("import sys, json; sys.path.insert(0, %r); import importlib.util as u; s = u.spec_from_file_location('rate', %r); "
            "k = u.module_from_spec(s); s.loader.exec_module(k); print('RESULT ' + json.dumps(k.run(%r, %r, %d, %d)))"
            % (root, os.path.abspath(__file__), root, mode, n_scene, steps))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="*", default=[1, 64])
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "body_wrench_rate_run1.json"))
    a = ap.parse_args()
    res = dict(steps=a.steps, reps=a.reps, runs=[], medians={})
    for n in a.scenes:
        runs = {"cleared": [], "set": [], "parent": []}
        for rep in range(a.reps):
            for mode in ("cleared", "set"):      # a fresh process per run: every run pays the same first-use costs
                runs[mode].append(child(ROOT, mode, n, a.steps))
            if a.parent:
                runs["parent"].append(child(os.path.abspath(a.parent), "cleared", n, a.steps))
            print(n, "scenes, repetition", rep, {k: round(v[-1]["steps_per_s"], 1) for k, v in runs.items() if v}, flush=True)
        ref = runs["cleared"][0]["x"]
        spread = {k: max(max(abs(a - b) for a, b in zip(r["x"], ref)) for r in v) for k, v in runs.items() if v}
        res["runs"] += [dict({key: val for key, val in r.items() if key != "x"}, build=k) for k in runs for r in runs[k]]
        res["medians"][str(n)] = dict({k: statistics.median(r["steps_per_s"] for r in v) for k, v in runs.items() if v},
                                      spread={k: [min(r["steps_per_s"] for r in v), max(r["steps_per_s"] for r in v)] for k, v in runs.items() if v},
                                      end_state_diff=spread)
        print(n, "scenes:", json.dumps(res["medians"][str(n)]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
