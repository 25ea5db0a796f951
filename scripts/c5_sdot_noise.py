"""How often the first C5 evaluation of a fresh handle misses the two sdot criteria the GPU suite applies to it: tests/test_gpu_scale.py
(_check_vs_oracle: 1e-6, 1e-3 on items with >= 2 near-null eigenvalues of K) and tests/test_sdot_sensitivity.py (50 x the oracle's own noise
on those items).  The sums of K are atomic, their order differs from launch to launch, and items 324, 802 and 1804 of the pile sit at the
bounds: 80 handles of one build, MI355X: 5 and 24 misses (profiles/pass_opts_ab.json, "c5_sdot_noise").
usage: [PFC_LIB=<library>] python scripts/c5_sdot_noise.py <label> <handles>"""
import os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np, pfc_pkg, helpers as H
import test_sdot_sensitivity as T
pfc = pfc_pkg.load()
w = pfc.configs.c5_pile()
ref = H.oracle_run(pfc, w, debug=True)
touch = [k for k, r in enumerate(ref) if r.has_K]
nn = {k: T._near_null(ref[k]) for k in touch}
bound = {}
for k in touch:
    if nn[k] >= 2:
        r, c = ref[k], w.instructions[int(w.ins_ids[k])]
        _, sens = T._ulp_sensitivity(r, c, w.s[k], n_trial=12)
        bound[k] = max(50.0 * sens * max(1.0, np.sqrt(float(r.counts[3]))), 1e-9)
n = int(sys.argv[2]); f1 = f2 = 0; worst = {}
for trial in range(n):
    m = pfc.configs.build_scenario(w)
    wr, sd, ct = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    m.close()
    b1 = b2 = False
    for k in touch:
        d = H.rel_err(sd[k], ref[k].sdot)
        if nn[k] >= 2:
            if d >= 1e-3: b1 = True; worst[("scale", k)] = max(worst.get(("scale", k), 0), d)
            if d > bound[k] or d >= 1e-3: b2 = True; worst[("sens", k)] = max(worst.get(("sens", k), 0), d / bound[k])
        else:
            if d >= 1e-6: b1 = b2 = True; worst[("regular", k)] = max(worst.get(("regular", k), 0), d)
    f1 += b1; f2 += b2
print(sys.argv[1], f"of {n} fresh handles: test_gpu_scale criterion fails {f1}, test_sdot_sensitivity criterion fails {f2};", {k: float("%.3g" % v) for k, v in worst.items()}, flush=True)
