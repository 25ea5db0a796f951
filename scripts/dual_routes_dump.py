"""Every output array of a fixed list of host-pointer calls, written to an .npz: the sequence of tests/test_gpu_dual.py::
test_host_dual_routes (helpers.dual_route_steps: all five routes of pfc_eval_dual and their reuse, with and without ins_ids and s)
and pfc_eval at 1, 513 and 4097 items (just above the 512- and 4096-item in-place limits).  For comparing two builds bit by bit:
    python scripts/dual_routes_dump.py a.npz            (PFC_LIB selects another build of the library)
    python scripts/dual_routes_dump.py --compare parent_1.npz parent_2.npz branch.npz [out.json]
The comparison sorts every array element into "exact" (the two parent runs agree in bytes; the branch must too) and "noisy" (the
parent runs differ, atomic order; the branch may be as far from a parent run as they are from each other: counted against the
nearer run, noisy_exceed, which decides, and against the farther one, noisy_exceed_farther, for the record)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def dump(path):
    import pfc_pkg, helpers as H
    pfc = pfc_pkg.load()
    out, routes = {}, {}
    for scene, (w, k) in H.dual_route_scenes(pfc).items():
        seeds = {name: H.dual_route_seeds(w, k, nd, 100 + j) for j, (name, nd) in enumerate((("A", 6), ("B", 6), ("C", 2), ("D", 2)))}
        m = pfc.configs.build_scenario(w)
        variants = [(True, True), (False, True)] + ([(True, False), (False, False)] if scene == "boxes" else [])
        for ids_given, s_given in variants:
            for label, n, name, got, r in H.dual_route_steps(m, w, seeds, ids_given, s_given):
                key = f"{scene}/ids{int(ids_given)}s{int(s_given)}/{label}"
                routes[key] = r
                for nm, a in zip(("wrench", "sdot", "d_wrench", "d_sdot", "counts"), got):
                    out[f"{key}/{nm}"] = np.array(a)
        m.close()
    for n in (1, 513, 4097):
        w = pfc.configs.c2_box_on_plane(n, montecarlo=True)
        m = pfc.configs.build_scenario(w)
        for rep in range(2):
            got = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
            for nm, a in zip(("wrench", "sdot", "counts"), got):
                out[f"eval{n}/call{rep}/{nm}"] = np.array(a)
        m.close()
    np.savez(path, **out)
    print("wrote", len(out), "arrays;", "routes", json.dumps(routes))


def compare(p1, p2, br, out_json=None):
    a, b, c = np.load(p1), np.load(p2), np.load(br)
    assert sorted(a.files) == sorted(b.files) == sorted(c.files)
    res = {"arrays": len(a.files), "exact_elements": 0, "exact_mismatch": 0, "noisy_elements": 0, "noisy_exceed": 0, "noisy_exceed_farther": 0,
           "per_array": {}}
    for f in sorted(a.files):
        x, y, z = a[f], b[f], c[f]
        assert x.shape == y.shape == z.shape and x.dtype == y.dtype == z.dtype, f
        bits = lambda v: np.ascontiguousarray(v).view(np.int64 if v.dtype.itemsize == 8 else np.int32)
        same = bits(x) == bits(y)
        bad = int((same & (bits(z) != bits(x))).sum())
        noisy = ~same
        exceed = farther = 0
        if noisy.any():
            xf, yf, zf = x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)
            exceed = int((noisy & (np.minimum(np.abs(zf - xf), np.abs(zf - yf)) > np.abs(xf - yf))).sum())
            farther = int((noisy & (np.maximum(np.abs(zf - xf), np.abs(zf - yf)) > np.abs(xf - yf))).sum())
        res["exact_elements"] += int(same.sum()); res["exact_mismatch"] += bad
        res["noisy_elements"] += int(noisy.sum()); res["noisy_exceed"] += exceed; res["noisy_exceed_farther"] += farther
        if bad or noisy.any():
            res["per_array"][f] = {"exact_mismatch": bad, "noisy": int(noisy.sum()), "noisy_exceed": exceed, "noisy_exceed_farther": farther}
    res["pass"] = res["exact_mismatch"] == 0 and res["noisy_exceed"] == 0
    print(json.dumps({k: v for k, v in res.items() if k != "per_array"}))
    if out_json:
        with open(out_json, "w") as fh:
            json.dump(res, fh, indent=1)
    return res["pass"]


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(0 if compare(*sys.argv[2:]) else 1)
    dump(sys.argv[1])
