"""Option integ_spec: a scenario without a regularized instruction integrates its kept polygons in the bristle-only forms of k_integ
(k_integ_br at two waves per SIMD, k_integ_br3 at three: integ_body<.., false>, pfc_np.h), which do not compile the regularized lane.
Nothing else differs: under fixed_order the three values must return the same BYTES; in default order the counts are the oracle's
and equal across the values, wrench and sdot within the benchmark's validation rule (bench.py, validate).  A scenario with any
regularized instruction must stay on the general kernel whatever the option says -- a regularized item sent through a bristle-only
kernel would lose its friction wrench, which the oracle comparison catches.

Option quad_const: where every instruction has quadrature rule 2, those forms and the per-corner k_fric take the rule as a compile-time
constant (k_integ_br*_q3, k_fric_q3) -- the same literals and expressions, so the same bytes under fixed_order; a scenario with a
rule-1 instruction must stay on the kernels that read the rule, which the traction-point counts show.

Small batches reach the clip-only kernels through the threshold options (fused 0, clip_min 1, clip_queue 2, bin_split -5), as in
test_gpu_binned_fill.py."""
import dataclasses

import numpy as np
import pytest

from test_gpu_binned_fill import check_oracle

pytestmark = pytest.mark.gpu

FORCE = {"fused": 0, "clip_min": 1, "clip_queue": 2, "bin_split": -5}
SPECS = (0, 1, 2)

_cache = {}


def mixed_workload(pfc):
    """Eight regularized box-on-plane scenes and eight bristle blob / tool poses in ONE scenario, items interleaved: a 64-polygon piece
    of k_integ holds runs of both models."""
    C = pfc.configs
    a, b = C.c2_box_on_plane(8, montecarlo=True, n_div=5), C.c3_blob_tool(8, seed=5, n_div_blob=6, n_div_tool=5)
    off = len(a.meshes)
    ins = list(a.instructions) + [dataclasses.replace(c, id_1=c.id_1 + off, id_2=c.id_2 + off) for c in b.instructions]
    ids = np.concatenate([a.ins_ids, b.ins_ids + len(a.instructions)]).astype(np.int32)
    order = np.arange(16).reshape(2, 8).T.reshape(-1)      # 0, 8, 1, 9, ...
    cat = lambda x, y: np.concatenate([x, y])[order]
    return C.Workload("regularized boxes beside bristle blobs", list(a.meshes) + list(b.meshes), ins, ids[order], cat(a.pose, b.pose),
                      cat(a.twist, b.twist), cat(a.s, b.s))


def mixed_rules_workload(pfc, rules):
    """32 reduced C3 poses, two bristle instructions on the same meshes with the given quadrature rules, items alternating."""
    w = pfc.configs.c3_blob_tool(32, seed=5, n_div_blob=6, n_div_tool=5)
    ins = [dataclasses.replace(w.instructions[0], n_quad_rule=r) for r in rules]
    return dataclasses.replace(w, instructions=ins, ins_ids=(np.arange(32) % 2).astype(np.int32))


def scene(pfc, name):
    """(workload, oracle results of every item or None), built once per session and left unchanged."""
    if name not in _cache:
        import helpers as H
        C = pfc.configs

        def c5_first_64():
            w = C.c5_pile()
            return dataclasses.replace(w, ins_ids=w.ins_ids[:64].copy(), pose=w.pose[:64].copy(), twist=w.twist[:64].copy(), s=w.s[:64].copy())
        make = {
            "C3 full x24": lambda: C.c3_blob_tool(24),
            "C5 first 64": c5_first_64,
            "mixed": lambda: mixed_workload(pfc),
            "C4 x16": lambda: C.c2_box_on_plane(16, montecarlo=True, n_div=5),
            "C3 x1100 two halves": lambda: C.c3_blob_tool(1100, seed=31, n_div_blob=8, n_div_tool=6),
            "rules 1 and 2": lambda: mixed_rules_workload(pfc, (2, 1)),
            "rules 2 and 2": lambda: mixed_rules_workload(pfc, (2, 2)),
        }
        w = make[name]()
        _cache[name] = (w, H.oracle_run(pfc, w, debug=True) if w.n_items <= 400 else None)
    return _cache[name]


def evaluate(pfc, w, spec, **options):
    m = pfc.configs.build_scenario(w)
    for k, v in options.items():
        m.set_option(k, v)
    if spec is not None:
        m.set_option("integ_spec", spec)
    out = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)      # (a status other than clean raises)
    parts = m.last_parts()
    m.close()
    return out, parts


def test_same_bytes_under_fixed_order(pfc):
    """24 full-size C3 poses with fixed_order on fresh handles: wrench, sdot and counts of integ_spec 0, 1 and 2 are byte-equal -- the
    specialisation changed no expression and no order of a sum."""
    w, ref = scene(pfc, "C3 full x24")
    first = (0, 0)      # k_integ_fixed + k_fric_fixed<true>, the kernels from before the options
    outs = {(sp, qc): evaluate(pfc, w, sp, fixed_order=1, quad_const=qc, **FORCE)[0] for qc in (0, 1) for sp in SPECS}
    for key, out in outs.items():
        for name, x, y in zip(("wrench", "sdot", "counts"), out, outs[first]):
            assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), (key, name, np.abs(np.asarray(x) - y).max())
    check_oracle("fixed_order integ_spec 0", outs[first], ref)


@pytest.mark.parametrize("name", ["C3 full x24", "C5 first 64"])
def test_default_order_parity(pfc, name):
    """Default order: counts bit-equal to the oracle's and among the three values, wrench 1e-9, sdot 1e-6, slivers as bench.py's validate."""
    w, ref = scene(pfc, name)
    outs = {}
    for sp in SPECS:
        outs[sp], _ = evaluate(pfc, w, sp, **FORCE)
        check_oracle(f"{name} integ_spec {sp}", outs[sp], ref)
    outs["2, rule read"], _ = evaluate(pfc, w, 2, quad_const=0, **FORCE)      # k_integ_br3 / k_fric<true> (the others: their _q3 forms)
    check_oracle(f"{name} integ_spec 2 quad_const 0", outs["2, rule read"], ref)
    for sp in list(outs)[1:]:
        assert np.array_equal(outs[sp][2], outs[0][2]), (name, sp)


def test_mixed_rules_stay_on_the_kernels_that_read_the_rule(pfc):
    """Two bristle instructions with quadrature rules 2 and 1 in one scenario, integ_spec 2 and quad_const 1: every count -- the traction
    points, counts[:, 3], among them -- equal to the oracle's, so the rule was not fixed at 2; the same poses with rule 2 throughout (the
    constant-rule kernels) count more points on the items that had rule 1."""
    w, ref = scene(pfc, "rules 1 and 2")
    out, _ = evaluate(pfc, w, 2, quad_const=1, **FORCE)
    check_oracle("rules 1 and 2", out, ref)
    w2, ref2 = scene(pfc, "rules 2 and 2")
    out2, _ = evaluate(pfc, w2, 2, quad_const=1, **FORCE)
    check_oracle("rules 2 and 2", out2, ref2)
    odd = np.arange(1, 32, 2)
    assert np.array_equal(out[2][::2], out2[2][::2]) and np.all(out[2][odd, 3] < out2[2][odd, 3])


def test_mixed_scenario_stays_on_the_general_kernel(pfc):
    """One regularized and one bristle instruction in a scenario, integ_spec 2: oracle parity on every item, the regularized ones
    (their friction wrench comes from k_integ's regularized lane) included."""
    w, ref = scene(pfc, "mixed")
    assert {c.model for c in w.instructions} == {"regularized", "bristle"}
    out, _ = evaluate(pfc, w, 2, **FORCE)
    check_oracle("mixed integ_spec 2", out, ref)
    assert all(r.counts[3] > 0 for r in ref)      # every item of both models is in contact


def test_regularized_only(pfc):
    """16 regularized box-on-plane scenes, integ_spec 2: the general kernel, oracle parity."""
    w, ref = scene(pfc, "C4 x16")
    out, _ = evaluate(pfc, w, 2, **FORCE)
    check_oracle("C4 integ_spec 2", out, ref)


def test_dual_value_pass(pfc, O):
    """One Dual(6) evaluation of 24 poses whose value pass runs the clip-only kernel and k_integ_br3 with the Dual list on (surv /
    poly_cand), against the Dual oracle at test_gpu_dual.py's tolerances."""
    from test_gpu_dual import run_case
    w = pfc.configs.c3_blob_tool(24, seed=12, n_div_blob=7, n_div_tool=5)
    run_case(pfc, O, w, 6, 41, options={"fused": 0, "clip_min": 1, "clip_queue": 2, "integ_spec": 2})


def test_two_half_evaluation_takes_the_flag_over(pfc):
    """1 100 poses with the library's own thresholds: two concurrent halves, the second on the twin handle, which must carry the
    scenario flag and the option.  A sample against the oracle, every item's counts against integ_spec 0."""
    import helpers as H
    w, _ = scene(pfc, "C3 x1100 two halves")
    sample = [0, 549, 550, 1099] + [int(k) for k in np.random.default_rng(6).integers(0, w.n_items, 12)]
    ref = H.oracle_run(pfc, w, items=sample, debug=True)
    outs = {}
    for sp in (2, 0):
        outs[sp], parts = evaluate(pfc, w, sp)
        assert parts == 2
        check_oracle(f"two halves integ_spec {sp}", outs[sp], ref, items=sample)
    assert np.array_equal(outs[2][2], outs[0][2])


def test_rejects_other_values(pfc):
    w, _ = scene(pfc, "C4 x16")
    m = pfc.configs.build_scenario(w)
    for bad in (-1, 3, 4, 64):
        with pytest.raises(pfc._lib.PFCError):
            m.set_option("integ_spec", bad)
    for bad in (-1, 2, 3):
        with pytest.raises(pfc._lib.PFCError):
            m.set_option("quad_const", bad)
    for good in SPECS:
        m.set_option("integ_spec", good)
    for good in (0, 1):
        m.set_option("quad_const", good)
    m.close()
