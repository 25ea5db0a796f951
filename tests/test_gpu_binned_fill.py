"""Option bin_split: k_clip_queue fills a chunk's slot range from both ends by vertex count and k_integ / k_fric walk it piece by
piece (kept_slot, pfc_np.h).  The fill changes WHERE a kept polygon sits and therefore the order of the per-item sums and the
reference point of a run's moments, nothing else: every count column must be equal to the oracle's and equal across the settings,
wrench and sdot stay within the benchmark's validation rule (bench.py, validate), and the paths the option does not cover
(fixed_order, Dual evaluations, tet-tet scenes) give what they give with the option off.

Small batches reach the clip-only kernels through the threshold options (fused 0, clip_min 1, clip_queue 2), as in test_gpu_scale.py.
A launch of fewer than 2^20 candidates has 64- to 256-candidate chunks (np_chunk); a positive bin_split leaves such a launch dense
(np_bin_split, pfc_np.h), so every small scene runs with 4, 5 and 0 AND with -4 and -5, the form that bins at every chunk size --
there the two regions of a chunk mostly end in one shared 64-slot block.  The 512-candidate chunks of the benchmark's step need 2^20
candidates, which the two `big chunks` cases bring with 4, 5 and 0 (their oracle check is on a sample, every other item is compared
with the dense fill)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORCE = {"fused": 0, "clip_min": 1, "clip_queue": 2}      # the clip-only kernel k_clip_queue + k_integ + k_fric at any launch size
SPLITS = (4, 5, 0)
SMALL = (4, 5, -4, -5, 0)      # launches below 2^20 candidates: the positive values leave them dense, the negative ones bin them

_cache = {}


def scene(pfc, name):
    """(workload, oracle results of every item or None), built once per session."""
    if name not in _cache:
        import helpers as H
        C = pfc.configs
        make = {
            "C3 full x48": lambda: C.c3_blob_tool(48),
            "C3 reduced x32": lambda: C.c3_blob_tool(32, seed=5, n_div_blob=4, n_div_tool=3),
            "C5 pile n_side 3": lambda: C.c5_pile(n_side=3),
            "C4 box on plane": lambda: C.c2_box_on_plane(48, montecarlo=True, n_div=5),
            "C3 full x640": lambda: C.c3_blob_tool(640, seed=17),
            "C3 reduced x6400": lambda: C.c3_blob_tool(6400, seed=23, n_div_blob=6, n_div_tool=5),
            "C3 x1300 two halves": lambda: C.c3_blob_tool(1300, seed=31, n_div_blob=7, n_div_tool=5),
            "C3 x40 Dual": lambda: C.c3_blob_tool(40, n_div_blob=8, n_div_tool=6),
            "tet-tet": lambda: C.vol_vol(8, model="bristle"),
        }
        w = make[name]()
        ref = H.oracle_run(pfc, w, debug=True) if w.n_items <= 400 else None
        _cache[name] = (w, ref)
    return _cache[name]


def handle(pfc, w, bin_split, **options):
    m = pfc.configs.build_scenario(w)
    for k, v in options.items():
        m.set_option(k, v)
    if bin_split is not None:
        m.set_option("bin_split", bin_split)
    return m


def evaluate(pfc, w, bin_split, **options):
    m = handle(pfc, w, bin_split, **options)
    out = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)      # (a status other than clean raises)
    info = (m.stats(), m.last_parts())
    m.close()
    return out, info


def check_item(label, k, wrench, sdot, counts, r):
    """bench.py's validate rule for one item against its oracle result r: counts bit-equal, wrench 1e-9, sdot 1e-6; an item whose K̄ has
    a (near-)null eigenvalue: both 1e-6; two or more: sdot 1e-3."""
    assert np.array_equal(counts, r.counts), (label, k, counts, r.counts)
    n_null = 0
    if r.has_K:
        Kb = np.diag(r.Sinv) @ r.K @ np.diag(r.Sinv)
        ev = np.linalg.eigvalsh((Kb + Kb.T) / 2)
        n_null = int(np.sum(ev < 1e-12 * ev[-1]))
    worst = {}
    for name, a, b, tol in (("wrench", wrench, r.wrench, 1e-9), ("sdot", sdot, r.sdot, 1e-6)):
        nb = float(np.linalg.norm(b))
        if nb == 0.0:
            assert float(np.linalg.norm(a)) == 0.0, (label, k, name)
            continue
        if n_null >= 1:
            tol = 1e-6
        if n_null >= 2 and name == "sdot":
            tol = 1e-3
        err = float(np.linalg.norm(np.asarray(a) - b) / nb)
        worst[(name, min(n_null, 2))] = err
        assert err < tol, (label, k, name, err, tol, n_null)
    return worst


def check_oracle(label, out, ref, items=None):
    worst = {}
    for j, k in enumerate(range(len(ref)) if items is None else items):
        for key, v in check_item(label, k, out[0][k], out[1][k], out[2][k], ref[j]).items():
            worst[key] = max(worst.get(key, 0.0), v)
    print(f"{label}: " + ", ".join(f"{n}/{c} {v:.2e}" for (n, c), v in sorted(worst.items())))


def check_settings(pfc, name, splits=SMALL, **options):
    """Every setting against the oracle, counts equal across the settings."""
    w, ref = scene(pfc, name)
    outs = {}
    for b in splits:
        outs[b], _ = evaluate(pfc, w, b, **options)
        check_oracle(f"{name} bin_split {b}", outs[b], ref)
    first = outs[splits[0]]
    for b in splits[1:]:
        assert np.array_equal(outs[b][2], first[2]), (name, b)
    return w, outs


def traction_rows(m, item):
    """The traction points of an item as a sorted list of byte rows: a set of bit patterns, whatever order the device appended them in."""
    t = np.ascontiguousarray(m.debug_tractions(item))
    return sorted(t[i].tobytes() for i in range(t.shape[0]))


def test_parity_on_full_size_poses(pfc):
    """48 full-size C3 poses with bin_split 4, 5, -4, -5 and 0: counts equal to the oracle's and across the settings, wrench and sdot within
    the benchmark's rule; the traction points pfc_debug_tractions hands out for three of the items are the same set of bits under
    every setting and as many as the binned passes counted."""
    w, outs = check_settings(pfc, "C3 full x48", **FORCE)
    rows = {}
    for b in SMALL:
        m = handle(pfc, w, b, **FORCE)
        m.set_option("debug", 1)
        m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
        rows[b] = [traction_rows(m, k) for k in (0, 17, 47)]
        m.close()
    for b in SMALL:
        assert rows[b] == rows[0], b
        for j, k in enumerate((0, 17, 47)):
            assert len(rows[b][j]) == outs[b][2][k, 3], (b, k)


@pytest.mark.parametrize("name", ["C3 reduced x32", "C5 pile n_side 3"])
def test_boundary_chunks(pfc, name):
    """Items of 70 to 90 candidates (a reduced C3 pair) and the pile of 27 boxes (351 pairs, from none to thousands of candidates
    each): a chunk holds several items, and runs of several items in both of its regions."""
    check_settings(pfc, name, **FORCE)


def test_one_class_empty(pfc):
    """Regularized boxes on a plane (k_integ's lane_reg path; the plane cuts a tet in a triangle or a quadrilateral, so bin_split 5 leaves
    the back region of a chunk empty wherever the ground's diagonal does not cut the polygon further), and bin_split 3 on C3, which leaves the front region empty."""
    check_settings(pfc, "C4 box on plane", splits=(5, -5, 4, -4, 0), **FORCE)
    check_settings(pfc, "C3 full x48", splits=(3, -3, 0), **FORCE)
    check_settings(pfc, "C3 reduced x32", splits=(-3, -9, 0), **FORCE)


@pytest.mark.parametrize("name", ["C3 full x640", "C3 reduced x6400"])
def test_big_chunks(pfc, name):
    """More than 2^20 candidates in one launch: the 512-candidate chunks of the benchmark's step, with one item over several chunks
    (full-size pair) and several items per chunk (reduced pair).  Counts equal across the settings for every item and every wrench
    within 1e-6 of the dense fill's, a sample of the items against the oracle under every setting."""
    import helpers as H
    w, _ = scene(pfc, name)
    sample = [0, 1, w.n_items // 2, w.n_items - 1] + [int(k) for k in np.random.default_rng(3).integers(0, w.n_items, 20)]
    ref = H.oracle_run(pfc, w, items=sample, debug=True)
    outs = {}
    for b in SPLITS:
        outs[b], (stats, parts) = evaluate(pfc, w, b, split_min=0, **FORCE)
        assert stats["candidates"] >= 1 << 20 and parts == 1, (name, stats["candidates"], parts)
        check_oracle(f"{name} bin_split {b}", outs[b], ref, items=sample)
    for b in SPLITS[:2]:
        assert np.array_equal(outs[b][2], outs[0][2]), (name, b)
        # (items outside the sample have no oracle result to class them by: the rule's bound for an item with a null direction)
        nb = np.linalg.norm(outs[0][0], axis=1)
        assert np.all(np.linalg.norm(outs[b][0] - outs[0][0], axis=1) <= 1e-6 * nb), (name, b)


def test_two_half_evaluation_takes_the_option_over(pfc):
    """A batch above split_min with the library's own thresholds: two concurrent halves, the second on the twin handle (256-candidate
    chunks: -5 bins both halves)."""
    import helpers as H
    w, _ = scene(pfc, "C3 x1300 two halves")
    sample = [0, 649, 650, 1299] + [int(k) for k in np.random.default_rng(4).integers(0, w.n_items, 12)]
    ref = H.oracle_run(pfc, w, items=sample, debug=True)
    outs = {}
    for b in (None, -5, 0):
        outs[b], (_, parts) = evaluate(pfc, w, b)
        assert parts == 2
        check_oracle(f"two halves bin_split {b}", outs[b], ref, items=sample)
    assert np.array_equal(outs[None][2], outs[0][2]) and np.array_equal(outs[-5][2], outs[0][2])


def test_holes_first_evaluation_on_poisoned_lists(pfc):
    """The first evaluation of a fresh handle with option poison (work lists and polygon keys filled with entries that must never be
    followed; the lists grow from their initial sizes and the evaluation is re-issued): clean status, the oracle's results."""
    for name in ("C3 full x48", "C5 pile n_side 3"):
        w, ref = scene(pfc, name)
        for b in (-4, -5, 5):
            out, _ = evaluate(pfc, w, b, poison=1, **FORCE)
            check_oracle(f"{name} poisoned bin_split {b}", out, ref)


def test_rejects_other_values(pfc):
    w, _ = scene(pfc, "tet-tet")
    m = pfc.configs.build_scenario(w)
    for bad in (1, 2, 10, -1, -2, -10):
        with pytest.raises(pfc._lib.PFCError):
            m.set_option("bin_split", bad)
    m.close()


def test_untouched_fixed_order(pfc):
    """fixed_order keeps the dense fill: with bin_split at its default, at -5 and at 0 the same handle returns the same bits."""
    w, ref = scene(pfc, "C3 reduced x32")
    m = handle(pfc, w, None, fixed_order=1)
    a = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    for other in (-5, 0):
        m.set_option("bin_split", other)
        b = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), other
    m.close()
    check_oracle("fixed_order", a, ref)


def test_untouched_dual_with_a_further_chunk(pfc):
    """A Dual(6) evaluation and a further chunk of six directions on its value pass (the Dual list on: dense fill), bin_split at its
    default and -5 against 0 on the same handle: values under the module's checks, partials equal to reduction-order accuracy."""
    import torch
    w, ref = scene(pfc, "C3 x40 Dual")
    n = w.n_items
    rng = np.random.default_rng(37)
    dev = torch.device("cuda", 0)
    T = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    t_in = [T(w.ins_ids, torch.int32), T(w.pose), T(w.twist), T(w.s)]
    seeds = [[T(rng.standard_normal((n, 6, 24)) * 1e-2), T(rng.standard_normal((n, 6, 6)) * 0.1), T(rng.standard_normal((n, 6, 6)) * 1e-3)]
             for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    m = handle(pfc, w, None, **FORCE)
    got = {}
    for b in (None, -5, 0):
        if b is not None:
            m.set_option("bin_split", b)
        o_w, o_sd = torch.zeros((n, 6), dtype=torch.float64, device=dev), torch.zeros((n, 6), dtype=torch.float64, device=dev)
        o_ct = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        d = [torch.zeros((n, 6, 6), dtype=torch.float64, device=dev) for _ in range(4)]
        for _ in range(40):      # (a fresh handle's lists grow: re-issued until clean)
            m.eval_dual_device(n, 6, *[x.data_ptr() for x in t_in], *[x.data_ptr() for x in seeds[0]], o_w.data_ptr(), o_sd.data_ptr(),
                               d[0].data_ptr(), d[1].data_ptr(), o_ct.data_ptr(), stream)
            if m.check() == 0:
                break
        m.eval_dual_device_more(6, *[x.data_ptr() for x in seeds[1]], d[2].data_ptr(), d[3].data_ptr(), stream)
        assert m.check() == 0
        got[b] = [x.cpu().numpy() for x in (o_w, o_sd, o_ct, *d)]
        check_oracle(f"Dual values bin_split {b}", got[b], ref)
    m.close()
    for b in (None, -5):
        assert np.array_equal(got[b][2], got[0][2])
        for k, tol in ((3, 1e-9), (4, 1e-6), (5, 1e-9), (6, 1e-6)):      # (the bounds of test_gpu_dual.py's further-chunk test)
            np.testing.assert_allclose(got[b][k], got[0][k], rtol=tol, atol=tol * np.abs(got[0][k]).max())


def test_untouched_tet_tet(pfc):
    """A scene with tet-tet instructions clips in k_narrow<true, 2>, dense fill: default and -5 against 0 on the same handle."""
    w, ref = scene(pfc, "tet-tet")
    m = handle(pfc, w, None, **FORCE)
    outs = {None: m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)}
    for b in (-5, 0):
        m.set_option("bin_split", b)
        outs[b] = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    m.close()
    for b, out in outs.items():
        check_oracle(f"tet-tet bin_split {b}", out, ref)
        assert np.array_equal(out[2], outs[0][2])
