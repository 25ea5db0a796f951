"""The host-pointer forms of the device calls share one staging block per context (csrc/pfc_hip.hip, Stage): what sharing it can get
wrong.  Calls of different forms interleaved on one handle (the block's need going large -> small -> large), every optional host
pointer null in turn, and a surface call whose second attempt finds the block regrown.

Scene: five fuzz items (helpers.fuzz_workload) of four instructions bound to three bodies in two scenes, nv = 5, n_dir 1 and 3,
item counts 3 and 5: odd on purpose, so that an int field ends off an 8-byte boundary in front of a double field.

Compared as bytes (two calls on two fresh handles return identical bytes): items_from_bodies, dual_seeds_from_bodies,
apply_local_jacobian, scatter_generalized_dual (kernels without atomics), contact_surface and contact_surface_fric (one canonical
order, tests/test_gpu_contact_friction.py::_same_bytes), and local_jacobian under option fixed_order.  With tolerances:
scatter_generalized (k_scatter adds atomically) at 1e-12 relative plus 1e-12 of the largest entry
(tests/test_gpu_scale.py::test_scatter_generalized_third_law); local_jacobian on a default handle at 1e-9 of the largest entry for
wrench and the wrench rows of L, 1e-7 for sdot and the sdot rows
(tests/test_gpu_local_jacobian.py::test_multi_device_handle_gives_the_single_handle_L), counts exactly."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(pfc):
    return H.HostFormsCase(pfc)


ORDER = H.HOST_FORMS_ORDER
_alone = {}


def alone(pfc, case, form, devices, **options):
    """The form's outputs from its only call on a fresh handle (computed once per kind of handle, never changed)."""
    key = (form, devices is not None, tuple(sorted(options.items())))
    if key not in _alone:
        m = case.handle(pfc, devices, **options)
        _alone[key] = case.run(pfc, m, form)
        m.close()
    return _alone[key]


def _bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _compare(form, got, ref, where):
    assert got.keys() == ref.keys(), (form, where)
    for k in ref:
        g, r = got[k], ref[k]
        same = _bytes(g, r)
        if form == "scatter":
            print(f"{where} {form}.{k}: bytes {same}, max diff {np.abs(g - r).max():.3e}")
            np.testing.assert_allclose(g, r, rtol=1e-12, atol=1e-12 * np.abs(r).max(), err_msg=f"{form}.{k} {where}")
        elif form == "local_jacobian" and k != "counts":
            print(f"{where} {form}.{k}: bytes {same}, max diff {np.abs(g - r).max():.3e}")
            rows = [(slice(None), 1e-9)] if k == "wrench" else [(slice(None), 1e-7)] if k == "sdot" else \
                [((slice(None), slice(0, 6)), 1e-9), ((slice(None), slice(6, 12)), 1e-7)]
            for sl, tol in rows:
                assert np.abs(g[sl] - r[sl]).max() <= tol * np.abs(r[sl]).max(), (form, k, where)
        else:
            assert same, (form, k, where)


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["single", "multi"])
def test_interleaved_forms_equal_their_calls_alone(pfc, case, devices):
    m = case.handle(pfc, devices)
    for lap in range(2):
        for form in ORDER:
            _compare(form, case.run(pfc, m, form), alone(pfc, case, form, devices), f"lap {lap}")
    m.close()
    assert np.abs(alone(pfc, case, "local_jacobian", devices)["L"]).max() > 0


# (form, argument made null, what null stands for: None -- the output is just not written --, "zeros", or "same": ids 0 .. n - 1, which
# the full call passes anyway)
OPTIONAL = [("items", k, None) for k in ("pose", "twist", "x_w_r2", "body_1", "body_2")] + [
    ("items", "ins_ids", "same"), ("items", "scene", "zeros"),
    ("seeds", "d_x_w_b", "zeros"), ("seeds", "d_twist_w_b", "zeros"), ("seeds", "d_pose", None), ("seeds", "d_twist", None),
    ("seeds", "d_x_w_r2", None),
    ("local_jacobian_c1", "s", "zeros"), ("local_jacobian3", "ins_ids", "same"), ("local_jacobian3", "counts", None),
    ("apply", "d_s", "zeros"),
    ("scatter_dual", "d_x_w_r2", "zeros"), ("scatter_dual", "d_jac", "zeros"), ("scatter_dual", "f", None), ("scatter_dual", "scene", "zeros"),
    ("surface_fric", "stiff", None), ("surface_fric", "counts", None)]


@pytest.fixture(scope="module")
def fixed_handles(pfc, case):
    """One handle for every optional-argument case, and one of C1 (no bristle instruction: the library takes a null s): under
    fixed_order, so that local_jacobian returns the same bytes call after call."""
    ms = {False: case.handle(pfc, None, fixed_order=1), True: case.handle(pfc, None, c1=True, fixed_order=1)}
    yield ms
    for m in ms.values():
        m.close()


@pytest.mark.parametrize("form,name,stands_for", OPTIONAL, ids=[f"{f}-{k}" for f, k, _ in OPTIONAL])
def test_null_optional_argument(pfc, case, fixed_handles, form, name, stands_for):
    """A null input must not read what an earlier call left in its slot of the shared block (the slot's place depends on the
    element counts only, and the block never shrinks): the call with the pointer dropped runs directly behind a call of the same
    form that uploaded OTHER values there -- the case's non-zero arrays, permuted ids --, the call with the stand-in after it.
    (C1's regularized items do not read s, so its row only shows that a null s is taken.)"""
    m = fixed_handles[form == "local_jacobian_c1"]
    default = None if stands_for is None else case.args(form)[0][name]
    if stands_for == "same":
        assert np.array_equal(default, np.arange(3))
        case.run(pfc, m, form, **{name: default[::-1].copy()})
    elif stands_for == "zeros":
        prime = np.ones_like(default) if form == "local_jacobian_c1" else default
        assert np.count_nonzero(prime) > 0
        case.run(pfc, m, form, **{name: prime})
    got = case.run(pfc, m, form, drop=(name,))
    full = case.run(pfc, m, form, **({name: np.zeros_like(default)} if stands_for == "zeros" else {}))
    assert set(got) == set(full) - {name}
    for k in got:
        assert _bytes(got[k], full[k]), (form, name, k)
    assert any(np.abs(v).max() > 0 for v in got.values())
    if stands_for is not None and form != "local_jacobian_c1":      # the slot's earlier content would have shown
        primed = case.run(pfc, m, form, **{name: default[::-1].copy() if stands_for == "same" else default})
        assert any(not _bytes(primed[k], full[k]) for k in full), (form, name)


@pytest.mark.parametrize("fric", [False, True], ids=["surface", "surface_fric"])
def test_block_regrown_between_the_attempts_of_a_surface_call(pfc, case, fric):
    """A handle's first surface call stages no list entries, learns the totals and runs again on a larger block: the inputs must
    survive that, here right behind a small call of another form that left the block small."""
    form = "surface_fric" if fric else "surface"
    m = case.handle(pfc)
    case.run(pfc, m, "items")
    _compare(form, case.run(pfc, m, form), alone(pfc, case, form, None), "behind items")
    m.close()
