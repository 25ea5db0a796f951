"""pfc_contact_surface_fric: the C ABI and the host-side FrictionSurface view, without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_friction_symbols_are_declared_exported_and_bound(pfc):
    hdr = open(os.path.join(ROOT, "include", "pfc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in (("pfc_contact_surface_fric", 19), ("pfc_contact_surface_fric_device", 20)):
        m = re.search(name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        res, args = pfc._lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, name
    out = subprocess.run(["nm", "-D", "--defined-only", pfc._lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pfc_[a-z_0-9]+)", out))
    assert {"pfc_contact_surface_fric", "pfc_contact_surface_fric_device"} <= exported
    L = pfc._lib.lib()
    assert L.pfc_contact_surface_fric.argtypes[6] is C.c_longlong and L.pfc_contact_surface_fric.argtypes[7] is C.c_longlong
    assert L.pfc_contact_surface_fric_device.argtypes[6] is C.c_longlong and L.pfc_contact_surface_fric_device.argtypes[-1] is C.c_void_p
    assert L.pfc_version() == 100


def _surface(pfc, n=2, P=3, T=7):
    return pfc.ContactSurface(poly_off=np.array([0, 1, P], dtype=np.int64), poly_idx=np.zeros((P, 3), np.int32),
                              poly_xyz=np.zeros((P, 8, 3)), poly_trac=np.array([0, 3, 5, T], dtype=np.int64),
                              trac=np.arange(T * 8, dtype=np.float64).reshape(T, 8), summary=np.zeros((n, 11)),
                              counts=np.zeros((n, 4), np.int32))


def _parts(pfc):
    S = _surface(pfc)
    T, n = S.trac.shape[0], S.n_items
    return dict(surface=S, fric=np.arange(T * 4, dtype=np.float64).reshape(T, 4),
                fric_summary=np.arange(n * 20, dtype=np.float64).reshape(n, 20),
                stiff=np.arange(n * 84, dtype=np.float64).reshape(n, 84))


def test_friction_surface_view(pfc):
    F = pfc.FrictionSurface(**_parts(pfc))
    assert F.n_items == 2
    a, b = F.item(0), F.item(1)
    assert a["fric"].shape == (3, 4) and b["fric"].shape == (4, 4)
    assert np.array_equal(a["fric"], F.fric[0:3]) and np.array_equal(b["fric"], F.fric[3:7])
    assert a["trac"].shape == (3, 8) and np.array_equal(b["trac"], F.surface.trac[3:7])
    assert np.array_equal(b["total_wrench"], F.fric_summary[1, 0:6]) and np.array_equal(b["fric_wrench"], F.fric_summary[1, 6:12])
    assert np.array_equal(b["sdot"], F.fric_summary[1, 12:18])
    assert b["first_p_dA"] == F.fric_summary[1, 18] and b["n_first"] == int(F.fric_summary[1, 19])
    assert np.array_equal(b["K"], F.stiff[1, 0:36].reshape(6, 6, order="F"))
    assert np.array_equal(b["Kbar_inv_sqrt"], F.stiff[1, 36:72].reshape(6, 6, order="F"))
    assert np.array_equal(b["Sinv"], F.stiff[1, 72:78]) and np.array_equal(b["Delta"], F.stiff[1, 78:84])
    assert list(b["poly_trac"]) == [0, 2, 4] and b["keys"].shape == (2, 2)      # ContactSurface.item's keys are kept
    with pytest.raises(IndexError):
        F.item(2)


@pytest.mark.parametrize("field,bad", [("fric", np.zeros((6, 4))), ("fric", np.zeros((7, 3))), ("fric_summary", np.zeros((2, 19))),
                                       ("fric_summary", np.zeros((3, 20))), ("stiff", np.zeros((2, 36))), ("stiff", np.zeros((1, 84)))])
def test_friction_surface_validates_shapes(pfc, field, bad):
    p = _parts(pfc)
    p[field] = bad
    with pytest.raises(ValueError):
        pfc.FrictionSurface(**p)


def test_friction_surface_needs_a_surface(pfc):
    p = _parts(pfc)
    p["surface"] = dict(trac=np.zeros((7, 8)))
    with pytest.raises(ValueError):
        pfc.FrictionSurface(**p)
