"""pfc_contact_surface: the C ABI and the host-side ContactSurface view, without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_surface_symbols_are_declared_exported_and_bound(pfc):
    hdr = open(os.path.join(ROOT, "include", "pfc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in (("pfc_contact_surface", 15), ("pfc_contact_surface_device", 16)):
        m = re.search(name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        res, args = pfc._lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, name
    out = subprocess.run(["nm", "-D", "--defined-only", pfc._lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pfc_[a-z_0-9]+)", out))
    assert {"pfc_contact_surface", "pfc_contact_surface_device"} <= exported
    L = pfc._lib.lib()
    assert L.pfc_contact_surface.argtypes[5] is C.c_longlong and L.pfc_contact_surface_device.argtypes[-1] is C.c_void_p


def _parts(n=2, P=3, T=7):
    poly_off = np.array([0, 1, P][: n + 1] if n == 2 else np.linspace(0, P, n + 1).astype(np.int64), dtype=np.int64)
    return dict(poly_off=poly_off, poly_idx=np.zeros((P, 3), np.int32), poly_xyz=np.zeros((P, 8, 3)),
                poly_trac=np.array([0, 3, 5, T], dtype=np.int64)[: P + 1], trac=np.zeros((T, 8)), summary=np.zeros((n, 11)),
                counts=np.zeros((n, 4), np.int32))


def test_contact_surface_view(pfc):
    S = pfc.ContactSurface(**_parts())
    assert S.n_items == 2
    a, b = S.item(0), S.item(1)
    assert a["keys"].shape == (1, 2) and b["keys"].shape == (2, 2)
    assert a["trac"].shape == (3, 8) and b["trac"].shape == (4, 8)
    assert list(b["poly_trac"]) == [0, 2, 4]
    with pytest.raises(IndexError):
        S.item(2)
    empty = pfc.ContactSurface(np.zeros(1, np.int64), np.zeros((0, 3), np.int32), np.zeros((0, 8, 3)), np.zeros(1, np.int64),
                               np.zeros((0, 8)), np.zeros((0, 11)), np.zeros((0, 4), np.int32))
    assert empty.n_items == 0


@pytest.mark.parametrize("field,bad", [("poly_idx", np.zeros((3, 2), np.int32)), ("poly_xyz", np.zeros((3, 4, 3))),
                                       ("poly_trac", np.zeros(3, np.int64)), ("trac", np.zeros((7, 6))),
                                       ("summary", np.zeros((2, 6))), ("counts", np.zeros((3, 4), np.int32)),
                                       ("poly_off", np.zeros((3, 1), np.int64))])
def test_contact_surface_validates_shapes(pfc, field, bad):
    p = _parts()
    p[field] = bad
    with pytest.raises(ValueError):
        pfc.ContactSurface(**p)


def test_contact_surface_validates_offsets(pfc):
    p = _parts()
    p["poly_off"] = np.array([0, 1, 2], dtype=np.int64)       # does not end at the polygon count
    with pytest.raises(ValueError):
        pfc.ContactSurface(**p)
    p = _parts()
    p["poly_trac"] = np.array([0, 3, 5, 6], dtype=np.int64)   # does not end at the point count
    with pytest.raises(ValueError):
        pfc.ContactSurface(**p)
