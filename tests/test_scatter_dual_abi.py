"""pfc_scatter_generalized_dual[_device]: the C ABI, without a device."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = (("pfc_scatter_generalized_dual", 17), ("pfc_scatter_generalized_dual_device", 18))


def test_scatter_dual_symbols_are_declared_exported_and_bound(pfc):
    hdr = open(os.path.join(ROOT, "include", "pfc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in NAMES:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        res, args = pfc._lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, name
    out = subprocess.run(["nm", "-D", "--defined-only", pfc._lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pfc_[a-z_0-9]+)", out))
    assert {name for name, _ in NAMES} <= exported
    L = pfc._lib.lib()
    host, dev = L.pfc_scatter_generalized_dual, L.pfc_scatter_generalized_dual_device
    assert host.argtypes[2] is C.c_int and host.argtypes[10] is C.c_int and host.argtypes[11] is C.c_int and host.argtypes[12] is C.c_int
    assert dev.argtypes[2] is C.c_int and dev.argtypes[10] is C.c_int and dev.argtypes[11] is C.c_int
    assert dev.argtypes[16] is C.c_int and dev.argtypes[17] is C.c_void_p
    assert L.pfc_version() == 100


def test_scatter_dual_kernels_are_built_from_their_header(pfc):
    srcs = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "_lib.py")).read()
    assert '"pfc_scatter.h"' in srcs      # a change of the kernels rebuilds the library
    src = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc", "pfc_hip.hip")).read()
    assert '#include "pfc_scatter.h"' in src
