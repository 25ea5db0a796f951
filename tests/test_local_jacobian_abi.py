"""pfc_local_jacobian[_device] and pfc_apply_local_jacobian[_device]: the C ABI and the tangent helper, without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from test_oracle_dual import pose_of, rodrigues, tangents

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = (("pfc_local_jacobian_device", 3), ("pfc_local_jacobian", 10), ("pfc_apply_local_jacobian_device", 10),
         ("pfc_apply_local_jacobian", 9))


def test_local_jacobian_symbols_are_declared_exported_and_bound(pfc):
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
    assert L.pfc_local_jacobian.argtypes[1] is C.c_int
    assert L.pfc_apply_local_jacobian_device.argtypes[1] is C.c_int and L.pfc_apply_local_jacobian_device.argtypes[2] is C.c_int
    assert L.pfc_apply_local_jacobian.argtypes[1] is C.c_int and L.pfc_apply_local_jacobian.argtypes[2] is C.c_int
    assert L.pfc_version() == 100


def test_local_jacobian_kernels_are_built_from_their_header(pfc):
    srcs = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "_lib.py")).read()
    assert '"pfc_ljac.h"' in srcs      # a change of the kernels rebuilds the library
    src = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc", "pfc_hip.hip")).read()
    assert '#include "pfc_ljac.h"' in src


def test_tangent_helper_contracts_the_pose_columns_with_consistent_seeds(pfc):
    """local_jacobian_tangent(L, pose) . (δθ, δt, twist, s) = L . (tangents(δθ, δt), twist, s) for any L."""
    rng = np.random.default_rng(3)
    n = 3
    L = rng.standard_normal((n, 12, 36))
    pose = np.stack([pose_of(rodrigues(rng.standard_normal(3)), rng.standard_normal(3), np.zeros(6)) for _ in range(n)])
    Lt = pfc.scenario.local_jacobian_tangent(L, pose)
    assert Lt.shape == (n, 12, 18)
    for k in range(n):
        R0 = pose[k, :9].reshape(3, 3, order="F"); t0 = pose[k, 9:12]
        q = rng.standard_normal((5, 18))
        full = np.concatenate([tangents(R0, t0, q[:, :6]), q[:, 6:]], axis=1)      # 5 x 36
        ref = L[k] @ full.T
        assert np.abs(Lt[k] @ q.T - ref).max() <= 1e-8 * np.abs(ref).max()
    assert np.array_equal(pfc.scenario.local_jacobian_tangent(L[0], pose[0]), Lt[0])
