"""Every device and pinned block the library allocates is freed exactly once by the time its handles are closed.

The host context owns its GPU resources through move-only types (csrc/pfc_hip.hip, "owning types"); with PFC_LOG_ALLOC=1 they
log every allocation with its address range and every free with its address.  A fresh child process drives one single-device
handle and one {0, 0} multi-device handle through the paths that allocate -- a split batch (a twin context), a small fused
scene, a host Dual evaluation with a broadphase pose, the device Dual evaluation and a further chunk, the contact Jacobian,
both surface calls, both scatter calls, an evaluation under fixed_order -- closes them and exits; this process pairs the log."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


def _drive(pfc, H, devices, n_split):
    import torch
    C = pfc.configs
    rng = np.random.default_rng(11)
    # a split batch: more than split_min items per device, so every context makes its twin
    big = H.fuzz_workload(pfc, rng, n_split, False)
    m = C.build_scenario(big, devices=devices)
    m.force_all_elastic_intersections(big.pose, big.twist, big.s, big.ins_ids)
    assert m.last_parts() == 2, m.last_parts()
    m.close()
    # small scenes, regularized and bristle instructions
    w = H.fuzz_workload(pfc, rng, 24, False)
    n, nd = w.n_items, 3
    m = C.build_scenario(w, devices=devices)
    m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    if devices is None:
        assert m.last_parts() == 0, m.last_parts()      # the one-launch kernel
    dp, dt, ds = rng.standard_normal((n, nd, 24)) * 1e-3, rng.standard_normal((n, nd, 6)), rng.standard_normal((n, nd, 6)) * 1e-3
    for _ in range(2):      # a first chunk and a further one at the same point
        m.force_all_elastic_intersections_dual(w.pose, w.twist, w.s, dp, dt, ds, w.ins_ids, bp_pose=w.pose)
    dev = torch.device("cuda:0")
    t = lambda a, ty=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=ty, device=dev)
    T = dict(ids=t(w.ins_ids, torch.int32), pose=t(w.pose), twist=t(w.twist), s=t(w.s), dp=t(dp), dt=t(dt), ds=t(ds))
    z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=dev)
    o = dict(w=z(n, 6), sd=z(n, 6), dw=z(n, nd, 6), dsd=z(n, nd, 6), c=torch.zeros((n, 4), dtype=torch.int32, device=dev))
    st = torch.cuda.current_stream().cuda_stream
    for attempt in range(6):
        m.eval_dual_device(n, nd, T["ids"].data_ptr(), T["pose"].data_ptr(), T["twist"].data_ptr(), T["s"].data_ptr(), T["dp"].data_ptr(),
                           T["dt"].data_ptr(), T["ds"].data_ptr(), o["w"].data_ptr(), o["sd"].data_ptr(), o["dw"].data_ptr(),
                           o["dsd"].data_ptr(), o["c"].data_ptr(), st)
        if m.check() == pfc._lib.OK:
            break
    else:
        raise RuntimeError("the Dual evaluation did not settle")
    m.eval_dual_device_more(nd, T["dp"].data_ptr(), T["dt"].data_ptr(), T["ds"].data_ptr(), o["dw"].data_ptr(), o["dsd"].data_ptr(), st)
    assert m.check() == pfc._lib.OK
    torch.cuda.synchronize()
    wrench, _, L, _ = m.local_jacobian(w.pose, w.twist, w.s, w.ins_ids)
    assert np.isfinite(L).all()
    m.contact_surface(w.pose, w.twist, w.ins_ids)
    m.contact_surface_fric(w.pose, w.twist, w.s, w.ins_ids)
    x = np.tile(np.concatenate([np.eye(3).reshape(-1, order="F"), np.zeros(3)]), (n, 1))
    b1 = rng.integers(-1, 3, n).astype(np.int32); b2 = rng.integers(0, 3, n).astype(np.int32)
    jac = rng.standard_normal((3, 5, 6))
    m.scatter_generalized(wrench, x, b1, b2, jac, scene=(np.arange(n) % 2).astype(np.int32), n_scene=2)
    m.scatter_generalized_dual(wrench, rng.standard_normal((n, nd, 6)), x, None, b1, b2, jac, None,
                               scene=(np.arange(n) % 2).astype(np.int32), n_scene=2)
    m.set_option("fixed_order", 1)
    m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    m.close()


def child():
    """The child process: every path on both kinds of handle, handles closed, exit status 0."""
    import pfc_pkg
    import helpers as H
    pfc = pfc_pkg.load()
    _drive(pfc, H, None, 1100)
    _drive(pfc, H, [0, 0], 2400)


_ALLOC = re.compile(r"^pfc (alloc|pinned) (0x[0-9a-f]+) \.\. ")
_FREE = re.compile(r"^pfc (free|unpinned) (0x[0-9a-f]+)$")


def test_every_allocation_is_freed_once():
    env = dict(os.environ, PFC_LOG_ALLOC="1")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_gpu_ownership as t; t.child()"
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    live, n_alloc, n_pinned = set(), 0, 0
    for ln in r.stderr.splitlines():
        a, f = _ALLOC.match(ln), _FREE.match(ln)
        if a:
            key = ("pinned" if a.group(1) == "pinned" else "device", a.group(2))
            assert key not in live, f"allocated twice without a free in between: {ln}"
            live.add(key)
            n_alloc += 1
            n_pinned += key[0] == "pinned"
        elif f:
            key = ("pinned" if f.group(1) == "unpinned" else "device", f.group(2))
            assert key in live, f"freed without a live allocation (a second free?): {ln}"
            live.remove(key)
        else:
            assert not ln.startswith("pfc alloc") and not ln.startswith("pfc pinned") and not ln.startswith("pfc free") and \
                not ln.startswith("pfc unpinned"), f"allocation log line not understood (a failed allocation?): {ln}"
    assert n_alloc - n_pinned >= 100 and n_pinned >= 10, (n_alloc, n_pinned)      # the log is on and the paths ran
    assert not live, f"{len(live)} blocks never freed, e.g. {sorted(live)[:5]}"
