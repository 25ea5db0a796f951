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


# The six blocks of the Radau handle on the two-scene slider (tests/test_gpu_radau_program.py: n_scene = 2, one regularized item,
# nq = nv = 2, NX = 4, n_body = 2, n_chunk = 6, controller n_act = 2 / n_seg = 1 with seg_ff, program n_ins = 3 / n_grip = 1), as
# (bytes, element size) in the order of the calls.  Recorded from the log of the commit before the part-block type; the formulas:
#   pfc_radau_configure rounds each part up to 32 doubles / 64 ints, an empty part taking one element:
#     doubles  10 x 32 (x, t, h, enorm, nstate, X, F, xdot0, -J, LU0) + 64 (LU1) + 32 (tau) + 1152 (16 value parts)
#              + 1824 (16 partial parts) + 32 (t_final) = 3424;   ints  13 parts x 64 = 832
#   pfc_radau_set_controller packs:  kp 2 + kd 2 + a_max 2 + seg_t 2 + seg_q 4 + seg_ff 4 + t_last 2 = 18;  act 2 + fires 2 = 4
#   pfc_radau_set_program packs:     prog_dt 6 + prog_q 12 + prog_slip 6 + records 8 = 32;  grip 1 + cursors 4 = 5
_RADAU_BLOCKS = {"configure": [(8 * 3424, 8), (4 * 832, 4)], "controller": [(8 * 18, 8), (4 * 4, 4)], "program": [(8 * 32, 8), (4 * 5, 4)]}


def radau_child():
    """The child process: the three calls that allocate a pair of blocks, each between two marks in the log, a step, the close."""
    import pfc_pkg
    import test_gpu_radau_program as P
    pfc = pfc_pkg.load()
    m = P.T._slider(pfc, two=True)

    def marked(name, call):
        print(f"mark {name}", file=sys.stderr, flush=True)
        call()
        print("mark end", file=sys.stderr, flush=True)

    marked("configure", lambda: m.radau_configure(2, [0]))
    m.radau_set_state(P.SLIDER_X0)
    marked("controller", lambda: m.radau_set_controller(**P.SLIDER_CTL))
    marked("program", lambda: m.radau_set_program(**P.SLIDER_PROG))
    assert m.radau_step()["flags"].tolist() == [0, 0]
    m.close()


def test_radau_blocks_have_their_sizes_and_are_freed_once():
    """Both layout rules of the handle's part blocks (rounded parts for the step's two blocks, packed parts for the controller's
    and the program's), the double block before the int block, and each of the six freed exactly once."""
    env = dict(os.environ, PFC_LOG_ALLOC="1")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_gpu_ownership as t; t.radau_child()"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    alloc = re.compile(r"^pfc alloc (0x[0-9a-f]+) \.\. 0x[0-9a-f]+ \((\d+) bytes, element (\d+)\)$")
    free = re.compile(r"^pfc free (0x[0-9a-f]+)$")
    call, got, live, others, n_freed = None, {}, set(), set(), 0
    for ln in r.stderr.splitlines():
        a, f = alloc.match(ln), free.match(ln)
        if ln.startswith("mark "):
            call = None if ln == "mark end" else ln[5:]
        elif a:
            assert a.group(1) not in live and a.group(1) not in others, f"allocated twice without a free in between: {ln}"
            (live if call else others).add(a.group(1))
            if call:
                got.setdefault(call, []).append((int(a.group(2)), int(a.group(3))))
        elif f:
            assert f.group(1) in live or f.group(1) in others, f"freed without a live allocation (a second free?): {ln}"
            n_freed += f.group(1) in live
            live.discard(f.group(1))
            others.discard(f.group(1))
    print("radau blocks:", got)
    assert got == _RADAU_BLOCKS, got
    assert not live and n_freed == 6, (live, n_freed)
