"""The gripper program of the Radau step (pfc_radau_program_device, pfc_radau_set_program, pfc_radau_clear_program,
pfc_radau_program_state; kernel k_radau_program): the symbols, the scalar statement of include/pfc.h in Python floats
(scenario.rotation_angle, scenario.gripper_program_step) against an independent model written the way the reference's get_grip_ins
is written, and the data of configs.pencil_gripper.  tests/test_gpu_radau_program.py compares the device with this statement in
bytes."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAMES = [("pfc_radau_program_device", 23), ("pfc_radau_set_program", 10), ("pfc_radau_clear_program", 1), ("pfc_radau_program_state", 7),
         ("pfc_radau_get_tau", 2)]
TAU_SOFT, TAU_HARD = 0.3, 2.5


def test_program_symbols_are_declared_exported_and_bound(pfc):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfc.h")).read(), flags=re.S)
    for name, n_args in NAMES:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        res, args = pfc._lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, name
    dev = pfc._lib.SIGNATURES["pfc_radau_program_device"][1]
    assert dev[9] is C.c_double and dev[10] is C.c_double                  # tau_soft, tau_hard
    assert pfc._lib.SIGNATURES["pfc_radau_set_program"][1][4:6] == [C.c_double, C.c_double]
    out = subprocess.run(["nm", "-D", "--defined-only", pfc._lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pfc_[a-z_0-9]+)", out))
    assert {name for name, _ in NAMES} <= exported
    M = pfc.scenario.MechanismScenario
    for meth in ("radau_set_program", "radau_clear_program", "radau_program_state", "radau_program_device", "gripper_program_fn"):
        assert callable(getattr(M, meth)), meth
    csrc = os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc")
    prog = open(os.path.join(csrc, "pfc_radau_program.h")).read()
    assert "fma(" not in prog and "void __launch_bounds__(kRadProgBlock) k_radau_program(" in prog
    body = prog[prog.index("k_radau_program(RadauProgramArgs g) {"):]
    assert "__shared__" not in body and "atomic" not in body               # no LDS, plain stores
    assert "k_radau_program" not in open(os.path.join(csrc, "pfc_radau.h")).read()      # the controller's header is as it was
    assert '"pfc_radau_program.h"' in open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "_lib.py")).read()
    assert "parity unpinned" in open(os.path.join(ROOT, "include", "pfc.h")).read().split("pfc_radau_controller_state(pfc_handle")[-1]


# ---- the independent model: get_grip_ins and the tau_grip choice of test/pencil.jl, a list popped from the front ---------------------
class _Ins:
    def __init__(self, dt, q, slip):
        self.dt, self.q, self.slip, self.t0, self.rot_0 = dt, q, slip, INF, INF


def _model_call(queue, t, angle):
    ins = queue[0]
    if ins.t0 == INF:
        ins.t0 = t
    if len(queue) > 1 and ins.dt < (t - ins.t0):                           # the last instruction never expires (stated deviation)
        queue.pop(0)
        ins = queue[0]
        ins.t0 = t
        ins.rot_0 = angle
    if ins.slip == -INF:
        tau = 0.0
    elif ins.slip == 0.0:
        tau = TAU_HARD
    elif ins.slip == INF:
        tau = TAU_SOFT
    else:
        tau = TAU_SOFT if abs(angle - ins.rot_0) < ins.slip else TAU_HARD
    return ins, tau


def _next_up(x):
    return math.nextafter(x, INF)


def test_statement_is_the_popped_list_and_is_idempotent(pfc):
    """200 seeded random sequences of (t, angle) with random programs; every third step is a forced tie (t - t0 == prog_dt exactly:
    no pop) followed by the same t one ulp later (pop).  Every call is made twice at the same (t, angle): the second returns the
    first's record and outputs -- the idempotence that justifies one evaluation per batch step."""
    step = pfc.scenario.gripper_program_step
    slips = [-INF, 0.0, -0.0, INF, 0.05, 0.5, -0.1]
    ties = pops_at_ulp = 0
    for seed in range(200):
        rng = np.random.default_rng(seed)
        n_ins, n_act = int(rng.integers(1, 7)), int(rng.integers(0, 4))
        # durations on a binary grid, like t: t - t0 is exact, so a tie can be forced
        prog_dt = [float(rng.integers(0, 6)) / 8.0 for _ in range(n_ins)]
        if seed % 5 == 0:
            prog_dt[int(rng.integers(0, n_ins))] = INF
        prog_q = rng.standard_normal((n_ins, n_act)).tolist()
        prog_slip = [slips[int(rng.integers(0, len(slips)))] for _ in range(n_ins)]
        queue = [_Ins(prog_dt[j], prog_q[j], prog_slip[j]) for j in range(n_ins)]
        rec = dict(pfc.scenario.PROGRAM_RECORD0)
        t, popped, was_tie = float(rng.integers(0, 4)) / 8.0, 0, False
        for k in range(40):
            angle = float(rng.uniform(0.0, math.pi))
            cand = rec["t0"] + prog_dt[rec["cursor"]]
            if k % 3 == 1 and rec["cursor"] < n_ins - 1 and math.isfinite(cand) and cand >= t and cand - rec["t0"] == prog_dt[rec["cursor"]]:
                t = cand                                                   # the tie: t - t0 == prog_dt exactly
                tie = True
            elif k % 3 == 2 and k > 0 and was_tie:
                t = _next_up(t)                                            # one ulp more
                tie = False
            else:
                t = t + float(rng.integers(0, 5)) / 8.0
                tie = False
            before = rec["cursor"]
            for rep in range(2):
                ins, tau = _model_call(queue, t, angle)
                new, seg_q, tau_grip = step(rec, t, angle, prog_dt, prog_q, prog_slip, TAU_SOFT, TAU_HARD)
                if rep == 1:
                    assert new == rec and (seg_q, tau_grip) == first, (seed, k)
                rec, first = new, (seg_q, tau_grip)
                assert rec["cursor"] == n_ins - len(queue) and rec["t0"] == ins.t0 and rec["angle"] == angle
                assert rec["rot_0"] == ins.rot_0 and seg_q == ins.q and tau_grip == tau == rec["tau_grip"], (seed, k)
                assert math.copysign(1.0, tau_grip) == 1.0
            if tie:
                assert rec["cursor"] == before
                ties += 1
            if k % 3 == 2 and was_tie and rec["cursor"] == before + 1:
                pops_at_ulp += 1
            popped += rec["cursor"] - before
            assert rec["cursor"] - before in (0, 1) and rec["pops"] == popped
            was_tie = tie
    assert ties > 100 and pops_at_ulp > 50, (ties, pops_at_ulp)


def _one(pfc, slip, angle, rot_0, cursor=0, prog_dt=(INF, INF)):
    rec = dict(pfc.scenario.PROGRAM_RECORD0, t0=0.0, rot_0=rot_0, cursor=cursor)
    new, _, tau = pfc.scenario.gripper_program_step(rec, 1.0, angle, list(prog_dt), [[0.0], [1.0]], [slip, slip], TAU_SOFT, TAU_HARD)
    assert new["cursor"] == cursor and new["pops"] == 0
    return tau


def test_slip_classes(pfc):
    assert _one(pfc, -INF, 1.0, 0.5) == 0.0
    assert _one(pfc, 0.0, 1.0, 0.5) == TAU_HARD and _one(pfc, -0.0, 1.0, 0.5) == TAU_HARD
    assert _one(pfc, INF, 1.0, 0.5) == TAU_SOFT
    assert _one(pfc, 0.2, 0.69, 0.5) == TAU_SOFT and _one(pfc, 0.2, 0.31, 0.5) == TAU_SOFT      # below the threshold, either way
    assert _one(pfc, 0.2, 0.71, 0.5) == TAU_HARD and _one(pfc, 0.2, 0.29, 0.5) == TAU_HARD      # beyond it
    assert _one(pfc, 0.25, 0.75, 0.5) == TAU_HARD                          # |angle - rot_0| == slip exactly: strict <, hard
    assert _one(pfc, 0.2, 1.0, INF) == TAU_HARD                            # the first instruction: rot_0 = +inf
    assert _one(pfc, 0.2, float("nan"), 0.5) == TAU_HARD                   # a NaN angle
    assert _one(pfc, -0.1, 0.5, 0.5) == TAU_HARD                           # a negative finite slip: nothing is below it


def test_last_instruction_never_expires(pfc):
    step = pfc.scenario.gripper_program_step
    rec = dict(pfc.scenario.PROGRAM_RECORD0)
    prog_dt, prog_q, prog_slip = [0.0, 0.0], [[1.0], [2.0]], [INF, 0.0]
    rec, q, tau = step(rec, 0.0, 0.1, prog_dt, prog_q, prog_slip, TAU_SOFT, TAU_HARD)
    assert (rec["cursor"], rec["t0"], q, tau) == (0, 0.0, [1.0], TAU_SOFT)       # latched: t - t0 = 0 is not > 0
    rec, q, tau = step(rec, 0.5, 0.2, prog_dt, prog_q, prog_slip, TAU_SOFT, TAU_HARD)
    assert (rec["cursor"], rec["pops"], rec["t0"], rec["rot_0"], q, tau) == (1, 1, 0.5, 0.2, [2.0], TAU_HARD)
    for t in (1.0, 1.0e9, INF):
        rec, q, tau = step(rec, t, 0.3, prog_dt, prog_q, prog_slip, TAU_SOFT, TAU_HARD)
        assert (rec["cursor"], rec["pops"], rec["t0"], rec["rot_0"], q) == (1, 1, 0.5, 0.2, [2.0])
    one = step(dict(pfc.scenario.PROGRAM_RECORD0), 5.0, 0.3, [0.0], [[7.0]], [-INF], TAU_SOFT, TAU_HARD)      # a program of one
    assert one[0]["cursor"] == 0 and one[0]["t0"] == 5.0 and one[1] == [7.0] and one[2] == 0.0


def test_rotation_angle(pfc):
    ang = pfc.scenario.rotation_angle
    assert ang(np.eye(3)) == 0.0
    assert ang(np.diag([1.0, -1.0, -1.0])) == math.pi
    rz = pfc.configs.rot_z(-math.pi / 2)
    assert abs(ang(rz) - math.pi / 2) <= math.ulp(math.pi / 2)
    assert ang(rz) == ang(rz.reshape(-1, order="F")) == ang(np.concatenate([rz.reshape(-1, order="F"), [1.0, 2.0, 3.0]]))      # x_w_b's record
    seen = []
    assert ang(pfc.configs.rot_x(0.3), atan2=lambda s, w: seen.append((s, w)) or 0.25) == 0.25                # the caller's atan2 is used
    assert abs(math.atan2(*seen[0]) - 0.3) < 1e-15


def test_pencil_gripper_data(pfc):
    for bristle, nx in ((False, 20), (True, 32)):
        d = pfc.configs.pencil_gripper(bristle)
        parent, jt, x_p_j, axis = d["mechanism"]
        ndof = {0: 0, 1: 1, 2: 1, 3: 6}
        assert sum(ndof[int(t)] for t in jt) == 10 and d["x0"].size == nx       # nq = nv = 10, NX = nq + nv + 6 bristle items
        assert parent.tolist() == [-1, 0, 1, 1, -1] and jt.tolist() == [2, 1, 2, 2, 3]
        assert axis[:4].tolist() == [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0]]
        w = d["workload"]
        assert [m.name for m in w.meshes] == ["plane", "rev_y", "pad_n", "pad_p", "pencil"]
        assert w.meshes[2].mesh.n_tet == w.meshes[3].mesh.n_tet == 320 and w.meshes[4].mesh.n_tri == 48
        assert [c.model for c in w.instructions] == (["bristle"] * 2 if bristle else ["regularized"] * 2) + ["regularized"] * 2
        assert [(c.id_1, c.id_2) for c in w.instructions] == [(4, 2), (4, 3), (4, 0), (2, 3)] and d["ins_bodies"] == [(4, 2), (4, 3), (4, -1), (2, 3)]
        assert d["inertia"].shape == (5, 13) and d["inertia"][0].tolist() == [1.0] * 9 + [0.0] * 3 + [1.0]
    p, c = d["program"], d["controller"]
    assert p["prog_dt"].tolist() == [1.2, 0.25, 1.3, 0.5, 2.0, 1.5, 0.5, 2.5, 2.5, 2.5, INF]
    assert p["prog_slip"].tolist() == [-INF, INF, INF, 0.0, 0.0, INF, 0.0, 0.0, 0.2, 0.2, INF]
    z_low, z_high = 0.0035, 1.2 * 0.16
    assert p["prog_q"][:, 0].tolist() == [z_low, z_low] + [z_high] * 9
    assert p["prog_q"][:, 1].tolist() == [0.0] * 4 + [math.pi / 2] * 3 + [-math.pi / 2] * 4 and not p["prog_q"][:, 2:].any()
    assert set(p["grip"].tolist()) == {2, 3} < set(c["act"].tolist()) == {0, 1, 2, 3} and p["body"] == 4
    assert (p["tau_soft"], p["tau_hard"], c["dt"]) == (0.3, 2.5, 0.01) and c["a_max"].tolist() == [1.0, INF, INF, INF]
    assert c["kp"] == (2 * math.pi / 0.75) ** 2 and c["kd"] == 2 * (2 * math.pi / 0.75)
    assert d["x0"][:10].tolist()[:4] == [0.10, math.pi / 4, 0.0, 0.0] and d["x0"][7] == -0.128 and not d["x0"][10:].any()
    pencil = pfc.scenario.joint_kinematics(parent, jt, x_p_j, axis, d["x0"][:10], d["x0"][10:20])[0][4]
    assert abs(pfc.scenario.rotation_angle(pencil[:9]) - math.pi / 2) < 1e-15 and pencil[9:].tolist() == [-0.128, 0.0, 0.0]      # RotZ(-pi/2)
    assert np.abs(pencil[:9].reshape(3, 3, order="F") - pfc.configs.rot_z(-math.pi / 2)).max() < 1e-15
    assert (d["radau"]["h_max"], d["radau"]["h_min"], d["radau"]["t_final"], d["radau"]["max_steps"]) == (0.01, 1.0e-14, 18.0, 8200)
