"""The discrete controller of the Radau step (pfc_radau_control_device, pfc_radau_set_controller, pfc_radau_clear_controller,
pfc_radau_controller_state): the symbols, and the scalar statement of include/pfc.h in Python floats (scenario.discrete_clock,
scenario.computed_torque_pd) on hand cases.  tests/test_gpu_radau_control.py compares the device with this statement in bytes."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAMES = [("pfc_radau_control_device", 24), ("pfc_radau_set_controller", 12), ("pfc_radau_clear_controller", 1),
         ("pfc_radau_controller_state", 3)]


def test_control_symbols_are_declared_exported_and_bound(pfc):
    hdr = open(os.path.join(ROOT, "include", "pfc.h")).read()
    assert "a caller with a controller integrates one batch step at a time" not in hdr
    assert "#define PFC_RADAU_MAX_FIRES 4096" in hdr and pfc.scenario.RADAU_MAX_FIRES == 4096
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in NAMES:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        res, args = pfc._lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, name
    assert pfc._lib.SIGNATURES["pfc_radau_control_device"][1][6] is C.c_double      # dt
    assert pfc._lib.SIGNATURES["pfc_radau_set_controller"][1][6] is C.c_double
    out = subprocess.run(["nm", "-D", "--defined-only", pfc._lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pfc_[a-z_0-9]+)", out))
    assert {name for name, _ in NAMES} <= exported
    M = pfc.scenario.MechanismScenario
    for meth in ("radau_set_controller", "radau_clear_controller", "radau_controller_state", "radau_control_device",
                 "computed_torque_pd_fn", "integrate_scenario_radau"):
        assert callable(getattr(M, meth)), meth
    rad = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc", "pfc_radau.h")).read()
    assert "fma(" not in rad and "k_radau_control(" in rad
    body = rad[rad.index("k_radau_control(RadauControlArgs g) {"):]
    assert "__shared__" not in body and "atomic" not in body      # no LDS, plain stores


# ---- the clock ------------------------------------------------------------------------------------------------------------------
def test_clock_fires_at_equality_and_adds_repeatedly(pfc):
    clock = pfc.scenario.discrete_clock
    assert clock(0.5, 0.5, 0.25) == (0.75, 1)                              # t_last == t fires: the reference's `<=`
    assert clock(0.5, 0.49999999999999994, 0.25) == (0.5, 0)               # one ulp earlier: not due, t_last untouched
    t_last, fires = clock(0.0, 0.25, 0.1)                                  # three additions in one call: 0.1, 0.2, 0.30000000000000004
    assert fires == 3 and t_last == ((0.0 + 0.1) + 0.1) + 0.1 == 0.30000000000000004
    assert clock(0.30000000000000004, 0.3, 0.1) == (0.30000000000000004, 0)      # the bits of repeated addition decide, not 3 dt
    # the bound: a clock far behind stops after RADAU_MAX_FIRES additions and is still due
    t_last, fires = clock(0.0, 1.0e6, 1.0)
    assert fires == 4096 and t_last == 4096.0
    t_last, fires = clock(1.0e20, 1.0e20, 1.0)                             # dt below the spacing at t_last: never catches up, still ends
    assert fires == 4096 and t_last == 1.0e20


# ---- the law --------------------------------------------------------------------------------------------------------------------
H3 = [[2.0, 0.5, 0.25], [0.5, 3.0, 0.125], [0.25, 0.125, 4.0]]
C3 = [0.1, -0.2, 0.3]


def test_law_written_order_and_segment_choice(pfc):
    law = pfc.scenario.computed_torque_pd
    q, v = [0.3, -0.1, 0.2], [1.0, 2.0, -0.5]
    act, kp, kd = [0, 2], [10.0, 20.0], [1.0, 2.0]
    seg_t = [123.0, 1.0, 2.0]                                              # entry 0 is not read
    seg_q = [[0.0, 0.0], [0.1, 0.1], [0.2, -0.2]]
    seg_ff = [[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [-1.0, -2.0, -3.0]]

    def by_hand(k):
        a0 = (-(1.0 * 1.0)) - 10.0 * (0.3 - seg_q[k][0])
        a2 = (-(2.0 * -0.5)) - 20.0 * (0.2 - seg_q[k][1])
        t0 = (((0.0 + 2.0 * a0) + 0.25 * a2) + 0.1) + seg_ff[k][0]
        t2 = (((0.0 + 0.25 * a0) + 4.0 * a2) + 0.3) + seg_ff[k][2]
        return [t0, seg_ff[k][1], t2]

    assert law(q, v, H3, C3, 0.999, act, kp, kd, seg_t, seg_q, seg_ff) == by_hand(0)
    assert law(q, v, H3, C3, 1.0, act, kp, kd, seg_t, seg_q, seg_ff) == by_hand(1)        # t == seg_t[1]: the segment has begun
    assert law(q, v, H3, C3, 1.9999999999999998, act, kp, kd, seg_t, seg_q, seg_ff) == by_hand(1)
    assert law(q, v, H3, C3, 2.0, act, kp, kd, seg_t, seg_q, seg_ff) == by_hand(2)
    assert law(q, v, H3, C3, -5.0, act, kp, kd, seg_t, seg_q, seg_ff) == by_hand(0)       # before every start: segment 0
    assert law(q, v, H3, C3, 2.0, act, kp, kd, [0.0, 2.0, 2.0], seg_q, seg_ff) == by_hand(2)      # equal starts: the later one
    no_ff = law(q, v, H3, C3, 0.0, act, kp, kd, seg_t, seg_q)
    assert no_ff[1] == 0.0 and no_ff[0] == by_hand(0)[0] and no_ff[2] == by_hand(0)[2]    # segment 0 has zero feed-forward
    assert law(q, v, H3, C3, 0.0, act, kp, kd, [0.0], seg_q[:1]) == no_ff                 # one segment, no start time read


def test_law_clamp_on_both_sides_and_infinity(pfc):
    law = pfc.scenario.computed_torque_pd
    H, c = [[2.0]], [0.5]
    free = lambda q: (-(3.0 * 0.0)) - 100.0 * (q - 0.0)
    for q, a_max, acc in ((1.0, 7.0, -7.0), (-1.0, 7.0, 7.0), (0.01, 7.0, free(0.01)), (1.0, INF, free(1.0)), (-1.0, INF, free(-1.0)),
                          (0.07, 7.0, -7.0), (-0.07, 7.0, 7.0)):
        tau = law([q], [0.0], H, c, 0.0, [0], [100.0], [3.0], [0.0], [[0.0]], None, [a_max])
        assert tau == [((0.0 + 2.0 * acc) + 0.5) + 0.0], (q, a_max)
    assert free(0.07) == -7.000000000000001 and law([0.07], [0.0], H, c, 0.0, [0], [100.0], [3.0], [0.0], [[0.0]], None, [7.0]) == \
        [((0.0 + 2.0 * -7.0) + 0.5) + 0.0]                                 # one ulp beyond the bound is clamped
    assert law([1.0], [0.0], H, c, 0.0, [0], [100.0], [3.0], [0.0], [[0.0]]) == law([1.0], [0.0], H, c, 0.0, [0], [100.0], [3.0],
                                                                                  [0.0], [[0.0]], None, [INF])


def test_law_without_actuated_coordinates_is_the_feed_forward(pfc):
    law = pfc.scenario.computed_torque_pd
    assert law([0.3, 0.1, 0.2], [1.0, 2.0, 3.0], H3, C3, 1.5, [], [], [], [0.0, 1.0], [[], []], [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]) == \
        [4.0, 5.0, 6.0]
    assert law([0.3, 0.1, 0.2], [1.0, 2.0, 3.0], H3, C3, 1.5, [], [], [], [0.0, 1.0], [[], []]) == [0.0, 0.0, 0.0]


def test_zero_product_keeps_the_written_zero(pfc):
    """The row sum starts from a written +0.0: with acc, c and the feed-forward all -0.0 the torque is +0.0, as on the device (a
    sum that started from its first product would give -0.0)."""
    import math
    law = pfc.scenario.computed_torque_pd
    tau = law([0.0], [0.0], [[1.0]], [-0.0], 0.0, [0], [0.0], [0.0], [0.0], [[0.0]], [[-0.0]])
    assert tau == [0.0] and math.copysign(1.0, tau[0]) == 1.0
