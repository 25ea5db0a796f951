"""Continuous joint feedback (pfc_feedback_device, pfc_feedback_dual_device, pfc_radau_set_feedback, pfc_radau_clear_feedback,
pfc_radau_stage_times): the symbols, and the scalar statements of include/pfc.h in Python floats (scenario.feedback_pd,
scenario.feedback_pd_partials).  tests/test_gpu_feedback.py compares the device with these statements in bytes."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAMES = [("pfc_feedback_device", 21), ("pfc_feedback_dual_device", 23), ("pfc_radau_set_feedback", 10), ("pfc_radau_clear_feedback", 1),
         ("pfc_radau_stage_times", 2)]


def test_feedback_symbols_are_declared_exported_and_bound(pfc):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfc.h")).read(), flags=re.S)
    for name, n_args in NAMES:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        res, args = pfc._lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, name
    sig = pfc._lib.SIGNATURES
    assert sig["pfc_feedback_device"][1][1:6] == [C.c_int] * 5 and sig["pfc_feedback_device"][1][6] is C.c_void_p
    assert sig["pfc_feedback_dual_device"][1][1:7] == [C.c_int] * 6 and sig["pfc_feedback_dual_device"][1][7] is C.c_void_p
    assert sig["pfc_radau_set_feedback"][1][1] is C.c_int and sig["pfc_radau_set_feedback"][1][6] is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", pfc._lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pfc_[a-z_0-9]+)", out))
    assert {name for name, _ in NAMES} <= exported
    M = pfc.scenario.MechanismScenario
    for meth in ("radau_set_feedback", "radau_clear_feedback", "radau_stage_times", "feedback_device", "feedback_dual_device"):
        assert callable(getattr(M, meth)), meth
    import inspect
    assert "continuous_controller" in inspect.signature(M.integrate_scenario_radau).parameters
    src = open(os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc", "pfc_feedback.h")).read()
    assert "fma(" not in src and "__shared__" not in src and "atomic" not in src.split("#pragma once")[1]


# ---- the value ------------------------------------------------------------------------------------------------------------------
H3 = [[2.0, 0.5, 0.25], [0.5, 3.0, 0.125], [0.25, 0.125, 4.0]]
C3 = [0.1, -0.2, 0.3]
LAW = dict(act=[0, 2], kp=[10.0, 20.0], kd=[1.0, 2.0], seg_t=[123.0, 1.0, 2.0], seg_q=[[0.0, 0.0], [0.1, 0.1], [0.2, -0.2]])
FF = [[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [-1.0, -2.0, -3.0]]
Q, V = [0.3, -0.1, 0.2], [1.0, 2.0, -0.5]


def _bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


@pytest.mark.parametrize("t", [-5.0, 1.0, 1.9999999999999998, 2.0])
@pytest.mark.parametrize("ff", [None, FF])
@pytest.mark.parametrize("a_max", [None, [0.5, INF]])
def test_without_tau_in_the_law_is_computed_torque_pd_in_bits(pfc, t, ff, a_max):
    S = pfc.scenario
    assert _bits(S.feedback_pd(Q, V, H3, C3, t, None, seg_ff=ff, a_max=a_max, **LAW)) == \
        _bits(S.computed_torque_pd(Q, V, H3, C3, t, seg_ff=ff, a_max=a_max, **LAW))


def test_tau_in_is_added_behind_the_law_and_copied_where_there_is_none(pfc):
    S = pfc.scenario
    tau_in = [0.25, -0.0, -1.5]
    law = S.computed_torque_pd(Q, V, H3, C3, 1.0, seg_ff=FF, **LAW)
    assert S.feedback_pd(Q, V, H3, C3, 1.0, tau_in, seg_ff=FF, **LAW) == [law[0] + 0.25, 2.0 + -0.0, law[2] + -1.5]
    law = S.computed_torque_pd(Q, V, H3, C3, 1.0, **LAW)
    out = S.feedback_pd(Q, V, H3, C3, 1.0, tau_in, **LAW)
    assert out == [law[0] + 0.25, 0.0, law[2] + -1.5]
    assert math.copysign(1.0, out[1]) == -1.0                               # copied: 0.0 + -0.0 would be +0.0
    assert math.copysign(1.0, S.feedback_pd(Q, V, H3, C3, 1.0, None, **LAW)[1]) == 1.0
    # no actuated coordinate: the feed-forward plus tau_in, or tau_in itself
    none = dict(act=[], kp=[], kd=[], seg_t=[0.0], seg_q=[[]])
    assert S.feedback_pd(Q, V, H3, C3, 0.0, tau_in, seg_ff=[[1.0, 0.0, 3.0]], **none) == [1.25, 0.0, 1.5]
    assert _bits(S.feedback_pd(Q, V, H3, C3, 0.0, tau_in, **none)) == _bits(tau_in)


# ---- the partials ---------------------------------------------------------------------------------------------------------------
def _dyadic(rng, shape, bits, scale):
    """Multiples of 2^-bits in [-scale, scale]."""
    return np.round(rng.uniform(-scale, scale, shape) * 2.0 ** bits) / 2.0 ** bits


def _case(n_act, clamp, seed):
    """Random inputs, nv = n_act + 2.  q, v, the setpoints and the seeds are multiples of 2^-10 below 4 and the gains multiples of
    2^-4 below 256, so that e, kd v, kp e, acc and dacc are exact in doubles (at most 28 significant bits each): the only rounded
    operations are those of the H acc chain, whose factors H, dH and the addend dc are full random doubles."""
    rng = np.random.default_rng(seed)
    nv = n_act + 2
    act = sorted(rng.permutation(nv)[:n_act].tolist())
    d = dict(q=_dyadic(rng, nv, 10, 4.0), v=_dyadic(rng, nv, 10, 4.0), dq=_dyadic(rng, nv, 10, 4.0), dv=_dyadic(rng, nv, 10, 4.0),
             H=rng.standard_normal((nv, nv)), dH=rng.standard_normal((nv, nv)), dc=rng.standard_normal(nv),
             kp=np.abs(_dyadic(rng, n_act, 4, 256.0)), kd=np.abs(_dyadic(rng, n_act, 4, 256.0)), seg_q=_dyadic(rng, (2, n_act), 10, 4.0))
    raw = [(-(d["kd"][a] * d["v"][co])) - d["kp"][a] * (d["q"][co] - d["seg_q"][1][a]) for a, co in enumerate(act)]
    a_max = None
    if clamp:      # entry 0 clamped (half its raw magnitude, a dyadic number itself), the others far from their bound
        a_max = [abs(raw[0]) / 2.0 if abs(raw[0]) > 0 else 1.0] + [2.0 ** 40] * (n_act - 1)
    return act, d, a_max, raw


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("n_act", [1, 2, 5])
def test_partials_against_the_analytic_derivative_in_50_digits(pfc, n_act, clamp):
    """dtau_a = sum_b (dH[a][b] acc_b + H[a][b] dacc_b) + dc_a with acc_b clamped and dacc_b = -kd_b dv_b - kp_b dq_b, 0 where
    clamped, evaluated with mpmath at 50 digits.  The bound: dtau_a is a recursive sum of 2 n_act products plus one add -- every
    term passes one product rounding, one pair add, at most n_act chain adds (the first, to a written 0, is exact) and the add of
    dc, n_act + 2 <= 2 n_act + 2 roundings -- so its error is at most (2 n_act + 2) 2^-53 sum |terms|.  acc and dacc carry no
    error of their own on these inputs (_case)."""
    import mpmath
    mpmath.mp.dps = 50
    mpf = mpmath.mpf
    S = pfc.scenario
    worst = 0.0
    for seed in range(20):
        act, d, a_max, raw = _case(n_act, clamp, 100 * n_act + seed)
        nv = n_act + 2
        got = S.feedback_pd_partials(d["q"].tolist(), d["v"].tolist(), d["H"].tolist(), 0.5, d["dq"].tolist(), d["dv"].tolist(),
                                     d["dH"].tolist(), d["dc"].tolist(), act, d["kp"].tolist(), d["kd"].tolist(), [0.0, 0.25],
                                     d["seg_q"].tolist(), a_max)
        acc, dacc = [], []
        for a, co in enumerate(act):
            x = -(mpf(d["kd"][a]) * mpf(d["v"][co])) - mpf(d["kp"][a]) * (mpf(d["q"][co]) - mpf(d["seg_q"][1][a]))
            dx = -(mpf(d["kd"][a]) * mpf(d["dv"][co])) - mpf(d["kp"][a]) * mpf(d["dq"][co])
            assert x == mpf(raw[a])                                         # exact in doubles, as _case says
            if a_max is not None and abs(x) > mpf(a_max[a]):
                x, dx = mpmath.sign(x) * mpf(a_max[a]), mpf(0)
            acc.append(x); dacc.append(dx)
        assert (a_max is not None) == (dacc[0] == 0 and clamp)
        for i in range(nv):
            if i not in act:
                assert got[i] == 0.0 and math.copysign(1.0, got[i]) == 1.0
                continue
            terms = [mpf(d["dH"][i][cb]) * acc[b] for b, cb in enumerate(act)] + [mpf(d["H"][i][cb]) * dacc[b] for b, cb in enumerate(act)]
            terms.append(mpf(d["dc"][i]))
            ref, mag = mpmath.fsum(terms), mpmath.fsum(abs(x) for x in terms)
            bound = (2 * n_act + 2) * mpf(2) ** -53 * mag
            err = abs(mpf(got[i]) - ref)
            worst = max(worst, float(err / bound))
            assert err <= bound, (seed, i, float(err), float(bound))
    print("n_act", n_act, "clamp", clamp, "largest error / bound", worst)


@pytest.mark.parametrize("n_act", [1, 2, 5])
def test_the_partial_with_respect_to_a_clamped_coordinate_is_exactly_zero(pfc, n_act):
    """Directions that seed q or v of the clamped coordinate alone, with H and c held (dH = 0, dc = 0): every entry of dtau is
    exactly +0.0 -- the clamp has cut the only path from that coordinate to the torque.  The same seeds on a handle without the
    clamp give a non-zero partial: the zero is the clamp's."""
    S = pfc.scenario
    act, d, a_max, raw = _case(n_act, True, 7 + n_act)
    nv = n_act + 2
    zH, zc = np.zeros((nv, nv)).tolist(), [0.0] * nv
    args = lambda dq, dv, am: (d["q"].tolist(), d["v"].tolist(), d["H"].tolist(), 0.5, dq, dv, zH, zc, act, d["kp"].tolist(), d["kd"].tolist(),
                               [0.0, 0.25], d["seg_q"].tolist(), am)
    unit = [1.0 if i == act[0] else 0.0 for i in range(nv)]
    for dq, dv in ((unit, None), (None, unit), (unit, unit)):
        got = S.feedback_pd_partials(*args(dq, dv, a_max))
        assert _bits(got) == _bits([0.0] * nv), got
        free = S.feedback_pd_partials(*args(dq, dv, None))
        assert free[act[0]] != 0.0
    if n_act > 1:      # a coordinate that is not clamped still reaches the clamped coordinate's torque through H
        other = [1.0 if i == act[1] else 0.0 for i in range(nv)]
        got = S.feedback_pd_partials(*args(other, None, a_max))
        assert got[act[0]] != 0.0 and got[act[1]] != 0.0
