"""The pending call of a handle (pfc_context::Pending): an unchecked device-pointer call that is replaced, topped by
a surface call, followed by a zero-item evaluation, checked twice or drained by a debug reader, and the team slot it held.  One
handle per case, device-pointer entry points on torch tensors; "equal to a fresh handle" at the tolerances of
test_gpu_dual.py::test_one_handle_across_the_entry_points, counts exact.  Every call sequence is legal under include/pfc.h."""
import numpy as np
import pytest

import helpers as H
from test_gpu_multi import _dual_inputs

pytestmark = pytest.mark.gpu

ND = 6


class Dev:
    """A workload's inputs and two sets of outputs in device memory, and the device-pointer calls of one handle on them."""

    def __init__(self, pfc, w, m, seeds=(11, 12)):
        import torch
        self.pfc, self.w, self.m, self.n, self.torch = pfc, w, m, w.n_items, torch
        dev = torch.device("cuda:0")
        self.t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
        self.z = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.vin = [self.t(w.ins_ids, torch.int32), self.t(w.pose), self.t(w.twist), self.t(w.s)]
        self.seeds = [_dual_inputs(w, ND, s) for s in seeds]
        self.din = [[self.t(x) for x in sd] for sd in self.seeds]
        n = self.n
        # [wrench, sdot, d_wrench, d_sdot, counts], twice: what a call writes must not be what an earlier, replaced one wrote
        self.out = [[self.z(n, 6), self.z(n, 6), self.z(n, ND, 6), self.z(n, ND, 6), self.z(n, 4, dt=torch.int32)] for _ in range(2)]

    def value(self, k=0, n=None):
        o = self.out[k]
        self.m.eval_device(self.n if n is None else n, *[x.data_ptr() for x in self.vin], o[0].data_ptr(), o[1].data_ptr(), o[4].data_ptr(),
                           self.stream)

    def dual(self, k=0, n=None):
        o = self.out[k]
        self.m.eval_dual_device(self.n if n is None else n, ND, *[x.data_ptr() for x in self.vin], *[x.data_ptr() for x in self.din[0]],
                                *[x.data_ptr() for x in o], self.stream)

    def more(self, chunk=1, k=0):
        o = self.out[k]
        self.m.eval_dual_device_more(ND, *[x.data_ptr() for x in self.din[chunk]], o[2].data_ptr(), o[3].data_ptr(), self.stream)

    def checked(self, call, *a, **kw):
        """call + check(), re-issued while the check asks for it (work lists or a speculation that grew)."""
        for _ in range(40):
            call(*a, **kw)
            if self.m.check() == self.pfc._lib.OK:
                return
        pytest.fail("the evaluation did not settle")

    def more_is_refused(self):
        with pytest.raises(self.pfc._lib.PFCError) as e:
            self.more()
        assert e.value.status == self.pfc._lib.ERR_STATE, e.value

    def got(self, k=0):
        return [x.cpu().numpy() for x in self.out[k]]


def _close(got, ref, ks, what):
    tol = {0: 1e-11, 1: 1e-7, 2: 1e-9, 3: 1e-6}
    for k in ks:
        np.testing.assert_allclose(got[k], ref[k], rtol=tol[k], atol=tol[k] * max(np.abs(ref[k]).max(), 1e-300), err_msg=f"{what} {k}")


@pytest.fixture(scope="module")
def c1(pfc):
    """C1 and what fresh handles return for it: value, Dual of the first seed chunk, Dual of the second."""
    w = pfc.configs.c1_boxes()
    seeds = [_dual_inputs(w, ND, s) for s in (11, 12)]
    ref = []
    for sd in (None, seeds[0], seeds[1]):
        f = pfc.configs.build_scenario(w)
        ref.append(f.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids) if sd is None else
                   f.force_all_elastic_intersections_dual(w.pose, w.twist, w.s, *sd, w.ins_ids))
        f.close()
    return w, ref


@pytest.mark.parametrize("route", ["hand-over", "batched"])
def test_replaced_before_its_check(pfc, c1, route):
    """eval_dual_device unchecked, then eval_device into other outputs: the check judges the value evaluation alone and records
    no kept pass."""
    w, (ref_value, _, _) = c1
    m = pfc.configs.build_scenario(w)
    if route == "batched":
        m.set_option("fused", 0)
    d = Dev(pfc, w, m)
    d.checked(d.dual)
    assert m.last_team() == (1 if route == "hand-over" else 0)      # the route this handle's Dual evaluations take
    d.dual(0)
    d.value(1)
    assert m.check() == pfc._lib.OK
    got = d.got(1)
    assert np.array_equal(got[4], ref_value[2])
    _close(got, ref_value, (0, 1), route)
    d.more_is_refused()
    m.close()


def test_surface_on_top_of_dual_passes(pfc, c1):
    """A checked Dual evaluation, further Dual passes unchecked, then a surface call: the check is the surface call's."""
    import torch
    w, _ = c1
    f = pfc.configs.build_scenario(w)
    S = f.contact_surface(w.pose, w.twist, w.ins_ids)
    f.close()
    n, P, T = w.n_items, S.poly_idx.shape[0], S.trac.shape[0]
    assert P > 0 and T > 0
    m = pfc.configs.build_scenario(w)
    d = Dev(pfc, w, m)
    d.checked(d.dual)
    d.more()
    o = dict(off=d.z(n + 1, dt=torch.int64), idx=d.z(P, 3, dt=torch.int32), xyz=d.z(P, 8, 3), ptr=d.z(P + 1, dt=torch.int64), trac=d.z(T, 8),
             sm=d.z(n, 11), cnt=d.z(n, 4, dt=torch.int32), tot=d.z(2, dt=torch.int64))

    def surface(cap_poly, cap_trac):
        m.contact_surface_device(n, d.vin[0].data_ptr(), d.vin[1].data_ptr(), d.vin[2].data_ptr(), cap_poly, cap_trac, o["off"].data_ptr(),
                                 o["idx"].data_ptr(), o["xyz"].data_ptr(), o["ptr"].data_ptr(), o["trac"].data_ptr(), o["sm"].data_ptr(),
                                 o["cnt"].data_ptr(), o["tot"].data_ptr(), d.stream)

    # capacities of zero: only a check that judges the surface call asks for a re-issue (the Dual passes' check cannot)
    for _ in range(4):
        surface(0, 0)
        assert m.check() == pfc._lib.ERR_OVERFLOW
        if list(o["tot"].cpu().numpy()) == [P, T]:
            break
    else:
        pytest.fail("the surface call did not report its totals")
    d.checked(surface, P, T)
    assert list(o["tot"].cpu().numpy()) == [P, T]
    assert np.array_equal(o["off"].cpu().numpy(), S.poly_off) and np.array_equal(o["cnt"].cpu().numpy(), S.counts)
    d.more_is_refused()
    m.close()


@pytest.mark.parametrize("start", ["unchecked", "checked"])
@pytest.mark.parametrize("zero", ["value", "dual"])
def test_zero_items_is_an_evaluation(pfc, c1, start, zero):
    """A zero-item evaluation drops what was pending (a Dual evaluation on the hand-over route) and ends the kept pass."""
    w, _ = c1
    m = pfc.configs.build_scenario(w)
    d = Dev(pfc, w, m)
    d.checked(d.dual)
    assert m.last_team() == 1                                        # the hand-over route
    if start == "unchecked":
        d.dual()
    (d.value if zero == "value" else d.dual)(1, n=0)
    assert m.check() == pfc._lib.OK
    d.more_is_refused()
    m.close()


def test_check_twice(pfc, c1):
    """A second check() after a checked call of every kind returns OK and leaves stats() alone."""
    import torch
    w, _ = c1
    n = w.n_items
    m = pfc.configs.build_scenario(w)
    d = Dev(pfc, w, m)
    o = dict(off=d.z(n + 1, dt=torch.int64), ptr=d.z(1, dt=torch.int64), sm=d.z(n, 11), tot=d.z(2, dt=torch.int64))

    def surface():      # (capacities of zero: offsets, summary and totals only)
        m.contact_surface_device(n, d.vin[0].data_ptr(), d.vin[1].data_ptr(), d.vin[2].data_ptr(), 0, 0, o["off"].data_ptr(), 0, 0,
                                 o["ptr"].data_ptr(), 0, o["sm"].data_ptr(), 0, o["tot"].data_ptr(), d.stream)

    def again(what):
        before = m.stats()
        assert m.check() == pfc._lib.OK, what
        assert m.stats() == before, what

    d.checked(d.value); again("value")
    d.checked(d.dual); again("dual, hand-over")
    d.checked(d.dual); d.more(); assert m.check() == pfc._lib.OK; again("further Dual passes")
    surface(); m.check(); again("surface")
    m.set_option("fused", 0)
    d.checked(d.dual); again("dual, batched")
    m.close()


def test_debug_reader_judges_a_pending_dual_evaluation(pfc, c1):
    """pfc_debug_pairs with a Dual evaluation pending drains it completely: the check that follows has nothing left to judge, and
    the kept pass it recorded takes a further chunk."""
    w, (_, _, ref_second) = c1
    f = pfc.configs.build_scenario(w)
    f.set_option("debug", 1)
    f.force_all_elastic_intersections_dual(w.pose, w.twist, w.s, *_dual_inputs(w, ND, 11), w.ins_ids)
    want = H.sorted_pairs(*f.debug_pairs(0))
    f.close()
    m = pfc.configs.build_scenario(w)
    m.set_option("debug", 1)
    d = Dev(pfc, w, m)
    d.dual()
    got = H.sorted_pairs(*m.debug_pairs(0))
    assert len(want[0]) > 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert m.check() == pfc._lib.OK
    d.more(chunk=1)
    assert m.check() == pfc._lib.OK
    _close(d.got(), ref_second, (2, 3), "second chunk")
    m.close()


def test_team_slot_is_released_by_the_drop(pfc):
    """A team launch left unchecked and replaced by a surface call gives its device's team slot back: another handle gets its
    team, and so does this one afterwards."""
    import torch
    w = pfc.configs.c3_blob_tool(2, n_div_blob=6, n_div_tool=4)
    n = w.n_items
    f = pfc.configs.build_scenario(w)
    f.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    team = f.last_team()
    S = f.contact_surface(w.pose, w.twist, w.ins_ids)
    f.close()
    assert team > 1
    P, T = S.poly_idx.shape[0], S.trac.shape[0]
    m, m2 = pfc.configs.build_scenario(w), pfc.configs.build_scenario(w)
    d, d2 = Dev(pfc, w, m), Dev(pfc, w, m2)
    o = dict(off=d.z(n + 1, dt=torch.int64), idx=d.z(P, 3, dt=torch.int32), xyz=d.z(P, 8, 3), ptr=d.z(P + 1, dt=torch.int64), trac=d.z(T, 8),
             sm=d.z(n, 11), tot=d.z(2, dt=torch.int64))
    d.value()                                                        # holds the slot until it is checked or dropped
    d.checked(m.contact_surface_device, n, d.vin[0].data_ptr(), d.vin[1].data_ptr(), d.vin[2].data_ptr(), P, T, o["off"].data_ptr(),
              o["idx"].data_ptr(), o["xyz"].data_ptr(), o["ptr"].data_ptr(), o["trac"].data_ptr(), o["sm"].data_ptr(), 0, o["tot"].data_ptr(),
              d.stream)
    assert list(o["tot"].cpu().numpy()) == [P, T]
    d2.checked(d2.value)
    assert m2.last_team() == team
    d.checked(d.value)
    assert m.last_team() == team
    m.close(); m2.close()
