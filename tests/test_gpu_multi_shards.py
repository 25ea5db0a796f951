"""Multi-device handles with 3 and 8 shards (pfc_create_multi over [0] * K: K shard contexts on the one visible device).

tests/test_gpu_multi.py builds every handle over {0, 0}; with two shards the cut loop of the partition stops at its first
boundary, no shard is ever idle beside a working one and no staging offset of a shard k >= 2 is taken.  Here K is 3 and 8, the
workloads are small, and every result is held against the single-device handle on the same inputs (counters bit-equal, wrench
1e-9 -- 1e-6 on the pile --, sdot 1e-6 -- not on the pile --, wrench partials 1e-6 and sdot partials 1e-5 of the item's largest
partial; the pile's Dual partials under the rule of test_gpu_multi.py::test_multi_handle_dual_host_buffers: flat face-to-face
patches carry rounding noise along the clamped null direction of their stiffness, so every item without contact and 95 % of
those with contact are held to 1e-6) and sampled items against the CPU oracle.  After every evaluation pfc_last_shard_bounds
must equal the partition rule as tests/partition_reference.py states it, fed with what multi_partition is documented to feed it
(Expect below): a wrong range is otherwise silent -- an item no shard evaluates keeps what the caller's buffer held, so every
output buffer starts as NaN / -1.

Everything except hipMemcpyPeerAsync itself runs: distinct devices, peer copies and the scaling curve are NOT validated here."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import helpers as H
import partition_reference as P
from test_gpu_multi import _close, _dual_inputs, _nearby_pose
from test_gpu_ownership import _ALLOC, _FREE

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
KS = (3, 8)
N_DIR = 3


def _per_item(pfc, w):
    """The same items with one instruction PER ITEM, so that a call may leave ins_ids out (item i is instruction i)."""
    return pfc.configs.Workload(w.name + ", an instruction per item", w.meshes, [w.instructions[int(i)] for i in w.ins_ids],
                                np.arange(w.n_items, dtype=np.int32), w.pose, w.twist, w.s)


WORKLOADS = {
    "c4": lambda pfc: pfc.configs.c2_box_on_plane(64, montecarlo=True),
    "c3": lambda pfc: pfc.configs.c3_blob_tool(40, n_div_blob=6, n_div_tool=4),
    "c3_item": lambda pfc: _per_item(pfc, pfc.configs.c3_blob_tool(40, n_div_blob=6, n_div_tool=4)),
    "pile": lambda pfc: pfc.configs.c5_pile(n_side=3),
    "volvol": lambda pfc: pfc.configs.vol_vol(12, n_div=3, model="bristle"),
}
_REF = {}


def _ref(pfc, name):
    """The workload, its Dual seeds and broadphase pose, and what the single-device handle gives for them: made once, never changed."""
    if name not in _REF:
        w = WORKLOADS[name](pfc)
        r = SimpleNamespace(w=w, name=name, seeds={"A": _dual_inputs(w, N_DIR, 31), "B": _dual_inputs(w, N_DIR, 32)},
                            bp=_nearby_pose(w, 5, scale=8e-3 if name == "c4" else 2e-2), iota=bool(np.array_equal(w.ins_ids, np.arange(w.n_items))))
        m = pfc.configs.build_scenario(w)
        r.value = m.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
        r.dual = {k: m.force_all_elastic_intersections_dual(w.pose, w.twist, w.s, *sd, w.ins_ids) for k, sd in r.seeds.items()}
        r.dual_bp = m.force_all_elastic_intersections_dual(w.pose, w.twist, w.s, *r.seeds["A"], w.ins_ids, bp_pose=r.bp)
        r.L = m.local_jacobian(w.pose, w.twist, w.s, w.ins_ids)[2]
        m.close()
        assert (r.value[2][:, 3] > 0).any(), name
        assert not np.array_equal(r.dual_bp[4], r.value[2]), "the broadphase pose does not change the candidate sets of " + name
        r.items = sorted({0, 1, w.n_items // 3, w.n_items // 2, w.n_items - 2, w.n_items - 1})
        r.oracle = dict(zip(r.items, H.oracle_run(pfc, w, items=r.items, debug=False)))
        for a in (*r.value, *r.dual_bp, r.L, *(x for d in r.dual.values() for x in d)):
            a.setflags(write=False)
        _REF[name] = r
    return _REF[name]


class Expect:
    """The bounds a multi-device handle must report: tests/partition_reference.py fed the way multi_partition feeds
    csrc/pfc_partition.h.  The list of an evaluation is (n, ids or none, host- or device-pointer entry point); the host-pointer
    entry points also compare the ids.  Costs are the counters of the previous evaluation while the list is the one the ranges
    were cut for and that evaluation succeeded, else the leaf-count products (64 each where the ids are device data)."""

    def __init__(self, w, K, min_items=8):
        self.leaves = [int((np.asarray(ms.tree.child)[:, 0] < 0).sum()) for ms in w.meshes]
        self.ins = [(c.id_1, c.id_2) for c in w.instructions]
        self.part, self.counts = P.Partitioner(K, min_items), None

    def leaf_costs(self, n, ids):
        idx = range(n) if ids is None else [int(i) for i in ids]
        return [P.cost_leaves(self.leaves[self.ins[k][0]], self.leaves[self.ins[k][1]]) if 0 <= k < len(self.ins) else P.cost_leaves(0, 0)
                for k in idx]

    def step(self, n, ids=None, dev=False, dev_ids=False):
        """Before (or after) the call, ahead of done(): (bound[0 .. n_used], whether the previous ranges were kept)."""
        key = (n, dev, dev_ids if dev else ids is not None, None if dev or ids is None else tuple(int(i) for i in ids))
        if self.part.key == key and self.counts is not None:
            cost = [P.cost_counters(int(a), int(b)) for a, b in self.counts[:n, :2]]
        elif dev and dev_ids:
            cost = [P.cost_leaves(0, 0)] * n
        else:
            cost = self.leaf_costs(n, ids)
        self.cost = cost
        return self.part.step(key, cost)

    def done(self, counts):
        """The counters the evaluation returned; None: it failed."""
        self.counts = None if counts is None else np.array(counts)


def _bounds(m, ex, n, **step):
    """last_shard_bounds() against the statement; the ranges are a partition of [0, n)."""
    want, kept = ex.step(n, **step)
    got = m.last_shard_bounds()
    assert got == want, (got, want, kept)
    assert got[0] == 0 and got[-1] == n and all(a < b for a, b in zip(got, got[1:])), got
    assert m.last_shards() == len(got) - 1
    return got, kept


# ---- raw calls with pre-filled outputs ------------------------------------------------------------------------------
def _c(a, dt=np.float64):
    return None if a is None else np.ascontiguousarray(a, dtype=dt)


def _host_eval(pfc, m, ids, pose, twist, s):
    n, p = pose.shape[0], H._ptr
    wr, sd, ct = np.full((n, 6), np.nan), np.full((n, 6), np.nan), np.full((n, 4), -1, dtype=np.int32)
    m._check(pfc._lib.lib().pfc_eval(m._h, n, p(_c(ids, np.int32)), p(_c(pose)), p(_c(twist)), p(_c(s)), p(wr), p(sd), p(ct)))
    return wr, sd, ct


def _host_dual(pfc, m, ids, pose, twist, s, seeds, bp=None):
    n, p = pose.shape[0], H._ptr
    wr, sd, ct = np.full((n, 6), np.nan), np.full((n, 6), np.nan), np.full((n, 4), -1, dtype=np.int32)
    dw, dsd = np.full((n, N_DIR, 6), np.nan), np.full((n, N_DIR, 6), np.nan)
    m._check(pfc._lib.lib().pfc_eval_dual_bp(m._h, n, N_DIR, p(_c(ids, np.int32)), p(_c(pose)), p(_c(bp)), p(_c(twist)), p(_c(s)),
                                             *[p(_c(a)) for a in seeds], p(wr), p(sd), p(dw), p(dsd), p(ct)))
    return wr, sd, dw, dsd, ct


def _filled(*arrays):
    for a in arrays:
        assert not (np.isnan(a).any() if a.dtype.kind == "f" else (a < 0).any()), "a range of the output was not written"


def _check_value(name, got, want, idx=slice(None)):
    wr, sd, ct = got
    _filled(wr, sd, ct)
    assert np.array_equal(ct, want[2][idx]), name
    _close(wr, want[0][idx], 1e-6 if name == "pile" else 1e-9)
    if name != "pile":      # (the pile's sdot of sliver patches: the 1e-3 rule of tests/test_gpu_scale.py, not a matter of the shards)
        _close(sd, want[1][idx], 1e-6)


def _check_partials(name, dw, dsd, rdw, rdsd, counts):
    _filled(dw, dsd)
    sw = np.abs(rdw).max(axis=(1, 2), keepdims=True) + 1e-300
    ok = (np.abs(dw - rdw) <= 1e-6 * sw).all(axis=(1, 2))
    if name == "pile":
        contact = counts[:, 3] > 0
        assert ok[~contact].all() and ok[contact].mean() > 0.95, (name, np.nonzero(~ok)[0])
        return
    assert ok.all(), (name, np.nonzero(~ok)[0])
    ss = np.abs(rdsd).max(axis=(1, 2), keepdims=True) + 1e-300
    assert (np.abs(dsd - rdsd) <= 1e-5 * ss).all(), name


def _check_dual(name, got, want):
    wr, sd, dw, dsd, ct = got
    _check_value(name, (wr, sd, ct), (want[0], want[1], want[4]))
    _check_partials(name, dw, dsd, want[2], want[3], want[4])


def _check_oracle(r, wr, sd, ct):
    for k, o in r.oracle.items():
        assert np.array_equal(ct[k], o.counts), (r.name, k)
        if np.linalg.norm(o.wrench) > 0:
            assert H.rel_err(wr[k], o.wrench) < (1e-6 if r.name == "pile" else 1e-9), (r.name, k)
        if r.name != "pile" and np.linalg.norm(o.sdot) > 0:
            assert H.rel_err(sd[k], o.sdot) < 1e-6, (r.name, k)


# ---- host-pointer entry points ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", sorted(WORKLOADS))
def test_host_pointer_value_and_dual(pfc, name, K):
    """pfc_eval, pfc_eval_dual_bp without and with a broadphase pose, three evaluations each, ins_ids given and (where item i is
    instruction i) None; then the same items in reverse order: another list of the same length, leaf-product costs again."""
    r = _ref(pfc, name)
    w, n = r.w, r.w.n_items
    m = pfc.configs.build_scenario(w, devices=[0] * K)
    ex = Expect(w, K)
    for ids in (w.ins_ids, None) if r.iota else (w.ins_ids,):
        first = True
        for call in ("value", "dual", "dual_bp"):
            hist = []
            for rep in range(3):
                if call == "value":
                    got = _host_eval(pfc, m, ids, w.pose, w.twist, w.s)
                    _check_value(name, got, r.value)
                    _check_oracle(r, *got)
                else:
                    want = r.dual_bp if call == "dual_bp" else r.dual["A"]
                    got = _host_dual(pfc, m, ids, w.pose, w.twist, w.s, r.seeds["A"], r.bp if call == "dual_bp" else None)
                    _check_dual(name, got, want)
                b, kept = _bounds(m, ex, n, ids=ids)
                assert len(b) - 1 == min(K, n // 8)
                if first:      # a list this handle has not seen: cut by the leaf-count products
                    assert not kept and ex.cost == ex.leaf_costs(n, ids)
                    first = False
                ex.done(got[-1])
                hist.append(b)
            assert hist[2] == hist[1]      # the same counters twice: the ranges stay
    rev = w.ins_ids[::-1]
    if not np.array_equal(rev, w.ins_ids):
        got = _host_eval(pfc, m, rev, w.pose[::-1], w.twist[::-1], w.s[::-1])
        _check_value(name, got, r.value, slice(None, None, -1))
        b, kept = _bounds(m, ex, n, ids=rev)
        assert not kept and ex.cost == ex.leaf_costs(n, rev)
        ex.done(got[2])
    m.close()


def test_partly_used_handles(pfc):
    """K = 8 and multi_min = 8: 20 items use two shards and leave six idle, 200 use all, 20 again two; pfc_get_stats counts the
    used shards only.  multi_min = 1: three items on three shards, one item on one."""
    r = _ref(pfc, "pile")
    w = r.w
    m = pfc.configs.build_scenario(w, devices=[0] * 8)
    ex = Expect(w, 8)

    def run(n, ids_given, shards):
        ids = w.ins_ids[:n] if ids_given else None
        got = _host_eval(pfc, m, ids, w.pose[:n], w.twist[:n], w.s[:n])
        _check_value("pile", got, r.value, slice(0, n))
        b, _ = _bounds(m, ex, n, ids=ids)
        ex.done(got[2])
        assert len(b) - 1 == shards == m.last_shards()
        st = m.stats()
        assert st["n_items"] == n and st["node_tests"] == int(got[2][:, 0].sum()) and st["candidates"] == int(got[2][:, 1].sum()), (n, st)
        return b

    for ids_given in (True, False):
        for n, shards in ((20, 2), (200, 8), (20, 2), (20, 2), (351, 8), (23, 2)):
            run(n, ids_given, shards)
    m.set_option("multi_min", 1); ex.part.set_min_items(1)
    assert run(3, True, 3) == [0, 1, 2, 3]
    assert run(1, True, 1) == [0, 1]
    assert run(7, False, 7) == list(range(8))
    assert len(run(9, True, 8)) == 9
    m.close()


def _dominated(pfc, where, n_box=40):
    """40 box-on-plane items (108-tet boxes) and ONE reduced blob-tool item (2 880 tets against 1 280 triangles: it outweighs a
    shard's share by its leaf-count product and by its counters): first, in the middle or last."""
    Cf = pfc.configs
    box, blob = Cf.c2_box_on_plane(n_box, montecarlo=True, n_div=3), Cf.c3_blob_tool(1, n_div_blob=12, n_div_tool=8)
    meshes = list(box.meshes) + list(blob.meshes)
    b = blob.instructions[0]
    ins = [box.instructions[0], Cf.InsSpec(b.id_1 + 2, b.id_2 + 2, "bristle", chi=b.chi, mu_d=b.mu_d, tau=b.tau, k_bar=b.k_bar, magic=b.magic)]
    at = {"first": 0, "middle": n_box // 2, "last": n_box}[where]
    ins_ids = np.insert(np.zeros(n_box, dtype=np.int32), at, 1).astype(np.int32)
    cat = lambda a, c: np.ascontiguousarray(np.insert(a, at, c[0], axis=0))
    return Cf.Workload("one dominating item, " + where, meshes, ins, ins_ids, cat(box.pose, blob.pose), cat(box.twist, blob.twist),
                       cat(box.s, blob.s)), at


def _unclamped(cost, ku):
    """Where the half-item rule alone would put the boundaries."""
    total, acc, i, out = sum(cost), 0.0, 0, [0]
    for k in range(1, ku):
        while i < len(cost) and acc + 0.5 * cost[i] < total * k / ku:
            acc += cost[i]; i += 1
        out.append(i)
    return out + [len(cost)]


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_dominating_item(pfc, where):
    """The contiguous cut when one item outweighs a shard's share: its range is that item alone, the clamps (every used shard gets
    an item) move the boundaries the half-item rule piles up on it in the first cut, the 15 % rule never holds, and cutting again under the
    same costs gives the same ranges.  Results are the single handle's."""
    w, at = _dominated(pfc, where)
    n = w.n_items
    m1 = pfc.configs.build_scenario(w)
    ref = m1.force_all_elastic_intersections(w.pose, w.twist, w.s, w.ins_ids)
    m1.close()
    assert ref[2][at, 3] > 0 and (ref[2][:, 3] > 0).sum() > n // 2
    m = pfc.configs.build_scenario(w, devices=[0] * 8)
    ex = Expect(w, 8)
    hist = []
    for rep in range(3):
        got = _host_eval(pfc, m, w.ins_ids, w.pose, w.twist, w.s)
        _check_value(w.name, got, ref)
        b, kept = _bounds(m, ex, n, ids=w.ins_ids)
        ku = len(b) - 1
        assert ku == n // 8 == 5 and not kept
        assert max(ex.cost) == ex.cost[at] > sum(ex.cost) / ku                  # the item outweighs a shard's share
        assert at in b and at + 1 in b                                          # ... and is a range of its own
        if rep == 0:      # by leaf products the item is worth four shares: several boundaries land on it and are moved by the clamps
            assert ex.cost[at] > 4 * sum(ex.cost) / ku and _unclamped(ex.cost, ku) != b, "the clamps do not bind in this case"
        assert not P.keeps(ex.cost, b + [n] * (8 - ku), ku)
        ex.done(got[2])
        hist.append(b)
    assert hist[2] == hist[1]      # (the second and third cut see the same counters)
    m.close()


# ---- device-pointer entry points ----------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _t(a, dt=None):
    torch = _torch()
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt or torch.float64, device=torch.device("cuda", 0))


def _full(shape, value, dt=None):
    torch = _torch()
    return torch.full(shape, value, dtype=dt or torch.float64, device=torch.device("cuda", 0))


class DeviceCalls:
    """The device-pointer entry points of one handle over one workload's buffers on device 0; every evaluation is re-issued while
    pfc_check answers PFC_ERR_OVERFLOW (the lists of a fresh handle grow), and every issue is a partition of its own."""

    def __init__(self, pfc, r, m, ex):
        torch = _torch()
        self.pfc, self.r, self.m, self.ex, self.n = pfc, r, m, ex, r.w.n_items
        w = r.w
        self.T = dict(ids=_t(w.ins_ids, torch.int32), pose=_t(w.pose), twist=_t(w.twist), s=_t(w.s), bp=_t(r.bp))
        self.S = {k: [_t(a) for a in sd] for k, sd in r.seeds.items()}
        self.st = torch.cuda.current_stream().cuda_stream

    def _issue(self, call, use_ids, counts_back):
        """-> the bounds of the issue that pfc_check accepted."""
        for attempt in range(40):
            call()
            b, _ = _bounds(self.m, self.ex, self.n, dev=True, dev_ids=use_ids)
            ok = self.m.check() == self.pfc._lib.OK
            self.ex.done(counts_back if ok else None)
            if ok:
                return b
        raise AssertionError("the evaluation did not settle")

    def value(self, use_ids, use_counts, pose=None, ids=None):
        torch, T, n = _torch(), self.T, self.n
        o = dict(w=_full((n, 6), np.nan), sd=_full((n, 6), np.nan), c=_full((n, 4), -1, torch.int32))
        pose = T["pose"] if pose is None else pose
        ids = T["ids"] if ids is None else ids
        b = self._issue(lambda: self.m.eval_device(n, ids.data_ptr() if use_ids else 0, pose.data_ptr(), T["twist"].data_ptr(), T["s"].data_ptr(),
                                                   o["w"].data_ptr(), o["sd"].data_ptr(), o["c"].data_ptr() if use_counts else 0, self.st),
                        use_ids, self.r.value[2])
        got = {k: v.cpu().numpy() for k, v in o.items()}
        return (got["w"], got["sd"], got["c"] if use_counts else np.array(self.r.value[2])), b

    def dual(self, use_ids, use_counts, seeds, bp):
        torch, T, n = _torch(), self.T, self.n
        o = dict(w=_full((n, 6), np.nan), sd=_full((n, 6), np.nan), dw=_full((n, N_DIR, 6), np.nan), dsd=_full((n, N_DIR, 6), np.nan),
                 c=_full((n, 4), -1, torch.int32))
        want = self.r.dual_bp if bp else self.r.dual[seeds]
        S = self.S[seeds]
        b = self._issue(lambda: self.m.eval_dual_device(n, N_DIR, T["ids"].data_ptr() if use_ids else 0, T["pose"].data_ptr(), T["twist"].data_ptr(),
                                                        T["s"].data_ptr(), S[0].data_ptr(), S[1].data_ptr(), S[2].data_ptr(), o["w"].data_ptr(),
                                                        o["sd"].data_ptr(), o["dw"].data_ptr(), o["dsd"].data_ptr(),
                                                        o["c"].data_ptr() if use_counts else 0, self.st, d_bp_pose=T["bp"].data_ptr() if bp else 0),
                        use_ids, want[4])
        got = {k: v.cpu().numpy() for k, v in o.items()}
        return (got["w"], got["sd"], got["dw"], got["dsd"], got["c"] if use_counts else np.array(want[4])), b

    def more(self, seeds):
        n, S = self.n, self.S[seeds]
        dw, dsd = _full((n, N_DIR, 6), np.nan), _full((n, N_DIR, 6), np.nan)
        self.m.eval_dual_device_more(N_DIR, S[0].data_ptr(), S[1].data_ptr(), S[2].data_ptr(), dw.data_ptr(), dsd.data_ptr(), self.st)
        assert self.m.check() == self.pfc._lib.OK
        return dw.cpu().numpy(), dsd.cpu().numpy()

    def jacobian(self):
        L = _full((self.n, 12, 36), np.nan)
        self.m.local_jacobian_device(L.data_ptr(), self.st)
        assert self.m.check() == self.pfc._lib.OK
        return L.cpu().numpy()


def _ranges(b):
    return [slice(lo, hi) for lo, hi in zip(b, b[1:])]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", sorted(WORKLOADS))
def test_device_pointer_entry_points(pfc, name, K):
    """pfc_eval_device, pfc_eval_dual_device[_bp], pfc_eval_dual_device_more twice and pfc_local_jacobian_device, each followed by
    pfc_check, with d_ins_ids given and NULL (shards k >= 2 read their ids from the shard's iota at its first item) and d_counts
    given and NULL; every range of every result against the single-device handle.  A value evaluation ends the Dual reuse."""
    r = _ref(pfc, name)
    L = pfc._lib
    m = pfc.configs.build_scenario(r.w, devices=[0] * K)
    ex = Expect(r.w, K)
    D = DeviceCalls(pfc, r, m, ex)
    for use_ids in (True, False) if r.iota else (True,):
        for use_counts in (True, False):
            got, b = D.value(use_ids, use_counts)
            for rg in _ranges(b):
                _check_value(name, tuple(a[rg] for a in got), r.value, rg)
            st = m.stats()
            assert st["candidates"] == int(r.value[2][:, 1].sum()) and st["node_tests"] == int(r.value[2][:, 0].sum()) and st["n_items"] == D.n
            if use_counts:
                got, b = D.dual(use_ids, True, "A", bp=True)
                _check_dual(name, got, r.dual_bp)
            got, b = D.dual(use_ids, use_counts, "A", bp=False)
            want = r.dual["A"]
            for rg in _ranges(b):
                _check_dual(name, tuple(a[rg] for a in got), tuple(a[rg] for a in want))
            assert m.last_shard_bounds() == b
            for seeds in ("B", "A"):      # two further chunks on the kept partition
                dw, dsd = D.more(seeds)
                assert m.last_dual_reused() and m.last_shard_bounds() == b
                for rg in _ranges(b):
                    _check_partials(name, dw[rg], dsd[rg], r.dual[seeds][2][rg], r.dual[seeds][3][rg], want[4][rg])
            Lj = D.jacobian()
            assert m.last_shard_bounds() == b
            for rg in _ranges(b):      # rows 0..5: the wrench's partials, rows 6..11: sdot's
                _check_partials(name, Lj[rg, :6], Lj[rg, 6:], r.L[rg, :6], r.L[rg, 6:], want[4][rg])
            D.value(use_ids, use_counts)      # a value evaluation in between: nothing is kept any more
            for call in (lambda: D.more("B"), D.jacobian):
                with pytest.raises(L.PFCError) as ei:
                    call()
                assert ei.value.status == L.ERR_STATE
    m.close()


# ---- debug views and errors ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_debug_views_and_errors_in_every_shard(pfc, K):
    """pfc_debug_pairs / pfc_debug_tractions of an item in the first, a middle and the last shard against the oracle; a bad
    instruction id and a NaN pose in the range of a middle and of the last shard come back with the single handle's status and
    message, through pfc_eval and through pfc_eval_device + pfc_check, and the next evaluation is clean."""
    r = _ref(pfc, "c4")
    w, n, L = r.w, r.w.n_items, pfc._lib
    m = pfc.configs.build_scenario(w, devices=[0] * K, debug=True)
    ex = Expect(w, K)
    got = _host_eval(pfc, m, w.ins_ids, w.pose, w.twist, w.s)
    _check_value("c4", got, r.value)
    b, _ = _bounds(m, ex, n, ids=w.ins_ids)
    ex.done(got[2])
    assert len(b) - 1 == K
    picks = [b[0] + 1, b[K // 2] + 1, b[K - 1], n - 1]      # (the last shard: its first and its last item)
    for k, o in zip(picks, H.oracle_run(pfc, w, items=picks)):
        gp, gc = H.sorted_pairs(*m.debug_pairs(k))
        rp, rc = H.sorted_pairs(o.pairs, o.clip_n)
        assert np.array_equal(gp, rp) and np.array_equal(gc, rc), k
        trac = m.debug_tractions(k)
        assert trac.shape[0] == o.counts[3] > 0, k
        assert H.rel_err(H.normal_wrench_from_tractions(trac), H.normal_wrench_from_tractions(o.trac)) < 1e-9, k
    for bad_item in (n, -1):
        with pytest.raises(L.PFCError) as ei:
            m.debug_pairs(bad_item)
        assert ei.value.status == L.ERR_BAD_ARG

    single = pfc.configs.build_scenario(w)
    D = DeviceCalls(pfc, r, m, ex)
    torch = _torch()

    def failure(h, call):
        with pytest.raises(L.PFCError) as ei:
            call(h)
        return ei.value.status, str(ei.value)

    for at in (b[K // 2] + 2, n - 2):
        bad_ids = w.ins_ids.copy(); bad_ids[at] = 7
        bad_pose = w.pose.copy(); bad_pose[at, 2] = np.nan
        for ids, pose, status in ((bad_ids, w.pose, L.ERR_BAD_ARG), (w.ins_ids, bad_pose, L.ERR_NONFINITE)):
            want = failure(single, lambda h: _host_eval(pfc, h, ids, pose, w.twist, w.s))
            assert want[0] == status
            assert failure(m, lambda h: _host_eval(pfc, h, ids, pose, w.twist, w.s)) == want
            ex.step(n, ids=ids); ex.done(None)
            again = _host_eval(pfc, m, w.ins_ids, w.pose, w.twist, w.s)
            _check_value("c4", again, r.value)
            _bounds(m, ex, n, ids=w.ins_ids); ex.done(again[2])
            # the device-pointer path: the status comes back from pfc_check
            d_ids, d_pose = _t(ids, torch.int32), _t(pose)
            o = [_full((n, 6), 0.0), _full((n, 6), 0.0), _full((n, 4), 0, torch.int32)]

            def dev_call(h):
                h.eval_device(n, d_ids.data_ptr(), d_pose.data_ptr(), D.T["twist"].data_ptr(), D.T["s"].data_ptr(), o[0].data_ptr(),
                              o[1].data_ptr(), o[2].data_ptr(), D.st)
                h.check()

            assert failure(single, dev_call) == want
            assert failure(m, dev_call) == want
            ex.step(n, dev=True, dev_ids=True); ex.done(None)
            again, _ = D.value(True, True)
            _check_value("c4", again, r.value)
    single.close()
    m.close()


# ---- options, teardown --------------------------------------------------------------------------------------------
def test_options_reach_every_shard(pfc):
    """fixed_order = 1 on K = 8: fresh handles cut the same ranges (a handle's first evaluation cuts by the leaf counts, its second by
    the first's counters) and give the same bits, value and Dual; so does a fresh handle with poison = 1 (work lists filled with
    garbage before every evaluation)."""
    r = _ref(pfc, "pile")
    w, n = r.w, r.w.n_items
    outs = []
    for poison in (0, 1, 0):
        m = pfc.configs.build_scenario(w, devices=[0] * 8)
        m.set_option("fixed_order", 1)
        m.set_option("poison", poison)
        ex = Expect(w, 8)
        v = _host_eval(pfc, m, w.ins_ids, w.pose, w.twist, w.s)
        bv, _ = _bounds(m, ex, n, ids=w.ins_ids); ex.done(v[2])
        d = _host_dual(pfc, m, w.ins_ids, w.pose, w.twist, w.s, r.seeds["A"])
        bd, _ = _bounds(m, ex, n, ids=w.ins_ids); ex.done(d[4])
        m.close()
        assert len(bv) == len(bd) == 9
        outs.append((v + d, bv, bd))
    _check_value("pile", outs[0][0][:3], r.value)
    _check_dual("pile", outs[0][0][3:], r.dual["A"])
    for other, what in ((outs[1], "poison changed a result"), (outs[2], "two fresh handles differ")):
        assert other[1:] == outs[0][1:], what + ": the ranges"
        for a, c in zip(outs[0][0], other[0]):
            assert np.array_equal(a, c), what


def child():
    """The child process of the teardown test: a K = 8 handle opened, used through both kinds of entry point and closed, three times."""
    import pfc_pkg
    pfc = pfc_pkg.load()
    r = _ref(pfc, "c3")
    for rep in range(3):
        m = pfc.configs.build_scenario(r.w, devices=[0] * 8)
        ex = Expect(r.w, 8)
        _host_dual(pfc, m, r.w.ins_ids, r.w.pose, r.w.twist, r.w.s, r.seeds["A"], r.bp)
        D = DeviceCalls(pfc, r, m, ex)
        ex.step(D.n, ids=r.w.ins_ids); ex.done(r.dual_bp[4])
        D.dual(True, True, "A", bp=False)
        D.more("B")
        D.jacobian()
        assert m.last_shards() == 5
        m.close()


def test_teardown_of_eight_shards_frees_every_block():
    """PFC_LOG_ALLOC=1 in a fresh child process (tests/test_gpu_ownership.py): every device and pinned block of three K = 8
    handles -- eight contexts, their staging buffers, the pinned counters -- is freed exactly once by the time they are closed."""
    env = dict(os.environ, PFC_LOG_ALLOC="1")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_gpu_multi_shards as t; t.child()"
    run = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-4000:])
    live, n_alloc = set(), 0
    for ln in run.stderr.splitlines():
        a, f = _ALLOC.match(ln), _FREE.match(ln)
        if a:
            key = ("pinned" if a.group(1) == "pinned" else "device", a.group(2))
            assert key not in live, f"allocated twice without a free in between: {ln}"
            live.add(key); n_alloc += 1
        elif f:
            key = ("pinned" if f.group(1) == "unpinned" else "device", f.group(2))
            assert key in live, f"freed without a live allocation (a second free?): {ln}"
            live.remove(key)
        else:
            assert not ln.startswith(("pfc alloc", "pfc pinned", "pfc free", "pfc unpinned")), f"allocation log line not understood: {ln}"
    assert n_alloc >= 3 * 8 * 4, n_alloc      # the log is on and every shard allocated
    assert not live, f"{len(live)} blocks never freed, e.g. {sorted(live)[:5]}"
