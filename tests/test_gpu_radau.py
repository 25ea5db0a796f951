"""The parts of the Radau IIA step on the device (pfc_radau_{seed,jacobian,factor,unpack,newton,finish}_device): bytes against the
scalar statements of tests/test_radau_abi.py, guard words around every output, the scenes a part must leave alone, and the refusals.

Everything is compared as bytes: the parts use no transcendental function and no atomic sum (a square root is correctly rounded on
the device, tests/test_gpu_parity.py)."""
import numpy as np
import pytest

import test_radau_abi as R
from test_gpu_items_from_bodies import ISENTINEL, SENTINEL, Guarded, _dev, _torch

pytestmark = pytest.mark.gpu

SHAPES = {1: (1, 0, 0), 2: (1, 1, 0), 7: (1, 0, 1), 18: (6, 6, 1), 64: (20, 20, 4)}      # NX -> (nq, nv, bristle items)


@pytest.fixture(scope="module")
def scen(pfc):
    m = pfc.configs.build_scenario(pfc.configs.c1_boxes())
    yield m
    m.close()


def layout(n_scene, nx):
    nq, nv, n_br = SHAPES[nx]
    return (n_scene, nx, nq, nv, n_br + 1, [k + 1 for k in range(n_br)])      # item 0 of a scene is not bristle


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _col_major(LU, cplx=False):
    n = len(LU)
    out = np.zeros((n, n, 2 if cplx else 1))
    for i in range(n):
        for j in range(n):
            out[j, i] = LU[i][j]
    return out.reshape(-1)


def _problem(n_scene, nx, rule, seed):
    """-J (n_scene, nx, nx) [i][j], h and rule per scene: a different h per scene, rules alternating from `rule`; scene 0 needs a row
    exchange in both factors (a large entry below a small diagonal); in a batch of five, scene 3's real factor is singular."""
    rng = np.random.default_rng(seed)
    neg_J = rng.standard_normal((n_scene, nx, nx)) * 50.0
    h = 1e-4 * (1.0 + np.arange(n_scene))
    rules = np.array([rule if s % 2 == 0 else 3 - rule for s in range(n_scene)], dtype=np.int32)
    if nx > 1:
        neg_J[0, 1, 0] = 1e6
    if n_scene > 3:
        t = R.radau_tables(int(rules[3]))
        neg_J[3] = 0.0
        for k in range(nx):
            neg_J[3, k, k] = -((1.0 / h[3]) * t["lam"][0].real)
    return neg_J, h, rules


def _factor_on_device(scen, neg_J, h, rules, active=None):
    torch = _torch()
    n_scene, nx = neg_J.shape[0], neg_J.shape[1]
    d_J = _dev(np.ascontiguousarray(neg_J.transpose(0, 2, 1)))      # column-major per scene
    d_h, d_rule = _dev(h), _dev(rules)
    d_act = None if active is None else _dev(np.asarray(active, dtype=np.int32))
    lu0, lu1 = Guarded(n_scene, nx * nx), Guarded(n_scene, 2 * nx * nx)
    perm, info = Guarded(n_scene, 2 * nx, True), Guarded(n_scene, 2, True)
    scen.radau_factor_device(n_scene, nx, d_J.data_ptr(), d_h.data_ptr(), d_rule.data_ptr(), 0 if d_act is None else d_act.data_ptr(),
                             lu0.ptr, lu1.ptr, perm.ptr, info.ptr)
    torch.cuda.synchronize()
    return lu0, lu1, perm, info


def _factor_reference(neg_J, h, rules):
    return [R.factor_scalar(neg_J[s].tolist(), float(h[s]), int(rules[s])) for s in range(neg_J.shape[0])]


def _synthetic_F(lay, rng, scale=1.0):
    n_scene, nx, nq, nv, n_ips, br = lay
    qd = rng.standard_normal((3 * n_scene, nq)) * scale
    vd = rng.standard_normal((3 * n_scene, nv)) * scale
    sd = rng.standard_normal((3 * n_scene * n_ips, 6)) * scale
    return qd, vd, sd


def _F_of(lay, qd, vd, sd, ss):
    n_scene, nx, nq, nv, n_ips, br = lay
    return [float(e) for e in qd[ss]] + [float(e) for e in vd[ss]] + [float(e) for b in br for e in sd[ss * n_ips + b]]


def _records_arrays(recs):
    return (np.array([r["nstate"] for r in recs], dtype=np.float64), np.array([r["istate"] for r in recs], dtype=np.int32))


def _newton_on_device(scen, lay, F, x0, h, rules, fac_bufs, X, nstate, istate, **par):
    torch = _torch()
    n_scene, nx = lay[0], lay[1]
    lu0, lu1, perm, info = fac_bufs
    d_F = [_dev(a) for a in F]
    d_x0, d_h, d_rule = _dev(x0), _dev(h), _dev(rules)
    gX, gn, gi, gc = Guarded(3 * n_scene, nx), Guarded(n_scene, 8), Guarded(n_scene, 8, True), Guarded(1, 1, True)
    gF = Guarded(3 * n_scene, nx)
    gX.t[16:16 + X.size] = _dev(X.reshape(-1)); gn.t[16:16 + nstate.size] = _dev(nstate.reshape(-1))
    gi.t[16:16 + istate.size] = _dev(istate.reshape(-1))
    scen.radau_newton_device(lay, *[a.data_ptr() if a.numel() else 0 for a in d_F], d_x0.data_ptr(), d_h.data_ptr(), d_rule.data_ptr(),
                             lu0, lu1, perm, info, par.get("tol_newton", 1e-16), par.get("k_iter_max", 15), gX.ptr, gF.ptr, gn.ptr, gi.ptr, gc.ptr)
    torch.cuda.synchronize()
    # F of the iteration is kept for the scenes that iterated with usable factors, in X's layout; the other rows are untouched
    e_F = np.full((3 * n_scene, nx), SENTINEL)
    for s in range(n_scene):
        if istate[s, R.ITER] == 1 and not par.get("singular", {}).get(s, False):
            for k in range(3 if rules[s] == 2 else 1):
                e_F[k * n_scene + s] = _F_of(lay, *F, k * n_scene + s)
    assert _bits(gF.rows()) == _bits(e_F), np.argwhere(gF.rows() != e_F)[:4]
    return gX.rows(), gn.rows(), gi.rows(), int(gc.rows()[0])


def _newton_reference(lay, F, x0, h, rules, facs, X, nstate, istate, **par):
    n_scene, nx = lay[0], lay[1]
    X, nstate, istate = X.copy(), nstate.copy(), istate.copy()
    count = 0
    for s in range(n_scene):
        NS = 3 if rules[s] == 2 else 1
        st = dict(h=float(h[s]), rule=int(rules[s]), nstate=[float(e) for e in nstate[s]], istate=[int(e) for e in istate[s]])
        Xs = [[float(e) for e in X[k * n_scene + s]] for k in range(NS)]
        Fs = [_F_of(lay, *F, k * n_scene + s) for k in range(NS)]
        R.newton_scalar(st, facs[s], [float(e) for e in x0[s]], Xs, Fs, par.get("tol_newton", 1e-16), par.get("k_iter_max", 15))
        for k in range(NS):
            X[k * n_scene + s] = Xs[k]
        nstate[s], istate[s] = st["nstate"], st["istate"]
        count += st["istate"][R.ITER] == 1
    return X, nstate, istate, count


# ---- factor + solves ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [1, 2])
@pytest.mark.parametrize("n_scene", [1, 5])
@pytest.mark.parametrize("nx", [1, 2, 7, 18, 64])
def test_factors_and_solves_are_the_bytes_of_the_scalar_statement(scen, nx, n_scene, rule):
    neg_J, h, rules = _problem(n_scene, nx, rule, 1000 * nx + 10 * n_scene + rule)
    active = None if n_scene == 1 else [1, 1, 0, 1, 1]
    lu0, lu1, perm, info = _factor_on_device(scen, neg_J, h, rules, active)
    g_lu0, g_lu1, g_perm, g_info = lu0.rows().reshape(n_scene, -1), lu1.rows().reshape(n_scene, -1), perm.rows().reshape(n_scene, 2, nx), info.rows().reshape(n_scene, 2)
    facs = _factor_reference(neg_J, h, rules)
    swapped = False
    for s, (r0, p0, i0, r1, p1, i1) in enumerate(facs):
        if active is not None and not active[s]:      # left alone
            assert (g_lu0[s] == SENTINEL).all() and (g_lu1[s] == SENTINEL).all() and (g_perm[s] == ISENTINEL).all() and (g_info[s] == ISENTINEL).all()
            continue
        assert _bits(g_lu0[s]) == _bits(_col_major(r0)), ("lu0", s)
        assert g_perm[s, 0].tolist() == p0 and g_info[s].tolist() == [i0, i1], (s, g_info[s], i0, i1)
        if rules[s] == 2:
            assert _bits(g_lu1[s]) == _bits(_col_major(r1, True)), ("lu1", s)
            assert g_perm[s, 1].tolist() == p1
        else:
            assert (g_lu1[s] == SENTINEL).all() and (g_perm[s, 1] == ISENTINEL).all()
        swapped = swapped or p0 != list(range(nx))
    assert swapped or nx == 1
    if n_scene == 5:
        assert g_info[3, 0] == 1 and facs[3][2] == 1                      # the singular scene: flagged, its neighbours' bytes compared above
    # the solves: one Newton iteration of every scene on synthetic F
    lay = layout(n_scene, nx)
    rng = np.random.default_rng(7 + nx)
    F = _synthetic_F(lay, rng)
    x0 = rng.standard_normal((n_scene, nx))
    X = np.tile(x0, (3, 1)) + 1e-3 * rng.standard_normal((3 * n_scene, nx))
    recs = [R.new_records() for _ in range(n_scene)]
    for s, r in enumerate(recs):
        R.arm(r)
        if active is not None and not active[s]:
            r["istate"][R.ITER] = 0                                        # its factor buffers hold sentinels: not iterating
    nstate, istate = _records_arrays(recs)
    got = _newton_on_device(scen, lay, F, x0, h, rules, (lu0.ptr, lu1.ptr, perm.ptr, info.ptr), X, nstate, istate,
                            singular={3: True} if n_scene == 5 else {})
    ref = _newton_reference(lay, F, x0, h, rules, facs, X, nstate, istate)
    assert _bits(got[0]) == _bits(ref[0]), np.argwhere(got[0] != ref[0])[:4]
    assert _bits(got[1].reshape(ref[1].shape)) == _bits(ref[1]), (got[1], ref[1])
    assert np.array_equal(got[2].reshape(ref[2].shape), ref[2]) and got[3] == ref[3]
    if n_scene == 5:
        assert ref[2][3, R.FLAG] == 4


# ---- seed + jacobian ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_chunk", [1, 6, 16])
def test_seeds_and_jacobian_columns_are_bytes(scen, n_chunk):
    torch = _torch()
    n_scene, nx = 3, 18
    lay = layout(n_scene, nx)
    _, _, nq, nv, n_ips, br = lay
    rng = np.random.default_rng(n_chunk)
    neg_J = Guarded(n_scene, nx * nx)
    xdot0 = Guarded(n_scene, nx)
    recs = [R.new_records() for _ in range(n_scene)]
    recs[1]["istate"][R.EXIT] = 5                                          # retired: not armed
    nstate, istate = _records_arrays(recs)
    gn, gi = Guarded(n_scene, 8), Guarded(n_scene, 8, True)
    gn.t[16:16 + nstate.size] = _dev(nstate.reshape(-1)); gi.t[16:16 + istate.size] = _dev(istate.reshape(-1))
    qd, vd, sd = rng.standard_normal((n_scene, nq)), rng.standard_normal((n_scene, nv)), rng.standard_normal((n_scene * n_ips, 6))
    ref_J = np.full((n_scene, nx, nx), SENTINEL)                           # [scene][column][row]
    for chunk in range((nx + n_chunk - 1) // n_chunk):
        j0 = chunk * n_chunk
        n_dir = min(n_chunk, nx - j0)
        dq, dv, ds = Guarded(n_scene * n_dir, nq), Guarded(n_scene * n_dir, nv), Guarded(n_scene * n_ips * n_dir, 6)
        scen.radau_seed_device(lay, chunk, n_chunk, dq.ptr, dv.ptr, ds.ptr)
        torch.cuda.synchronize()
        e_dq, e_dv, e_ds = np.zeros((n_scene, n_dir, nq)), np.zeros((n_scene, n_dir, nv)), np.zeros((n_scene, n_ips, n_dir, 6))
        for d in range(n_dir):
            j = j0 + d
            if j < nq:
                e_dq[:, d, j] = 1.0
            elif j < nq + nv:
                e_dv[:, d, j - nq] = 1.0
            else:
                e_ds[:, br[(j - nq - nv) // 6], d, (j - nq - nv) % 6] = 1.0
        assert _bits(dq.rows()) == _bits(e_dq) and _bits(dv.rows()) == _bits(e_dv) and _bits(ds.rows()) == _bits(e_ds), chunk
        # synthetic chunk outputs
        dqd, dvd = rng.standard_normal((n_scene, n_dir, nq)), rng.standard_normal((n_scene, n_dir, nv))
        dsd = rng.standard_normal((n_scene, n_ips, n_dir, 6))
        dqd[0, 0, 0] = 0.0                                                 # -(+0.0) is -0.0
        d_in = [_dev(a) for a in (dqd, dvd, dsd, qd, vd, sd)]
        first = chunk == 0
        scen.radau_jacobian_device(lay, chunk, n_chunk, *[a.data_ptr() for a in d_in[:3]], *[a.data_ptr() if first else 0 for a in d_in[3:]],
                                   neg_J.ptr, xdot0.ptr if first else 0, gn.ptr, gi.ptr)
        torch.cuda.synchronize()
        for d in range(n_dir):
            ref_J[:, j0 + d, :] = -np.concatenate([dqd[:, d], dvd[:, d]] + [dsd[:, b, d] for b in br], axis=1)
        assert _bits(neg_J.rows()) == _bits(ref_J), chunk                  # the columns of later chunks are still sentinels
    assert _bits(xdot0.rows()) == _bits(np.concatenate([qd, vd] + [sd.reshape(n_scene, n_ips, 6)[:, b] for b in br], axis=1))
    for r in recs:
        R.arm(r)
    e_n, e_i = _records_arrays(recs)
    assert _bits(gn.rows()) == _bits(e_n) and np.array_equal(gi.rows(), e_i) and e_i[1, R.ITER] == 0 and e_i[0, R.ITER] == 1


# ---- unpack --------------------------------------------------------------------------------------------------------------------
def test_unpack_fills_the_stage_scenes(scen):
    torch = _torch()
    n_scene, nx = 4, 18
    lay = layout(n_scene, nx)
    _, _, nq, nv, n_ips, br = lay
    rng = np.random.default_rng(3)
    x0, X = rng.standard_normal((n_scene, nx)), rng.standard_normal((3 * n_scene, nx))
    rules = np.array([2, 1, 2, 1], dtype=np.int32)
    istate = np.zeros((n_scene, 8), dtype=np.int32)
    istate[0, :2] = [1, 3]          # iterating, rule 2: its own stages
    istate[1, :2] = [1, 2]          # iterating, rule 1: stage 0 three times
    istate[2, :2] = [1, 0]          # the start of an attempt: x0, and X becomes x0
    istate[3, :2] = [0, 5]          # not iterating: x0, X stays
    gX = Guarded(3 * n_scene, nx)
    gX.t[16:16 + X.size] = _dev(X.reshape(-1))
    q, v, s = Guarded(3 * n_scene, nq), Guarded(3 * n_scene, nv), Guarded(3 * n_scene * n_ips, 6)
    d_x0, d_rule, d_is = _dev(x0), _dev(rules), _dev(istate)
    scen.radau_unpack_device(lay, d_x0.data_ptr(), d_rule.data_ptr(), d_is.data_ptr(), gX.ptr, q.ptr, v.ptr, s.ptr)
    torch.cuda.synchronize()
    e_X = X.copy()
    src = np.zeros((3 * n_scene, nx))
    for k in range(3):
        src[k * n_scene + 0] = X[k * n_scene + 0]
        src[k * n_scene + 1] = X[1]
        src[k * n_scene + 2] = x0[2]; e_X[k * n_scene + 2] = x0[2]
        src[k * n_scene + 3] = x0[3]
    e_s = np.zeros((3 * n_scene, n_ips, 6))
    for k, b in enumerate(br):
        e_s[:, b] = src[:, nq + nv + 6 * k: nq + nv + 6 * k + 6]
    assert _bits(gX.rows()) == _bits(e_X)
    assert _bits(q.rows()) == _bits(src[:, :nq]) and _bits(v.rows()) == _bits(src[:, nq:nq + nv]) and _bits(s.rows()) == _bits(e_s)


# ---- newton: every flag path ---------------------------------------------------------------------------------------------------
def test_newton_flag_paths_are_bytes_and_inactive_scenes_are_untouched(scen):
    n_scene, nx = 9, 18
    lay = layout(n_scene, nx)
    rng = np.random.default_rng(11)
    neg_J = rng.standard_normal((n_scene, nx, nx)) * 20.0
    h = 1e-4 * (1.0 + 0.25 * np.arange(n_scene))
    rules = np.array([2, 1, 2, 1, 2, 1, 2, 2, 1], dtype=np.int32)
    neg_J[6] = 0.0
    for k in range(nx):
        neg_J[6, k, k] = -((1.0 / h[6]) * R.radau_tables(2)["lam"][0].real)      # scene 6: singular real factor -> flag 4
    fac_dev = _factor_on_device(scen, neg_J, h, rules)
    facs = _factor_reference(neg_J, h, rules)
    qd, vd, sd = _synthetic_F(lay, rng)
    x0 = rng.standard_normal((n_scene, nx))
    X = np.tile(x0, (3, 1)) + 1e-3 * rng.standard_normal((3 * n_scene, nx))
    recs = [R.new_records() for _ in range(n_scene)]
    for r in recs:
        R.arm(r)
    ss = lambda k, s: k * n_scene + s
    # 0: goes on iterating (rule 2); 1: goes on, second iteration (theta, Psi_k from the one before; rule 1)
    recs[1]["istate"][R.KITER] = 1; recs[1]["nstate"][R.THETA] = 0.25; recs[1]["nstate"][R.RES1] = 1e30
    # 2: converged: F = 0 and X = x0
    for k in range(3):
        qd[ss(k, 2)] = 0.0; vd[ss(k, 2)] = 0.0; sd[ss(k, 2) * lay[4]:(ss(k, 2) + 1) * lay[4]] = 0.0; X[ss(k, 2)] = x0[2]
    # 3: an update above 10
    qd[ss(0, 3)] = 1e9
    # 4: a non-finite derivative in stage 1
    vd[ss(1, 4), 2] = np.nan
    # 5: residuals rising twice
    recs[5]["istate"][R.KITER] = 2; recs[5]["nstate"][R.RES1] = 1e-30; recs[5]["nstate"][R.RES2] = 1e-31; recs[5]["nstate"][R.THETA] = 1e-15
    # 7: the iteration limit; 8: not iterating
    recs[7]["istate"][R.KITER] = 14; recs[7]["nstate"][R.THETA] = 0.5
    recs[8]["istate"][R.ITER] = 0
    nstate, istate = _records_arrays(recs)
    ref = _newton_reference(lay, (qd, vd, sd), x0, h, rules, facs, X, nstate, istate)
    assert ref[2][:, R.FLAG].tolist() == [-1, -1, 0, 3, 3, 3, 4, 1, -1] and ref[3] == 2
    assert _bits(ref[0][ss(0, 4)]) == _bits(X[ss(0, 4)])                   # non-finite: nothing updated
    ptrs = tuple(b.ptr for b in fac_dev)
    for rep in range(2):                                                   # a second call on the same inputs: the same bytes
        got = _newton_on_device(scen, lay, (qd, vd, sd), x0, h, rules, ptrs, X, nstate, istate, singular={6: True})
        assert _bits(got[0]) == _bits(ref[0]), (rep, np.argwhere(got[0] != ref[0])[:4])
        assert _bits(got[1].reshape(ref[1].shape)) == _bits(ref[1]), rep
        assert np.array_equal(got[2].reshape(ref[2].shape), ref[2]) and got[3] == ref[3], rep


# ---- finish --------------------------------------------------------------------------------------------------------------------
def test_finish_paths_are_bytes(scen):
    torch = _torch()
    n_scene, nx = 7, 18
    lay = layout(n_scene, nx)
    rng = np.random.default_rng(23)
    neg_J = rng.standard_normal((n_scene, nx, nx)) * 20.0
    h = np.array([1e-4, 2e-4, 3e-4, 5e-8, 1e-3, 1e-4, 1e-4])
    rules = np.array([1, 2, 1, 1, 2, 2, 1], dtype=np.int32)
    cool = np.array([5, 3, 1, 7, 4, 2, 2], dtype=np.int32)
    fac_dev = _factor_on_device(scen, neg_J, h, rules)
    facs = _factor_reference(neg_J, h, rules)
    F = _synthetic_F(lay, rng)
    x = rng.standard_normal((n_scene, nx)) * 0.3
    X = np.tile(x, (3, 1)) + 1e-3 * rng.standard_normal((3 * n_scene, nx))
    X[2 * n_scene + 4, :3] = [0.9, -0.8, 0.3]                              # scene 4 (rule 2: stage 2 is final): |sigma|^2 > 1
    xdot0 = rng.standard_normal((n_scene, nx))
    t = 0.1 * np.arange(n_scene)
    enorm = rng.uniform(0.1, 1.0, (n_scene, 2))
    recs = [R.new_records() for _ in range(n_scene)]
    for s, r in enumerate(recs):
        R.arm(r)
        r["h"], r["rule"], r["cool"], r["enorm"] = float(h[s]), int(rules[s]), int(cool[s]), [float(e) for e in enorm[s]]
        r["istate"][R.ITER], r["istate"][R.KITER] = 0, 3 + s
    flags = [0, 3, 0, 1, 0, 0, -1]      # success; failure, rule down; success, rule up; failure below h_min; success with the MRP; 5, 6 below
    for s, f in enumerate(flags):
        recs[s]["istate"][R.FLAG] = f
    recs[2]["nstate"][R.PSI] = 0.01
    recs[5]["istate"][R.PHASE] = 0      # no attempt open: untouched
    recs[6]["istate"][R.ITER] = 1       # still iterating: untouched
    nstate, istate = _records_arrays(recs)
    d_F = _dev(np.array([_F_of(lay, *F, ss) for ss in range(3 * n_scene)]))      # X's layout, as the newton part keeps it
    bufs = [Guarded(n_scene, nx), Guarded(n_scene, 1), Guarded(n_scene, 1), Guarded(n_scene, 1, True), Guarded(n_scene, 1, True),
            Guarded(n_scene, 2), Guarded(n_scene, 8), Guarded(n_scene, 8, True), Guarded(1, 1, True)]
    for b, a in zip(bufs, (x, t, h, rules, cool, enorm, nstate, istate)):
        b.t[16:16 + a.size] = _dev(a.reshape(-1))
    d_xdot0, d_X = _dev(xdot0), _dev(X)
    scen.radau_finish_device(lay, [0], (1e-4, 1e-4, 0.01, 1e-8), 15, 2, 10, d_F.data_ptr(), d_xdot0.data_ptr(),
                             d_X.data_ptr(), fac_dev[0].ptr, fac_dev[2].ptr, *[b.ptr for b in bufs])
    torch.cuda.synchronize()
    e_x, e_t = x.copy(), t.copy()
    for s, r in enumerate(recs):
        NS = 3 if rules[s] == 2 else 1
        Xs = [[float(e) for e in X[k * n_scene + s]] for k in range(NS)]
        Fs = [_F_of(lay, *F, k * n_scene + s) for k in range(NS)]
        e_x[s], e_t[s] = R.finish_scalar(r, facs[s], [float(e) for e in x[s]], float(t[s]), Xs, Fs, [float(e) for e in xdot0[s]], mrp_off=(0,))
    e_n, e_i = _records_arrays(recs)
    got = [b.rows() for b in bufs]
    assert [r["istate"][R.EXIT] for r in recs[:5]] == [0, 3, 0, 5, 0] and [r["rule"] for r in recs] == [1, 1, 2, 1, 2, 2, 1]
    assert e_x[4, 0] == -(0.9 / ((0.9 * 0.9 + 0.8 * 0.8) + 0.3 * 0.3))
    assert _bits(got[0]) == _bits(e_x) and _bits(got[1]) == _bits(e_t)
    assert _bits(got[2]) == _bits(np.array([r["h"] for r in recs])), (got[2], [r["h"] for r in recs])
    assert got[3].tolist() == [r["rule"] for r in recs] and got[4].tolist() == [r["cool"] for r in recs]
    assert _bits(got[5]) == _bits(np.array([r["enorm"] for r in recs]))
    assert _bits(got[6].reshape(e_n.shape)) == _bits(e_n) and np.array_equal(got[7].reshape(e_i.shape), e_i)
    assert int(got[8][0]) == 1                                             # scene 1 was armed for another attempt


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(pfc, scen):
    torch = _torch()
    L = pfc._lib
    out = [Guarded(1, 65 * 65), Guarded(1, 2 * 65 * 65), Guarded(1, 2 * 65, True), Guarded(1, 2, True)]
    d = _dev(np.ones(65 * 65)); d_rule = _dev(np.array([1], dtype=np.int32))

    def refused(call, word):
        with pytest.raises(L.PFCError) as e:
            call()
        assert e.value.status == L.ERR_BAD_ARG and word in str(e.value), str(e.value)

    refused(lambda: scen.radau_factor_device(1, 65, d.data_ptr(), d.data_ptr(), d_rule.data_ptr(), 0, *[o.ptr for o in out]), "PFC_MAX_NX_RADAU")
    refused(lambda: scen.radau_factor_device(1, 0, d.data_ptr(), d.data_ptr(), d_rule.data_ptr(), 0, *[o.ptr for o in out]), "PFC_MAX_NX_RADAU")
    lay = layout(1, 18)
    seeds = [Guarded(17, 6), Guarded(17, 6), Guarded(2 * 17, 6)]
    refused(lambda: scen.radau_seed_device(lay, 0, 17, *[o.ptr for o in seeds]), "n_chunk")
    refused(lambda: scen.radau_seed_device(lay, 3, 6, *[o.ptr for o in seeds]), "chunk")
    refused(lambda: scen.radau_seed_device((1, 19, 6, 6, 2, [1]), 0, 6, *[o.ptr for o in seeds]), "nq + nv")
    refused(lambda: scen.radau_seed_device((1, 18, 6, 6, 2, [2]), 0, 6, *[o.ptr for o in seeds]), "n_ips")
    fin = [Guarded(1, 18), Guarded(1, 1), Guarded(1, 1), Guarded(1, 1, True), Guarded(1, 1, True), Guarded(1, 2), Guarded(1, 8),
           Guarded(1, 8, True), Guarded(1, 1, True)]
    args = [d.data_ptr()] * 4 + [d_rule.data_ptr()] + [o.ptr for o in fin]
    refused(lambda: scen.radau_finish_device(lay, [0], (1e-4, 1e-4, 0.01, 1e-8), 15, 3, 10, *args), "max_rule")      # rule 3 is not built
    refused(lambda: scen.radau_finish_device(lay, [5], (1e-4, 1e-4, 0.01, 1e-8), 15, 2, 10, *args), "MRP")
    torch.cuda.synchronize()
    for o in out + seeds + fin:
        assert o.untouched()
    with pytest.raises(L.PFCError):
        pfc.scenario.radau_table(3)


# ---- the step ------------------------------------------------------------------------------------------------------------------
BOX_MASS, BOX_R = 0.8, 0.05


def _box_scenario(pfc, fixed_order=False):
    """One floating box (C2's geometry at its smallest mesh, n_div = 1) and the ground, a bristle instruction between them."""
    import test_dynamics_abi as D
    import test_kinematics_abi as K
    w = pfc.configs.c2_box_on_plane(1, n_div=1)
    w.instructions = [pfc.configs.InsSpec(0, 1, "bristle", chi=0.5, mu_d=0.3)]
    m = pfc.configs.build_scenario(w)
    if fixed_order:
        m.set_option("fixed_order", 1)
    mech = K.make_mech([-1], [K.FLOATING], [K.WORLD_X], [[0.0, 0.0, 0.0]])
    m.set_mechanism(mech["parent"], mech["joint_type"], mech["x_p_j"], mech["axis"])
    m.set_instruction_bodies(0, -1, 0)
    Ic = np.eye(3) * (2.0 / 3.0) * BOX_MASS * BOX_R * BOX_R
    m.set_inertia(D.make_inertia(BOX_MASS, [0.0, 0.0, 0.0], Ic).reshape(1, 13), D.GRAVITY)
    return m


def _box_states(n_scene, z, vz, seed=5):
    """x = [p (3) t (3); w (3) v (3); s (6)] per scene: small tilts, heights z, vertical velocities vz."""
    rng = np.random.default_rng(seed)
    x = np.zeros((n_scene, 18))
    x[:, 0:3] = 0.01 * rng.standard_normal((n_scene, 3))
    x[:, 3:5] = 0.1 * rng.standard_normal((n_scene, 2))
    x[:, 5] = z
    x[:, 9:11] = 0.05 * rng.standard_normal((n_scene, 2))
    x[:, 11] = vz
    return x


@pytest.mark.parametrize("rule", [1, 2])
def test_step_free_fall_is_the_analytic_step(pfc, rule):
    """Three boxes a metre above the ground, no rotation, three different h: tdot = v, vdot = g.  A rule-2 step (order 5) is exact,
    z0 + vz0 h - g h^2 / 2 and vz0 - g h; a rule-1 step is implicit Euler's z0 + h (vz0 - g h).  The bound of the CPU test
    (tests/test_radau_abi.py::test_free_fall_steps_are_the_analytic_values): 8 eps of the terms."""
    m = _box_scenario(pfc)
    assert m.radau_configure(3, [0]) == 18 and m.radau_sizes()[1].tolist() == [0]
    x0 = np.zeros((3, 18))
    x0[:, 5] = [1.0, 1.5, 2.0]
    x0[:, 11] = [0.0, -0.7, 1.3]
    hs = np.array([1e-4, 3e-3, 0.01])
    m.radau_set_state(x0, [0.0, 0.5, 1.0])
    m.radau_set_rule_state(h=hs, rule=rule)
    assert _bits(m.radau_rule_state()["h"]) == _bits(hs) and m.radau_rule_state()["rule"].tolist() == [rule] * 3
    out = m.radau_step()
    x, t = m.radau_get_state()
    g = 9.81
    assert out["flags"].tolist() == [0, 0, 0] and out["attempts"].tolist() == [1, 1, 1] and _bits(out["h_taken"]) == _bits(hs)
    assert t.tolist() == [0.0 + hs[0], 0.5 + hs[1], 1.0 + hs[2]]
    for s in range(3):
        z0, v0, h = x0[s, 5], x0[s, 11], hs[s]
        z_ref = z0 + v0 * h - g * h * h / 2 if rule == 2 else z0 + h * (v0 - g * h)
        print("free fall rule", rule, "scene", s, x[s, 5] - z_ref, x[s, 11] - (v0 - g * h))
        assert abs(x[s, 5] - z_ref) <= 8 * R.EPS * (abs(z0) + h * abs(v0) + g * h * h)
        assert abs(x[s, 11] - (v0 - g * h)) <= 8 * R.EPS * (abs(v0) + g * h)
        assert np.abs(np.delete(x[s], [5, 11])).max() == 0.0
    rs = m.radau_rule_state()
    assert rs["rule"].tolist() == [rule] * 3 and rs["cooldown"].tolist() == [9, 9, 9] and (rs["h"] > 0).all() and (rs["h"] <= 2 * hs).all()
    with pytest.raises(pfc._lib.PFCError):
        m.radau_set_rule_state(rule=3)
    with pytest.raises(pfc._lib.PFCError):
        m.radau_set_rule_state(h=[1e-4, 0.0, 1e-4])
    assert _bits(m.radau_rule_state()["h"]) == _bits(rs["h"])      # a refused call changes nothing
    m.close()


def _host_de_batch(m):
    """de_batch and de_dual_batch of R.radau_step_batch from the host forms of a handle, one item (instruction 0) per scene: the
    evaluation shapes of pfc_radau_step.  (An evaluation's last bits depend on the batch it is part of even under fixed_order --
    six box scenes together and one by one differ by 1e-7 in sdot -- so the statement is driven in the step's own shapes.)"""
    def split(rows):
        x = np.asarray(rows, dtype=np.float64)
        return x[:, 0:6], x[:, 6:12], x[:, 12:18], [0] * x.shape[0], np.arange(x.shape[0], dtype=np.int32)

    def de_batch(rows):
        q, v, s, ids, sc = split(rows)
        qd, vd, sd, info = m.state_derivative(q, v, s, ins_ids=ids, scene=sc)[:4]
        assert not info.any()
        return np.concatenate([qd, vd, sd], axis=1).tolist()

    def de_dual_batch(rows, seeds):
        q, v, s, ids, sc = split(rows)
        n, nd = q.shape[0], len(seeds)
        sd_a = np.tile(np.array(seeds, dtype=np.float64)[None], (n, 1, 1))
        qd, vd, sd, dqd, dvd, dsd, info = m.state_derivative_dual(q, v, s, sd_a[:, :, 0:6], sd_a[:, :, 6:12], sd_a[:, :, 12:18],
                                                                    ins_ids=ids, scene=sc)[:7]
        assert not info.any()
        dsd = np.asarray(dsd).reshape(n, nd, 6)
        return (np.concatenate([qd, vd, sd], axis=1).tolist(),
                [[np.concatenate([dqd[k, d], dvd[k, d], dsd[k, d]]).tolist() for d in range(nd)] for k in range(n)])

    return de_batch, de_dual_batch


def test_step_box_on_plane_is_the_statement_driven_by_the_host_forms(pfc):
    """Two boxes resting in the ground with 1 and 2 mm penetration, 5 steps.  Under fixed_order every sum is ordered: x, t, h, rule,
    flags and iteration counts are the bytes of the statement (R.radau_step_batch: the scene statements in the step's evaluation
    shapes) driven by the host-form state_derivative / state_derivative_dual of a
    second handle.  On a default handle (atomic sums) the flags are equal and x differs by <= 1e-3 in the step's own error norm
    (Eq. 8.21 with the step's tol_a, tol_r): a thousandth of the local error the step accepts."""
    A, B, Cd = _box_scenario(pfc, True), _box_scenario(pfc, True), _box_scenario(pfc, False)
    x0 = _box_states(2, [BOX_R - 1e-3, BOX_R - 2e-3], [0.0, -0.02])
    de_batch, de_dual_batch = _host_de_batch(B)
    # scene 0 starts at rule 2 (three stages, the complex factor); scene 1 at rule 1 and, with a cooldown of 2, rises to rule 2 after
    # its second step: steps of both rules and the change between them are compared
    recs = [R.new_records(cooldown=2) for _ in range(2)]
    recs[0]["rule"] = 2
    xs, ts = [x0[s].tolist() for s in range(2)], [0.0, 0.0]
    for m in (A, Cd):
        m.radau_configure(2, [0], cooldown=2)
        m.radau_set_state(x0)
        m.radau_set_rule_state(rule=[2, 1])
    rules_run = []
    for step in range(5):
        rules_run.append([r["rule"] for r in recs])
        outs = [m.radau_step() for m in (A, Cd)]
        xs, ts = R.radau_step_batch(de_batch, de_dual_batch, xs, ts, recs, mrp_off=(0,), cooldown=2)
        x, t = A.radau_get_state()
        rs = A.radau_rule_state()
        assert outs[0]["flags"].tolist() == [r["istate"][R.EXIT] for r in recs] == [0, 0], step
        assert outs[0]["iters"].tolist() == [r["istate"][R.EXITITER] for r in recs], (step, outs[0]["iters"])
        assert outs[0]["attempts"].tolist() == [r["istate"][R.ATTEMPTS] for r in recs], step
        assert _bits(x) == _bits(np.array(xs)), (step, np.abs(x - np.array(xs)).max())
        assert _bits(t) == _bits(np.array(ts)) and _bits(rs["h"]) == _bits(np.array([r["h"] for r in recs])), step
        assert rs["rule"].tolist() == [r["rule"] for r in recs] and rs["cooldown"].tolist() == [r["cool"] for r in recs], step
        assert _bits(rs["x_err_norm_next"]) == _bits(np.array([r["enorm"][1] for r in recs])), step
        # the default handle
        xd, td = Cd.radau_get_state()
        assert outs[1]["flags"].tolist() == [0, 0]
        sc = 1e-4 + np.maximum(np.abs(x), np.abs(xd)) * 1e-4
        norm = np.sqrt((((x - xd) / sc) ** 2).sum(axis=1) / 18)
        print("step", step, "default vs fixed_order, error norm", norm)
        assert (norm <= 1e-3).all(), (step, norm)
    assert rules_run[0] == [2, 1] and [2, 2] in rules_run, rules_run          # scene 1 ran steps of both rules
    for m in (A, B, Cd):
        m.close()


def test_step_forced_retry_matches_the_statement(pfc):
    """The box 0.1 mm in the ground at 3 m/s downwards, h = h_max = 0.01 and rule 2: the first attempt fails, the second (h = 1e-3, rule
    1) as well, the third (h = 1e-4) succeeds -- the input was run through R.radau_step_batch on the device's host forms beforehand:
    attempts [3, 1].  The second scene falls freely and stays on its first attempt: it is evaluated at its committed x, and its
    factors are left alone, while the first is factored and iterated again.  Attempts, iterations, x, t, the next h and the rule are
    those of the statement (bytes under fixed_order)."""
    A, B = _box_scenario(pfc, True), _box_scenario(pfc, True)
    x0 = np.zeros((2, 18))
    x0[0, 5], x0[0, 11] = BOX_R - 1e-4, -3.0
    x0[1, 5], x0[1, 11] = 1.0, -0.3
    de_batch, de_dual_batch = _host_de_batch(B)
    recs = [R.new_records(h0=0.01) for _ in range(2)]
    for r in recs:
        r["rule"] = 2
    A.radau_configure(2, [0], h0=0.01)
    A.radau_set_state(x0)
    A.radau_set_rule_state(rule=2)
    out = A.radau_step()
    xs, ts = R.radau_step_batch(de_batch, de_dual_batch, [x0[0].tolist(), x0[1].tolist()], [0.0, 0.0], recs, mrp_off=(0,))
    x, t = A.radau_get_state()
    rs = A.radau_rule_state()
    print("forced retry", out, [r["h"] for r in recs])
    assert out["attempts"].tolist() == [r["istate"][R.ATTEMPTS] for r in recs] == [3, 1]
    assert out["flags"].tolist() == [0, 0] and out["iters"].tolist() == [r["istate"][R.EXITITER] for r in recs]
    assert _bits(out["h_taken"]) == _bits(np.array([r["nstate"][R.HTAKEN] for r in recs])) and out["h_taken"][1] == 0.01 and out["h_taken"][0] < 0.01
    assert _bits(x) == _bits(np.array(xs)) and _bits(t) == _bits(np.array(ts)), np.abs(x - np.array(xs)).max()
    assert _bits(rs["h"]) == _bits(np.array([r["h"] for r in recs]))
    assert rs["rule"].tolist() == [r["rule"] for r in recs] == [1, 2] and rs["cooldown"].tolist() == [r["cool"] for r in recs] == [9, 9]
    A.close(); B.close()


def test_integrate_radau_and_two_fresh_handles_agree(pfc):
    x0 = _box_states(2, [BOX_R - 1e-3, BOX_R + 0.01], [0.0, -0.1], seed=9)
    res = []
    for _ in range(2):
        m = _box_scenario(pfc, True)
        m.radau_configure(2, [0], n_chunk=16)
        m.radau_set_state(x0)
        x, t, steps = m.integrate_radau(1.5e-3, max_steps=40)
        res.append((x, t, steps, m.radau_rule_state()["h"]))
        m.close()
    assert res[0][2] == res[1][2] and (res[0][1] >= 1.5e-3).all() and res[0][2] < 40
    assert _bits(res[0][0]) == _bits(res[1][0]) and _bits(res[0][1]) == _bits(res[1][1]) and _bits(res[0][3]) == _bits(res[1][3])


def test_configure_refusals(pfc):
    import test_dynamics_abi as D
    import test_kinematics_abi as K
    from test_gpu_dynamics import chain_mech
    L = pfc._lib
    w = pfc.configs.c2_box_on_plane(1, n_div=1)
    m = pfc.configs.build_scenario(w)

    def refused(status, word, **kw):
        with pytest.raises(L.PFCError) as e:
            m.radau_configure(kw.pop("n_scene", 1), [0], **kw)
        assert e.value.status == status and word in str(e.value), str(e.value)

    refused(L.ERR_STATE, "pfc_set_mechanism")
    mech = K.make_mech([-1], [K.FLOATING], [K.WORLD_X], [[0.0, 0.0, 0.0]])
    m.set_mechanism(mech["parent"], mech["joint_type"], mech["x_p_j"], mech["axis"])
    m.set_instruction_bodies(0, -1, 0)
    refused(L.ERR_STATE, "pfc_set_inertia")
    m.set_inertia(D.make_inertia(1.0, [0.0, 0.0, 0.0], np.eye(3)).reshape(1, 13), D.GRAVITY)
    refused(L.ERR_BAD_ARG, "rules 1 and 2", max_rule=3)
    refused(L.ERR_BAD_ARG, "n_chunk", n_chunk=17)
    refused(L.ERR_BAD_ARG, "n_chunk", n_chunk=0)
    with pytest.raises(L.PFCError) as e:
        m.radau_step()
    assert e.value.status == L.ERR_STATE and "pfc_radau_configure" in str(e.value)
    big = chain_mech(33)                                                   # nq + nv = 66 > 64
    m.set_mechanism(big["parent"], big["joint_type"], big["x_p_j"], big["axis"])
    m.set_inertia(D.random_inertia(big, np.random.default_rng(1)), D.GRAVITY)
    refused(L.ERR_BAD_ARG, "PFC_MAX_NX_RADAU")
    m.close()
