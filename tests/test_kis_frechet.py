"""The Dual path's eigen step, d(K̄^{-1/2}) along dK̄ (decompose_K!, src/contact_algorithms_friction.jl:85-117), pinned to
an mpmath reference at 60 digits -- on the oracle (pfo_kis_dual, the code pfo_eval_dual runs) and on the device
(pfc_selftest_kis, the code k_dual_eig runs).  Every Dual result of a bristle item passes through this step, and the
oracle and the device state it the same way, so their parity tests cannot see an error the two share.

The function is F(K̄) = V diag(f(x)) V' with f(x) = x^{-1/2}, x = max(lambda, floor), floor = 1e-16 sigma_max.  The
reference of its derivative does not depend on the formula under test where no eigenvalue is clamped: a central
difference (F(K̄ + t dK̄) - F(K̄ - t dK̄)) / 2t with t = 1e-25 at 60 digits (truncation ~ (t |dK̄| / lambda_min)^2, rounding
~ 1e-60 / t: both far below 1e-30).  With clamped eigenvalues F is not smooth at the clamp, so the reference is the
Daleckii-Krein form at 60 digits on mp.eigsy's decomposition, the floor differentiated as the code does
(d floor = 1e-16 v_max' dK̄ v_max).

Per-entry bound.  With the reference decomposition K̄ = Q diag(lambda) Q', M = Q' dK̄ Q, E = Q' (dKis - dKis_ref) Q:

    |E_ij| <= 64 eps (sigma_max max_k |f[x_i, x_k, x_j]| max|M|  +  (|Q|'|Q| |G o M| |Q|'|Q|)_ij)

where f[a, b, c] = (s_a + s_b + s_c) / (s_a s_b s_c (s_a + s_b)(s_b + s_c)(s_a + s_c)), s = sqrt, is the second divided
difference of x^{-1/2} and G o M = Q' dKis_ref Q.  Derivation of the first term: a backward-stable eigen-solver returns the
exact decomposition of K̄ + Delta with |Delta| ~ eps sigma_max, and nothing better; to first order that moves the
derivative by the second Frechet derivative, which in the eigen-basis is
    (d2F[Delta, dK̄])_ij = sum_k f[x_i, x_k, x_j] (Delta~_ik M_kj + M_ik Delta~_kj),      Delta~ = Q' Delta Q,
so |E_ij| <= 2 * 6 * max_k |f[x_i, x_k, x_j]| max|Delta~| max|M|; 64 = 12 x a backward error of ~5 eps sigma_max.  It is tight on
the stiff block (where clusters live) and loose on the soft entries.  The second term is the rounding of the result itself:
dKis = V (G o M) V' is formed and stored in the standard basis, entry by entry relative to eps, and rotating those roundings
into the eigen-basis gives the term (|Q| |G o M| |Q|' is the size of the products, |Q|' . |Q| the rotation back).  Where the
soft eigenvectors are not aligned with the axes (family (c): graded spectra under random rotations), the correctly rounded
reference itself exceeds the first term by ~1e5 -- the soft block's eps-sized roundings land on every entry -- so the first
term alone cannot be met by any float64 result.  On clusters with kappa <= 60 both terms are of the same order.

Assertions: where kappa <= 1e3 on the unclamped part (families a, b, d), value to 1e-13 and derivative to 1e-12 norm-wise;
everywhere, the per-entry bound.  The former Daleckii-Krein divided difference (f_i - f_j) / (lambda_i - lambda_j) exceeds
the bound on every cluster gap up to 1e-8 and on the scene matrices: rounding noise over a rounding-sized gap.
"""
import ctypes as C
import functools

import mpmath as mp
import numpy as np
import pytest

import helpers as H

DPS = 60
EPS = np.finfo(np.float64).eps
BOUND_C = 64.0
FLOOR = 1.0e-16                                  # decompose_K!'s clamp, max(sigma, 1e-16 sigma_max) (friction.jl:92)
CLUSTER_GAPS = (0.0, 1e-16, 1e-15, 1e-14, 1e-13, 1e-12, 1e-10, 1e-8)


def _mpm(A):
    return mp.matrix([[mp.mpf(float(A[i, j])) for j in range(6)] for i in range(6)])


def _np(A):
    return np.array([[float(A[i, j]) for j in range(A.cols)] for i in range(A.rows)])


def _isqrt(A):
    E, Q = mp.eigsy(A)
    return Q * mp.diag([1 / mp.sqrt(E[k]) for k in range(6)]) * Q.T


def _dd2(a, b, c):
    """Second divided difference f[a, b, c] of f(x) = x^{-1/2} (symmetric, no subtraction: exact at ties)."""
    sa, sb, sc = mp.sqrt(a), mp.sqrt(b), mp.sqrt(c)
    return (sa + sb + sc) / (sa * sb * sc * (sa + sb) * (sb + sc) * (sa + sc))


class Ref:
    """60-digit reference of F(K̄) and dF[dK̄] for one float64 input, and the per-entry bound of the module docstring."""

    def __init__(self, K, dK):
        self.K, self.dK = K, dK
        with mp.workdps(DPS):
            Km, dKm = _mpm(K), _mpm(dK)
            E, Q = mp.eigsy(Km)
            lam = [E[k] for k in range(6)]
            imx = max(range(6), key=lambda k: lam[k])
            smax = lam[imx]
            floor = smax * mp.mpf(FLOOR)
            x = [l if l > floor else floor for l in lam]
            M = Q.T * dKm * Q
            self.clamped = [not (l > floor) for l in lam]
            val = Q * mp.diag([1 / mp.sqrt(v) for v in x]) * Q.T
            if not any(self.clamped):
                t = mp.mpf("1e-25")
                der = (_isqrt(Km + t * dKm) - _isqrt(Km - t * dKm)) / (2 * t)
                GM = Q.T * der * Q
            else:
                F = [1 / mp.sqrt(v) for v in x]
                Fp = [0 if c else -F[k] / (2 * x[k]) for k, c in enumerate(self.clamped)]
                GM = mp.matrix(6, 6)
                for i in range(6):
                    for j in range(6):
                        g = (F[i] - F[j]) / (lam[i] - lam[j]) if lam[i] != lam[j] else Fp[i]
                        GM[i, j] = g * M[i, j]
                    if self.clamped[i]:                 # d floor = 1e-16 v_max' dK̄ v_max
                        GM[i, i] += -F[i] / (2 * x[i]) * mp.mpf(FLOOR) * M[imx, imx]
                der = Q * GM * Q.T
            mM = max(abs(M[i, j]) for i in range(6) for j in range(6))
            t1 = np.array([[float(smax * max(_dd2(x[i], x[k], x[j]) for k in range(6)) * mM) for j in range(6)]
                           for i in range(6)])
            aQ = np.abs(_np(Q))
            P = aQ.T @ aQ
            t2 = P @ np.abs(_np(GM)) @ P
            self.bound = BOUND_C * EPS * (t1 + t2)
            self.Q, self.der_mp, self.val_mp = Q, der, val
            self.lam = np.array([float(l) for l in lam])
            self.val = _np(val)
            self.der = _np(der)
            self.kappa = float(smax / min(x[k] for k in range(6) if not self.clamped[k]))

    def entry_ratio(self, dKis):
        """max_ij |E_ij| / bound_ij for a float64 result dKis."""
        with mp.workdps(DPS):
            E = self.Q.T * (_mpm(dKis) - self.der_mp) * self.Q
            return float(max(abs(E[i, j]) / mp.mpf(self.bound[i, j]) for i in range(6) for j in range(6)))

    def pair_ratio(self, a, b):
        """The same bound on the difference of two float64 results (device against oracle)."""
        with mp.workdps(DPS):
            E = self.Q.T * (_mpm(a) - _mpm(b)) * self.Q
            return float(max(abs(E[i, j]) / mp.mpf(self.bound[i, j]) for i in range(6) for j in range(6)))

    def normwise(self, Kis, dKis):
        return (np.linalg.norm(Kis - self.val) / np.linalg.norm(self.val),
                np.linalg.norm(dKis - self.der) / np.linalg.norm(self.der))

    def vlam42(self):
        """The reference decomposition rounded to float64, as pfc_selftest_kis's stored_v input (V column-major, lambda)."""
        return np.concatenate([_np(self.Q).reshape(-1, order="F"), self.lam])


# ---- input families ----

def _rot(rng):
    q, r = np.linalg.qr(rng.standard_normal((6, 6)))
    return q * np.sign(np.diag(r))


def _sym(rng):
    a = rng.standard_normal((6, 6))
    return (a + a.T) / 2


def _spd(rng, spec):
    Q = _rot(rng)
    K = Q @ np.diag(spec) @ Q.T
    return (K + K.T) / 2


def _separated(rng, n=8):
    out = []
    while len(out) < n:
        spec = rng.uniform(0.05, 3.0, 6)
        s = np.sort(spec)
        if np.all(s[1:] / s[:-1] > 1.1):
            out.append((_spd(rng, spec), _sym(rng)))
    return out


def _cluster(gap):
    """Double and triple clusters c, c (1 + gap), (c (1 + 2 gap)) with c in U(0.05, 3) (never a power of two: at 1.0 the
    old formula happened to be exact), the other eigenvalues >= 0.05, under random rotations."""
    def gen(rng):
        out = []
        for mult in (2, 2, 2, 3, 3, 3):
            c = rng.uniform(0.05, 3.0)
            spec = np.concatenate([c * (1.0 + gap * np.arange(mult)), rng.uniform(0.05, 3.0, 6 - mult)])
            out.append((_spd(rng, spec), _sym(rng)))
        return out
    return gen


def _graded(rng):
    out = []
    for depth in (4, 7, 10, 10):
        spec = 10.0 ** -np.linspace(0, depth, 6) * rng.uniform(0.7, 1.4, 6) * rng.uniform(0.1, 10)
        out.append((_spd(rng, spec), _sym(rng)))
    return out


def _zero_rows(rng):
    """One or two exactly zero rows and columns (a patch whose normal is a frame axis): Jacobi never rotates them, so the
    clamp decision does not depend on rounding."""
    out = []
    for nz in (1, 1, 2, 2):
        A = np.zeros((6, 6))
        keep = np.sort(rng.permutation(6)[nz:])
        Q = np.linalg.qr(rng.standard_normal((6 - nz, 6 - nz)))[0]
        B = Q @ np.diag(rng.uniform(0.05, 3.0, 6 - nz)) @ Q.T
        A[np.ix_(keep, keep)] = (B + B.T) / 2
        out.append((A, _sym(rng)))
    return out


def _scene_kbar(pfc, w, items=None, cap=None):
    """K̄ = S^{-1} K S^{-1} of the bristle items in contact, formed as decompose_K! forms it (upper triangle)."""
    out = []
    for r in H.oracle_run(pfc, w, items=items):
        if not r.has_K:
            continue
        K, s = r.K, r.Sinv
        Kb = np.array([[(s[i] * K[min(i, j), max(i, j)]) * s[j] for j in range(6)] for i in range(6)])
        out.append(Kb)
        if cap and len(out) >= cap:
            break
    return out


def _scenes(pfc, rng):
    """K̄ of real scenes: C1 boxes and the flat C2 box switched to bristle, face-to-face C5 pile items.  Only matrices
    with no eigenvalue within a factor 4 of the floor are kept: an eigenvalue there (a flat patch whose normal is not a
    frame axis has one at rounding level) puts the clamp decision itself within rounding -- the reference's own
    discontinuity (friction.jl:92) -- and no accuracy can be asked of the derivative there."""
    ws = []
    for w in (pfc.configs.c1_boxes(), pfc.configs.c2_box_on_plane(1)):
        for c in w.instructions:
            c.model = "bristle"
        ws.append((w, None, None))
    ws.append((pfc.configs.c5_pile(n_side=2), None, 6))
    out = []
    for w, items, cap in ws:
        for Kb in _scene_kbar(pfc, w, items, cap):
            lam = np.linalg.eigvalsh(Kb)
            floor = FLOOR * lam.max()
            if np.any((lam > floor / 4) & (lam < 4 * floor)):
                continue
            out.append((Kb, _sym(rng) * np.abs(Kb).max()))
    return out


CLUSTERS = [f"cluster_gap{g:g}" for g in CLUSTER_GAPS]
NORMWISE = ["separated"] + CLUSTERS + ["zero_rows"]
FAMILIES = {"separated": (_separated, 11), **{n: (_cluster(g), 100 + k) for k, (n, g) in enumerate(zip(CLUSTERS, CLUSTER_GAPS))},
            "graded": (_graded, 13), "zero_rows": (_zero_rows, 14), "scenes": (_scenes, 15)}


@functools.lru_cache(maxsize=None)
def _family(name, pfc=None):
    gen, seed = FAMILIES[name]
    rng = np.random.default_rng(seed)
    cases = gen(pfc, rng) if name == "scenes" else gen(rng)
    return [Ref(K, dK) for K, dK in cases]


def _cases(name, pfc):
    refs = _family(name, pfc if name == "scenes" else None)
    assert refs, name
    return refs


def _stack(refs):
    return np.stack([r.K for r in refs]), np.stack([r.dK for r in refs])


# ---- the oracle (CPU) ----

@pytest.mark.parametrize("family", list(FAMILIES))
def test_oracle_per_entry(pfc, O, family):
    refs = _cases(family, pfc)
    Kis, dKis = O.kis_dual(*_stack(refs))
    ratios = [r.entry_ratio(d) for r, d in zip(refs, dKis)]
    print(f"oracle {family}: {len(refs)} matrices, worst |E_ij| / bound_ij = {max(ratios):.3g}")
    bad = [(k, refs[k].lam.tolist(), q) for k, q in enumerate(ratios) if not q <= 1.0]
    assert not bad, bad


@pytest.mark.parametrize("family", NORMWISE)
def test_oracle_normwise(pfc, O, family):
    refs = _cases(family, pfc)
    Kis, dKis = O.kis_dual(*_stack(refs))
    for k, r in enumerate(refs):
        assert r.kappa <= 1e3, (family, k, r.kappa)
        ev, ed = r.normwise(Kis[k], dKis[k])
        assert ev <= 1e-13 and ed <= 1e-12, (family, k, ev, ed, r.lam)


def test_cluster_families_are_clusters(pfc):
    """The inputs are what they claim: the cluster family's matrices carry eigenvalue pairs within their gap, the zero-row
    family is clamped and the scene family holds matrices whose two largest eigenvalues are a cluster (a flat patch)."""
    for name, gap in zip(CLUSTERS, CLUSTER_GAPS):
        for k, r in enumerate(_cases(name, pfc)):
            s = np.sort(r.lam)
            assert np.min(np.diff(s) / s[1:]) <= gap + 1e-15, (name, k, r.lam)
    assert all(any(r.clamped) for r in _cases("zero_rows", pfc))
    sc = _cases("scenes", pfc)
    assert len(sc) >= 6
    assert sum(1 for r in sc if (lambda s: (s[-1] - s[-2]) / s[-1] < 1e-12)(np.sort(r.lam))) >= 2


# ---- the device (MI355X): the same families through the code k_dual_eig runs ----

def _device_kis(pfc, refs, stored):
    Kb, dKb = _stack(refs)
    n = len(refs)
    kc = np.ascontiguousarray(Kb.transpose(0, 2, 1))            # column-major per matrix
    dc = np.ascontiguousarray(dKb.transpose(0, 2, 1))
    vl = np.ascontiguousarray(np.stack([r.vlam42() for r in refs])) if stored else None
    out = np.zeros((n, 2, 6, 6))
    dp = C.POINTER(C.c_double)
    w = pfc.configs.c1_boxes()
    m = pfc.configs.build_scenario(w)
    try:
        rc = pfc._lib.lib().pfc_selftest_kis(m._h, n, kc.ctypes.data_as(dp), dc.ctypes.data_as(dp),
                                             vl.ctypes.data_as(dp) if stored else None, out.ctypes.data_as(dp))
    finally:
        m.close()
    assert rc == 0
    out = out.transpose(0, 1, 3, 2)
    return out[:, 0], out[:, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("stored", [False, True], ids=["jacobi", "stored_v"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_device_per_entry(pfc, O, family, stored):
    refs = _cases(family, pfc)
    Kis, dKis = _device_kis(pfc, refs, stored)
    ratios = [r.entry_ratio(d) for r, d in zip(refs, dKis)]
    tag = "stored_v" if stored else "jacobi"
    print(f"device[{tag}] {family}: {len(refs)} matrices, worst |E_ij| / bound_ij = {max(ratios):.3g}")
    bad = [(k, refs[k].lam.tolist(), q) for k, q in enumerate(ratios) if not q <= 1.0]
    assert not bad, bad
    if not stored:
        _, oKis = O.kis_dual(*_stack(refs))
        pr = [r.pair_ratio(d, o) for r, d, o in zip(refs, dKis, oKis)]
        print(f"device - oracle {family}: worst |E_ij| / bound_ij = {max(pr):.3g}")
        bad = [(k, q) for k, q in enumerate(pr) if not q <= 1.0]
        assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("stored", [False, True], ids=["jacobi", "stored_v"])
@pytest.mark.parametrize("family", NORMWISE)
def test_device_normwise(pfc, family, stored):
    refs = _cases(family, pfc)
    Kis, dKis = _device_kis(pfc, refs, stored)
    for k, r in enumerate(refs):
        ev, ed = r.normwise(Kis[k], dKis[k])
        assert ev <= 1e-13 and ed <= 1e-12, (family, k, ev, ed, r.lam)
