// pfc_radau.h -- parts of the simplified-Newton Radau IIA step of the reference's integrator (src/radau/radau_functions.jl,
// radau_solve.jl), rules 1 and 2, for a batch of independent scenes of NX <= 64 states: the factorisations of updateInvC!
// (k_radau_factor; pfc_radau_factor_device), one iteration of simple_newton! -- calcEw!, the solves, updateStageX! and the
// loop's bookkeeping (k_radau_newton; pfc_radau_newton_device) --, the end of an attempt (k_radau_finish) and the elementwise parts
// around them: seed_indices! (k_radau_seed), write_indices! (k_radau_jac), the stage states into the evaluation's inputs
// (k_radau_unpack).  pfc_radau_step (pfc_hip.hip) strings them together with the state-derivative calls; pfc_radau_integrate runs
// the same body to per-scene end times with k_radau_finish<true>, which records the trajectory and parks the scenes that have arrived
// (k_radau_set_end starts a trajectory).  k_radau_control is the zero-order-hold joint controller that runs at the top of a batch
// step when pfc_radau_set_controller gave one (the reference's DiscreteControl, src/example_integrator.jl:25-30).
// Included by pfc_hip.hip inside namespace pfc (device code only), after pfc_dyn.h.
//
// Arithmetic (the contract, stated in include/pfc.h): plain Float64, every sum in a written order, no fma (the build has
// -ffp-contract=off); complex product and quotient by the textbook formulas, written out (rad_mul, rad_div).
// One 64-lane workgroup (one wave) per (scene, factor) in k_radau_factor and per scene in k_radau_newton; lane = row of the matrix
// = index of the state.
//   k_radau_factor  -J + (lam / h) I into LDS, column-major (lane = row: neighbouring lanes, neighbouring words; 8 NX^2 bytes for
//               the real factor, 16 NX^2 = 64 KiB at the cap for the complex one -- nothing else is kept in LDS: the pivot search is a
//               wave reduction, the row permutation a register per lane); right-looking LU with partial pivoting, the pivot the first
//               row of maximal |re| + |im|; L (unit diagonal, not stored) and U over each other, the permutation and the flag out.
//               Factor 0 is real (lam_1), factor 1, rule 2 only, complex (lam_2).  The matrix of lam_3 = conj(lam_2) is the
//               conjugate of factor 1 (J is real) and is not factored.
//   k_radau_newton  nothing in LDS: a lane keeps its component of every vector in registers, a sum over the states is a wave
//               butterfly (rad_wave_sum: the written order), the substitutions broadcast one unknown at a time with a lane read and
//               read a column of the factor from global memory, lane = row (coalesced); the loads of a column do not depend on the
//               unknowns, so several are in flight.
// No index is followed out of range: n_scene bounds the grids, nx <= 64 and the layout sizes are validated on the host, a lane
// i >= nx reads and writes nothing, the permutation read back from memory is used as a lane index only (it wraps at 64), the item
// indices of the bristle rows are kernel arguments, validated on the host against n_ips.
#pragma once

constexpr int kRadWave = 64;                 // lanes per workgroup: PFC_MAX_NX_RADAU
constexpr int kRadMaxBr = kRadWave / 6;      // bristle items of a scene: 6 states each

struct RadC { double re, im; };

__device__ inline double rad_mag(double a) { return fabs(a); }
__device__ inline double rad_mag(RadC a) { return fabs(a.re) + fabs(a.im); }
__device__ inline bool rad_is_zero(double a) { return a == 0.0; }
__device__ inline bool rad_is_zero(RadC a) { return a.re == 0.0 && a.im == 0.0; }
__device__ inline double rad_sub(double a, double b) { return a - b; }
__device__ inline RadC rad_sub(RadC a, RadC b) { return RadC{a.re - b.re, a.im - b.im}; }
__device__ inline double rad_mul(double a, double b) { return a * b; }
__device__ inline RadC rad_mul(RadC a, RadC b) { return RadC{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ inline double rad_div(double a, double b) { return a / b; }
__device__ inline RadC rad_div(RadC a, RadC b) {
    const double den = b.re * b.re + b.im * b.im;
    return RadC{(a.re * b.re + a.im * b.im) / den, (a.im * b.re - a.re * b.im) / den};
}
__device__ inline double rad_lane(double a, int lane) { return __shfl(a, lane, kRadWave); }
__device__ inline RadC rad_lane(RadC a, int lane) { return RadC{__shfl(a.re, lane, kRadWave), __shfl(a.im, lane, kRadWave)}; }
// An entry of -J + shift I.
__device__ inline double rad_entry(double j, bool diag, double shift) { return diag ? j + shift : j; }
__device__ inline RadC rad_entry(double j, bool diag, RadC shift) { return diag ? RadC{j + shift.re, shift.im} : RadC{j, 0.0}; }

// The sum over the wave in the written order: six exchange rounds, partner lane ^ 32, ^ 16, .. ^ 1, v = v + partner's v.
// Addition commutes, so every lane ends with the same bits.
__device__ inline double rad_wave_sum(double v) {
#pragma unroll
    for (int off = kRadWave / 2; off; off >>= 1) v = v + __shfl_xor(v, off, kRadWave);
    return v;
}
__device__ inline double rad_wave_max(double v) {
#pragma unroll
    for (int off = kRadWave / 2; off; off >>= 1) { const double o = __shfl_xor(v, off, kRadWave); v = o > v ? o : v; }
    return v;
}
// The first lane of maximal m (m is never NaN).
__device__ inline int rad_wave_argmax(double m, int i) {
    int idx = i;
#pragma unroll
    for (int off = kRadWave / 2; off; off >>= 1) {
        const double m2 = __shfl_xor(m, off, kRadWave);
        const int i2 = __shfl_xor(idx, off, kRadWave);
        if (m2 > m || (m2 == m && i2 < idx)) { m = m2; idx = i2; }
    }
    return idx;
}

struct RadauFactorArgs {
    int n_scene, nx;
    const double *neg_J;                // n_scene x nx x nx, column-major: -J(i, j) of scene s at (s nx + j) nx + i
    const double *h;                    // n_scene
    const int *rule;                    // n_scene: 1 or 2
    const int *active;                  // n_scene, or NULL (all): a scene whose word is 0 is left alone
    int active_stride;                  // words between two scenes' entries of active (the step passes its records: 8)
    double lam0[2], lam1_re, lam1_im;   // lam_1 of rule 1 and of rule 2; lam_2 of rule 2
    double *lu0;                        // n_scene x nx x nx, column-major
    double *lu1;                        // n_scene x nx x nx x 2 (re, im), column-major
    int *perm;                          // n_scene x 2 x nx: row i of P A is row perm[i] of A
    int *info;                          // n_scene x 2: 0, or k + 1 for the first column k whose pivot is zero
};

// A in LDS (n x n, column-major) -> P A = L U in place; lane i = row i.  Returns 0, or k + 1 at the first zero pivot (the same for
// every lane), where the factorisation stops: columns < k are final, the rest is the reduced matrix as it stands.
template <class T> __device__ inline int radau_lu(T *A, int n, int i, int &perm) {
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    perm = i;
    for (int k = 0; k < n; ++k) {
        double m = -1.0;
        if (i >= k && i < n) {
            m = rad_mag(A[k * n + i]);
            if (m != m) m = inf;
        }
        const int p = rad_wave_argmax(m, i);
        const T piv = A[k * n + p];
        if (rad_is_zero(piv)) return k + 1;
        __syncthreads();
        if (p != k) {
            if (i < n) { const T t = A[i * n + k]; A[i * n + k] = A[i * n + p]; A[i * n + p] = t; }      // lane = column
            const int a = __shfl(perm, k, kRadWave), b = __shfl(perm, p, kRadWave);
            if (i == k) perm = b; else if (i == p) perm = a;
        }
        __syncthreads();
        if (i > k && i < n) {
            const T l = rad_div(A[k * n + i], piv);
            A[k * n + i] = l;
            for (int j = k + 1; j < n; ++j) A[j * n + i] = rad_sub(A[j * n + i], rad_mul(l, A[j * n + k]));
        }
        __syncthreads();
    }
    return 0;
}

template <class T> __device__ inline void radau_factor_one(const RadauFactorArgs &g, int sc, T shift, T *A, T *out, int *perm_out, int *info_out) {
    const int n = g.nx, i = (int)threadIdx.x;
    const double *J = g.neg_J + (size_t)sc * (size_t)n * (size_t)n;
    for (int e = i; e < n * n; e += kRadWave) A[e] = rad_entry(J[e], e / n == e % n, shift);
    __syncthreads();
    int perm;
    const int bad = radau_lu<T>(A, n, i, perm);
    __syncthreads();
    for (int e = i; e < n * n; e += kRadWave) out[e] = A[e];
    if (i < n) perm_out[i] = perm;
    if (i == 0) *info_out = bad;
}

// Block 2 s + f: factor f of scene s.  One launch for both factors, so every block reserves the complex factor's 16 NX^2 bytes of
// LDS although a real one uses half of it: at the cap two blocks fit a CU's 160 KiB where five real ones would.  Two launches with
// exact sizes were measured and are slower at the batch sizes in use (64 scenes: 57 against 32 us at NX = 18, 357 against 204 us at
// NX = 64, profiles/radau_rate_run2.json against run3): the second launch waits for the first, and 2 n_scene one-wave blocks do
// not fill the device anyway.
__global__ void __launch_bounds__(kRadWave) k_radau_factor(RadauFactorArgs g) {
    extern __shared__ double rad_lds[];
    const int sc = (int)(blockIdx.x >> 1), f = (int)(blockIdx.x & 1u), n = g.nx;
    if (g.active && g.active[(size_t)sc * (size_t)g.active_stride] != 1) return;
    const int rule = g.rule[sc] == 2 ? 2 : 1;
    const double hinv = 1.0 / g.h[sc];
    const size_t nn = (size_t)n * (size_t)n;
    if (f == 0) {
        radau_factor_one<double>(g, sc, hinv * g.lam0[rule - 1], rad_lds, g.lu0 + (size_t)sc * nn, g.perm + (size_t)(2 * sc) * n, g.info + 2 * sc);
    } else if (rule == 2) {
        radau_factor_one<RadC>(g, sc, RadC{hinv * g.lam1_re, hinv * g.lam1_im}, reinterpret_cast<RadC *>(rad_lds),
                               reinterpret_cast<RadC *>(g.lu1) + (size_t)sc * nn, g.perm + (size_t)(2 * sc + 1) * n, g.info + 2 * sc + 1);
    } else if (threadIdx.x == 0) {
        g.info[2 * sc + 1] = 0;      // rule 1 has no second factor
    }
}

// What k_radau_newton reads of a rule's table (NS = 1 or 3 stages; A by rows with stride NS).
struct RadauTab {
    double A[9], lam0, lam1_re, lam1_im;
    double T0[3], T1_re[3], T1_im[3];           // columns 0 and 1 of T
    double Ti0[3], Ti1_re[3], Ti1_im[3];        // rows 0 and 1 of T^-1
};

// The state layout of a scene: x = [q (nq); v (nv); 6 per bristle item], the reference's copyto! (src/extensions.jl:21-51).
struct RadauLayout {
    int n_scene, nx, nq, nv, n_ips, n_br;
    int br_items[kRadMaxBr];            // n_br: the items of a scene whose s / sdot rows are states, increasing
};

// Words of a scene's integer and Float64 records (n_scene x 8 each).
// kRadIntSpare is the parked mark: 1 from the commit that took the scene past its end time or filled its last trajectory row
// (k_radau_finish<true>) until the records are reset; the callers without an end leave it 0.
enum { kRadIter = 0, kRadKIter, kRadFlag, kRadPhase, kRadAttempts, kRadExit, kRadExitIter, kRadIntSpare };
enum { kRadTheta = 0, kRadThetaPrev, kRadPsi, kRadRes1, kRadRes2, kRadRes, kRadHTaken, kRadDblSpare };

struct RadauNewtonArgs {
    RadauLayout L;
    int k_iter_max;
    double tol_newton;
    const double *qdot, *vdot, *sdot;   // F of the stage-scenes (stage n_scene + scene): 3 n_scene x nq, x nv; 3 n_scene n_ips x 6
    const double *x0, *h;               // n_scene x nx; n_scene
    const int *rule;                    // n_scene
    const double *lu0, *lu1;            // k_radau_factor's outputs
    const int *perm, *info;
    RadauTab tab[2];
    double *X;                          // 3 n_scene x nx: the stage states, row stage n_scene + scene
    double *F_save;                     // 3 n_scene x nx, or NULL: F of this iteration's stages, kept for k_radau_finish
    double *nstate;                     // n_scene x 8 (kRadTheta ..)
    int *istate;                        // n_scene x 8 (kRadIter ..)
    int *count;                         // += 1 per scene still iterating
};

// Component i of the derivative of (stage-)scene ss: [qdot; vdot; the sdot rows of the bristle items].
__device__ inline double radau_F(const RadauLayout &L, const double *qdot, const double *vdot, const double *sdot, size_t ss, int i) {
    if (i < L.nq) return qdot[ss * (size_t)L.nq + (size_t)i];
    i -= L.nq;
    if (i < L.nv) return vdot[ss * (size_t)L.nv + (size_t)i];
    i -= L.nv;
    return sdot[(ss * (size_t)L.n_ips + (size_t)L.br_items[i / 6]) * 6 + (size_t)(i % 6)];
}

// x = (P^-1 L U)^-1 b with k_radau_factor's factor: lane i enters with b_i and leaves with x_i.
template <class T> __device__ inline T radau_solve(const T *LU, const int *perm, int n, int i, T b) {
    const bool act = i < n;
    T acc = rad_lane(b, act ? perm[i] : i);
    // The column of step k + 1 is loaded before step k's arithmetic: the loads do not wait for the unknowns.
    T col = act && i > 0 ? LU[i] : T{};
    for (int k = 0; k < n; ++k) {           // L y = P b, k ascending; the diagonal of L is 1
        const T nxt = act && i > k + 1 ? LU[(size_t)(k + 1) * n + i] : T{};
        const T yk = rad_lane(acc, k);
        if (act && i > k) acc = rad_sub(acc, rad_mul(col, yk));
        col = nxt;
    }
    col = act ? LU[(size_t)(n - 1) * n + i] : T{};
    for (int k = n - 1; k >= 0; --k) {      // U x = y, k descending; lane k holds u_kk
        const T nxt = k > 0 && i < k ? LU[(size_t)(k - 1) * n + i] : T{};
        const T xk = rad_div(rad_lane(acc, k), rad_lane(col, k));
        if (i == k) acc = xk;
        if (i < k) acc = rad_sub(acc, rad_mul(col, xk));
        col = nxt;
    }
    return acc;
}

template <int NS> __device__ inline void radau_newton_scene(const RadauNewtonArgs &g, const RadauTab &tb, int sc) {
    const int n = g.L.nx, i = (int)threadIdx.x;
    const bool act = i < n;
    int *is = g.istate + 8 * (size_t)sc;
    double *st = g.nstate + 8 * (size_t)sc;
    const int k_iter = is[kRadKIter] + 1;
    if (g.info[2 * sc] != 0 || (NS == 3 && g.info[2 * sc + 1] != 0)) {      // a singular factor: exit flag 4
        if (i == 0) { is[kRadIter] = 0; is[kRadKIter] = k_iter; is[kRadFlag] = 4; }
        return;
    }
    const double h = g.h[sc], hinv = 1.0 / h, mh = -h;
    const double x0 = act ? g.x0[(size_t)sc * n + i] : 0.0;
    double X[NS], F[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const size_t ss = (size_t)s * (size_t)g.L.n_scene + (size_t)sc;
        X[s] = act ? g.X[ss * n + i] : 0.0;
        F[s] = act ? radau_F(g.L, g.qdot, g.vdot, g.sdot, ss, i) : 0.0;
        if (act && g.F_save) g.F_save[ss * n + i] = F[s];
    }
    // calcEw!: r_s = ((X_s - x0) + (-h A[s,0]) F_0) + ..., residual += r_s . r_s, Ew_j += ((1/h) lam_j Tinv[j,s]) r_s
    double residual = 0.0, e0 = 0.0;
    RadC e1{0.0, 0.0};
    const RadC l1{hinv * tb.lam1_re, hinv * tb.lam1_im};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        double r = X[s] - x0;
#pragma unroll
        for (int j = 0; j < NS; ++j) r = r + (mh * tb.A[s * NS + j]) * F[j];
        residual = residual + rad_wave_sum(r * r);
        e0 = e0 + ((hinv * tb.lam0) * tb.Ti0[s]) * r;
        if (NS == 3) {
            const RadC cf = rad_mul(l1, RadC{tb.Ti1_re[s], tb.Ti1_im[s]});
            e1.re = e1.re + cf.re * r;
            e1.im = e1.im + cf.im * r;
        }
    }
    const size_t nn = (size_t)n * (size_t)n;
    const double w0 = radau_solve<double>(g.lu0 + (size_t)sc * nn, g.perm + (size_t)(2 * sc) * n, n, i, e0);
    RadC w1{0.0, 0.0};
    if (NS == 3) w1 = radau_solve<RadC>(reinterpret_cast<const RadC *>(g.lu1) + (size_t)sc * nn, g.perm + (size_t)(2 * sc + 1) * n, n, i, e1);
    // Delta Z_s = T[s,0] w_0 + 2 Re(T[s,1] w_1)
    double dz[NS];
    bool finite = residual - residual == 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        dz[s] = tb.T0[s] * w0;
        if (NS == 3) dz[s] = dz[s] + 2.0 * (tb.T1_re[s] * w1.re - tb.T1_im[s] * w1.im);
        if (act && !(dz[s] - dz[s] == 0.0)) finite = false;
    }
    finite = __all(finite) != 0;
    int flag = -1, n_upd = 0;
    if (!finite) {
        flag = 3;
    } else {      // updateStageX!: stage by stage
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (flag < 0) {
                if (1.0e1 < rad_wave_max(act ? fabs(dz[s]) : 0.0)) flag = 3;
                else { X[s] = X[s] - dz[s]; n_upd = s + 1; }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s)
        if (act && s < n_upd) g.X[((size_t)s * (size_t)g.L.n_scene + (size_t)sc) * n + i] = X[s];
    double theta = st[kRadTheta], theta_prev = st[kRadThetaPrev], psi = st[kRadPsi], res1 = st[kRadRes1], res2 = st[kRadRes2];
    if (flag < 0) {
        if (residual < g.tol_newton) {
            flag = 0;
        } else {
            if (k_iter != 1) { theta_prev = theta; theta = sqrt(residual); psi = sqrt(theta_prev * theta); }
            else { theta = sqrt(residual); psi = theta; }
            const double res3 = res2;
            res2 = res1; res1 = residual;
            if (res3 < res2 && res2 < res1) flag = 3;
            else if (k_iter >= g.k_iter_max) flag = 1;
        }
    }
    if (i == 0) {
        st[kRadTheta] = theta; st[kRadThetaPrev] = theta_prev; st[kRadPsi] = psi; st[kRadRes1] = res1; st[kRadRes2] = res2;
        st[kRadRes] = residual != residual ? __longlong_as_double(0x7ff8000000000000ll) : residual;      // one NaN, whatever its sign
        is[kRadIter] = flag < 0 ? 1 : 0; is[kRadKIter] = k_iter; is[kRadFlag] = flag;
        if (flag < 0) atomicAdd(g.count, 1);
    }
}

__global__ void __launch_bounds__(kRadWave) k_radau_newton(RadauNewtonArgs g) {
    const int sc = (int)blockIdx.x;
    if (g.istate[8 * (size_t)sc + kRadIter] != 1) return;      // retired or converged: nothing of the scene is written
    if (g.rule[sc] == 2) radau_newton_scene<3>(g, g.tab[1], sc);
    else radau_newton_scene<1>(g, g.tab[0], sc);
}

// ---- the elementwise parts: one thread per entry, grid-stride ---------------------------------------------------------------------
constexpr int kRadBlock = 256;

// Column c of a scene's [q; v; s of every item] row -> the state index, or -1 for the s row of an item that is not bristle.
__device__ inline int radau_state_index(const RadauLayout &L, int c) {
    if (c < L.nq + L.nv) return c;
    const int it = (c - L.nq - L.nv) / 6, r = (c - L.nq - L.nv) % 6;
    int idx = -1;
    for (int b = 0; b < L.n_br; ++b)
        if (L.br_items[b] == it) idx = L.nq + L.nv + 6 * b + r;
    return idx;
}

// seed_indices!: the unit seeds of the chunk whose first state is j0 -- direction d seeds state j0 + d -- into the layouts of
// pfc_state_derivative_dual_device: dq (n_scene x n_dir x nq), dv (.. x nv), ds (n_scene n_ips x n_dir x 6).  Every entry is written.
struct RadauSeedArgs {
    RadauLayout L;
    int j0, n_dir;
    double *dq, *dv, *ds;
};

__global__ void __launch_bounds__(kRadBlock) k_radau_seed(RadauSeedArgs g) {
    const RadauLayout &L = g.L;
    const size_t width = (size_t)(L.nq + L.nv + 6 * L.n_ips), nd = (size_t)g.n_dir, total = (size_t)L.n_scene * nd * width;
    for (size_t e = (size_t)blockIdx.x * kRadBlock + threadIdx.x; e < total; e += (size_t)gridDim.x * kRadBlock) {
        const int c = (int)(e % width), d = (int)((e / width) % nd);
        const size_t s = e / (width * nd);
        const double val = radau_state_index(L, c) == g.j0 + d ? 1.0 : 0.0;
        if (c < L.nq) g.dq[(s * nd + d) * (size_t)L.nq + c] = val;
        else if (c < L.nq + L.nv) g.dv[(s * nd + d) * (size_t)L.nv + (c - L.nq)] = val;
        else {
            const int it = (c - L.nq - L.nv) / 6, r = (c - L.nq - L.nv) % 6;
            g.ds[((s * (size_t)L.n_ips + it) * nd + d) * 6 + r] = val;
        }
    }
}

// write_indices!: columns j0 .. j0 + n_dir of -J from the partials of a chunk; with `first`, xdot0 = [qdot; vdot; sdot] of the value
// buffers as well, and the scene is armed for the first attempt of a step -- unless it is retired with exit flag 5 (nothing is
// written) or parked at its end (kRadIntSpare != 0: its exit flag becomes 6 and its attempts 0).
struct RadauJacArgs {
    RadauLayout L;
    int j0, n_dir, first;
    const double *dqdot, *dvdot, *dsdot;    // n_scene x n_dir x nq, x nv; n_scene n_ips x n_dir x 6
    const double *qdot, *vdot, *sdot;       // n_scene x nq, x nv; n_scene n_ips x 6 (first only)
    double *neg_J, *xdot0;                  // n_scene x nx x nx column-major; n_scene x nx
    double *nstate;                         // may be NULL with istate: nothing is armed
    int *istate;
};

__global__ void __launch_bounds__(kRadBlock) k_radau_jac(RadauJacArgs g) {
    const RadauLayout &L = g.L;
    const size_t n = (size_t)L.nx, nd = (size_t)g.n_dir, rows = nd + (g.first ? 1 : 0), total = (size_t)L.n_scene * rows * n;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (size_t e = (size_t)blockIdx.x * kRadBlock + threadIdx.x; e < total; e += (size_t)gridDim.x * kRadBlock) {
        const int i = (int)(e % n), d = (int)((e / n) % rows);
        const size_t s = e / (n * rows);
        if (d < g.n_dir) {
            double p;
            if (i < L.nq) p = g.dqdot[(s * nd + d) * (size_t)L.nq + i];
            else if (i < L.nq + L.nv) p = g.dvdot[(s * nd + d) * (size_t)L.nv + (i - L.nq)];
            else {
                const int b = (i - L.nq - L.nv) / 6, r = (i - L.nq - L.nv) % 6;
                p = g.dsdot[((s * (size_t)L.n_ips + L.br_items[b]) * nd + d) * 6 + r];
            }
            g.neg_J[(s * n + (size_t)(g.j0 + d)) * n + i] = -p;
        } else {
            g.xdot0[s * n + i] = radau_F(L, g.qdot, g.vdot, g.sdot, s, i);
            if (i == 0 && g.istate && g.nstate && g.istate[8 * s + kRadExit] != 5) {
                int *is = g.istate + 8 * s;
                if (is[kRadIntSpare] == 0) {
                    is[kRadIter] = 1; is[kRadKIter] = 0; is[kRadFlag] = -1; is[kRadPhase] = 1; is[kRadAttempts] = 1;
                    g.nstate[8 * s + kRadRes1] = inf; g.nstate[8 * s + kRadRes2] = inf;
                } else {      // parked at its end (k_radau_finish<true>): exit flag 6, "at or past its end; nothing done"
                    is[kRadExit] = 6; is[kRadAttempts] = 0;
                }
            }
        }
    }
}

// The stage states into the (q, v, s) of the 3 n_scene stage-scenes pfc_state_derivative_device evaluates (the shape never changes).
// A scene at the start of an attempt (k_iter = 0) gets initialize_X_with_X0!: its three X rows become x0.  A scene that is not
// iterating is evaluated at x0 and ignored; the unused stages of a rule-1 scene carry its stage 0.  s rows of items that are not
// bristle are +0.0.
struct RadauUnpackArgs {
    RadauLayout L;
    const double *x0;                       // n_scene x nx
    const int *rule, *istate;
    double *X;                              // 3 n_scene x nx
    double *q, *v, *s;                      // 3 n_scene x nq, x nv; 3 n_scene n_ips x 6
};

__global__ void __launch_bounds__(kRadBlock) k_radau_unpack(RadauUnpackArgs g) {
    const RadauLayout &L = g.L;
    const size_t width = (size_t)(L.nq + L.nv + 6 * L.n_ips), ns = (size_t)L.n_scene, n = (size_t)L.nx, total = 3 * ns * width;
    for (size_t e = (size_t)blockIdx.x * kRadBlock + threadIdx.x; e < total; e += (size_t)gridDim.x * kRadBlock) {
        const int c = (int)(e % width);
        const size_t ss = e / width, sc = ss % ns, stage = ss / ns;
        const int i = radau_state_index(L, c);
        double val = 0.0;
        if (i >= 0) {
            const bool iterating = g.istate[8 * sc + kRadIter] == 1, start = g.istate[8 * sc + kRadKIter] == 0;
            const size_t src = g.rule[sc] == 2 ? stage : 0;
            val = !iterating || start ? g.x0[sc * n + i] : g.X[(src * ns + sc) * n + i];
            if (iterating && start) g.X[ss * n + i] = val;
        }
        if (c < L.nq) g.q[ss * (size_t)L.nq + c] = val;
        else if (c < L.nq + L.nv) g.v[ss * (size_t)L.nv + (c - L.nq)] = val;
        else g.s[ss * 6 * (size_t)L.n_ips + (size_t)(c - L.nq - L.nv)] = val;
    }
}

// ---- the end of an attempt: update_x_err_norm!, calc_and_update_h!, update_rule!, the commit or the re-arming -------------------
struct RadauFinishArgs {
    RadauLayout L;
    int k_iter_max, max_rule, cooldown_reset, n_mrp;
    int mrp_off[kRadMaxBr];                 // offsets in q of the floating joints' MRPs
    double tol_a, tol_r, h_max, h_min;
    double bhat0[2], bhat[2][3], a_last[2][3];      // per rule: bhat0, bhat, the last row of A
    const double *F;                        // 3 n_scene x nx: k_radau_newton's F_save (F of the attempt's last iteration)
    const double *xdot0, *X, *lu0;
    const int *perm;
    double *x, *t, *h;                      // n_scene x nx; n_scene; n_scene
    int *rule, *cool;                       // n_scene
    double *enorm;                          // n_scene x 2: x_err_norm, x_err_norm k+1
    double *nstate;
    int *istate;
    int *count;                             // += 1 per scene armed for another attempt
    // k_radau_finish<true> only: the end of each scene and its trajectory
    const double *t_final;                  // n_scene, or NULL (+inf): the scene parks at the commit that leaves t_final < t
    double *traj;                           // n_scene x max_rows x (1 + nx): row r of scene s at (s max_rows + r) (1 + nx), t then x
    int *rows;                              // n_scene: the rows written; a scene also parks at the commit that fills its last row
    int max_rows;                           // 0: nothing is recorded (traj and rows are not touched)
    int *live;                              // += 1 per scene that committed and did not park
};

// END = false: the step without ends.  END = true adds, at a commit: the row (t, x) after principal_value!, the row count, the park
// decision (kRadIntSpare = 1; kRadExit of the arriving step stays 0) and the count of scenes that go on.  A failed attempt and a
// retirement (exit flag 5) record nothing and count as not live.
template <bool END> __global__ void __launch_bounds__(kRadWave) k_radau_finish(RadauFinishArgs g) {
    const RadauLayout &L = g.L;
    const int sc = (int)blockIdx.x, n = L.nx, i = (int)threadIdx.x;
    const bool act = i < n;
    int *is = g.istate + 8 * (size_t)sc;
    double *st = g.nstate + 8 * (size_t)sc;
    if (is[kRadPhase] != 1 || is[kRadIter] != 0) return;      // no attempt of this scene has just ended
    const int flag = is[kRadFlag], k_iter = is[kRadKIter], attempts = is[kRadAttempts];
    const int rule = g.rule[sc] == 2 ? 2 : 1, r = rule - 1, NS = 2 * rule - 1;
    const double h = g.h[sc], psi = st[kRadPsi];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const double x0 = act ? g.x[(size_t)sc * n + i] : 0.0;
    double est, xf = 0.0, err = 0.0;
    if (flag == 0) {
        // Eq. 8.17: xhat - x = (0 + (bhat0 h) xdot0) + ((bhat_k - A[NS,k]) h) F_k ..; Eq. 8.19: the solve with factor 0; Eq. 8.21
        double v = 0.0 + (g.bhat0[r] * h) * (act ? g.xdot0[(size_t)sc * n + i] : 0.0);
        for (int k = 0; k < NS; ++k) {
            const double F = act ? g.F[((size_t)k * (size_t)L.n_scene + (size_t)sc) * n + i] : 0.0;
            v = v + ((g.bhat[r][k] - g.a_last[r][k]) * h) * F;
        }
        const double e = radau_solve<double>(g.lu0 + (size_t)sc * n * n, g.perm + (size_t)(2 * sc) * n, n, i, v);
        xf = act ? g.X[((size_t)(NS - 1) * (size_t)L.n_scene + (size_t)sc) * n + i] : 0.0;
        const double ax = fabs(xf), a0 = fabs(x0);
        const double sck = g.tol_a + (ax < a0 ? a0 : ax) * g.tol_r;
        const double qk = e / sck;
        err = sqrt(rad_wave_sum(act ? qk * qk : 0.0) / (double)n);
        // Eq. 8.25, first half; (1 / err)^(1 / (1 + NS)) by square roots
        const int k2 = 2 * g.k_iter_max;
        const double fac = (0.9 * (double)(k2 + 1)) / (double)(k2 + k_iter);
        const double inv = 1.0 / err;
        est = (fac * h) * (NS == 3 ? sqrt(sqrt(inv)) : sqrt(inv));
    } else {
        est = h * 0.1;
    }
    double h_new = g.h_max;
    if (2.0 * h < h_new) h_new = 2.0 * h;
    if (est < h_new) h_new = est;
    int new_rule = rule, cool = g.cool[sc];
    if (flag == 0) {
        cool -= 1;
        if (cool < 1 && psi < 0.1) new_rule = rule + 1 < g.max_rule ? rule + 1 : g.max_rule;
        double xi = xf;
        for (int m = 0; m < g.n_mrp; ++m) {      // principal_value!: sigma <- -sigma / |sigma|^2 where |sigma|^2 > 1
            const int o = g.mrp_off[m];
            const double s0 = rad_lane(xf, o), s1 = rad_lane(xf, o + 1), s2 = rad_lane(xf, o + 2);
            const double nn = (s0 * s0 + s1 * s1) + s2 * s2;
            if (nn > 1.0 && i >= o && i < o + 3) xi = -(xf / nn);
        }
        if (act) g.x[(size_t)sc * n + i] = xi;
        if (END) {
            if (g.max_rows > 0) {
                const int row = g.rows[sc];      // read by every lane before lane 0 writes it: the stores below follow the reads in program order
                if (act && row < g.max_rows) g.traj[((size_t)sc * (size_t)g.max_rows + (size_t)row) * (size_t)(1 + n) + 1 + (size_t)i] = xi;
            }
        }
    } else {
        cool = g.cooldown_reset;
        new_rule = rule - 1 > 1 ? rule - 1 : 1;
    }
    if (i == 0) {
        g.h[sc] = h_new; g.rule[sc] = new_rule; g.cool[sc] = cool;
        is[kRadExitIter] = k_iter;
        if (flag == 0) {
            g.enorm[2 * sc] = g.enorm[2 * sc + 1]; g.enorm[2 * sc + 1] = err;
            const double tn = g.t[sc] + h;
            g.t[sc] = tn;
            st[kRadHTaken] = h;
            is[kRadExit] = 0; is[kRadPhase] = 0;
            if (END) {
                bool park = g.t_final && g.t_final[sc] < tn;      // strict, as the reference's `while !(t_final < t)`
                if (g.max_rows > 0) {
                    const int row = g.rows[sc];
                    if (row < g.max_rows) {
                        g.traj[((size_t)sc * (size_t)g.max_rows + (size_t)row) * (size_t)(1 + n)] = tn;
                        g.rows[sc] = row + 1;
                    }
                    if (row + 1 >= g.max_rows) park = true;
                }
                if (park) is[kRadIntSpare] = 1; else atomicAdd(g.live, 1);
            }
        } else if (h_new < g.h_min) {
            is[kRadExit] = 5; is[kRadPhase] = 0;      // "time step is too small, something is wrong": x and t stay
        } else {
            is[kRadExit] = flag;
            is[kRadIter] = 1; is[kRadKIter] = 0; is[kRadFlag] = -1; is[kRadAttempts] = attempts + 1;
            st[kRadRes1] = inf; st[kRadRes2] = inf;
            atomicAdd(g.count, 1);
        }
    }
}

// ---- the end-setting call: row 0 of every scene's trajectory = its (t, x) now, one row counted, no scene parked -------------------
struct RadauSetEndArgs {
    int n_scene, nx, max_rows;              // max_rows = 0: no trajectory (traj and rows may be NULL)
    const double *x, *t;                    // n_scene x nx; n_scene
    double *traj;                           // n_scene x max_rows x (1 + nx)
    int *rows;                              // n_scene
    int *istate;                            // n_scene x 8: kRadIntSpare <- 0
};

__global__ void __launch_bounds__(kRadBlock) k_radau_set_end(RadauSetEndArgs g) {
    const size_t w = (size_t)(1 + g.nx), total = (size_t)g.n_scene * w;
    for (size_t e = (size_t)blockIdx.x * kRadBlock + threadIdx.x; e < total; e += (size_t)gridDim.x * kRadBlock) {
        const size_t s = e / w;
        const int c = (int)(e % w);
        if (g.max_rows > 0) g.traj[s * (size_t)g.max_rows * w + (size_t)c] = c == 0 ? g.t[s] : g.x[s * (size_t)g.nx + (size_t)(c - 1)];
        if (c == 0) {
            if (g.rows) g.rows[s] = g.max_rows > 0 ? 1 : 0;
            g.istate[8 * s + kRadIntSpare] = 0;
        }
    }
}

// ---- the discrete controller: the reference's DiscreteControl loop and a computed-torque PD law, once per batch step -----------------
// The statement is in include/pfc.h (pfc_radau_control_device).  One wave per scene, lane i = coordinate i (nv <= 64); lane b < n_act
// also computes the clamped acc of actuated coordinate act[b], which the row sums read with a lane read, b ascending.  The t_last
// loop and the segment search depend on the scene only: wave-uniform.  Nothing in LDS, no scratch, plain vector stores, no atomics.
// Every lane stays until the last lane read: the early returns above it are taken by the whole wave.
// No index is followed out of range: n_scene bounds the grid, nv, nq <= 64, n_act <= nv and act[] < min(nq, nv) are validated on the
// host, the segment index is a count of at most n_seg - 1 comparisons, lanes >= nv load and store nothing.
constexpr int kRadMaxFires = 4096;          // PFC_RADAU_MAX_FIRES: additions to t_last per scene and call

struct RadauControlArgs {
    int n_scene, nq, nv, n_act, n_seg;
    double dt;
    const int *act;                         // n_act: the actuated coordinates, strictly increasing, < min(nq, nv)
    const double *kp, *kd, *a_max;          // n_act
    const double *seg_t;                    // n_scene x n_seg: entry 0 of a scene is not read
    const double *seg_q;                    // n_scene x n_seg x n_act
    const double *seg_ff;                   // n_scene x n_seg x nv, or NULL (zeros)
    const double *t, *q, *v, *H, *c;        // n_scene; n_scene x nq; x nv; x nv x nv row-major; x nv
    const int *istate;                      // n_scene x 8, or NULL: a scene with exit flag 5 or the parked mark is left alone
    double *t_last;                         // n_scene
    int *fires;                             // n_scene: += the additions to t_last
    double *tau;                            // 3 n_scene x nv: rows scene, n_scene + scene, 2 n_scene + scene
};

__global__ void __launch_bounds__(kRadWave) k_radau_control(RadauControlArgs g) {
    const int sc = (int)blockIdx.x, i = (int)threadIdx.x, nv = g.nv;
    if (g.istate && (g.istate[8 * (size_t)sc + kRadExit] == 5 || g.istate[8 * (size_t)sc + kRadIntSpare] != 0)) return;
    const double t = g.t[sc];
    double t_last = g.t_last[sc];
    int fires = 0;
    while (t_last <= t && fires < kRadMaxFires) { t_last = t_last + g.dt; ++fires; }
    if (fires == 0) return;                 // not due: tau is held
    const double *st = g.seg_t + (size_t)sc * (size_t)g.n_seg;
    int k = 0;
    for (int j = 1; j < g.n_seg; ++j) k += st[j] <= t ? 1 : 0;
    const size_t seg = (size_t)sc * (size_t)g.n_seg + (size_t)k;
    double acc = 0.0;
    if (i < g.n_act) {
        const int co = g.act[i];
        const double e = g.q[(size_t)sc * (size_t)g.nq + (size_t)co] - g.seg_q[seg * (size_t)g.n_act + (size_t)i];
        acc = (-(g.kd[i] * g.v[(size_t)sc * (size_t)nv + (size_t)co])) - g.kp[i] * e;
        const double am = g.a_max[i];
        if (acc < -am) acc = -am;
        if (acc > am) acc = am;
    }
    const bool lane = i < nv;
    const double *Hrow = g.H + ((size_t)sc * (size_t)nv + (size_t)(lane ? i : 0)) * (size_t)nv;
    const double ff = lane && g.seg_ff ? g.seg_ff[seg * (size_t)nv + (size_t)i] : 0.0;
    const double ci = lane ? g.c[(size_t)sc * (size_t)nv + (size_t)i] : 0.0;
    double sum = 0.0;
    bool actuated = false;
    for (int b = 0; b < g.n_act; ++b) {
        const int co = g.act[b];
        const double ab = rad_lane(acc, b);
        if (lane) sum = sum + Hrow[co] * ab;
        actuated = actuated || co == i;
    }
    const double tau = actuated ? (sum + ci) + ff : ff;
    if (lane) {
        const size_t ns = (size_t)g.n_scene;
        g.tau[((size_t)sc) * (size_t)nv + (size_t)i] = tau;
        g.tau[(ns + (size_t)sc) * (size_t)nv + (size_t)i] = tau;
        g.tau[(2 * ns + (size_t)sc) * (size_t)nv + (size_t)i] = tau;
    }
    if (i == 0) { g.t_last[sc] = t_last; g.fires[sc] = g.fires[sc] + fires; }
}
