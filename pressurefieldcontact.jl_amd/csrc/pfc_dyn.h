// pfc_dyn.h -- forward dynamics from joint states (pfc_set_inertia, pfc_dynamics[_device], pfc_accelerations[_device],
// pfc_state_derivative[_device]): what configuration_derivative!, mass_matrix!, dynamics_bias!, sum_all_forces!, cholesky! and ldiv!
// (src/contact_algorithms_non_friction.jl:18-52) give the reference per evaluation -- qdot, the mass matrix H, the bias c and
// vdot = H^-1 ((f - c) + tau) -- formed on the device from (q, v), pfc_kinematics_device's poses and twists and the bodies' inertias.
// Included by pfc_hip.hip inside namespace pfc (device code only), after pfc_kin.h.
//
// Arithmetic (the contract, stated in include/pfc.h): plain Float64, every dot product and every subtree sum in a written order, no
// fma (the build has -ffp-contract=off), no atomics.  One statement over the number type T (dyn_inertia_to_world, dyn_mul,
// dyn_crossm, dyn_crossf, dyn_dot6, dyn_add, dyn_mrp_rate), as kin_*<T> are: a later Dual instantiation on ScatDual restates nothing.
// The motion-subspace columns are formed again from the world poses with kin_column<double> -- a column depends on the pose and the
// axis only, so these are S_w's bytes -- and nothing is read from the handle's S_w buffer.
// The kernels, one 64-lane workgroup (one wave) per scene, the scene's intermediate tables in LDS, a workgroup barrier between stages:
//   k_dynamics  (1) lanes over bodies: qdot; the body's world inertia, its joint's columns S and the joint twist S_b v_b
//               (2) lanes over bodies: the bias acceleration a_b along the root -> b path, the body wrench w_b
//               (3) lanes over bodies: composite inertia and joint wrench, summed over the subtree in increasing body order
//               (4) lanes over coordinates: F_i = Ic_body(i) S_i, c_i = S_i . W_body(i)
//               (5) lanes over the nv x nv entries: H[i,j] = S_j . F_i for j <= i where anc says so, +0.0 otherwise, and its mirror
//               A stage whose outputs nobody asked for is skipped (uniformly: the flags are kernel arguments).
//   k_accel     the lower triangle of H into LDS (column-major: lane = row, so neighbouring lanes read neighbouring words), the
//               left-looking Cholesky factorisation one column at a time, the two substitutions one unknown at a time; lane = row.
// No id is followed out of range: the tables are validated on the host, n_scene bounds the grids, every loop over bodies,
// coordinates or entries is bounded by n_body, nv or nv^2, and the LDS the host asks for is computed from the same n_body and nv.
#pragma once

constexpr int kDynWave = 64;                 // lanes per workgroup of k_dynamics and k_accel
constexpr int kDynBodyDoubles = 44;          // LDS doubles per body: I (10), tw (6), S_b v_b (6), w (6), Ic (10), W (6)
constexpr int kDynCoordDoubles = 12;         // LDS doubles per coordinate: S (6), F (6)
constexpr size_t kDynMaxLds = 64 * 1024;     // what a workgroup may ask for without an opt-in

__host__ __device__ inline size_t dyn_lds_bytes(int n_body, int nv) {
    return sizeof(double) * ((size_t)kDynBodyDoubles * (size_t)n_body + (size_t)kDynCoordDoubles * (size_t)nv) + sizeof(int) * (size_t)nv;
}
__host__ __device__ inline size_t accel_lds_bytes(int nv) { return sizeof(double) * ((size_t)nv * (size_t)nv + (size_t)nv) + sizeof(int); }

struct DynArgs {
    KinArgs k;                          // the tables, n_scene, q and v; its outputs are not read
    const double *inertia;              // n_body x 13: moment (9, column-major, about the frame origin), m com (3), m
    const int *sub_off, *sub;           // CSR: the subtree of b, b first and in increasing body order, is sub[sub_off[b] .. sub_off[b + 1])
    double g[3];                        // gravity, world
    const double *x_w_b, *twist_w_b;    // n_scene n_body x 12, x 6: pfc_kinematics_device's outputs
    double *qdot, *H, *c;               // n_scene x nq, x nv x nv, x nv; each may be NULL (not wanted)
};

struct AccelArgs {
    int n_scene, nv;
    const double *H, *c, *f, *tau;      // n_scene x nv x nv, x nv, x nv, x nv (tau may be NULL: zeros)
    double *vdot;                       // n_scene x nv
    int *info;                          // n_scene, or NULL
};

// a x b for 3-vectors.
template <class T> __device__ inline void dyn_cross(const T *a, const T *b, T *o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// A body's spatial inertia in world about the world origin, I (10) = [J00 J01 J02 J11 J12 J22; h (3); m], from its record in the
// body frame (13: moment M column-major, cross_part cp = m com, m) and the body's world pose x = (R, t).
template <class T> __device__ inline void dyn_inertia_to_world(const T *in, const T *x, T *I) {
    const T two = kin_lit<T>(2.0);
    const T m = in[12];
    const T *t = x + 9;
    T hc[3], mt[3], B[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        hc[r] = (x[r] * in[9] + x[3 + r] * in[10]) + x[6 + r] * in[11];
        mt[r] = m * t[r];
        I[6 + r] = hc[r] + mt[r];
    }
    I[9] = m;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) B[3 * c + r] = (x[r] * in[3 * c] + x[3 + r] * in[3 * c + 1]) + x[6 + r] * in[3 * c + 2];   // B = R M
    const T s1 = (t[0] * hc[0] + t[1] * hc[1]) + t[2] * hc[2];
    const T s2 = (t[0] * mt[0] + t[1] * mt[1]) + t[2] * mt[2];
    const T d = two * s1 + s2;
    int e = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = r; c < 3; ++c) {
            const T A = (B[r] * x[c] + B[3 + r] * x[3 + c]) + B[6 + r] * x[6 + c];                   // (R M R')_rc
            const T J = (A - (hc[r] * t[c] + t[r] * hc[c])) - mt[r] * t[c];
            I[e++] = r == c ? J + d : J;
        }
}

// o (6, a wrench [moment; force]) = I m for a motion vector m = [ang; lin].
template <class T> __device__ inline void dyn_mul(const T *I, const T *m, T *o) {
    const T *h = I + 6;
    o[0] = ((I[0] * m[0] + I[1] * m[1]) + I[2] * m[2]) + (h[1] * m[5] - h[2] * m[4]);
    o[1] = ((I[1] * m[0] + I[3] * m[1]) + I[4] * m[2]) + (h[2] * m[3] - h[0] * m[5]);
    o[2] = ((I[2] * m[0] + I[4] * m[1]) + I[5] * m[2]) + (h[0] * m[4] - h[1] * m[3]);
    o[3] = I[9] * m[3] - (h[1] * m[2] - h[2] * m[1]);
    o[4] = I[9] * m[4] - (h[2] * m[0] - h[0] * m[2]);
    o[5] = I[9] * m[5] - (h[0] * m[1] - h[1] * m[0]);
}

// o = a x_m b, the motion cross product: [a_ang x b_ang; (a_ang x b_lin) + (a_lin x b_ang)].
template <class T> __device__ inline void dyn_crossm(const T *a, const T *b, T *o) {
    T p[3], q[3];
    dyn_cross<T>(a, b, o);
    dyn_cross<T>(a, b + 3, p);
    dyn_cross<T>(a + 3, b, q);
#pragma unroll
    for (int r = 0; r < 3; ++r) o[3 + r] = p[r] + q[r];
}

// o = a x* f, the force cross product: [(a_ang x f_mom) + (a_lin x f_lin); a_ang x f_lin].
template <class T> __device__ inline void dyn_crossf(const T *a, const T *f, T *o) {
    T p[3], q[3];
    dyn_cross<T>(a, f, p);
    dyn_cross<T>(a + 3, f + 3, q);
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = p[r] + q[r];
    dyn_cross<T>(a, f + 3, o + 3);
}

template <class T> __device__ inline T dyn_dot6(const T *a, const T *b) {
    return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5];
}

// qdot (6) of a floating joint: pdot = 1/4 [((1 - p.p) w + 2 (p x w)) + (2 (p.w)) p], tdot = R_j(p) v_lin; q = [p; t], v = [w; v_lin]
// in the frame after.
template <class T> __device__ inline void dyn_mrp_rate(const T *q, const T *v, T *qd) {
    const T one = kin_lit<T>(1.0), two = kin_lit<T>(2.0), quarter = kin_lit<T>(0.25);
    const T p2 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
    const T pw = (q[0] * v[0] + q[1] * v[1]) + q[2] * v[2];
    const T a = one - p2, b = two * pw;
    T cr[3], xj[12], tj[6], ax[3] = {kin_lit<T>(0.0), kin_lit<T>(0.0), kin_lit<T>(0.0)};
    dyn_cross<T>(q, v, cr);
#pragma unroll
    for (int r = 0; r < 3; ++r) qd[r] = quarter * ((a * v[r] + two * cr[r]) + b * q[r]);
    kin_joint<T>(PFC_JOINT_FLOATING_MRP, ax, q, (const T *)nullptr, xj, tj);
#pragma unroll
    for (int r = 0; r < 3; ++r) qd[3 + r] = (xj[r] * v[3] + xj[3 + r] * v[4]) + xj[6 + r] * v[5];
}

__global__ void __launch_bounds__(kDynWave) k_dynamics(DynArgs d) {
    extern __shared__ double dyn_lds[];
    const KinArgs &g = d.k;
    const int nb = g.n_body, nv = g.nv, tid = (int)threadIdx.x, sc = (int)blockIdx.x;
    double *sI = dyn_lds, *sTw = sI + 10 * nb, *sJt = sTw + 6 * nb, *sW = sJt + 6 * nb, *sIc = sW + 6 * nb, *sWc = sIc + 10 * nb;
    double *sS = sWc + 6 * nb, *sF = sS + 6 * nv;
    int *sBody = reinterpret_cast<int *>(sF + 6 * nv);
    const double *q = g.q + (size_t)sc * (size_t)g.nq;
    const double *v = g.v + (size_t)sc * (size_t)nv;
    const bool want_H = d.H != nullptr, want_c = d.c != nullptr;

    // (1) qdot; world inertia, columns, joint twist
    for (int b = tid; b < nb; b += kDynWave) {
        const int type = g.jtype[b], n = kin_joint_nq(type), vo = g.voff[b];
        if (d.qdot) {
            double *out = d.qdot + (size_t)sc * (size_t)g.nq + (size_t)g.qoff[b];
            if (type == PFC_JOINT_FLOATING_MRP) {
                double qd[6];
                dyn_mrp_rate<double>(q + g.qoff[b], v + vo, qd);
#pragma unroll
                for (int e = 0; e < 6; ++e) out[e] = qd[e];
            } else if (n == 1) {
                out[0] = v[vo];
            }
        }
        if (want_H || want_c) {
            double x[12], in[13], I[10], ax[3], o[6], jt[6];
            const double *xin = d.x_w_b + 12 * ((size_t)sc * (size_t)nb + (size_t)b);
#pragma unroll
            for (int e = 0; e < 12; ++e) x[e] = xin[e];
#pragma unroll
            for (int e = 0; e < 13; ++e) in[e] = d.inertia[13 * (size_t)b + e];
#pragma unroll
            for (int e = 0; e < 3; ++e) ax[e] = g.axis[3 * (size_t)b + e];
            dyn_inertia_to_world<double>(in, x, I);
#pragma unroll
            for (int e = 0; e < 10; ++e) sI[10 * b + e] = I[e];
#pragma unroll
            for (int e = 0; e < 6; ++e) jt[e] = 0.0;
            for (int k = 0; k < n; ++k) {
                kin_column<double>(type, k, ax, x, o);
                sBody[vo + k] = b;
#pragma unroll
                for (int e = 0; e < 6; ++e) {
                    sS[6 * (vo + k) + e] = o[e];
                    if (want_c) jt[e] = k == 0 ? o[e] * v[vo] : jt[e] + o[e] * v[vo + k];
                }
            }
            if (want_c) {
                const double *twin = d.twist_w_b + 6 * ((size_t)sc * (size_t)nb + (size_t)b);
#pragma unroll
                for (int e = 0; e < 6; ++e) { sTw[6 * b + e] = twin[e]; sJt[6 * b + e] = jt[e]; }
            }
        }
    }
    if (!want_H && !want_c) return;
    __syncthreads();

    // (2) bias acceleration along the path, body wrench
    if (want_c) {
        for (int b = tid; b < nb; b += kDynWave) {
            double a[6] = {0.0, 0.0, 0.0, -d.g[0], -d.g[1], -d.g[2]}, o[6], w1[6], w2[6], w3[6];
            for (int k = g.path_off[b]; k < g.path_off[b + 1]; ++k) {
                const int p = g.path[k];
                dyn_crossm<double>(sTw + 6 * p, sJt + 6 * p, o);
#pragma unroll
                for (int e = 0; e < 6; ++e) a[e] = a[e] + o[e];
            }
            dyn_mul<double>(sI + 10 * b, a, w1);
            dyn_mul<double>(sI + 10 * b, sTw + 6 * b, w2);
            dyn_crossf<double>(sTw + 6 * b, w2, w3);
#pragma unroll
            for (int e = 0; e < 6; ++e) sW[6 * b + e] = w1[e] + w3[e];
        }
        __syncthreads();
    }

    // (3) composite inertia, joint wrench: the subtree in increasing body order, b itself first
    for (int b = tid; b < nb; b += kDynWave) {
        const int s0 = d.sub_off[b], s1 = d.sub_off[b + 1];
        if (want_H) {
            double I[10];
#pragma unroll
            for (int e = 0; e < 10; ++e) I[e] = sI[10 * b + e];
            for (int k = s0 + 1; k < s1; ++k) {
                const int p = d.sub[k];
#pragma unroll
                for (int e = 0; e < 10; ++e) I[e] = I[e] + sI[10 * p + e];
            }
#pragma unroll
            for (int e = 0; e < 10; ++e) sIc[10 * b + e] = I[e];
        }
        if (want_c) {
            double W[6];
#pragma unroll
            for (int e = 0; e < 6; ++e) W[e] = sW[6 * b + e];
            for (int k = s0 + 1; k < s1; ++k) {
                const int p = d.sub[k];
#pragma unroll
                for (int e = 0; e < 6; ++e) W[e] = W[e] + sW[6 * p + e];
            }
#pragma unroll
            for (int e = 0; e < 6; ++e) sWc[6 * b + e] = W[e];
        }
    }
    __syncthreads();

    // (4) F_i = Ic S_i; c_i = S_i . W
    for (int i = tid; i < nv; i += kDynWave) {
        const int b = sBody[i];
        if (want_H) {
            double F[6];
            dyn_mul<double>(sIc + 10 * b, sS + 6 * i, F);
#pragma unroll
            for (int e = 0; e < 6; ++e) sF[6 * i + e] = F[e];
        }
        if (want_c) d.c[(size_t)sc * (size_t)nv + (size_t)i] = dyn_dot6<double>(sS + 6 * i, sWc + 6 * b);
    }
    if (!want_H) return;
    __syncthreads();

    // (5) H: the lower triangle and its mirror
    double *H = d.H + (size_t)sc * (size_t)nv * (size_t)nv;
    for (int e = tid; e < nv * nv; e += kDynWave) {
        const int i = e / nv, j = e % nv;
        if (j > i) continue;
        const double h = g.anc[(size_t)sBody[i] * (size_t)nv + (size_t)j] ? dyn_dot6<double>(sS + 6 * j, sF + 6 * i) : 0.0;
        H[(size_t)i * nv + j] = h;
        H[(size_t)j * nv + i] = h;
    }
}

// vdot = H^-1 ((f - c) + tau) by H = L L', L y = rhs, L' x = y, in the order include/pfc.h states.  nv <= kDynWave: lane = row.
__global__ void __launch_bounds__(kDynWave) k_accel(AccelArgs g) {
    extern __shared__ double dyn_lds[];
    const int nv = g.nv, i = (int)threadIdx.x, sc = (int)blockIdx.x;
    double *L = dyn_lds, *sv = L + nv * nv;      // L(i, j) at L[j nv + i]
    int *flag = reinterpret_cast<int *>(sv + nv);
    const double *H = g.H + (size_t)sc * (size_t)nv * (size_t)nv;
    const size_t row = (size_t)sc * (size_t)nv;
    const bool act = i < nv;
    for (int e = i; e < nv * nv; e += kDynWave) {
        const int r = e / nv, c = e % nv;
        if (c <= r) L[c * nv + r] = H[e];
    }
    if (i == 0) *flag = 0;
    double acc = 0.0;
    if (act) acc = (g.f[row + i] - g.c[row + i]) + (g.tau ? g.tau[row + i] : 0.0);
    __syncthreads();
    for (int j = 0; j < nv; ++j) {
        double s = 0.0;
        if (act && i >= j) {
            s = L[j * nv + i];
            for (int k = 0; k < j; ++k) s = s - L[k * nv + i] * L[k * nv + j];
        }
        if (i == j) {
            if (s > 0.0) L[j * nv + j] = sqrt(s);
            else *flag = j + 1;      // not > 0, or NaN
        }
        __syncthreads();
        if (*flag) break;            // the same word for every lane
        if (act && i > j) L[j * nv + i] = s / L[j * nv + j];
        __syncthreads();
    }
    const int bad = *flag;
    if (!bad) {
        for (int k = 0; k < nv; ++k) {          // L y = rhs, k ascending
            if (i == k) sv[k] = acc / L[k * nv + k];
            __syncthreads();
            if (act && i > k) acc = acc - L[k * nv + i] * sv[k];
        }
        if (act) acc = sv[i];
        __syncthreads();
        for (int k = nv - 1; k >= 0; --k) {     // L' x = y, k descending
            if (i == k) sv[k] = acc / L[k * nv + k];
            __syncthreads();
            if (act && i < k) acc = acc - L[i * nv + k] * sv[k];
        }
    }
    if (act) g.vdot[row + i] = bad ? __longlong_as_double(0x7ff8000000000000ll) : sv[i];
    if (i == 0 && g.info) g.info[sc] = bad;
}
