// pfc_dyn.h -- forward dynamics from joint states (pfc_set_inertia, pfc_dynamics[_device], pfc_accelerations[_device],
// pfc_state_derivative[_device]): what configuration_derivative!, mass_matrix!, dynamics_bias!, sum_all_forces!, cholesky! and ldiv!
// (src/contact_algorithms_non_friction.jl:18-52) give the reference per evaluation -- qdot, the mass matrix H, the bias c and
// vdot = H^-1 ((f - c) + tau) -- formed on the device from (q, v), pfc_kinematics_device's poses and twists and the bodies' inertias.
// Included by pfc_hip.hip inside namespace pfc (device code only), after pfc_kin.h.
//
// Arithmetic (the contract, stated in include/pfc.h): plain Float64, every dot product and every subtree sum in a written order, no
// fma (the build has -ffp-contract=off), no atomics.  One statement over the number type T (dyn_inertia_to_world, dyn_mul,
// dyn_crossm, dyn_crossf, dyn_dot6, dyn_mrp_rate and the five stages themselves, dyn_stages<T>), as kin_*<T> are: the Dual
// instantiation on ScatDual (pfc_dynamics_dual[_device]) restates nothing.  DynIo<T> is what differs: where a stage's numbers come
// from and which part of a result is stored.
// The motion-subspace columns are formed again from the world poses with kin_column<double> -- a column depends on the pose and the
// axis only, so these are S_w's bytes -- and nothing is read from the handle's S_w buffer.
// The kernels, one 64-lane workgroup (one wave) per scene, the scene's intermediate tables in LDS, a workgroup barrier between stages:
//   k_dynamics  (1) lanes over bodies: qdot; the body's world inertia, its joint's columns S and the joint twist S_b v_b
//               (2) lanes over bodies: the bias acceleration a_b along the root -> b path, the body wrench w_b
//               (3) lanes over bodies: composite inertia and joint wrench, summed over the subtree in increasing body order
//               (4) lanes over coordinates: F_i = Ic_body(i) S_i, c_i = S_i . W_body(i)
//               (5) lanes over the nv x nv entries: H[i,j] = S_j . F_i for j <= i where anc says so, +0.0 otherwise, and its mirror
//               A stage whose outputs nobody asked for is skipped (uniformly: the flags are kernel arguments).
//   k_dynamics_dual  the same five stages on ScatDual, one workgroup per (scene, direction): the partials of qdot, H and c; the tables
//               in LDS are twice the value tables (the host refuses a mechanism whose Dual tables exceed 64 KiB).
//   k_accel     the lower triangle of H into LDS (column-major: lane = row, so neighbouring lanes read neighbouring words), the
//               left-looking Cholesky factorisation one column at a time (accel_factor), the two substitutions one unknown at a
//               time (accel_solve<1>); lane = row.
//   k_accel_dual<N>  accel_factor and accel_solve<1> as k_accel (vdot), then the right-hand sides ((df - dc) + dtau) - dH vdot of
//               all directions and accel_solve<N> with the same L: the exact derivative of the solve, not a Dual factorisation.
// No id is followed out of range: the tables are validated on the host, n_scene bounds the grids, every loop over bodies,
// coordinates or entries is bounded by n_body, nv or nv^2, and the LDS the host asks for is computed from the same n_body and nv.
#pragma once

constexpr int kDynWave = 64;                 // lanes per workgroup of k_dynamics and k_accel
constexpr int kDynBodyDoubles = 44;          // LDS doubles per body: I (10), tw (6), S_b v_b (6), w (6), Ic (10), W (6)
constexpr int kDynCoordDoubles = 12;         // LDS doubles per coordinate: S (6), F (6)
constexpr size_t kDynMaxLds = 64 * 1024;     // what a workgroup may ask for without an opt-in

// num: bytes per table entry, sizeof(double) for k_dynamics, sizeof(ScatDual) for k_dynamics_dual.
__host__ __device__ inline size_t dyn_lds_bytes(int n_body, int nv, size_t num = sizeof(double)) {
    return num * ((size_t)kDynBodyDoubles * (size_t)n_body + (size_t)kDynCoordDoubles * (size_t)nv) + sizeof(int) * (size_t)nv;
}
// n_rhs: right-hand sides kept in LDS, 1 for k_accel, 1 + n_dir for k_accel_dual.
__host__ __device__ inline size_t accel_lds_bytes(int nv, int n_rhs = 1) {
    return sizeof(double) * ((size_t)nv * (size_t)nv + (size_t)n_rhs * (size_t)nv) + sizeof(int);
}

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

// What the five stages read and write, per number type.  double: the value of one scene.  ScatDual: {value, the partial of one
// direction}; only the partial parts are stored.
template <class T> struct DynIo;

template <> struct DynIo<double> {
    const double *q_, *v_, *x_, *tw_;
    double *qdot_, *H_, *c_;
    __device__ DynIo(const DynArgs &d, int sc) {
        const KinArgs &g = d.k;
        const size_t nb = (size_t)g.n_body, nv = (size_t)g.nv;
        q_ = g.q + (size_t)sc * (size_t)g.nq; v_ = g.v + (size_t)sc * nv;
        x_ = d.x_w_b + 12 * ((size_t)sc * nb); tw_ = d.twist_w_b + 6 * ((size_t)sc * nb);
        qdot_ = d.qdot ? d.qdot + (size_t)sc * (size_t)g.nq : nullptr;
        H_ = d.H ? d.H + (size_t)sc * nv * nv : nullptr;
        c_ = d.c ? d.c + (size_t)sc * nv : nullptr;
    }
    __device__ double q(int i) const { return q_[i]; }
    __device__ double v(int i) const { return v_[i]; }
    __device__ double x(int b, int e) const { return x_[12 * (size_t)b + e]; }
    __device__ double tw(int b, int e) const { return tw_[6 * (size_t)b + e]; }
    __device__ bool want_qdot() const { return qdot_ != nullptr; }
    __device__ bool want_H() const { return H_ != nullptr; }
    __device__ bool want_c() const { return c_ != nullptr; }
    __device__ void qdot(int i, double a) const { qdot_[i] = a; }
    __device__ void H(size_t e, double a) const { H_[e] = a; }
    __device__ void c(int i, double a) const { c_[i] = a; }
};

struct DynDualArgs {
    DynArgs d;                          // the tables, the values (q, v, x_w_b, twist_w_b); its outputs are not written
    int n_dir;
    const double *dq, *dv;              // n_scene x n_dir x nq, x nv: the seeds; each may be NULL (zeros)
    const double *dx_w_b, *dtwist_w_b;  // n_scene n_body x n_dir x 12, x 6: pfc_kinematics_dual_device's outputs
    double *dqdot, *dH, *dc;            // n_scene x n_dir x nq, x nv x nv, x nv; each may be NULL (not wanted)
};

template <> struct DynIo<ScatDual> {
    DynIo<double> val;
    const double *dq_, *dv_, *dx_, *dtw_;
    double *dqdot_, *dH_, *dc_;
    int n_dir;
    __device__ DynIo(const DynDualArgs &h, int sc, int dir) : val(h.d, sc), n_dir(h.n_dir) {
        const KinArgs &g = h.d.k;
        const size_t nb = (size_t)g.n_body, nv = (size_t)g.nv, row = (size_t)sc * (size_t)h.n_dir + (size_t)dir;
        dq_ = h.dq ? h.dq + row * (size_t)g.nq : nullptr;
        dv_ = h.dv ? h.dv + row * nv : nullptr;
        dx_ = h.dx_w_b + 12 * ((size_t)sc * nb * (size_t)h.n_dir + (size_t)dir);          // body b: + 12 n_dir b
        dtw_ = h.dtwist_w_b + 6 * ((size_t)sc * nb * (size_t)h.n_dir + (size_t)dir);
        dqdot_ = h.dqdot ? h.dqdot + row * (size_t)g.nq : nullptr;
        dH_ = h.dH ? h.dH + row * nv * nv : nullptr;
        dc_ = h.dc ? h.dc + row * nv : nullptr;
    }
    __device__ ScatDual q(int i) const { return {val.q(i), dq_ ? dq_[i] : 0.0}; }
    __device__ ScatDual v(int i) const { return {val.v(i), dv_ ? dv_[i] : 0.0}; }
    __device__ ScatDual x(int b, int e) const { return {val.x(b, e), dx_[12 * (size_t)n_dir * (size_t)b + e]}; }
    __device__ ScatDual tw(int b, int e) const { return {val.tw(b, e), dtw_[6 * (size_t)n_dir * (size_t)b + e]}; }
    __device__ bool want_qdot() const { return dqdot_ != nullptr; }
    __device__ bool want_H() const { return dH_ != nullptr; }
    __device__ bool want_c() const { return dc_ != nullptr; }
    __device__ void qdot(int i, ScatDual a) const { dqdot_[i] = a.d; }
    __device__ void H(size_t e, ScatDual a) const { dH_[e] = a.d; }
    __device__ void c(int i, ScatDual a) const { dc_[i] = a.d; }
};

// The five stages for one scene (and, on ScatDual, one direction) by one 64-lane workgroup; lds holds dyn_lds_bytes(.., sizeof(T)).
template <class T> __device__ inline void dyn_stages(const DynArgs &d, const DynIo<T> &io, double *lds) {
    const KinArgs &g = d.k;
    const int nb = g.n_body, nv = g.nv, tid = (int)threadIdx.x;
    T *sI = reinterpret_cast<T *>(lds), *sTw = sI + 10 * nb, *sJt = sTw + 6 * nb, *sW = sJt + 6 * nb, *sIc = sW + 6 * nb, *sWc = sIc + 10 * nb;
    T *sS = sWc + 6 * nb, *sF = sS + 6 * nv;
    int *sBody = reinterpret_cast<int *>(sF + 6 * nv);
    const bool want_H = io.want_H(), want_c = io.want_c();
    const T zero = kin_lit<T>(0.0);

    // (1) qdot; world inertia, columns, joint twist
    for (int b = tid; b < nb; b += kDynWave) {
        const int type = g.jtype[b], n = kin_joint_nq(type), vo = g.voff[b], qo = g.qoff[b];
        if (io.want_qdot()) {
            if (type == PFC_JOINT_FLOATING_MRP) {
                T qj[6], vj[6], qd[6];
#pragma unroll
                for (int e = 0; e < 6; ++e) { qj[e] = io.q(qo + e); vj[e] = io.v(vo + e); }
                dyn_mrp_rate<T>(qj, vj, qd);
#pragma unroll
                for (int e = 0; e < 6; ++e) io.qdot(qo + e, qd[e]);
            } else if (n == 1) {
                io.qdot(qo, io.v(vo));
            }
        }
        if (want_H || want_c) {
            T x[12], in[13], I[10], ax[3], o[6], jt[6];
#pragma unroll
            for (int e = 0; e < 12; ++e) x[e] = io.x(b, e);
#pragma unroll
            for (int e = 0; e < 13; ++e) in[e] = kin_lit<T>(d.inertia[13 * (size_t)b + e]);
#pragma unroll
            for (int e = 0; e < 3; ++e) ax[e] = kin_lit<T>(g.axis[3 * (size_t)b + e]);
            dyn_inertia_to_world<T>(in, x, I);
#pragma unroll
            for (int e = 0; e < 10; ++e) sI[10 * b + e] = I[e];
#pragma unroll
            for (int e = 0; e < 6; ++e) jt[e] = zero;
            for (int k = 0; k < n; ++k) {
                kin_column<T>(type, k, ax, x, o);
                sBody[vo + k] = b;
#pragma unroll
                for (int e = 0; e < 6; ++e) {
                    sS[6 * (vo + k) + e] = o[e];
                    if (want_c) jt[e] = k == 0 ? o[e] * io.v(vo) : jt[e] + o[e] * io.v(vo + k);
                }
            }
            if (want_c) {
#pragma unroll
                for (int e = 0; e < 6; ++e) { sTw[6 * b + e] = io.tw(b, e); sJt[6 * b + e] = jt[e]; }
            }
        }
    }
    if (!want_H && !want_c) return;
    __syncthreads();

    // (2) bias acceleration along the path, body wrench
    if (want_c) {
        for (int b = tid; b < nb; b += kDynWave) {
            T a[6] = {zero, zero, zero, -kin_lit<T>(d.g[0]), -kin_lit<T>(d.g[1]), -kin_lit<T>(d.g[2])}, o[6], w1[6], w2[6], w3[6];
            for (int k = g.path_off[b]; k < g.path_off[b + 1]; ++k) {
                const int p = g.path[k];
                dyn_crossm<T>(sTw + 6 * p, sJt + 6 * p, o);
#pragma unroll
                for (int e = 0; e < 6; ++e) a[e] = a[e] + o[e];
            }
            dyn_mul<T>(sI + 10 * b, a, w1);
            dyn_mul<T>(sI + 10 * b, sTw + 6 * b, w2);
            dyn_crossf<T>(sTw + 6 * b, w2, w3);
#pragma unroll
            for (int e = 0; e < 6; ++e) sW[6 * b + e] = w1[e] + w3[e];
        }
        __syncthreads();
    }

    // (3) composite inertia, joint wrench: the subtree in increasing body order, b itself first
    for (int b = tid; b < nb; b += kDynWave) {
        const int s0 = d.sub_off[b], s1 = d.sub_off[b + 1];
        if (want_H) {
            T I[10];
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
            T W[6];
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
            T F[6];
            dyn_mul<T>(sIc + 10 * b, sS + 6 * i, F);
#pragma unroll
            for (int e = 0; e < 6; ++e) sF[6 * i + e] = F[e];
        }
        if (want_c) io.c(i, dyn_dot6<T>(sS + 6 * i, sWc + 6 * b));
    }
    if (!want_H) return;
    __syncthreads();

    // (5) H: the lower triangle and its mirror
    for (int e = tid; e < nv * nv; e += kDynWave) {
        const int i = e / nv, j = e % nv;
        if (j > i) continue;
        const T h = g.anc[(size_t)sBody[i] * (size_t)nv + (size_t)j] ? dyn_dot6<T>(sS + 6 * j, sF + 6 * i) : zero;
        io.H((size_t)i * nv + j, h);
        io.H((size_t)j * nv + i, h);
    }
}

__global__ void __launch_bounds__(kDynWave) k_dynamics(DynArgs d) {
    extern __shared__ double dyn_lds[];
    dyn_stages<double>(d, DynIo<double>(d, (int)blockIdx.x), dyn_lds);
}

// The same statement on ScatDual: one workgroup per (scene, direction), block scene n_dir + dir.
__global__ void __launch_bounds__(kDynWave) k_dynamics_dual(DynDualArgs h) {
    extern __shared__ double dyn_lds[];
    const int sc = (int)(blockIdx.x / (unsigned)h.n_dir), dir = (int)(blockIdx.x % (unsigned)h.n_dir);
    dyn_stages<ScatDual>(h.d, DynIo<ScatDual>(h, sc, dir), dyn_lds);
}

// The lower triangle of a scene's H into L (column-major: L(i, j) at L[j nv + i]) and its left-looking Cholesky factorisation, one
// column at a time; lane i = row i.  Returns 0, or j + 1 for the first pivot that is not > 0 (NaN included): the same for every lane.
__device__ inline int accel_factor(const double *H, int nv, int i, double *L, int *flag) {
    const bool act = i < nv;
    for (int e = i; e < nv * nv; e += kDynWave) {
        const int r = e / nv, c = e % nv;
        if (c <= r) L[c * nv + r] = H[e];
    }
    if (i == 0) *flag = 0;
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
    return *flag;
}

// L y = rhs, then L' x = y, for N right-hand sides together: lane i enters with rhs_i of side d in acc[d]; x of side d is left in
// sv[d nv .. d nv + nv), visible to every lane.  The sides share L and the barriers; nothing branches on a side, so their LDS
// reads are in flight together.
template <int N> __device__ inline void accel_solve(const double *L, int nv, int i, double (&acc)[N], double *sv) {
    const bool act = i < nv;
    for (int k = 0; k < nv; ++k) {          // L y = rhs, k ascending
        if (i == k) {
#pragma unroll
            for (int d = 0; d < N; ++d) sv[d * nv + k] = acc[d] / L[k * nv + k];
        }
        __syncthreads();
        if (act && i > k) {
#pragma unroll
            for (int d = 0; d < N; ++d) acc[d] = acc[d] - L[k * nv + i] * sv[d * nv + k];
        }
    }
    if (act) {
#pragma unroll
        for (int d = 0; d < N; ++d) acc[d] = sv[d * nv + i];
    }
    __syncthreads();
    for (int k = nv - 1; k >= 0; --k) {     // L' x = y, k descending
        if (i == k) {
#pragma unroll
            for (int d = 0; d < N; ++d) sv[d * nv + k] = acc[d] / L[k * nv + k];
        }
        __syncthreads();
        if (act && i < k) {
#pragma unroll
            for (int d = 0; d < N; ++d) acc[d] = acc[d] - L[i * nv + k] * sv[d * nv + k];
        }
    }
}

// vdot = H^-1 ((f - c) + tau) by H = L L', L y = rhs, L' x = y, in the order include/pfc.h states.  nv <= kDynWave: lane = row.
__global__ void __launch_bounds__(kDynWave) k_accel(AccelArgs g) {
    extern __shared__ double dyn_lds[];
    const int nv = g.nv, i = (int)threadIdx.x, sc = (int)blockIdx.x;
    double *L = dyn_lds, *sv = L + nv * nv;
    int *flag = reinterpret_cast<int *>(sv + nv);
    const size_t row = (size_t)sc * (size_t)nv;
    const bool act = i < nv;
    double acc[1] = {0.0};
    if (act) acc[0] = (g.f[row + i] - g.c[row + i]) + (g.tau ? g.tau[row + i] : 0.0);
    const int bad = accel_factor(g.H + row * (size_t)nv, nv, i, L, flag);
    if (!bad) accel_solve<1>(L, nv, i, acc, sv);
    if (act) g.vdot[row + i] = bad ? __longlong_as_double(0x7ff8000000000000ll) : sv[i];
    if (i == 0 && g.info) g.info[sc] = bad;
}

struct AccelDualArgs {
    AccelArgs a;                        // the value solve; a.vdot and a.info may be NULL
    int n_dir;
    const double *dH, *dc, *df, *dtau;  // n_scene x n_dir x nv x nv, x nv, x nv, x nv (dtau may be NULL: zeros)
    double *dvdot;                      // n_scene x n_dir x nv
};

__host__ __device__ inline int accel_dual_slots(int n_dir) { return n_dir <= 1 ? 1 : n_dir <= 2 ? 2 : n_dir <= 4 ? 4 : n_dir <= 8 ? 8 : 16; }

// k_accel's factor and vdot, then dvdot = H^-1 (((df - dc) + dtau) - dH vdot) for every direction with the same factor, the
// substitutions of all directions together.  N = accel_dual_slots(n_dir) accumulators per lane; a slot d >= n_dir repeats direction
// n_dir - 1 (so that no load, product or LDS access sits behind a branch on the direction) and is not stored.
// LDS: L, vdot (nv), the slots' unknowns (N nv), the flag.
template <int N> __global__ void __launch_bounds__(kDynWave) k_accel_dual(AccelDualArgs h) {
    extern __shared__ double dyn_lds[];
    const AccelArgs &g = h.a;
    const int nv = g.nv, n_dir = h.n_dir, i = (int)threadIdx.x, sc = (int)blockIdx.x;
    double *L = dyn_lds, *sv = L + nv * nv, *sd = sv + nv;
    int *flag = reinterpret_cast<int *>(sd + N * nv);
    const size_t row = (size_t)sc * (size_t)nv;
    const bool act = i < nv;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double acc[1] = {0.0};
    if (act) acc[0] = (g.f[row + i] - g.c[row + i]) + (g.tau ? g.tau[row + i] : 0.0);
    const int bad = accel_factor(g.H + row * (size_t)nv, nv, i, L, flag);
    if (!bad) accel_solve<1>(L, nv, i, acc, sv);      // ends behind a barrier: sv holds vdot for every lane
    if (act && g.vdot) g.vdot[row + i] = bad ? nan : sv[i];
    if (i == 0 && g.info) g.info[sc] = bad;
    double r[N];
#pragma unroll
    for (int d = 0; d < N; ++d) r[d] = 0.0;
    if (!bad) {
        if (act) {
            const size_t d0 = (size_t)sc * (size_t)n_dir * (size_t)nv, nn = (size_t)nv * (size_t)nv;
            const double *dHi = h.dH + (d0 + (size_t)i) * (size_t)nv;      // row i of direction 0; direction d: + d nv nv
            size_t off[N];
#pragma unroll
            for (int d = 0; d < N; ++d) off[d] = (size_t)(d < n_dir ? d : n_dir - 1);
            const double v0 = sv[0];
#pragma unroll
            for (int d = 0; d < N; ++d) r[d] = dHi[off[d] * nn] * v0;
            for (int j = 1; j < nv; ++j) {      // t_i, j ascending; the slots are the inner loop: their loads are in flight together
                const double vj = sv[j];
#pragma unroll
                for (int d = 0; d < N; ++d) r[d] = r[d] + dHi[off[d] * nn + j] * vj;
            }
#pragma unroll
            for (int d = 0; d < N; ++d) {
                const size_t e = d0 + off[d] * (size_t)nv + (size_t)i;
                r[d] = ((h.df[e] - h.dc[e]) + (h.dtau ? h.dtau[e] : 0.0)) - r[d];
            }
        }
        accel_solve<N>(L, nv, i, r, sd);
    }
    if (act) {
#pragma unroll
        for (int d = 0; d < N; ++d)
            if (d < n_dir) h.dvdot[((size_t)sc * (size_t)n_dir + (size_t)d) * (size_t)nv + i] = bad ? nan : sd[d * nv + i];
    }
}
