// pfc_kin.h -- body poses, twists and geometric Jacobians from joint states (pfc_set_mechanism, pfc_kinematics[_device],
// pfc_eval_state[_device]): what transform_to_root / twist_wrt_world (src/contact_algorithms_non_friction.jl:109-110,125-126) and
// refreshJacobians! (:86-92) give the reference per evaluation, formed on the device from the state vector (q, v) of a small tree
// of fixed, revolute, prismatic and MRP-floating (RigidBodyDynamics' SPQuatFloating) joints, in the layouts
// pfc_items_from_bodies_device and pfc_scatter_generalized_device consume.  Included by pfc_hip.hip inside namespace pfc (device
// code only).
//
// Arithmetic (the contract, stated in include/pfc.h): plain Float64, every 3-term dot product summed left to right, no fma (the
// build has -ffp-contract=off), a translation added last; the world goes through the same expressions with R = I, t = 0 and a zero
// twist.  One statement over the number type T (kin_joint, kin_compose, kin_twist_add, kin_column), as bodies_item<T> is: the Dual
// instantiation (the second half of this file) adds kin_lit, kin_sincos and operator/ on its type and restates nothing.
// The kernels:
//   k_kinematics    one lane per (scene, body), one wave per workgroup.  The lane walks its root -> body path from the flattened
//                   path table, repeating its ancestors' expressions in their order -- so it gets their bytes, without a
//                   dependency between lanes or a launch per tree level -- and writes its pose, its twist and its own joint's
//                   motion-subspace columns (S_w, n_scene x nv x 6).
//   k_kin_jacobian  one lane per (scene, body, coordinate): six doubles copied from S_w where the coordinate's joint lies on the
//                   body's path (the ancestor table), +0.0 six times otherwise; 48 consecutive bytes per lane, neighbouring lanes
//                   neighbouring columns.
// No id is followed out of range: the tables are validated on the host and n_scene bounds the grids.
#pragma once

constexpr int kKinWave = 64;            // (scene, body) lanes per workgroup of k_kinematics
constexpr int kKinJacBlock = 256;       // (scene, body, coordinate) lanes per workgroup of k_kin_jacobian

struct KinArgs {
    int n_scene, n_body, nq, nv;
    const int *jtype, *qoff, *voff;     // n_body: joint type, first configuration / velocity coordinate
    const int *path_off, *path;         // CSR: the bodies from the root to b, b included, are path[path_off[b] .. path_off[b + 1])
    const double *x_p_j;                // n_body x 12: joint_pose, R (9, column-major) then t
    const double *axis;                 // n_body x 3, in the joint frame (revolute, prismatic)
    const unsigned char *anc;           // n_body x nv: 1 where the coordinate's joint lies on the body's path
    const double *q, *v;                // n_scene x nq, n_scene x nv (v may be NULL: zeros)
    double *x_w_b, *twist_w_b;          // n_scene n_body x 12, x 6; each may be NULL (not wanted)
    double *S_w;                        // n_scene x nv x 6, or NULL (no Jacobian wanted)
    double *jac;                        // n_scene n_body x nv x 6 (k_kin_jacobian)
};

template <class T> __device__ inline T kin_lit(double x);
template <> __device__ inline double kin_lit<double>(double x) { return x; }
__device__ inline void kin_sincos(double th, double &c, double &s) { c = cos(th); s = sin(th); }

// x = a o b for poses (12: R column-major, t): R = R_a R_b, t = (R_a t_b) + t_a.
template <class T> __device__ inline void kin_compose(const T *a, const T *b, T *x) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) x[3 * c + r] = (a[r] * b[3 * c] + a[3 + r] * b[3 * c + 1]) + a[6 + r] * b[3 * c + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) x[9 + r] = ((a[r] * b[9] + a[3 + r] * b[10]) + a[6 + r] * b[11]) + a[9 + r];
}

// The joint transform X_j(q) (12) and the joint twist in the frame after (6: [angular; linear]).  a: the axis; q, v: the joint's
// own coordinates (v may be NULL: zeros).
template <class T> __device__ inline void kin_joint(int type, const T *a, const T *q, const T *v, T *xj, T *tj) {
    const T zero = kin_lit<T>(0.0), one = kin_lit<T>(1.0), two = kin_lit<T>(2.0);
#pragma unroll
    for (int e = 0; e < 12; ++e) xj[e] = (e == 0 || e == 4 || e == 8) ? one : zero;
#pragma unroll
    for (int e = 0; e < 6; ++e) tj[e] = zero;
    if (type == PFC_JOINT_PRISMATIC) {
        const T d = q[0], dd = v ? v[0] : zero;
#pragma unroll
        for (int r = 0; r < 3; ++r) { xj[9 + r] = a[r] * d; tj[3 + r] = a[r] * dd; }
    } else if (type == PFC_JOINT_REVOLUTE) {
        T c, s;
        kin_sincos(q[0], c, s);
        const T c1 = one - c, thd = v ? v[0] : zero;
        xj[0] = (c1 * a[0]) * a[0] + c; xj[4] = (c1 * a[1]) * a[1] + c; xj[8] = (c1 * a[2]) * a[2] + c;
        xj[1] = (c1 * a[0]) * a[1] + s * a[2]; xj[3] = (c1 * a[0]) * a[1] - s * a[2];
        xj[2] = (c1 * a[0]) * a[2] - s * a[1]; xj[6] = (c1 * a[0]) * a[2] + s * a[1];
        xj[5] = (c1 * a[1]) * a[2] + s * a[0]; xj[7] = (c1 * a[1]) * a[2] - s * a[0];
#pragma unroll
        for (int r = 0; r < 3; ++r) tj[r] = a[r] * thd;
    } else if (type == PFC_JOINT_FLOATING_MRP) {
        const T a2 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
        const T den = a2 + one;
        const T w = (one - a2) / den, x = (two * q[0]) / den, y = (two * q[1]) / den, z = (two * q[2]) / den;
        xj[0] = ((w * w + x * x) - y * y) - z * z; xj[1] = two * (x * y + z * w); xj[2] = two * (x * z - y * w);
        xj[3] = two * (x * y - z * w); xj[4] = ((w * w - x * x) + y * y) - z * z; xj[5] = two * (y * z + x * w);
        xj[6] = two * (x * z + y * w); xj[7] = two * (y * z - x * w); xj[8] = ((w * w - x * x) - y * y) + z * z;
#pragma unroll
        for (int r = 0; r < 3; ++r) xj[9 + r] = q[3 + r];
#pragma unroll
        for (int e = 0; e < 6; ++e) tj[e] = v ? v[e] : zero;
    }
}

// o (6) = [R m_ang; (R m_lin) + t x (R m_ang)]: a motion vector m of the body's frame in world about the world origin, x the body's
// world pose.
template <class T> __device__ inline void kin_to_world(const T *x, const T *m, T *o) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = (x[r] * m[0] + x[3 + r] * m[1]) + x[6 + r] * m[2];
    o[3] = ((x[0] * m[3] + x[3] * m[4]) + x[6] * m[5]) + (x[10] * o[2] - x[11] * o[1]);
    o[4] = ((x[1] * m[3] + x[4] * m[4]) + x[7] * m[5]) + (x[11] * o[0] - x[9] * o[2]);
    o[5] = ((x[2] * m[3] + x[5] * m[4]) + x[8] * m[5]) + (x[9] * o[1] - x[10] * o[0]);
}

// Motion-subspace column k of a joint in world (6), x the world pose of its body.
template <class T> __device__ inline void kin_column(int type, int k, const T *a, const T *x, T *o) {
    const T zero = kin_lit<T>(0.0);
    const bool angular = type == PFC_JOINT_REVOLUTE || (type == PFC_JOINT_FLOATING_MRP && k < 3);
    T d[3];
    if (type == PFC_JOINT_FLOATING_MRP) {
        const int c = k < 3 ? k : k - 3;
#pragma unroll
        for (int r = 0; r < 3; ++r) d[r] = x[3 * c + r];
    } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) d[r] = (x[r] * a[0] + x[3 + r] * a[1]) + x[6 + r] * a[2];
    }
    if (angular) {
        o[0] = d[0]; o[1] = d[1]; o[2] = d[2];
        o[3] = x[10] * d[2] - x[11] * d[1]; o[4] = x[11] * d[0] - x[9] * d[2]; o[5] = x[9] * d[1] - x[10] * d[0];
    } else {
        o[0] = zero; o[1] = zero; o[2] = zero;
        o[3] = d[0]; o[4] = d[1]; o[5] = d[2];
    }
}

__host__ __device__ inline int kin_joint_nq(int type) { return type == PFC_JOINT_FLOATING_MRP ? 6 : (type == PFC_JOINT_FIXED ? 0 : 1); }

__global__ void __launch_bounds__(kKinWave) k_kinematics(KinArgs g) {
    const long long i = (long long)blockIdx.x * kKinWave + (long long)threadIdx.x;
    if (i >= (long long)g.n_scene * g.n_body) return;
    const int sc = (int)(i / g.n_body), b = (int)(i % g.n_body);
    const double *q = g.q + (size_t)sc * (size_t)g.nq;
    const double *v = g.v ? g.v + (size_t)sc * (size_t)g.nv : nullptr;
    double x[12], tw[6], xj[12], tj[6], xa[12], xn[12], o[6], xp[12], ax[3];
#pragma unroll
    for (int e = 0; e < 12; ++e) x[e] = (e == 0 || e == 4 || e == 8) ? 1.0 : 0.0;      // the world
#pragma unroll
    for (int e = 0; e < 6; ++e) tw[e] = 0.0;
    for (int k = g.path_off[b]; k < g.path_off[b + 1]; ++k) {
        const int a = g.path[k], type = g.jtype[a];
#pragma unroll
        for (int e = 0; e < 12; ++e) xp[e] = g.x_p_j[12 * (size_t)a + e];
#pragma unroll
        for (int e = 0; e < 3; ++e) ax[e] = g.axis[3 * (size_t)a + e];
        kin_joint<double>(type, ax, q + g.qoff[a], v ? v + g.voff[a] : nullptr, xj, tj);
        kin_compose<double>(xp, xj, xa);
        kin_compose<double>(x, xa, xn);
#pragma unroll
        for (int e = 0; e < 12; ++e) x[e] = xn[e];
        kin_to_world<double>(x, tj, o);
#pragma unroll
        for (int e = 0; e < 6; ++e) tw[e] = tw[e] + o[e];
    }
    if (g.x_w_b) {
        double *out = g.x_w_b + 12 * (size_t)i;
#pragma unroll
        for (int e = 0; e < 12; ++e) out[e] = x[e];
    }
    if (g.twist_w_b) {
        double *out = g.twist_w_b + 6 * (size_t)i;
#pragma unroll
        for (int e = 0; e < 6; ++e) out[e] = tw[e];
    }
    if (g.S_w) {
        const int type = g.jtype[b], n = kin_joint_nq(type);      // ax is body b's: the path ends with b
        for (int k = 0; k < n; ++k) {
            kin_column<double>(type, k, ax, x, o);
            double *out = g.S_w + 6 * ((size_t)sc * (size_t)g.nv + (size_t)(g.voff[b] + k));
#pragma unroll
            for (int e = 0; e < 6; ++e) out[e] = o[e];
        }
    }
}

__global__ void __launch_bounds__(kKinJacBlock) k_kin_jacobian(KinArgs g) {
    const long long i = (long long)blockIdx.x * kKinJacBlock + (long long)threadIdx.x;
    const long long per_scene = (long long)g.n_body * g.nv;
    if (i >= (long long)g.n_scene * per_scene) return;
    const long long sc = i / per_scene, r = i % per_scene;      // r = b nv + c
    const int c = (int)(r % g.nv);
    double *out = g.jac + 6 * (size_t)i;
    if (g.anc[r]) {
        const double *in = g.S_w + 6 * ((size_t)sc * (size_t)g.nv + (size_t)c);
#pragma unroll
        for (int e = 0; e < 6; ++e) out[e] = in[e];
    } else {
#pragma unroll
        for (int e = 0; e < 6; ++e) out[e] = 0.0;
    }
}

// ---- the Dual half: partials of the poses, twists and Jacobians (pfc_kinematics_dual[_device], pfc_eval_dual_state_device[_more]) ----
// What the reference gets from RigidBodyDynamics on the Dual state of a Jacobian chunk (src/radau/radau_functions.jl:2-14): the
// statements above instantiated on ScatDual (pfc_scatter.h), the (value, one partial) pair with ForwardDiff's rules.  Nothing is
// restated and nothing is skipped for a zero seed: a direction that seeds none of a lane's joints runs the same expressions, and its
// partials are the signed zeros of that arithmetic.  Mechanism constants (x_p_j, the axes) and literals carry a zero partial.
// The kernels:
//   k_kinematics_dual    one lane per (scene, body, direction), one wave per workgroup, the walk of k_kinematics on ScatDual: the
//                        value parts are k_kinematics' bytes and are not stored; the partial parts of the pose (12), the twist (6)
//                        and the lane's own joint's columns (dS_w, n_scene x n_dir x nv x 6) are.
//   k_kin_jacobian_dual  one lane per (scene, body, direction, coordinate): six doubles copied from dS_w where anc says so, +0.0 six
//                        times otherwise.
// No atomics, no dependency between lanes, plain per-lane stores; n_scene and n_dir bound the grids.
template <> __device__ inline ScatDual kin_lit<ScatDual>(double x) { return {x, 0.0}; }
__device__ inline void kin_sincos(ScatDual th, ScatDual &c, ScatDual &s) {
    const double sv = sin(th.v), cv = cos(th.v);
    s = ScatDual{sv, cv * th.d};
    c = ScatDual{cv, -(sv * th.d)};
}

struct KinDualArgs {
    KinArgs k;                          // the tables, n_scene, q and v (values); its outputs are not read
    int n_dir;
    const double *dq, *dv;              // n_scene x n_dir x nq, x nv: the seeds; each may be NULL (zeros)
    double *dx_w_b, *dtwist_w_b;        // n_scene n_body x n_dir x 12, x 6; each may be NULL (not wanted)
    double *dS_w;                       // n_scene x n_dir x nv x 6, or NULL (no Jacobian partials wanted)
    double *djac;                       // n_scene n_body x n_dir x nv x 6 (k_kin_jacobian_dual)
};

__global__ void __launch_bounds__(kKinWave) k_kinematics_dual(KinDualArgs h) {
    const KinArgs &g = h.k;
    const long long i = (long long)blockIdx.x * kKinWave + (long long)threadIdx.x;      // (scene n_body + body) n_dir + dir
    if (i >= (long long)g.n_scene * g.n_body * h.n_dir) return;
    const int dir = (int)(i % h.n_dir);
    const long long sb = i / h.n_dir;
    const int sc = (int)(sb / g.n_body), b = (int)(sb % g.n_body);
    const size_t row = (size_t)sc * (size_t)h.n_dir + (size_t)dir;
    const double *q = g.q + (size_t)sc * (size_t)g.nq;
    const double *v = g.v ? g.v + (size_t)sc * (size_t)g.nv : nullptr;
    const double *dq = h.dq ? h.dq + row * (size_t)g.nq : nullptr;
    const double *dv = h.dv ? h.dv + row * (size_t)g.nv : nullptr;
    ScatDual x[12], tw[6], xj[12], tj[6], xa[12], xn[12], o[6], xp[12], ax[3], qj[6], vj[6];
#pragma unroll
    for (int e = 0; e < 12; ++e) x[e] = kin_lit<ScatDual>((e == 0 || e == 4 || e == 8) ? 1.0 : 0.0);      // the world
#pragma unroll
    for (int e = 0; e < 6; ++e) tw[e] = kin_lit<ScatDual>(0.0);
    for (int k = g.path_off[b]; k < g.path_off[b + 1]; ++k) {
        const int a = g.path[k], type = g.jtype[a], n = kin_joint_nq(type), qo = g.qoff[a], vo = g.voff[a];
#pragma unroll
        for (int e = 0; e < 12; ++e) xp[e] = kin_lit<ScatDual>(g.x_p_j[12 * (size_t)a + e]);
#pragma unroll
        for (int e = 0; e < 3; ++e) ax[e] = kin_lit<ScatDual>(g.axis[3 * (size_t)a + e]);
#pragma unroll
        for (int e = 0; e < 6; ++e) {      // the joint's own coordinates only: nothing is read past the state's rows
            qj[e] = e < n ? ScatDual{q[qo + e], dq ? dq[qo + e] : 0.0} : kin_lit<ScatDual>(0.0);
            vj[e] = (v && e < n) ? ScatDual{v[vo + e], dv ? dv[vo + e] : 0.0} : kin_lit<ScatDual>(0.0);
        }
        kin_joint<ScatDual>(type, ax, qj, vj, xj, tj);      // (without v, vj is the literal zero the statement takes for a null v)
        kin_compose<ScatDual>(xp, xj, xa);
        kin_compose<ScatDual>(x, xa, xn);
#pragma unroll
        for (int e = 0; e < 12; ++e) x[e] = xn[e];
        kin_to_world<ScatDual>(x, tj, o);
#pragma unroll
        for (int e = 0; e < 6; ++e) tw[e] = tw[e] + o[e];
    }
    if (h.dx_w_b) {
        double *out = h.dx_w_b + 12 * (size_t)i;
#pragma unroll
        for (int e = 0; e < 12; ++e) out[e] = x[e].d;
    }
    if (h.dtwist_w_b) {
        double *out = h.dtwist_w_b + 6 * (size_t)i;
#pragma unroll
        for (int e = 0; e < 6; ++e) out[e] = tw[e].d;
    }
    if (h.dS_w) {
        const int type = g.jtype[b], n = kin_joint_nq(type);      // ax is body b's: the path ends with b
        for (int k = 0; k < n; ++k) {
            kin_column<ScatDual>(type, k, ax, x, o);
            double *out = h.dS_w + 6 * (row * (size_t)g.nv + (size_t)(g.voff[b] + k));
#pragma unroll
            for (int e = 0; e < 6; ++e) out[e] = o[e].d;
        }
    }
}

__global__ void __launch_bounds__(kKinJacBlock) k_kin_jacobian_dual(KinDualArgs h) {
    const KinArgs &g = h.k;
    const long long i = (long long)blockIdx.x * kKinJacBlock + (long long)threadIdx.x;      // ((scene n_body + body) n_dir + dir) nv + c
    if (i >= (long long)g.n_scene * g.n_body * h.n_dir * g.nv) return;
    const int c = (int)(i % g.nv);
    const long long t = i / g.nv;
    const int dir = (int)(t % h.n_dir);
    const long long sb = t / h.n_dir;
    const long long sc = sb / g.n_body;
    const int b = (int)(sb % g.n_body);
    double *out = h.djac + 6 * (size_t)i;
    if (g.anc[(size_t)b * (size_t)g.nv + (size_t)c]) {
        const double *in = h.dS_w + 6 * (((size_t)sc * (size_t)h.n_dir + (size_t)dir) * (size_t)g.nv + (size_t)c);
#pragma unroll
        for (int e = 0; e < 6; ++e) out[e] = in[e];
    } else {
#pragma unroll
        for (int e = 0; e < 6; ++e) out[e] = 0.0;
    }
}
