// pfc_body_wrench.h -- applied body wrenches: a force and a moment on a body at a point of its frame, on a per-scene time schedule,
// projected into the joint space with the body's geometric Jacobian and added to tau between the dynamics (and the feedback law, if
// one is set) and the solve; and their partials along the directions of a Jacobian chunk -- the geometric stiffness of a world-frame
// force at an offset point, the rotation of a body-frame follower load.  What the reference's users write in continuous_controller
// as J' w.  The statements: include/pfc.h (pfc_body_wrench_device, pfc_body_wrench_dual_device).  A textual part of pfc_hip.hip,
// behind pfc_statecall.h (BodyWrenches), pfc_scatter.h (ScatDual, scat_world, scat_tau) and pfc_kin.h (kin_lit).
//
// pfc_feedback.h's conventions: plain Float64, no fma (the build has -ffp-contract=off), the written order, no atomics, nothing in
// LDS, no scratch, plain vector stores.  One 64-lane wave per row (k_body_wrench: a scene or a stage-scene) or per (scene, direction)
// (k_body_wrench_dual); lane j = velocity coordinate j (nv <= 64).  The segment search, the loop over the wrenches, the frame test and
// the world wrench W of a wrench depend on the row only: wave-uniform, every lane forms the same W from the same loads; a lane's own
// part is its Jacobian column.  There is no lane read, and no early return: a lane >= nv reads column 0 and stores nothing.
// bw_world is one template over the number type: the value (double) and the Dual (ScatDual) kernels run the same statement; frame 1
// is scat_world at the pose (R, r), frame 0 the cross product of pfc_dyn.h (dyn_cross), written out.
// No index is followed out of range: the grid is the row count, nv <= 64 is validated on the host, body[k] in [0, n_body) is the
// caller's guarantee (pfc_radau_set_body_wrenches validates it), the segment index is a count of at most n_seg - 1 comparisons, row r
// reads the schedule of scene r % n_sched.
#pragma once

constexpr int kBwWave = 64;

struct BodyWrenchArgs {
    BodyWrenches w;                         // the tables, t (n_rows) and tau (n_rows x nv, the output)
    int n_rows, nv;
    const double *x_w_b, *jac;              // n_rows n_body x 12; x nv x 6: pfc_kinematics_device's outputs
    const double *tau_in;                   // n_rows x nv, or NULL
};

struct BodyWrenchDualArgs {
    BodyWrenches w;                         // the tables, t (n_scene) and dtau (n_scene x n_dir x nv, the output)
    int n_scene, n_dir, nv;
    const double *x_w_b, *jac;              // the values, as above
    const double *dx_w_b, *djac;            // n_scene n_body x n_dir x 12; x nv x 6: pfc_kinematics_dual_device's outputs
    const double *dtau_in;                  // n_scene x n_dir x nv, or NULL
};

// The loads of row `sched` at time t: segment k = the number of j >= 1 with seg_t[j] <= t; n_w x 6 doubles from there.
__device__ inline const double *bw_segment(const BodyWrenches &w, int sched, double t) {
    int k = 0;
    if (w.n_seg > 1) {
        const double *st = w.seg_t + (size_t)sched * (size_t)w.n_seg;
        for (int j = 1; j < w.n_seg; ++j) k += st[j] <= t ? 1 : 0;
    }
    return w.seg_w + ((size_t)sched * (size_t)w.n_seg + (size_t)k) * (size_t)w.n_w * 6;
}

// The world wrench about the world origin, W = [M + r x F; F], of the load l = [moment; force] applied at point p of the body whose
// world pose is x = (R (9, column-major), t (3)): r = ((R[:,0] p0 + R[:,1] p1) + R[:,2] p2) + t; frame 1: M = R m, F = R f --
// transform(wrench, (R, r)), scat_world's statement --; frame 0: M = m, F = f.  p and l are constants.
template <class T> __device__ inline void bw_world(int frame, const T *x, const double *p, const double *l, T *W) {
    T xr[12], wl[6];
    const T p0 = kin_lit<T>(p[0]), p1 = kin_lit<T>(p[1]), p2 = kin_lit<T>(p[2]);
#pragma unroll
    for (int e = 0; e < 9; ++e) xr[e] = x[e];
#pragma unroll
    for (int i = 0; i < 3; ++i) xr[9 + i] = ((x[i] * p0 + x[3 + i] * p1) + x[6 + i] * p2) + x[9 + i];
#pragma unroll
    for (int e = 0; e < 6; ++e) wl[e] = kin_lit<T>(l[e]);
    if (frame == 1) {
        scat_world<T>(wl, xr, W);
    } else {      // dyn_cross's statement, written out: o0 = a1 b2 - a2 b1, o1 = a2 b0 - a0 b2, o2 = a0 b1 - a1 b0
        W[0] = wl[0] + (xr[10] * wl[5] - xr[11] * wl[4]);
        W[1] = wl[1] + (xr[11] * wl[3] - xr[9] * wl[5]);
        W[2] = wl[2] + (xr[9] * wl[4] - xr[10] * wl[3]);
        W[3] = wl[3]; W[4] = wl[4]; W[5] = wl[5];
    }
}

__global__ void __launch_bounds__(kBwWave) k_body_wrench(BodyWrenchArgs g) {
    const int row = (int)blockIdx.x, j = (int)threadIdx.x, nv = g.nv;
    const BodyWrenches &w = g.w;
    const double *loads = bw_segment(w, row % w.n_sched, w.t[row]);
    const bool lane = j < nv;
    const size_t col = (size_t)(lane ? j : 0), at = (size_t)row * (size_t)nv + col;
    double sum = g.tau_in ? g.tau_in[at] : 0.0;
    for (int k = 0; k < w.n_w; ++k) {
        const size_t rb = (size_t)row * (size_t)w.n_body + (size_t)w.body[k];
        const double *xp = g.x_w_b + rb * 12, *Jp = g.jac + (rb * (size_t)nv + col) * 6;
        double x[12], W[6], J[6];
#pragma unroll
        for (int e = 0; e < 12; ++e) x[e] = xp[e];
#pragma unroll
        for (int e = 0; e < 6; ++e) J[e] = Jp[e];
        bw_world<double>(w.frame[k], x, w.point + 3 * (size_t)k, loads + 6 * (size_t)k, W);
        sum = sum + scat_tau<double>(J, W);
    }
    if (lane) w.tau[at] = sum;
}

__global__ void __launch_bounds__(kBwWave) k_body_wrench_dual(BodyWrenchDualArgs g) {
    const int sc = (int)blockIdx.x / g.n_dir, dir = (int)blockIdx.x % g.n_dir, j = (int)threadIdx.x, nv = g.nv;
    const BodyWrenches &w = g.w;
    const double *loads = bw_segment(w, sc % w.n_sched, w.t[sc]);
    const bool lane = j < nv;
    const size_t col = (size_t)(lane ? j : 0), dat = (size_t)blockIdx.x * (size_t)nv + col;      // blockIdx.x = sc n_dir + dir
    double dsum = g.dtau_in ? g.dtau_in[dat] : 0.0;
    for (int k = 0; k < w.n_w; ++k) {
        const size_t rb = (size_t)sc * (size_t)w.n_body + (size_t)w.body[k], rd = rb * (size_t)g.n_dir + (size_t)dir;
        const double *xp = g.x_w_b + rb * 12, *dxp = g.dx_w_b + rd * 12;
        const double *Jp = g.jac + (rb * (size_t)nv + col) * 6, *dJp = g.djac + (rd * (size_t)nv + col) * 6;
        ScatDual x[12], W[6], J[6];
#pragma unroll
        for (int e = 0; e < 12; ++e) x[e] = ScatDual{xp[e], dxp[e]};
#pragma unroll
        for (int e = 0; e < 6; ++e) J[e] = ScatDual{Jp[e], dJp[e]};
        bw_world<ScatDual>(w.frame[k], x, w.point + 3 * (size_t)k, loads + 6 * (size_t)k, W);
        dsum = dsum + scat_tau<ScatDual>(J, W).d;
    }
    if (lane) w.dtau[dat] = dsum;
}
