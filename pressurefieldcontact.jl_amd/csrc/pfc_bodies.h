// pfc_bodies.h -- contact items from body states (pfc_items_from_bodies[_device], pfc_eval_bodies[_device]) and their Dual seeds
// (pfc_dual_seeds_from_bodies[_device], pfc_eval_dual_bodies_device[_more]; second half of this file): what
// refreshBodyBodyTransform! / refreshBodyBodyCache! (src/contact_algorithms_non_friction.jl:103-134) leave in the bodyBodyCache
// for every instruction -- x_r2_r1, x_r1_r2, twist_r2_r1_r2, x_rw_r2 and the two bodies -- formed on the device from the world
// poses and twists of the bodies, in the layouts pfc_eval_device and pfc_scatter_generalized_device consume.  Included by
// pfc_hip.hip inside namespace pfc (device code only).
//
// Arithmetic: the scalar statement of scenario.py's relative_pose / relative_twist in plain Float64 -- every 3-term dot product
// summed left to right, no fma (the build has -ffp-contract=off), the translation added last.  The world (body -1) is not a
// special case of it: it goes through the same expressions with R = I, t = 0 and a zero twist.
//   R2w = R_w2', t2w = -(R2w t_w2);  R21 = R2w R_w1, t21 = (R2w t_w1) + t2w;  R12 = R21', t12 = -(R12 t21)
//   tw = tw_2 - tw_1;  ang = R2w tw_ang;  lin = (R2w tw_lin) + t2w x ang
// The kernel, k_items_from_bodies: one item per lane, one wave per workgroup.  An item whose instruction or scene id is out of
// range, whose instruction is unbound or bound to a body outside [-1, n_body), writes nothing (no id is followed out of range).
// Every lane stores its own rows (24, 6 and 12 consecutive doubles at the stride of a row): staging a wave's rows through LDS so
// that they leave as contiguous runs measured the same 4 - 6 us alone -- the launch -- and slower in front of an evaluation
// ("Items from body states").
#pragma once

constexpr int kBodiesUnbound = -2;      // bind-table entry of an instruction pfc_set_instruction_bodies has not seen
constexpr int kBodiesWave = 64;         // items per workgroup

struct BodiesArgs {
    int n_items, n_ins, n_scene, n_body;
    const int *ins_ids;            // n_items, or NULL: item i uses instruction i
    const int *scene;              // n_items, or NULL: scene 0
    const int *bind;               // n_ins x 2: body of mesh_1, body of mesh_2 (-1: the world; kBodiesUnbound)
    const double *x_w_b;           // n_scene n_body x 12: R (9, column-major), t (3)
    const double *twist_w_b;       // n_scene n_body x 6: [angular; linear] in world about the world origin
    double *pose, *twist, *x_w_r2; // n_items x 24, x 6, x 12; each may be NULL (not wanted)
    int *body_1, *body_2;          // n_items; each may be NULL
};

// World pose (12) and twist (6) of `body` in the scene whose bodies start at `base`; the world is (I, 0) at rest.
__device__ inline void bodies_state(const BodiesArgs &g, size_t base, int body, double *x, double *tw) {
    if (body < 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) x[e] = (e == 0 || e == 4 || e == 8) ? 1.0 : 0.0;
#pragma unroll
        for (int e = 0; e < 6; ++e) tw[e] = 0.0;
        return;
    }
    const double *xs = g.x_w_b + 12 * (base + (size_t)body), *ts = g.twist_w_b + 6 * (base + (size_t)body);
#pragma unroll
    for (int e = 0; e < 12; ++e) x[e] = xs[e];
#pragma unroll
    for (int e = 0; e < 6; ++e) tw[e] = ts[e];
}

// pose (24) and twist (6) of an item from the world states of its two bodies.  x2[3 r + c] is R2w[r][c] (the transpose of a
// column-major matrix is its row-major reading), x1[3 c + k] is R_w1[k][c].  One statement, two number types: double
// (k_items_from_bodies) and ScatDual (k_dual_seeds_from_bodies).
template <class T> __device__ inline void bodies_item(const T *x1, const T *tw1, const T *x2, const T *tw2, T *pose, T *twist) {
    T t2w[3], d[6], ang[3], lin[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) t2w[r] = -((x2[3 * r] * x2[9] + x2[3 * r + 1] * x2[10]) + x2[3 * r + 2] * x2[11]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r)
            pose[3 * c + r] = (x2[3 * r] * x1[3 * c] + x2[3 * r + 1] * x1[3 * c + 1]) + x2[3 * r + 2] * x1[3 * c + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) pose[9 + r] = ((x2[3 * r] * x1[9] + x2[3 * r + 1] * x1[10]) + x2[3 * r + 2] * x1[11]) + t2w[r];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) pose[12 + 3 * c + r] = pose[3 * r + c];
#pragma unroll
    for (int r = 0; r < 3; ++r) pose[21 + r] = -((pose[3 * r] * pose[9] + pose[3 * r + 1] * pose[10]) + pose[3 * r + 2] * pose[11]);
#pragma unroll
    for (int e = 0; e < 6; ++e) d[e] = tw2[e] - tw1[e];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        ang[r] = (x2[3 * r] * d[0] + x2[3 * r + 1] * d[1]) + x2[3 * r + 2] * d[2];
        lin[r] = (x2[3 * r] * d[3] + x2[3 * r + 1] * d[4]) + x2[3 * r + 2] * d[5];
    }
    twist[0] = ang[0]; twist[1] = ang[1]; twist[2] = ang[2];
    twist[3] = lin[0] + (t2w[1] * ang[2] - t2w[2] * ang[1]);
    twist[4] = lin[1] + (t2w[2] * ang[0] - t2w[0] * ang[2]);
    twist[5] = lin[2] + (t2w[0] * ang[1] - t2w[1] * ang[0]);
}

__global__ void __launch_bounds__(kBodiesWave) k_items_from_bodies(BodiesArgs g) {
    const int i = blockIdx.x * kBodiesWave + (int)threadIdx.x;
    if (i >= g.n_items) return;
    const int ins = g.ins_ids ? g.ins_ids[i] : i;
    const int sc = g.scene ? g.scene[i] : 0;
    if (ins < 0 || ins >= g.n_ins || sc < 0 || sc >= g.n_scene) return;
    const int b1 = g.bind[2 * ins], b2 = g.bind[2 * ins + 1];
    if (b1 < -1 || b1 >= g.n_body || b2 < -1 || b2 >= g.n_body) return;
    double x1[12], x2[12], tw1[6], tw2[6], pose[24], twist[6];
    const size_t base = (size_t)sc * (size_t)g.n_body;
    bodies_state(g, base, b1, x1, tw1);
    bodies_state(g, base, b2, x2, tw2);
    bodies_item<double>(x1, tw1, x2, tw2, pose, twist);
    const int off = g.scene ? sc * g.n_body : 0;
    if (g.body_1) g.body_1[i] = b1 < 0 ? -1 : b1 + off;
    if (g.body_2) g.body_2[i] = b2 < 0 ? -1 : b2 + off;
    if (g.pose) {
        double *o = g.pose + 24 * (size_t)i;
#pragma unroll
        for (int e = 0; e < 24; ++e) o[e] = pose[e];
    }
    if (g.twist) {
        double *o = g.twist + 6 * (size_t)i;
#pragma unroll
        for (int e = 0; e < 6; ++e) o[e] = twist[e];
    }
    if (g.x_w_r2) {
        double *o = g.x_w_r2 + 12 * (size_t)i;
#pragma unroll
        for (int e = 0; e < 12; ++e) o[e] = x2[e];
    }
}

// ---- Dual seeds -------------------------------------------------------------------------------------------------------------
// k_dual_seeds_from_bodies: what the same refresh leaves in the bodyBodyCache when the body states are ForwardDiff.Duals -- the
// partials of pose, twist and x_rw_r2 for one seed direction per lane, in the layouts pfc_eval_dual_device[_more],
// pfc_apply_local_jacobian_device (d_dpose, d_dtwist) and pfc_scatter_generalized_dual_device (d_dx_w_r2) read.  bodies_item runs
// on ScatDual (pfc_scatter.h: value and one partial, ForwardDiff's rules), so a partial is a fixed function of the inputs: the
// same bytes on every call.  Lane k = item * n_dir + direction; the value states are read again by every direction of an item
// (cache hits); the invalid-item rule and the plain per-lane stores are those of k_items_from_bodies.
struct BodiesSeedArgs {
    int n_items, n_dir, n_ins, n_scene, n_body;
    const int *ins_ids, *scene, *bind;      // as BodiesArgs
    const double *x_w_b, *twist_w_b;        // as BodiesArgs
    const double *dx_w_b;                   // n_scene n_body x n_dir x 12: partials of x_w_b, or NULL (zeros)
    const double *dtwist_w_b;               // n_scene n_body x n_dir x 6: partials of twist_w_b, or NULL (zeros)
    double *dpose, *dtwist, *dx_w_r2;       // n_items n_dir x 24, x 6, x 12; each may be NULL (not wanted)
};

// bodies_state on Dual numbers: direction `dir` of the partials; the world and a NULL partial array are zeros.
__device__ inline void bodies_state_dual(const BodiesSeedArgs &g, size_t base, int body, int dir, ScatDual *x, ScatDual *tw) {
    if (body < 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) x[e] = ScatDual{(e == 0 || e == 4 || e == 8) ? 1.0 : 0.0, 0.0};
#pragma unroll
        for (int e = 0; e < 6; ++e) tw[e] = ScatDual{0.0, 0.0};
        return;
    }
    const size_t b = base + (size_t)body, bk = b * (size_t)g.n_dir + (size_t)dir;
    const double *xs = g.x_w_b + 12 * b, *ts = g.twist_w_b + 6 * b;
    const double *dxs = g.dx_w_b ? g.dx_w_b + 12 * bk : nullptr, *dts = g.dtwist_w_b ? g.dtwist_w_b + 6 * bk : nullptr;
#pragma unroll
    for (int e = 0; e < 12; ++e) x[e] = ScatDual{xs[e], dxs ? dxs[e] : 0.0};
#pragma unroll
    for (int e = 0; e < 6; ++e) tw[e] = ScatDual{ts[e], dts ? dts[e] : 0.0};
}

__global__ void __launch_bounds__(kBodiesWave) k_dual_seeds_from_bodies(BodiesSeedArgs g) {
    const long long k = (long long)blockIdx.x * kBodiesWave + (long long)threadIdx.x;
    if (k >= (long long)g.n_items * g.n_dir) return;
    const int i = (int)(k / g.n_dir), dir = (int)(k % g.n_dir);
    const int ins = g.ins_ids ? g.ins_ids[i] : i;
    const int sc = g.scene ? g.scene[i] : 0;
    if (ins < 0 || ins >= g.n_ins || sc < 0 || sc >= g.n_scene) return;
    const int b1 = g.bind[2 * ins], b2 = g.bind[2 * ins + 1];
    if (b1 < -1 || b1 >= g.n_body || b2 < -1 || b2 >= g.n_body) return;
    ScatDual x1[12], x2[12], tw1[6], tw2[6], pose[24], twist[6];
    const size_t base = (size_t)sc * (size_t)g.n_body;
    bodies_state_dual(g, base, b1, dir, x1, tw1);
    bodies_state_dual(g, base, b2, dir, x2, tw2);
    bodies_item<ScatDual>(x1, tw1, x2, tw2, pose, twist);
    if (g.dpose) {
        double *o = g.dpose + 24 * (size_t)k;
#pragma unroll
        for (int e = 0; e < 24; ++e) o[e] = pose[e].d;
    }
    if (g.dtwist) {
        double *o = g.dtwist + 6 * (size_t)k;
#pragma unroll
        for (int e = 0; e < 6; ++e) o[e] = twist[e].d;
    }
    if (g.dx_w_r2) {
        double *o = g.dx_w_r2 + 12 * (size_t)k;
#pragma unroll
        for (int e = 0; e < 12; ++e) o[e] = x2[e].d;
    }
}
