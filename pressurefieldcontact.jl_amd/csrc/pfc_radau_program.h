// pfc_radau_program.h -- the gripper program of the discrete controller: timed instructions and the slip-triggered grip torque of the
// reference's test/pencil.jl (get_grip_ins and the tau_grip choice of grip_control!), once per batch step in front of k_radau_control.
// The statement is in include/pfc.h (pfc_radau_program_device).  One lane per scene, 64-lane blocks: the work of a scene is nine
// loads, one sqrt, one atan2, a few compares and at most n_act + n_grip + 6 stores.  Nothing in LDS, no atomics, no scratch, plain
// vector stores.  A lane >= n_scene and a scene that is not due load only what the decision needs and store nothing.
// No index is followed out of range: the lane bounds the scene, cursor stays in 0 .. n_ins - 1 (it starts there and moves only while
// cursor < n_ins - 1), body < n_body, n_act <= nv and grip[] < nv are validated on the host.
#pragma once

constexpr int kRadProgBlock = 64;

struct RadauProgramArgs {
    int n_scene, n_body, nv, n_act, n_ins, body, n_grip;
    double tau_soft, tau_hard;
    const int *grip;                        // n_grip: the grip coordinates, each < nv
    const double *prog_dt, *prog_slip;      // n_scene x n_ins
    const double *prog_q;                   // n_scene x n_ins x n_act
    const double *t, *t_last;               // n_scene: the controller's clock as it is before k_radau_control advances it
    const double *x_w_b;                    // n_scene x n_body x 12: R column-major, then t
    const int *istate;                      // n_scene x 8, or NULL: a scene with exit flag 5 or the parked mark is left alone
    int *cursor;                            // n_scene x 2: cursor, pops
    double *pstate;                         // n_scene x 4: t0, rot_0, angle, tau_grip
    double *seg_q;                          // n_scene x n_act: the controller's one segment
    double *seg_ff;                         // n_scene x nv
};

__global__ void __launch_bounds__(kRadProgBlock) k_radau_program(RadauProgramArgs g) {
    const size_t sc = (size_t)blockIdx.x * kRadProgBlock + threadIdx.x;
    if (sc >= (size_t)g.n_scene) return;
    if (g.istate && (g.istate[8 * sc + kRadExit] == 5 || g.istate[8 * sc + kRadIntSpare] != 0)) return;
    const double t = g.t[sc];
    if (!(g.t_last[sc] <= t)) return;       // not due: the record and the segment stay byte for byte
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    // 1. the angle of the watched body's rotation
    const double *R = g.x_w_b + (sc * (size_t)g.n_body + (size_t)g.body) * 12;
    const double a = R[5] - R[7], b = R[6] - R[2], c = R[1] - R[3];
    const double s = sqrt((a * a + b * b) + c * c);
    const double w = ((R[0] + R[4]) + R[8]) - 1.0;
    const double angle = atan2(s, w);
    // 2., 3. the instruction in force: at most one pop, the last instruction never expires
    int cur = g.cursor[2 * sc], pops = g.cursor[2 * sc + 1];
    double t0 = g.pstate[4 * sc], rot_0 = g.pstate[4 * sc + 1];
    if (t0 == inf) t0 = t;
    const double *dt = g.prog_dt + sc * (size_t)g.n_ins;
    if (cur < g.n_ins - 1 && dt[cur] < (t - t0)) { cur += 1; pops += 1; t0 = t; rot_0 = angle; }
    // 4. the grip torque
    const double sl = g.prog_slip[sc * (size_t)g.n_ins + (size_t)cur];
    double tau_grip;
    if (sl == -inf) tau_grip = 0.0;
    else if (sl == 0.0) tau_grip = g.tau_hard;
    else if (sl == inf) tau_grip = g.tau_soft;
    else tau_grip = fabs(angle - rot_0) < sl ? g.tau_soft : g.tau_hard;
    // 5. the scene's segment, then the record
    const double *pq = g.prog_q + (sc * (size_t)g.n_ins + (size_t)cur) * (size_t)g.n_act;
    for (int k = 0; k < g.n_act; ++k) g.seg_q[sc * (size_t)g.n_act + (size_t)k] = pq[k];
    for (int k = 0; k < g.n_grip; ++k) g.seg_ff[sc * (size_t)g.nv + (size_t)g.grip[k]] = tau_grip;
    g.cursor[2 * sc] = cur; g.cursor[2 * sc + 1] = pops;
    g.pstate[4 * sc] = t0; g.pstate[4 * sc + 1] = rot_0; g.pstate[4 * sc + 2] = angle; g.pstate[4 * sc + 3] = tau_grip;
}
