// pfc_feedback.h -- the continuous joint feedback law: the computed-torque PD of k_radau_control (pfc_radau.h), evaluated inside the
// differential equation -- at every stage-scene's (q, v, H, c, t) between the dynamics and the solve -- and its partials along the
// directions of a Jacobian chunk.  The reference's continuous_controller(tm, t), called in calcXd!
// (src/contact_algorithms_non_friction.jl:29) on Float64 and on Dual states alike.  The statements: include/pfc.h
// (pfc_feedback_device, pfc_feedback_dual_device).  A textual part of pfc_hip.hip, behind pfc_statecall.h (FeedbackLaw).
//
// k_radau_control's conventions: plain Float64, no fma (the build has -ffp-contract=off), the written order, no atomics, nothing in
// LDS, no scratch, plain vector stores.  One 64-lane wave per row (k_feedback: a scene or a stage-scene) or per (scene, direction)
// (k_feedback_dual); lane i = coordinate i (nv <= 64, nq = nv); lane b < n_act also computes the clamped acc of actuated coordinate
// act[b] (and its partial), which the row sums read with a lane read, b ascending.  The segment search depends on the row only:
// wave-uniform.  Every lane stays until the last lane read: no early return.
// No index is followed out of range: the grid is the row count, nv <= 64 and n_act <= nv are validated on the host, act[] < nv is the
// caller's guarantee (pfc_radau_set_feedback validates it), the segment index is a count of at most n_seg - 1 comparisons, row r
// reads the schedule of scene r % n_sched, lanes >= nv load and store nothing.
#pragma once

constexpr int kFbWave = 64;

struct FeedbackArgs {
    FeedbackLaw w;                          // the tables, t (n_rows) and tau (n_rows x nv, the output)
    int n_rows, nv;
    const double *q, *v, *H, *c;            // n_rows x nv; x nv; x nv x nv row-major; x nv
    const double *tau_in;                   // n_rows x nv, or NULL
};

struct FeedbackDualArgs {
    FeedbackLaw w;                          // the tables, t (n_scene) and dtau (n_scene x n_dir x nv, the output)
    int n_scene, n_dir, nv;
    const double *q, *v, *H;                // the values: n_scene x nv; x nv; x nv x nv
    const double *dq, *dv;                  // n_scene x n_dir x nv: the seeds; each may be NULL (zeros)
    const double *dH, *dc;                  // n_scene x n_dir x nv x nv; x nv: pfc_dynamics_dual_device's outputs
};

// The segment of row `sched` at time t: the number of j >= 1 with seg_t[j] <= t.
__device__ inline size_t fb_segment(const FeedbackLaw &w, int sched, double t) {
    int k = 0;
    if (w.n_seg > 1) {
        const double *st = w.seg_t + (size_t)sched * (size_t)w.n_seg;
        for (int j = 1; j < w.n_seg; ++j) k += st[j] <= t ? 1 : 0;
    }
    return (size_t)sched * (size_t)w.n_seg + (size_t)k;
}

// acc of actuated entry b at (q, v) of a row, before the clamp; *am receives a_max (+inf without one).
__device__ inline double fb_acc(const FeedbackLaw &w, size_t seg, int b, const double *q, const double *v, double *am) {
    const int co = w.act[b];
    const double e = q[co] - w.seg_q[seg * (size_t)w.n_act + (size_t)b];
    *am = w.a_max ? w.a_max[b] : __builtin_inf();
    return (-(w.kd[b] * v[co])) - w.kp[b] * e;
}

__global__ void __launch_bounds__(kFbWave) k_feedback(FeedbackArgs g) {
    const int row = (int)blockIdx.x, i = (int)threadIdx.x, nv = g.nv;
    const FeedbackLaw &w = g.w;
    const size_t seg = fb_segment(w, row % w.n_sched, w.t[row]);
    const size_t at = (size_t)row * (size_t)nv;
    double acc = 0.0;
    if (i < w.n_act) {
        double am;
        acc = fb_acc(w, seg, i, g.q + at, g.v + at, &am);
        if (acc < -am) acc = -am;
        if (acc > am) acc = am;
    }
    const bool lane = i < nv;
    const double *Hrow = g.H + (at + (size_t)(lane ? i : 0)) * (size_t)nv;
    const double ff = lane && w.seg_ff ? w.seg_ff[seg * (size_t)nv + (size_t)i] : 0.0;
    const double ci = lane ? g.c[at + (size_t)i] : 0.0;
    const double ti = lane && g.tau_in ? g.tau_in[at + (size_t)i] : 0.0;
    double sum = 0.0;
    bool actuated = false;
    for (int b = 0; b < w.n_act; ++b) {
        const int co = w.act[b];
        const double ab = __shfl(acc, b, kFbWave);
        if (lane) sum = sum + Hrow[co] * ab;
        actuated = actuated || co == i;
    }
    if (!lane) return;      // behind the last lane read
    double tau;
    if (actuated) {
        const double law = (sum + ci) + ff;
        tau = g.tau_in ? law + ti : law;
    } else if (w.seg_ff) {
        tau = g.tau_in ? ff + ti : ff;
    } else {
        tau = ti;           // copied, not added to zero: a signed zero survives; +0.0 without tau_in
    }
    w.tau[at + (size_t)i] = tau;
}

__global__ void __launch_bounds__(kFbWave) k_feedback_dual(FeedbackDualArgs g) {
    const int sc = (int)blockIdx.x / g.n_dir, i = (int)threadIdx.x, nv = g.nv;
    const FeedbackLaw &w = g.w;
    const size_t seg = fb_segment(w, sc % w.n_sched, w.t[sc]);
    const size_t at = (size_t)sc * (size_t)nv, dat = (size_t)blockIdx.x * (size_t)nv;      // blockIdx.x = sc n_dir + dir
    double acc = 0.0, dacc = 0.0;
    if (i < w.n_act) {
        double am;
        const int co = w.act[i];
        acc = fb_acc(w, seg, i, g.q + at, g.v + at, &am);
        const double dqa = g.dq ? g.dq[dat + (size_t)co] : 0.0, dva = g.dv ? g.dv[dat + (size_t)co] : 0.0;
        dacc = (-(w.kd[i] * dva)) - w.kp[i] * dqa;
        if (acc < -am) { acc = -am; dacc = 0.0; }
        if (acc > am) { acc = am; dacc = 0.0; }
    }
    const bool lane = i < nv;
    const size_t r = (size_t)(lane ? i : 0) * (size_t)nv;
    const double *Hrow = g.H + at * (size_t)nv + r, *dHrow = g.dH + dat * (size_t)nv + r;
    double dsum = 0.0;
    bool actuated = false;
    for (int b = 0; b < w.n_act; ++b) {
        const int co = w.act[b];
        const double ab = __shfl(acc, b, kFbWave), dab = __shfl(dacc, b, kFbWave);
        if (lane) dsum = dsum + (dHrow[co] * ab + Hrow[co] * dab);      // the product rule of ScatDual: a.d b.v + a.v b.d
        actuated = actuated || co == i;
    }
    if (lane) w.dtau[dat + (size_t)i] = actuated ? dsum + g.dc[dat + (size_t)i] : 0.0;
}

// The stage times of an attempt: row s n_scene + i = (c_s h_i) + t_i for s < NS(rule_i) -- two roundings, the reference's
// table.c[i] * rr.step.h + t -- and t_i for every other row.  c: the nodes of rule 1 (one) and rule 2 (three).
struct StageTimeArgs {
    int n_scene;
    double c1, c2[3];
    const double *t, *h;                    // n_scene
    const int *rule;                        // n_scene: 1 or 2
    double *out;                            // 3 n_scene
};

__global__ void __launch_bounds__(256) k_radau_stage_times(StageTimeArgs g) {
    const size_t total = 3 * (size_t)g.n_scene;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int s = (int)(e / (size_t)g.n_scene);
        const size_t i = e % (size_t)g.n_scene;
        const int rule = g.rule[i];
        const double t = g.t[i];
        double out = t;
        if (rule == 2) out = ((s == 0 ? g.c2[0] : s == 1 ? g.c2[1] : g.c2[2]) * g.h[i]) + t;
        else if (s == 0) out = (g.c1 * g.h[i]) + t;
        g.out[e] = out;
    }
}
