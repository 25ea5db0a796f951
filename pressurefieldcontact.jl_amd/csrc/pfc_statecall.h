// pfc_statecall.h -- the buffers of a chained state call (pfc_eval_bodies_device .. pfc_state_derivative_dual_device_more), by name.
// Plain C++ (no HIP, no pfc_context).  The groups are those include/pfc.h documents; the same struct holds the values and, a second
// time, their partials along n_dir directions (a field without a partial -- body_1, body_2, counts, info -- stays null there).
// Every pointer is a device pointer.  A public entry fills one StateCall from its parameters -- the only place where a parameter
// position meets a field name -- and the chain and its stages read fields from then on.
#pragma once

struct StateBufs {
    const double *q = nullptr, *v = nullptr, *s = nullptr, *tau = nullptr;       // the state and the applied forces: inputs
    double *x_w_b = nullptr, *twist_w_b = nullptr, *jac = nullptr;               // body states (kinematics)
    double *pose = nullptr, *twist = nullptr, *x_w_r2 = nullptr;                 // items (formed from the body states)
    int *body_1 = nullptr, *body_2 = nullptr;
    double *wrench = nullptr, *sdot = nullptr, *f = nullptr;                     // results (the evaluation and the scatter)
    int *counts = nullptr;
    double *qdot = nullptr, *H = nullptr, *c = nullptr, *vdot = nullptr;         // dynamics and the solve
    int *info = nullptr;
};

// The continuous feedback law of a call (pfc_feedback_device's arguments; the kernels: pfc_feedback.h).  The tables have the shapes
// of pfc_radau_set_controller's for n_sched scenes; row r of a call reads the schedule of scene r % n_sched.
struct FeedbackLaw {
    int n_sched = 0, n_act = 0, n_seg = 0;
    const int *act = nullptr;                                                   // n_act
    const double *kp = nullptr, *kd = nullptr, *a_max = nullptr;                // n_act; a_max null: no clamp
    const double *seg_t = nullptr, *seg_q = nullptr, *seg_ff = nullptr;         // n_sched x n_seg, x n_act, x nv; seg_ff null: zeros
    const double *t = nullptr;                                                  // one time per row
    double *tau = nullptr;       // rows x nv: the law plus the call's tau -- what the solve reads
    double *dtau = nullptr;      // n_scene x n_dir x nv: its partials (Dual calls)
};

// The applied body wrenches of a call (pfc_body_wrench_device's arguments; the kernels: pfc_body_wrench.h).  The schedule has
// n_sched scenes; row r of a call reads the loads of scene r % n_sched.
struct BodyWrenches {
    int n_sched = 0, n_body = 0, n_w = 0, n_seg = 0;
    const int *body = nullptr, *frame = nullptr;                                // n_w: the body, 0 world axes / 1 body axes
    const double *point = nullptr;                                              // n_w x 3, in the body frame
    const double *seg_t = nullptr, *seg_w = nullptr;                            // n_sched x n_seg, x n_w x 6 [moment; force]
    const double *t = nullptr;                                                  // one time per row
    double *tau = nullptr;       // rows x nv: the wrenches' torques plus the tau in front of them -- what the solve reads
    double *dtau = nullptr;      // n_scene x n_dir x nv: its partials (Dual calls)
};

struct StateCall {
    int n_items = 0, n_dir = 0, n_scene = 0;
    const int *ins_ids = nullptr, *scene = nullptr;
    void *stream = nullptr;      // the caller's stream, null: the context's own
    StateBufs val, par;          // the values, and their partials (Dual calls)
    // null in every public entry: the chain launches what it launched without one.  Set (the Radau driver): the law is evaluated
    // between the dynamics and the solve, which then reads law->tau and, in a Dual call, law->dtau in place of val.tau and par.tau
    const FeedbackLaw *law = nullptr;
    // null in every public entry, likewise.  Set (the Radau driver): the wrenches are evaluated behind the law -- on law->tau and
    // law->dtau where a law is set, on val.tau and par.tau otherwise -- and the solve reads push->tau and push->dtau
    const BodyWrenches *push = nullptr;
};

// A buffer that an entry declares const -- the values of a `_more` entry, the body states of the `_bodies` entries -- as the record's
// field.  Such a call only reads it: every stage it launches takes that field through a const parameter, and a `more` call passes
// null where a first call passes a value output.
template <class T>
T *kept_value(const T *p) { return const_cast<T *>(p); }
