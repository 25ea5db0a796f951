// pfc_hip.hip — C ABI (include/pfc.h) and launch sequence of libpfc_hip (MI355X / gfx950).  See DESIGN.md.
//
// Device code lives in the headers included below (all in namespace pfc):
//   pfc_kernels.h  HBM records, small-vector math, SAT, wave64 helpers (ballot prefix, segmented DPP scans)
//   pfc_bp.h       broadphase: k_bp_expand (seed levels), k_bp_dfs32 (single-precision workgroup descent with the
//                  cooperative exact test), k_bp_dfs (all-Float64 descent, A/B option)         [tree_types.jl:88-111]
//   pfc_np.h       narrowphase: k_narrow (gather, clip in an LDS polygon ring, fan quadrature, pressure, regularized
//                  friction, bristle moments, kept polygons; MODE 2 = clip only for big batches), k_integ (quadrature
//                  and per-item sums over the compacted polygons), k_fric (bristle friction over kept polygons); their
//                  forms for scenarios without a regularized instruction / with rule 2 throughout (k_integ_br*, k_fric_q3)
//   pfc_fused.h    k_fused: a small scene's whole evaluation in one launch, one workgroup per item
//   pfc_dual.h     the same path on (value, partial) numbers: k_dual_flags / k_dual_select (the pairs a chunk's seeds
//                  touch), k_narrow_dual, k_dual_poly, k_dual_eig, k_dual_final
//   pfc_br.h       k_shift, k_eig (6x6 Jacobi, one wave per item), k_final (+ result packing), k_scatter, k_selftest
//   option "fixed_order" (bit-reproducible evaluations): k_integ_fixed / k_fric_fixed (pfc_np.h), k_shift_fixed (pfc_br.h),
//                  k_fixed_reduce (pfc_dual.h), the FixedSink record lists of accumulate_items / dual_accumulate, and
//                  pfc_sort.hip (a translation unit of its own: rocPRIM radix sort of the candidate list)
//   pfc_surface.h  k_surf_count / k_surf_summary / k_surf_emit: the contact surface in canonical order (pfc_contact_surface)
//   pfc_surface_fric.h  k_sfric_mom / k_sfric_eig / k_sfric_pass / k_sfric_final: its friction half (pfc_contact_surface_fric)
//   pfc_scatter.h  k_scat_keys / k_scat_off / k_scat_world / k_scat_proj: the third-law scatter on Dual numbers in the reference's
//                  item order (pfc_scatter_generalized_dual)
//   pfc_ljac.h     k_ljac_seeds / k_ljac_pack / k_ljac_apply: per-item contact Jacobians from unit-seed Dual passes and their
//                  product with further seed chunks (pfc_local_jacobian, pfc_apply_local_jacobian)
//   pfc_bodies.h   k_items_from_bodies: pose, twist, x_rw_r2 and body ids of every item from the bodies' world poses and twists
//                  (pfc_items_from_bodies, pfc_eval_bodies); k_dual_seeds_from_bodies: their partials from the partials of the body
//                  states (pfc_dual_seeds_from_bodies, pfc_eval_dual_bodies_device[_more])
//   pfc_kin.h      k_kinematics / k_kin_jacobian: the bodies' world poses, twists and geometric Jacobians from the joint state (q, v)
//                  of a small tree (pfc_set_mechanism, pfc_kinematics, pfc_eval_state); k_kinematics_dual / k_kin_jacobian_dual: their
//                  partials from the seed directions of a Jacobian chunk (pfc_kinematics_dual, pfc_eval_dual_state_device[_more])
//   pfc_dyn.h      k_dynamics: qdot, the mass matrix and the bias from (q, v), the bodies' world states and their inertias
//                  (pfc_set_inertia, pfc_dynamics); k_accel: vdot = H^-1 ((f - c) + tau) by Cholesky (pfc_accelerations,
//                  pfc_state_derivative); k_dynamics_dual / k_accel_dual: their partials for the seed directions of a Jacobian
//                  chunk (pfc_dynamics_dual, pfc_accelerations_dual, pfc_state_derivative_dual_device[_more])
//   pfc_feedback.h k_feedback / k_feedback_dual: the continuous joint feedback law between the dynamics and the solve, value and
//                  partials (pfc_feedback_device, pfc_feedback_dual_device, pfc_radau_set_feedback); k_radau_stage_times
//   pfc_body_wrench.h k_body_wrench / k_body_wrench_dual: applied body wrenches projected into tau behind the law, value and
//                  partials (pfc_body_wrench_device, pfc_body_wrench_dual_device, pfc_radau_set_body_wrenches)
//   pfc_multi.h    host code: multi-device handles (pfc_create_multi)
// This file: mesh record preparation (k_prep_tri, k_prep_tet), per-item setup (k_setup_items), work-list management,
// hipGraph capture / replay, the two-half evaluation and every extern "C" entry point.
#include "pfc_kernels.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pfc.h"
#include "pfc_sort.h"
#include "pfc_hostblocks.h"
#include "pfc_statecall.h"

namespace pfc {

// =================================================================================================================
// mesh preparation kernels (pfc_finalize)
// =================================================================================================================
__global__ void k_prep_tri(int n, const double *__restrict__ pt, const int *__restrict__ tri, TriRec *__restrict__ out) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    V3 a = ld3(pt + 3 * tri[3 * k]), b = ld3(pt + 3 * tri[3 * k + 1]), c = ld3(pt + 3 * tri[3 * k + 2]);
    V3 nh = normalize(vector_area(a, b, c));  // triangleNormal, geometry_kernel.jl:10
    TriRec r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = b.x; r.v[4] = b.y; r.v[5] = b.z;
    r.v[6] = c.x; r.v[7] = c.y; r.v[8] = c.z; r.n[0] = nh.x; r.n[1] = nh.y; r.n[2] = nh.z;
    r.pad[0] = r.pad[1] = r.pad[2] = r.pad[3] = 0.0;
    out[k] = r;
}

__global__ void k_prep_tet(int n, const double *__restrict__ pt, const double *__restrict__ eps,
                           const int *__restrict__ tet, TetRec *__restrict__ out, double *__restrict__ out_eps,
                           unsigned *status) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double A[16], e[4];
    TetRec r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int v = tet[4 * k + j];
        A[4 * j] = pt[3 * v]; A[4 * j + 1] = pt[3 * v + 1]; A[4 * j + 2] = pt[3 * v + 2]; A[4 * j + 3] = 1.0;
        r.xrz[3 * j] = A[4 * j]; r.xrz[3 * j + 1] = A[4 * j + 1]; r.xrz[3 * j + 2] = A[4 * j + 2];
        e[j] = eps[v];
        out_eps[4 * (size_t)k + j] = e[j];
    }
    double id = inv4(A, r.xzr);
    if (!(__builtin_fabs(id) <= 1.79769313486231570815e308)) atomicOr(status, kStNonFinite);
    // ϵ_r2 = ϵ2 * x_ζ2_r2 (1x4 times 4x4)
#pragma unroll
    for (int j = 0; j < 4; ++j)
        r.epsr[j] = ((e[0] * r.xzr[4 * j] + e[1] * r.xzr[4 * j + 1]) + e[2] * r.xzr[4 * j + 2]) + e[3] * r.xzr[4 * j + 3];
    out[k] = r;
}

// =================================================================================================================
// per-evaluation setup
// =================================================================================================================
struct EvalArgs {
    int n_items;
    const int *ins_ids;      // may be null
    const double *pose, *twist, *s;
    const double *bp_pose;   // may be null: the pose the broadphase culls with (pfc_eval_dual_bp), same packing as pose
    const InsDev *ins;
    const MeshDev *meshes;
    int n_ins;
    ItemRec *items;
    WorkRec *frontier0;
    int *fcount;             // [max_levels + 2]
    double *acc;             // n_items x kAccStride
    int *icnt;               // n_items x 4
    unsigned *status;
};

// (The record is written field by field: built in registers and stored whole -- 576 bytes -- the kernel spilled 18 VGPRs.)
__global__ void __launch_bounds__(64) k_setup_items(EvalArgs g) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    {   // the accumulators of the workgroup's items, cleared with consecutive lanes on consecutive doubles (44 stores of 512
        // contiguous bytes per wave instead of 44 stores to 64 different cache lines each)
        const int i0 = blockIdx.x * blockDim.x;
        const int n_here = g.n_items - i0 < (int)blockDim.x ? g.n_items - i0 : (int)blockDim.x;
        double *a0 = g.acc + (size_t)i0 * kAccStride;
        for (int k = threadIdx.x; k < n_here * kAccStride; k += blockDim.x) a0[k] = 0.0;
    }
    if (i >= g.n_items) return;
    int id = g.ins_ids ? g.ins_ids[i] : i;
    if (id < 0 || id >= g.n_ins) {
        atomicOr(g.status, kStBadIns);
        id = 0;
    }
    const InsDev in = g.ins[id];
    const MeshDev m1 = g.meshes[in.m1], m2 = g.meshes[in.m2];
    const double *p = g.pose + 24 * (size_t)i;
    // x_r1_r2 of the broadphase: the pose's own, or the one of m.float's state when the evaluation runs on Duals
    // (calcTriTetIntersections!, non_friction.jl:94-101; k_repose puts the pose's own back once the broadphase is through)
    const double *pb = (g.bp_pose ? g.bp_pose + 24 * (size_t)i : p) + 12;
    ItemRec &r = g.items[i];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 24; ++k) finite &= (__builtin_fabs(p[k]) <= 1.79769313486231570815e308);
#pragma unroll
    for (int k = 0; k < 9; ++k) r.R21[k] = p[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) r.t21[k] = p[9 + k];
    {
        double R12[9], t12[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) { R12[k] = pb[k]; r.R12[k] = R12[k]; r.R12f[k] = (float)R12[k]; finite &= (__builtin_fabs(R12[k]) <= 1.79769313486231570815e308); }
#pragma unroll
        for (int k = 0; k < 3; ++k) { t12[k] = pb[9 + k]; r.t12[k] = t12[k]; r.t12f[k] = (float)t12[k]; finite &= (__builtin_fabs(t12[k]) <= 1.79769313486231570815e308); }
        float q[4];
        r.pose_exact = pose_quat(R12, q) ? 0 : 1;
        r.q12[0] = q[0]; r.q12[1] = q[1]; r.q12[2] = q[2]; r.q12[3] = q[3];
        // absolute part of the single-precision test's error radius (pfc_bp.h, "Error radius E", (0)); a NaN / huge pose gives
        // NaN / inf here and every test of the item is settled exactly
        const double tm = fmax(fmax(__builtin_fabs(t12[0]), __builtin_fabs(t12[1])), __builtin_fabs(t12[2]));
        r.bp_eabs = (float)(1.4306e-6 * ((m1.cmax + m2.cmax) + tm)) * 1.000001f;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { r.w[k] = g.twist[6 * (size_t)i + k]; r.v[k] = g.twist[6 * (size_t)i + 3 + k]; }
#pragma unroll
    for (int k = 0; k < 6; ++k) r.s[k] = (g.s && in.model == PFC_BRISTLE) ? g.s[6 * (size_t)i + k] : 0.0;
    r.chi = in.chi; r.Ebar = m2.Ebar;  // Ē of mesh_2 only: non_friction.jl:131
    r.mu_s = in.mu_s; r.mu_d = in.mu_d; r.v_c = in.v_c; r.tau = in.tau; r.k_bar = in.k_bar; r.magic = in.magic;
    r.nodes1 = m1.nodes; r.nodes2 = m2.nodes; r.nf1 = m1.nodesf; r.nf2 = m2.nodesf; r.tri = m1.tri; r.tet = m2.tet;
    r.tet1 = m1.tri ? nullptr : m1.tet; r.eps1 = m1.tet_eps; r.eps2 = m2.tet_eps; r.Ebar1 = m1.Ebar;
    r.model = in.model; r.nq = (in.nq == 1) ? 1 : 3;  // quadrature POINTS of rule 1 / rule 2 (quadrature.jl:22,31)
    r.ins = id; r.pad = 0;
    r.pad2[0] = r.pad2[1] = 0;
    if (!finite) atomicOr(g.status, kStNonFinite);
    WorkRec w;
    // pad: bit 0 / bit 1 = node a / node b is a leaf (a one-element mesh: the root is the leaf), so that the
    // depth-first kernel can start a seed without reading the two nodes first
    w.item = i; w.a = 0; w.b = 0; w.pad = (m1.n_node == 1 ? 1 : 0) | (m2.n_node == 1 ? 2 : 0);
    g.frontier0[i] = w;
    *reinterpret_cast<int4 *>(g.icnt + 4 * (size_t)i) = make_int4(0, 0, 0, 0);
    if (i == 0) g.fcount[0] = g.n_items;
}

// After the broadphase of an evaluation with a broadphase pose of its own: x_r1_r2 of the item records becomes the pose's
// (the tet-tet op and the Dual passes read it: find_plane_tet, non_friction.jl:164,174-177).  What only the broadphase reads
// of a record -- q12, pose_exact, bp_eabs, R12f, t12f -- stays the broadphase pose's: those fields describe ONE pose between
// them (the single-precision test rotates with q12 and offsets with R12f, t12f), and nothing behind the broadphase reads them.
__global__ void k_repose(int n_items, const double *__restrict__ pose, ItemRec *__restrict__ items) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const double *p = pose + 24 * (size_t)i + 12;
#pragma unroll
    for (int k = 0; k < 9; ++k) items[i].R12[k] = p[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) items[i].t12[k] = p[9 + k];
}

#include "pfc_bp.h"
#include "pfc_clip.h"
#include "pfc_np.h"
#include "pfc_dual.h"
#include "pfc_br.h"
#include "pfc_fused.h"
#include "pfc_surface.h"
#include "pfc_surface_fric.h"
#include "pfc_scatter.h"
#include "pfc_ljac.h"
#include "pfc_bodies.h"
#include "pfc_kin.h"
#include "pfc_dyn.h"
#include "pfc_radau.h"
#include "pfc_radau_program.h"
#include "pfc_feedback.h"
#include "pfc_body_wrench.h"
#include "pfc_radau_tables.h"

}  // namespace pfc

// =================================================================================================================
// host side
// =================================================================================================================
using namespace pfc;
using namespace pfc_blocks;

namespace {

// ---- owning types -------------------------------------------------------------------------------------------------------
// Every GPU resource the host code holds -- device blocks, pinned host blocks, events, streams, graph executables -- is a
// member of one of these move-only types and is freed by its destructor: a context (pfc_context, pfc_multi) is torn down by
// `delete`, with its device current and its streams synchronised (pfc_destroy, multi_destroy).  No other code frees anything.
// PFC_LOG_ALLOC=1 logs every block with its address range when it is allocated and with its address when it is freed
// (diagnostic: match a faulting address with the buffer it lies behind; tests/test_gpu_ownership.py pairs the two).
inline bool log_alloc() { return std::getenv("PFC_LOG_ALLOC") != nullptr; }

// A device block of cap elements.  ensure() grows it (the content is lost) and reports through `moved` whether it did.
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t n, bool *moved = nullptr) { return grow(n, moved, false); }
    // fine-grained memory (host stores through the PCIe BAR: pfc_context::bar_in)
    hipError_t ensure_fine_grained(size_t n) { return grow(n, nullptr, true); }
    void release() {
        if (p) {
            if (log_alloc()) std::fprintf(stderr, "pfc free %p\n", (void *)p);
            (void)hipFree(p);
        }
        p = nullptr; cap = 0;
    }

private:
    hipError_t grow(size_t n, bool *moved, bool fine) {
        if (moved) *moved = false;
        if (n <= cap) return hipSuccess;
        release();
        if (moved) *moved = true;
        hipError_t e = fine ? hipExtMallocWithFlags((void **)&p, n * sizeof(T), hipDeviceMallocFinegrained) : hipMalloc((void **)&p, n * sizeof(T));
        if (e == hipSuccess) cap = n; else p = nullptr;
        if (log_alloc())
            std::fprintf(stderr, "pfc alloc %p .. %p (%zu bytes, element %zu)\n", (void *)p, (void *)((char *)p + n * sizeof(T)),
                         n * sizeof(T), sizeof(T));
        return e;
    }
};

// A block of doubles and a block of ints, each carved into the parts of an enum whose last value (ND, NI) counts them.  layout()
// turns the parts' sizes into offsets and totals -- kRound: every part rounded up to 32 doubles / 64 ints, an empty part taking one
// element; otherwise packed -- and ensure() allocates the double block, then the int block.  put() and get() are synchronous copies
// of n elements between the host and a part (from its element `at`); the host pointer's type picks the block.
template <auto ND, auto NI, bool kRound>
struct PartBlocks {
    using PartD = decltype(ND);
    using PartI = decltype(NI);
    DevBuf<double> dbl;
    DevBuf<int> itg;
    size_t od[ND] = {0}, oi[NI] = {0}, td = 0, ti = 0;
    double *D(PartD part) const { return &dbl.p[od[part]]; }
    int *I(PartI part) const { return &itg.p[oi[part]]; }
    void layout(const size_t (&sd)[ND], const size_t (&si)[NI]) {
        td = ti = 0;
        for (int k = 0; k < ND; ++k) { od[k] = td; td += kRound ? (std::max<size_t>(sd[k], 1) + 31) & ~(size_t)31 : sd[k]; }
        for (int k = 0; k < NI; ++k) { oi[k] = ti; ti += kRound ? (std::max<size_t>(si[k], 1) + 63) & ~(size_t)63 : si[k]; }
    }
    hipError_t ensure() {
        const hipError_t e = dbl.ensure(td);
        return e != hipSuccess ? e : itg.ensure(ti);
    }
    hipError_t put(PartD part, const double *host, size_t n, size_t at = 0) const {
        return hipMemcpy(D(part) + at, host, sizeof(double) * n, hipMemcpyHostToDevice);
    }
    hipError_t put(PartI part, const int *host, size_t n, size_t at = 0) const {
        return hipMemcpy(I(part) + at, host, sizeof(int) * n, hipMemcpyHostToDevice);
    }
    hipError_t get(double *host, PartD part, size_t n, size_t at = 0) const {
        return hipMemcpy(host, D(part) + at, sizeof(double) * n, hipMemcpyDeviceToHost);
    }
    hipError_t get(int *host, PartI part, size_t n, size_t at = 0) const {
        return hipMemcpy(host, I(part) + at, sizeof(int) * n, hipMemcpyDeviceToHost);
    }
};

// A pinned host block of cap elements: grown to kSlack times what is asked for, never shrunk, zeroed when it is allocated
// (completion words are polled from these blocks: never start from stale bytes).
template <class T, int kSlack = 1>
struct PinBuf {
    T *p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { release(); }
    hipError_t ensure(size_t n, bool *moved = nullptr) {
        if (moved) *moved = false;
        if (n <= cap) return hipSuccess;
        release();
        if (moved) *moved = true;
        const size_t bytes = n * kSlack * sizeof(T);
        hipError_t e = hipHostMalloc((void **)&p, bytes);
        if (e == hipSuccess) { cap = n * kSlack; std::memset(p, 0, bytes); } else p = nullptr;
        if (log_alloc()) std::fprintf(stderr, "pfc pinned %p .. %p\n", (void *)p, (void *)((char *)p + bytes));
        return e;
    }

private:
    void release() {
        if (p) {
            if (log_alloc()) std::fprintf(stderr, "pfc unpinned %p\n", (void *)p);
            (void)hipHostFree(p);
        }
        p = nullptr; cap = 0;
    }
};

// An event, stream or graph executable; converts to the raw handle for the runtime's calls, put() is where a create call
// writes a new one.
template <class H, hipError_t (*Destroy)(H)>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : h(o.h) { o.h = nullptr; }
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) { reset(); h = o.h; o.h = nullptr; }
        return *this;
    }
    ~Owned() { reset(); }
    void reset() { if (h) (void)Destroy(h); h = nullptr; }
    H *put() { reset(); return &h; }
    operator H() const { return h; }
};
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using GraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;

// What the host-pointer form of a _device call does with its arguments.  The fields are declared in order: a host pointer (null:
// the caller gave none), an element count and a direction.  commit() places each at the next 256-byte boundary of ONE device block
// (ints and doubles share it), grows the block (its content is lost) and enqueues the uploads of the inputs; at<T>(k) is field
// k's device pointer, null where the host gave none; finish() enqueues the downloads of the outputs and synchronises.  Every form
// synchronises before it returns, so one block per context (pfc_context::stage) serves them all.
struct Stage {
    enum { In = 1, Out = 2, Part = 4 };      // Part: an output whose used length the caller learns later (fetch)
    struct Field { void *host; size_t elem, count, off; int dir; };
    DevBuf<char> &buf;
    hipStream_t st;
    static constexpr int kMaxFields = 16;
    Field f[kMaxFields];
    int nf = 0;                              // fields declared; one past kMaxFields: too many, commit() fails
    size_t total = 0;
    Stage(DevBuf<char> &b, hipStream_t s) : buf(b), st(s) {}
    void clear() { nf = 0; total = 0; }
    template <class T> int add(int dir, const T *host, size_t count) {
        if (nf >= kMaxFields) { nf = kMaxFields + 1; return 0; }
        f[nf] = Field{const_cast<T *>(host), sizeof(T), count, total, dir};
        total = (total + sizeof(T) * count + 255) & ~(size_t)255;
        return nf++;
    }
    template <class T> int in(const T *host, size_t count) { return add(In, host, count); }
    template <class T> int out(T *host, size_t count) { return add(Out, host, count); }
    // a field without a host side: device scratch the caller fills (hipMemsetAsync)
    template <class T> int scratch(size_t count) { return add(0, (const T *)nullptr, count); }
    hipError_t commit() {
        hipError_t e = nf > kMaxFields ? hipErrorInvalidValue : buf.ensure(total);
        for (int k = 0; k < nf && e == hipSuccess; ++k)
            if ((f[k].dir & In) && f[k].host && f[k].count)
                e = hipMemcpyAsync(buf.p + f[k].off, f[k].host, f[k].elem * f[k].count, hipMemcpyHostToDevice, st);
        return e;
    }
    template <class T> T *at(int k) const { return f[k].host || !f[k].dir ? reinterpret_cast<T *>(buf.p + f[k].off) : nullptr; }
    // the download of the first `count` elements of field k, enqueued
    hipError_t fetch(int k, size_t count) {
        if (!f[k].host || !count) return hipSuccess;
        return hipMemcpyAsync(f[k].host, buf.p + f[k].off, f[k].elem * count, hipMemcpyDeviceToHost, st);
    }
    hipError_t finish() {
        hipError_t e = hipSuccess;
        for (int k = 0; k < nf && e == hipSuccess; ++k)
            if (f[k].dir & Out) e = fetch(k, f[k].count);
        return e == hipSuccess ? hipStreamSynchronize(st) : e;
    }
};

// The mechanism of pfc_set_mechanism, validated and packed: every table k_kinematics / k_kin_jacobian read lies in `blob` at a
// 256-byte boundary (KinArgs' names), so one copy uploads them.  k_dynamics' tables lie there too: each body's subtree (CSR) and the
// inertias of pfc_set_inertia (zeros until it is called: has_inertia).
struct KinHost {
    int n_body = 0, nq = 0, nv = 0;
    std::vector<char> blob;
    size_t o_jtype = 0, o_qoff = 0, o_voff = 0, o_path_off = 0, o_path = 0, o_x_p_j = 0, o_axis = 0, o_anc = 0;
    size_t o_sub_off = 0, o_sub = 0, o_inertia = 0;
    bool has_inertia = false;
    double gravity[3] = {0.0, 0.0, 0.0};
    template <class T> size_t put(const std::vector<T> &v) {
        const size_t off = blob.size(), bytes = sizeof(T) * v.size();
        blob.resize((off + bytes + 255) & ~(size_t)255);
        if (bytes) std::memcpy(blob.data() + off, v.data(), bytes);
        return off;
    }
};

struct HostMesh {
    int n_pt = 0, n_tri = 0, n_tet = 0, n_node = 0, n_leaf = 0, depth = 0;
    double Ebar = 0.0;
    std::vector<double> xyz, eps;
    std::vector<int> tri, tet;
    std::vector<NodeRec> nodes;
    std::vector<NodeF> nodesf;
    double cmax = 0.0;                   // max |c|_1 over the nodes (MeshDev.cmax)
    NodeRec *d_nodes = nullptr;
    NodeF *d_nodesf = nullptr;
    TriRec *d_tri = nullptr;
    TetRec *d_tet = nullptr;
    double *d_tet_eps = nullptr;
};

enum { EV_START = 0, EV_SETUP, EV_BP, EV_NP, EV_BR, EV_FIN, EV_COUNT };

// Parts of the Radau handle's two blocks (pfc_context::RadauHost, pfc_radau_configure).  The value buffers (RD_V*, RI_V*) are those of
// pfc_state_derivative_device on the 3 n_scene stage-scenes; the Jacobian chunks run on the first n_scene of them -- before the first
// attempt every stage-scene holds x0 -- and write their value outputs there as well, so only the partials (RD_DD*) have buffers of
// their own.
enum RadauD { RD_X, RD_T, RD_H, RD_ENORM, RD_NSTATE, RD_XS, RD_FS, RD_XDOT0, RD_NEGJ, RD_LU0, RD_LU1, RD_TAU,
              RD_VQ, RD_VV, RD_VS, RD_VXWB, RD_VTW, RD_VJAC, RD_VPOSE, RD_VTWI, RD_VXR2, RD_VWR, RD_VSD, RD_VF, RD_VQD, RD_VH, RD_VC, RD_VVD,
              RD_DDQ, RD_DDV, RD_DDS, RD_DDXWB, RD_DDTW, RD_DDJAC, RD_DDPOSE, RD_DDTWI, RD_DDXR2, RD_DDWR, RD_DDSD, RD_DDF, RD_DDQD, RD_DDH,
              RD_DDC, RD_DDVD, RD_TFINAL, RD_N };
// RI_COUNT has two words: the count a newton or finish part returns, and the scenes live after a batch step (k_radau_finish<true>).
enum RadauI { RI_RULE, RI_COOL, RI_ISTATE, RI_PERM, RI_INFO, RI_COUNT, RI_VINS, RI_VSC, RI_VB1, RI_VB2, RI_VCNT, RI_VINFO, RI_ROWS, RI_N };
// Parts of the controller's two blocks (pfc_radau_set_controller).
enum RadauCD { CD_KP, CD_KD, CD_AMAX, CD_SEGT, CD_SEGQ, CD_SEGFF, CD_TLAST, CD_N };
enum RadauCI { CI_ACT, CI_FIRES, CI_N };
// Parts of the continuous feedback law's two blocks (pfc_radau_set_feedback).
// FD_TAUS: the summed tau the solve reads, 3 n_scene x nv; FD_DDTAU: its partials, n_scene x n_chunk x nv; FD_TSTAGE: the stage
// times, 3 n_scene.
enum RadauFD { FD_KP, FD_KD, FD_AMAX, FD_SEGT, FD_SEGQ, FD_SEGFF, FD_TAUS, FD_DDTAU, FD_TSTAGE, FD_N };
enum RadauFI { FI_ACT, FI_N };
// Parts of the applied body wrenches' two blocks (pfc_radau_set_body_wrenches).
// WD_TAUS: the summed tau the solve reads, 3 n_scene x nv; WD_DDTAU: its partials, n_scene x n_chunk x nv; WD_TSTAGE: the stage
// times, 3 n_scene, used while no law is set (with a law its FD_TSTAGE is).
enum RadauWD { WD_POINT, WD_SEGT, WD_SEGW, WD_TAUS, WD_DDTAU, WD_TSTAGE, WD_N };
enum RadauWI { WI_BODY, WI_FRAME, WI_N };
// Parts of the program's two blocks (pfc_radau_set_program).
enum RadauPD { PD_DT, PD_Q, PD_SLIP, PD_STATE, PD_N };
enum RadauPI { PI_GRIP, PI_CURSOR, PI_N };

}  // namespace

struct pfc_multi;
struct pfc_context {
    int device = 0;
    bool finalized = false;
    pfc_multi *multi = nullptr;          // non-null: a multi-device handle (pfc_create_multi); everything below belongs to its shards
    // The streams come first: members are destroyed in reverse order, so everything made against a stream (events, graph
    // executables, buffers its work may touch) goes before it.
    Stream stream;
    Stream twin_stream;                  // created right behind `stream` (the runtime deals streams out to its hardware queues in order of creation), moved into the twin by make_twin
    PinBuf<char, 2> pin_bp;              // pinned host copy of the last broadphase pose block (pfc_eval_dual_bp)
    int pin_bp_n = 0;                    // items it holds (0: the last host-buffer Dual evaluation had none)
    bool team_owner = false;             // this handle holds its device's team slot (team_acquire)
    int opt_team_fault = -1;             // diagnostic option "team_fault": rank of every team that simulates a timed-out wait
    int opt_dual_fold = 1;               // option "dual_fold": pass B of the Dual evaluation formed inside pass A (tri-tet scenes, batched value pass)
    int opt_fused_f32 = 1;               // option "fused_f32": single-precision SAT filter in the one-launch kernel (A/B knob; same results)
    std::string err;
    std::vector<HostMesh> meshes;
    std::vector<InsDev> ins;
    // The mesh and instruction tables the kernels read: the handle's own (own_* below), or -- a twin -- its parent's, borrowed.
    MeshDev *d_meshes = nullptr;
    InsDev *d_ins = nullptr;
    InsFull *d_insfull = nullptr;        // small scenes: one self-contained record per instruction (pfc_fused.h)
    DevBuf<MeshDev> own_meshes;
    DevBuf<InsDev> own_ins;
    DevBuf<InsFull> own_insfull;
    // every mesh's device records (NodeF, NodeRec, TriRec / TetRec, raw eps) are carved out of ONE allocation, the
    // single-precision nodes of all meshes first (a pile of 128 meshes used to make ~600 small hipMallocs; measured neutral
    // for C5's evaluation time, kept for the contiguous hot set and the one free)
    DevBuf<char> mesh_arena;
    int max_levels = 1;
    int max_leaves = 2;                // largest n_leaf(mesh_1) + n_leaf(mesh_2) over the instructions
    bool any_bristle = false, any_tet_tet = false, any_regularized = false;
    bool all_rule2 = false;              // every instruction has quadrature rule 2 (three points per fan triangle)
    // options
    int opt_debug = 0, opt_profile = 0, opt_max_levels = 0, opt_bfs_levels = -1, opt_no_filter = 0;
    // work buffers
    DevBuf<ItemRec> items;
    DevBuf<WorkRec> frontier[2], cand;
    DevBuf<int> clip_n, icnt, trac_item;
    DevBuf<double> acc, res, trac_d, rec;   // trac_d: 8 arrays of tcap; rec: moment records of kRecStride doubles
    DevBuf<int> ctr;                   // [0]=ccount [1]=tcount [2..] fcount[levels+2]
    DevBuf<unsigned> status;
    DevBuf<unsigned long long> stamps;   // diagnostic builds
    DevBuf<int> tail;                    // packed status, totals, counters (block 0 of k_final)
    PinBuf<int> h_tail;                  // pinned host mirror of tail
    PinBuf<char, 2> pin_in, pin_out;     // pinned staging of the host-buffer path
    // Inputs of a very small scene written by the host straight into DEVICE memory (fine-grained allocation, reachable through
    // the PCIe BAR when the device has a large one): the one-launch kernel's first two dependent reads -- instruction id, then
    // the instruction's record -- start from HBM instead of from host memory (scripts/micro/bar_probe.hip: launch + two
    // dependent reads + completion word 7.5 -> 6.2 us).  Host stores into it are write-combined: written once per evaluation,
    // never read back; they leave the core with the locked update of the queue's write index that every launch begins with.
    DevBuf<char> bar_in;
    DevBuf<char> bar_din;                         // the same for the seeds of a small-scene Dual evaluation (up to kBarKeys (item, direction) pairs)
    int bar_state = 0;                            // 0: not probed, 1: in use, -1: no large BAR / allocation failed / PFC_NO_BAR_INPUTS
    PinBuf<char, 2> pin_din, pin_dout;            // pinned blocks of the small-scene Dual path (partials in / out)
    long long dual_hint = -1;                     // contributing pairs of the last Dual evaluation (-1: none yet)
    int dual_dev_hyb_skip = 0;                    // evaluations for which pfc_eval_dual_device leaves that path alone after a miss
    // The kept pass: the value pass the device lists hold, reused by further Dual evaluations at the same point (the chunks of
    // one Jacobian, src/radau/radau_functions.jl:2-14).  Recorded by pfc_check after pfc_eval_dual_device (Batched: the batched
    // value pass; HandOver: the small-scene kernel's hand-over, pair count in emit_ctr), by eval_dual_hybrid (Hybrid) and by
    // eval_dual_small (OneGraph); ended by every value pass (new_value_pass) and by end_kept_pass.
    struct KeptPass {
        enum Kind { None, Batched, HandOver, Hybrid, OneGraph } kind = None;
        int n = 0;                                // its item count
        bool ids = false;                         // ... given by ins_ids
    } kept;
    bool device_kept() const { return kept.kind == KeptPass::Batched || kept.kind == KeptPass::HandOver; }   // pfc_eval_dual_device_more may follow
    // The pending call: what is enqueued and not checked yet.  Set whole by the site that enqueues (begin), reset whole by drop_pending
    // (an entry point replaces it unchecked) and by the check_* that drain() dispatches to.  A twin keeps one of its own for its half.
    struct Pending {
        enum Kind { None, Batched, Fused, More, Surface } kind = None;   // a batched value pass, a small-scene launch, Dual passes on a kept pass (_more, pfc_local_jacobian_device), a surface call
        hipStream_t stream = nullptr;             // the stream it was enqueued on
        int split_n0 = 0, n_ctr = 0;              // Batched: items in the first half of a split evaluation (0: not split); Surface: its counter count
        // a pfc_eval_dual_device rides on the value pass -- Batched: the batched route, Fused: the small-scene kernel's hand-over -- and
        // pfc_check judges its speculation: directions, speculative polygon capacity, ins_ids given (the kept pass it records)
        enum Dual { NoDual, DualBatched, DualHandOver } dual = NoDual;
        int n_dir = 0; size_t dpcap = 0; bool ids = false;
    } pend;
    // What a pinned input block holds: the value inputs (pose | twist | s, n x 36 doubles; the ids ids_at doubles in) of n items
    // (0: nothing to compare with), of the value pass with that value_serial
    struct HostPoint {
        int n = 0;
        bool ids = false;
        unsigned long long serial = 0;
        size_t ids_at = 0;
    };
    HostPoint pin_in_pt;                          // pin_in: a small-scene Dual evaluation's (a repeat of its point goes to the hybrid path)
    HostPoint pin_din_pt;                         // pin_din / pin_dout: the one-sync path's evaluation (inputs, seeds; outputs)
    bool last_dual_reused = false;                // the last Dual evaluation ran on a reused value pass (pfc_last_dual_reused)
    int opt_dual_reuse = 1;
    unsigned long long value_serial = 0;          // bumped by every value pass that overwrites the device lists (new_value_pass)
    std::vector<int> dual_counts_cache;           // the per-item counters of pin_din_pt's evaluation
    DevBuf<double> dual_zero;                     // zeros standing in for a null d_ds
    unsigned long long epoch = 0;        // bumped whenever a device work buffer is reallocated
    // captured launch sequence (hipGraph) of the last evaluation shape
    GraphExec gexec[2];                  // [0] plain evaluation, [1] with the contributing-pair list (Dual)
    struct GraphKey {
        int n_items, levels, L, debug, bristle, surv;
        const void *p[9];
        void *stream;
        unsigned long long epoch;
    } gkey[2] = {};
    bool ghave[2] = {false, false};
    // value pass + Dual passes of a small scene as ONE graph (eval_dual_small)
    GraphExec dgexec;
    struct DualGraphKey { GraphKey v; int n_dir; size_t bound; const void *din, *dout; } dgkey = {};
    bool dghave = false;
    int opt_graph = 1;
    size_t fcap = 0, ccap = 0, tcap = 0, rcap = 0;
    // host-pointer path staging
    DevBuf<double> h_pose;               // device mirror of pfc_eval's pinned input block (pose | twist | s | ins_ids)
    // last evaluation
    int last_n_items = 0, last_levels = 0, last_bfs_levels = 0;
    long long stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    DevBuf<double> dual_in, dual_acc, dual_res, dual_out, dual_poly;   // pfc_eval_dual
    DevBuf<int2> dual_pkey;
    DevBuf<int> dual_sel, dual_flag;                        // pairs a chunk has work for; per-item marks (+ the list's counter)
    DevBuf<char> stage;                                     // the host-pointer forms' arguments on the device (Stage): every form synchronises before it returns
    DevBuf<double> sdual_w;                                 // pfc_scatter_generalized_dual[_device]: world wrenches
    DevBuf<int> sdual_i;                                    // its device form's CSR keys (+ the sort's second key array), offsets, count
    DevBuf<char> sdual_tmp;                                 // its rocPRIM sort storage
    DevBuf<int> surv;                                       // candidate indices of contributing pairs
    DevBuf<int> rgn;                                        // region counters of the polygon / record lists
    DevBuf<int> poly_item, pcnt, poly_cand;                 // kept polygons (k_narrow -> k_integ, k_fric): keys, count per chunk, candidate index (Dual list)
    DevBuf<double> poly;
    long long last_undecided = 0;      // node pairs the Float32 broadphase settled with the exact Float64 test
    long long last_active = 0;         // items of the last checked evaluation whose root pair overlapped (more than one node test)
    // what the last checked evaluation looked like: a SPARSE pile (at most a quarter of the items in contact: all pairs of a
    // pile of bodies, most of them apart) of mid-sized trees is latency-bound by the descents of its few big pairs, a dense
    // batch by throughput -- the next evaluation of the same shape is laid out accordingly (pile_mode)
    // (the last four shapes: a host that alternates a few batch sizes keeps a picture of each)
    struct ShapeHint { int n = 0; bool sparse = false; } hints[4];
    void note_shape(int n, bool sparse) {
        int k = 0;
        while (k < 3 && hints[k].n != n) ++k;      // the entry of this size, or the oldest
        for (; k > 0; --k) hints[k] = hints[k - 1];
        hints[0].n = n; hints[0].sparse = sparse;
    }
    bool shape_is_sparse(int n) const {
        for (const ShapeHint &e : hints) if (e.n == n) return e.sparse;
        return false;
    }
    long long last_tslots = 0;         // traction slots used by the last evaluation (>= traction points)
    Event ev[EV_COUNT];
    bool ev_valid = false;
    // Large batches are evaluated as two concurrent halves: a second set of work buffers on a second stream, so that
    // the broadphase of one half (vector-ALU bound) shares the CUs with the narrowphase of the other (parked on
    // s_waitcnt half of the time).  Measured on the C3 batch: 2.39 -> 2.04 ms per 2 048 poses; four parts are slower.
    pfc_context *twin = nullptr;
    bool is_twin = false;
    // small scenes: one fused kernel, one workgroup per item (pfc_fused.h)
    DevBuf<int> fout;                  // per item 8 ints (status, counts) of the fused kernel (device-buffer entry point)
    PinBuf<int> h_fout;                // pinned host mirror
    int opt_fused = 1;                 // option "fused"
    // option "fixed_order": the candidate list sorted (pfc_sort.hip), an item's run records added in chunk order (k_integ_fixed,
    // k_shift_fixed), the Dual passes' eigen-decomposition on the value pass's K -- batched path only, no graph, no split
    int opt_fixed_order = 0;
    DevBuf<int> det;                          // per item: last record, first chunk, last chunk
    DevBuf<unsigned long long> sort_keys[2];
    DevBuf<int> canon_off, canon_fill, canon_item;      // segments of the candidate list by item (pfc_canon_candidates)
    int sort_tmp_items = 0;
    bool fixed_whole_list = false;            // an item had more candidates than a segment sort takes: the whole list is sorted from then on
    DevBuf<char> sort_tmp;
    size_t sort_tmp_for = 0;                  // (capacity, bits) the temporary storage was sized for
    int sort_tmp_bits = 0;
    int max_elem1 = 1, max_elem2 = 1;         // most elements of a mesh on side 1 / side 2 of an instruction
    DevBuf<double> fx_rec, vfx_rec;           // records of the Dual passes' sums / of the value pass's friction sums (FixedSink)
    DevBuf<int> vfx_head;
    DevBuf<int> fx_head;                      // per key and accumulator block: last record; then the record counter
    long long surv_sorted_serial = -1;        // value pass whose list of contributing pairs has been sorted
    // Slots of the candidate list the sort covers: its capacity for the first evaluation and whenever the list turned out longer
    // than covered (the evaluation is then re-issued), else a power of two above twice the previous evaluation's candidates -- a
    // reference-sized scene sorts 1 024 keys in one launch instead of 65 536 in fifteen.
    size_t sort_cover = 0;                    // 0: the capacity
    size_t sort_cover_used = 0;               // what the pending evaluation covered
    int opt_vertex_fields = 1;         // option "vertex_fields": k_fric<true> evaluates the fan-point fields per corner; 0: the per-point kernels
    // option "bin_split": k_clip_queue fills a chunk's slot range from both ends by vertex count (n_poly < bin_split from the front,
    // the others from the back: kept_slot, pfc_np.h), so that a 64-polygon piece of k_integ / k_fric holds fans of like length.  Value
    // passes without a Dual list and without fixed_order only, and launches with 512-candidate chunks only (-s: split s at every chunk
    // size, np_bin_split); 0: dense fill everywhere
    int opt_bin_split = 5;             // (5: triangles and quadrilaterals from the front, 85 % of the C3 batch's polygons; 4 measured slower)
    // option "integ_spec": a scenario without a regularized instruction (any_regularized false) integrates its kept polygons in the
    // bristle-only k_integ_br (1, two waves per SIMD) or k_integ_br3 (2, three waves); 0, or any regularized instruction: k_integ
    int opt_integ_spec = 2;
    // option "quad_const": where every instruction has quadrature rule 2 (all_rule2), the bristle-only k_integ forms and the per-corner
    // k_fric run with the rule as a compile-time constant (k_integ_br*_q3, k_fric_q3); 0: the forms that read the item's rule
    int opt_quad_const = 1;
    int opt_clip_queue = 1;            // option "clip_queue": clip-only narrowphase of big tri-tet batches in k_clip_queue (survivors queued in the ring); 0: k_narrow<.., 2 / 3>
    int fused_skip = 0;                // evaluations left for which the fused kernel stays off after an item did not fit
    int fused_seq = 0;                 // sequence number of the last fused launch (completion word of the polled path)
    int last_fu_nw = 0, last_team = 0; // of the last fused launch / of the last checked evaluation (pfc_last_team)
    int n_cu = 0;                      // compute units of the device (a team launch keeps every workgroup resident: one per CU)
    int opt_team = 48;                 // option "team": big pairs (more leaves than one workgroup takes) run as teams of up to this many workgroups (0: batched path; <= kTeamMaxWg = 48: s_team and the gather's per-thread granule count are sized from it).  Eight single C3 poses, mean / worst us (an earlier build that allowed 64): 64: 113 / 122, 48: 112 / 118, 32: 113 / 122, 24: 126 / 190, 16: 178 / 249, batched 132 / 136 (scripts/lat_c3_poses.py)
    DevBuf<unsigned long long> team;   // team partial sums: kTeamMaxBlocks x 3 x 2 kTeamSlots granules, zeroed once (tags are launch sequence numbers >= 1)
    DevBuf<int> emit_ctr;              // pair counter of the fused kernel's hand-over to the batched Dual passes
    PinBuf<int> h_emit;                // pinned mirror
    PinBuf<unsigned> h_more;           // pinned: status word of the Dual passes of pfc_eval_dual_device_more (device word: status.p + 1)
    int dual_fused_skip = 0;           // Dual evaluations left for which the in-kernel Dual passes stay off (an item had too many polygons)
    bool last_fused = false;
    int opt_split_min = 1025;          // 0: never split.  (Paired sweeps at the end of round 2: 1 024 poses -- one seed per resident broadphase workgroup -- 0.80 ms unsplit / 0.90 split; 1 100 0.95 / 0.93, 1 280 1.09 / 1.01, 2 048 1.50 / 1.28.)
    int opt_clip_min = 384;            // items per launch from which the narrowphase runs as clip-only kernel + k_integ; 0: never.  (End of round 3, k_clip_queue for every such launch, scripts/sweep_clip_min.py: full-size C3 poses 256: 405 vs 405 us one-kernel / split, 400: 518 vs 502, 511: 598 vs 568; 400 box-on-plane scenes 120 vs 123 -- 384, was 512.)  (First set at 1 024 from scripts/sweep_clip.sh; a paired sweep with the final kernels: 512 poses 0.61 vs 0.63 ms, 768 0.80 vs 0.83, 1 536 as 2 x 768 1.14 vs 1.19, 1 920 1.33 vs 1.40; 384 poses and below are indifferent.)
    int opt_poison = 0;                // diagnostic: fill (re)allocated work lists with 0xFF bytes (item index -1)
    int last_parts = 1;                // 2 if the last checked evaluation ran as two halves
    Event ev_fork, ev_join, ev_join0;
    int twin_queue_fallback = 0;         // make_twin: 0 the two streams run side by side as created; 1 the twin's stream was re-created with another priority because they did not; 2 they still do not
    // pfc_contact_surface (pfc_surface.h): buffers of its own, so that no captured evaluation graph sees them move
    DevBuf<long long> surf_cnt, surf_off, surf_out;   // per list slot {polygon, points} and their exclusive scan; packed status block
    DevBuf<double> surf_part;                         // per candidate partial sums
    DevBuf<int> surf_seg, surf_canon_off, surf_canon_fill, surf_canon_item;
    // per-item contact Jacobians (pfc_ljac.h)
    DevBuf<double> ljac_seed;          // unit seeds of the three passes for ljac_seed.cap / kLjacSeedDoubles items (k_ljac_seeds)
    DevBuf<double> ljac_out;           // the passes' partials, n_items x 432
    // contact items from body states (pfc_bodies.h)
    std::vector<int> ins_bodies;       // per instruction {body of mesh_1, body of mesh_2} (pfc_set_instruction_bodies); grows with the ids it is given
    DevBuf<int> bodies_bind;           // its device copy, one pair per instruction (kBodiesUnbound where none was given)
    bool bodies_stale = true;          // the device copy is older than ins_bodies: uploaded by the next launch
    // kinematics from joint states (pfc_kin.h)
    KinHost kin;                       // the mechanism's tables as pfc_set_mechanism packed them (kin.n_body = 0: none given)
    DevBuf<char> kin_tab;              // their device copy, one block
    bool kin_stale = true;             // the device copy is older than kin: uploaded by the next kinematics call
    DevBuf<double> kin_sw;             // S_w, n_scene x nv x 6: grows on demand only
    DevBuf<double> kin_dsw;            // dS_w, n_scene x n_dir x nv x 6 (pfc_kinematics_dual): likewise
    DevBuf<unsigned long long> surf_keys[2];
    DevBuf<char> surf_tmp;                            // rocPRIM scan / sort
    PinBuf<long long> h_surf;                         // pinned mirror of surf_out
    bool surf_whole_list = false;       // an item had more candidates than the segment sort takes: the whole list is sorted from then on
    bool surf_cap_short = false;        // the last checked surface call failed only for the caller's capacities
    long long surf_cap_poly = 0, surf_cap_trac = 0;   // capacities of the pending call
    size_t surf_hcap_poly = 0, surf_hcap_trac = 0;    // host-pointer form: its outputs are staged for this many polygons / traction points
    // pfc_contact_surface_fric (pfc_surface_fric.h): per item the moment and friction records of its waves and eig_item's block
    DevBuf<double> sfric_mom, sfric_sum, sfric_res;
    // the Radau IIA step (pfc_radau.h): integrator state and workspace of pfc_radau_configure, carved out of two blocks
    // The blocks' parts are the enums above; RadauHost rounds its parts, the controller and the program pack theirs (PartBlocks).
    struct RadauHost : PartBlocks<RD_N, RI_N, true> {
        bool configured = false, has_state = false, has_tau = false;
        RadauLayout L;
        int n_chunk = 0, k_iter_max = 0, max_rule = 0, cooldown = 0, n_mrp = 0, mrp_off[kRadMaxBr];
        double h0 = 0, tol_newton = 0, fin[4];      // fin = {tol_a, tol_r, h_max, h_min}
        // pfc_radau_set_end: the end times live in dbl (RD_TFINAL) and the row counts in itg (RI_ROWS); the trajectory is a block of
        // its own, n_scene x max_rows x (1 + NX), replaced by the next pfc_radau_set_end and freed by pfc_radau_configure,
        // pfc_radau_set_state and with the handle
        bool has_end = false;
        int max_rows = 0;
        DevBuf<double> traj;
        void drop_end() { has_end = false; max_rows = 0; traj.release(); }
        // pfc_radau_set_controller: law, schedules, t_last (parts RadauCD) and act, the counters (parts RadauCI) in two blocks of
        // their own, replaced by the next pfc_radau_set_controller and freed by its clearing form, pfc_radau_configure and with the
        // handle.  t_last0 stays on the host for pfc_radau_set_state.
        struct Control : PartBlocks<CD_N, CI_N, false> {
            bool on = false, has_ff = false, has_t0 = false;
            int n_act = 0, n_seg = 0;
            double dt = 0;
            std::vector<double> t_last0;
            std::vector<int> act;                 // the actuated coordinates, for pfc_radau_set_program's validation
            // pfc_radau_set_program: the instructions and the records (parts RadauPD) and the grip coordinates and cursors (parts
            // RadauPI) in two blocks of their own, replaced by the next pfc_radau_set_program and freed by pfc_radau_clear_program,
            // with the controller (so by pfc_radau_set_controller and pfc_radau_configure) and with the handle.  seg_q0 and seg_ff0
            // are the controller's segment as pfc_radau_set_controller gave it: the program writes the segment on the device,
            // pfc_radau_clear_program and pfc_radau_set_state put it back.
            struct Program : PartBlocks<PD_N, PI_N, false> {
                bool on = false;
                int n_ins = 0, body = 0, n_grip = 0;
                double tau_soft = 0, tau_hard = 0;
                std::vector<double> seg_q0, seg_ff0;
            } prog;
        } ctl;
        void drop_control() { ctl = Control(); }
        // pfc_radau_set_feedback: the continuous law's tables and its workspace -- the summed tau, its partials, the stage times --
        // (parts RadauFD, RadauFI) in two blocks of their own, replaced by the next pfc_radau_set_feedback and freed by
        // pfc_radau_clear_feedback, pfc_radau_configure and with the handle: a handle without a law allocates what it allocated.
        struct Feedback : PartBlocks<FD_N, FI_N, false> {
            bool on = false, has_ff = false, has_amax = false;
            int n_act = 0, n_seg = 0;
        } fb;
        void drop_feedback() { fb = Feedback(); }
        // pfc_radau_set_body_wrenches: the wrenches' tables and their workspace (parts RadauWD, RadauWI) in two blocks of their
        // own, with the life cycle of the law's: a handle without wrenches allocates what it allocated.
        struct Push : PartBlocks<WD_N, WI_N, false> {
            bool on = false;
            int n_w = 0, n_seg = 0;
        } push;
        void drop_push() { push = Push(); }
    } radau;
};

namespace {

int fail(pfc_context *h, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    return code;
}

#define HIP_TRY(h, expr)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(h, PFC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

int tree_depth(const std::vector<NodeRec> &nodes) {
    // iterative DFS; also validates child indices
    int n = (int)nodes.size(), best = 0;
    std::vector<std::pair<int, int>> st;
    st.push_back({0, 0});
    size_t visited = 0;
    while (!st.empty()) {
        auto [k, d] = st.back();
        st.pop_back();
        if (k < 0 || k >= n || ++visited > (size_t)n) return -1;
        best = d > best ? d : best;
        if (nodes[k].leaf == kInternal) {
            st.push_back({nodes[k].child0, d + 1});
            st.push_back({nodes[k].child1, d + 1});
        }
    }
    return best;
}

int grid_for(size_t n, int block, int max_blocks) {
    size_t b = (n + block - 1) / block;
    if (b < 1) b = 1;
    if (b > (size_t)max_blocks) b = max_blocks;
    return (int)b;
}

// The kept pass (pfc_context::kept) ends: an option change, another broadphase pose, a device entry point, a reallocated pinned block.
void end_kept_pass(pfc_context *h) { h->kept = {}; }
// The pinned blocks no longer hold the value inputs of an evaluation a host Dual call could compare its own with.
void forget_host_points(pfc_context *h) { h->pin_in_pt = {}; h->pin_din_pt = {}; }
// A value pass is about to overwrite the device lists.
void new_value_pass(pfc_context *h) {
    end_kept_pass(h);
    ++h->value_serial;
}

// What one value pass is told beyond its buffers: filled by the entry point that starts the pass and handed down by const
// reference (fused_ok, fused_team, enqueue_eval, record_eval, enqueue_fused); nothing of it outlives the call.
struct PassOpts {
    const double *bp_pose = nullptr;   // broadphase pose (device-visible, n_items x 24, only x_r1_r2 is read), null: the evaluation's own
    bool list = false;                 // the narrowphase also lists the contributing candidates (the Dual passes walk them)
    int *tail = nullptr;               // device-visible block k_final packs the tail into (a small scene: pinned host memory), null: h->tail
    int *fout = nullptr;               // fused kernel: device-visible per-item block (8 ints per item, pinned host memory), null: h->fout
    const int *fout_host = nullptr;    // ... the host's view of it: completion words cleared before the launch, polled by check_fused
    bool emit = false;                 // ... hands item records, counters and the contributing candidates to the batched Dual passes
    int n_dir = 0;                     // ... runs the Dual passes itself: directions (0: none), seeds and partials (device-visible)
    const double *d_pose = nullptr, *d_twist = nullptr; double *d_wrench = nullptr, *d_sdot = nullptr;
    int nw = 1;                        // ... workgroups per item (teams: k_fused<.., true>)
    bool half = false;                 // the launches are one half of a two-half evaluation
};

// ---- sizes and tail layout of the Dual passes (launch_dual), each stated once ----------------------------------------
// Kept Dual polygons for up to `pairs` contributing pairs: a wave of k_narrow_dual takes 64 / n_dir pairs and owns 64 slots
// (option fixed_order: the same bound sizes the record list of the passes' sums, for every model) ...
size_t dual_poly_cap(const pfc_context *h, int n_dir, size_t pairs) { return (h->any_bristle || h->opt_fixed_order) ? ((pairs + 64 / n_dir - 1) / (64 / n_dir)) * 64 + 64 : 64; }
// ... and whether the pairs a checked value pass turned out to have fit the capacity its Dual passes were enqueued with ...
int dual_spec_fit(pfc_context *h, int n_dir, long long pairs, size_t dpcap) {
    h->dual_hint = pairs;
    if (dual_poly_cap(h, n_dir, (size_t)pairs) <= dpcap) return PFC_OK;
    return fail(h, PFC_ERR_OVERFLOW, "Dual evaluation: %lld contributing pairs exceed the speculative polygon capacity: re-issue", pairs);
}
// ... for the small-scene kernel's hand-over (h_emit: its pair count and status, fetched with the check): the list first.
int dual_handover_fit(pfc_context *h, int n_dir, size_t dpcap) {
    if (h->stats[6] & kStCandOvf) return fail(h, PFC_ERR_OVERFLOW, "hand-over list of the small-scene kernel overflowed: re-issue (batched path)");
    if ((unsigned)h->h_emit.p[2] & kStHole) return fail(h, PFC_ERR_STATE, "internal error: a work-list slot was read before it was written");
    return dual_spec_fit(h, n_dir, h->h_emit.p[0], dpcap);
}
// Pair bound of passes enqueued before the count is known: floor x 2^k above twice the previous Dual evaluation's count (hint,
// -1: none yet), so that buffers and captured graphs settle.
size_t dual_spec_bound(long long hint, size_t floor) { while (floor < (size_t)(hint > 0 ? hint : 0) * 2 + 64) floor *= 2; return floor; }
// ... and on a kept pass, whose contributing pairs are known exactly (dual_hint, from the value pass that was checked): no speculation.
size_t dual_exact_bound(const pfc_context *h) { return (size_t)(h->dual_hint > 0 ? h->dual_hint : 0) + 64; }
// ctr[] index of the kept-polygon total (behind the per-level frontier counts; 8-byte aligned pair: the contributing-pair
// counter follows it), that counter's index in the packed tail (12 ints of status and totals, then the counters), and the
// ints in front of the outputs where one block carries the tail and the results (16-byte multiple).
constexpr int ctr_pcount(int levels) { return (levels + 9) & ~1; }
constexpr int tail_pairs(int levels) { return 12 + ctr_pcount(levels) + 1; }
size_t tail_prefix(const pfc_context *h) { return (((size_t)h->max_levels + 40) + 3) & ~(size_t)3; }

// Kept-polygon slots: chunk ch of the candidate list owns slots [ch C, ch C + C) (pfc_np.h, np_chunk): the candidate
// capacity rounded up to a whole chunk.
constexpr int kNpMaxBlocks = 256 * 16;
constexpr int kNpChunkSwitch = 2048;   // a batch is cut into at least this many chunks before the chunks grow beyond a wave round (512: C5 +90 us; 8192: the 2 048-pose step +9 %)
size_t poly_cap(size_t ccap) { return (ccap + kNpChunkBig - 1) / kNpChunkBig * kNpChunkBig; }

// A blocking copy that stays off the legacy stream (hipMemcpy synchronises with it, and the runtime refuses that while ANY
// thread captures a graph: "operation would make the legacy stream depend on a capturing blocking stream" -- a second
// handle being finalized on one host thread while another thread's evaluation records its graph; scripts/soak_threads.py).
hipError_t copy_sync(pfc_context *h, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, h->stream);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(h->stream);
}

size_t fixed_fric_cap(size_t ccap, int n_items) { return 2 * (ccap / 64 + 1) + (size_t)n_items + 64; }      // (FixedSink of k_fric_fixed)

// A work buffer that kernels inside a captured launch sequence are given (the value graphs of enqueue_eval, the one-graph Dual
// path of eval_dual_small): captured graphs bake its address in, so when it moves, the epoch that is part of their keys moves
// on and the next evaluation records its graph again -- whichever path reallocates (the two-stage Dual path, which replays no
// graph itself, sizes the dual_* buffers the one-graph path's kernels were captured with).  A call that reallocates nothing
// leaves the epoch alone: a steady-state evaluation keeps replaying its graph.
template <class T>
hipError_t ensure_graphed(pfc_context *h, DevBuf<T> &b, size_t n, bool *moved = nullptr) {
    bool m = false;
    const hipError_t e = b.ensure(n, &m);
    if (m) ++h->epoch;
    if (moved) *moved = m;
    return e;
}

// ... and one the kernels rely on being zero on entry (they leave it so).  They run on non-blocking streams (the handle's, the
// twin's or the caller's), which are not ordered against the legacy null stream: a new block is cleared on the handle's stream
// and waited for.
template <class T>
hipError_t ensure_zeroed(pfc_context *h, DevBuf<T> &b, size_t n) {
    bool moved = false;
    hipError_t e = ensure_graphed(h, b, n, &moved);
    if (e != hipSuccess || !moved) return e;
    if ((e = hipMemsetAsync(b.p, 0, sizeof(T) * b.cap, h->stream)) != hipSuccess) return e;
    return hipStreamSynchronize(h->stream);
}

hipError_t ensure_work(pfc_context *h, int n_items, bool list) {
    hipError_t e;
    if ((e = ensure_graphed(h, h->items, n_items)) != hipSuccess) return e;
    if ((e = ensure_graphed(h, h->acc, (size_t)n_items * kAccStride)) != hipSuccess) return e;
    if ((e = ensure_graphed(h, h->res, (size_t)n_items * kResStride)) != hipSuccess) return e;
    if ((e = ensure_graphed(h, h->icnt, (size_t)n_items * 4)) != hipSuccess) return e;
    if ((e = ensure_zeroed(h, h->ctr, (size_t)h->max_levels + 12)) != hipSuccess) return e;
    if ((e = ensure_zeroed(h, h->status, 4)) != hipSuccess) return e;
    if ((e = ensure_zeroed(h, h->rgn, (size_t)kRgn * kRgnStride)) != hipSuccess) return e;
    if ((e = ensure_graphed(h, h->stamps, 16)) != hipSuccess) return e;
    size_t f = h->fcap ? h->fcap : 1u << 16;
    while (f < (size_t)n_items * 8) f *= 2;
    size_t c = h->ccap ? h->ccap : 1u << 16;
    while (c < (size_t)n_items * 4) c *= 2;
    size_t t = h->tcap ? h->tcap : 1u << 16;
    size_t rc = h->rcap ? h->rcap : 1u << 12;
    while (rc < c / 32 + (size_t)n_items * 2) rc *= 2;   // about one record per wave round and item boundary
    h->fcap = f; h->ccap = c; h->tcap = t; h->rcap = rc;
    if ((e = ensure_graphed(h, h->rec, rc * (h->opt_fixed_order ? kRecStrideFixed : kRecStride))) != hipSuccess) return e;
    if (h->opt_fixed_order) {
        if ((e = ensure_graphed(h, h->det, (size_t)n_items * 3)) != hipSuccess) return e;
        if ((e = ensure_graphed(h, h->vfx_rec, fixed_fric_cap(c, n_items) * kSinkStride)) != hipSuccess) return e;
        if ((e = ensure_graphed(h, h->vfx_head, (size_t)n_items + 2)) != hipSuccess) return e;
        if ((e = ensure_graphed(h, h->sort_keys[0], c)) != hipSuccess) return e;
        if ((e = ensure_graphed(h, h->sort_keys[1], c)) != hipSuccess) return e;
        int ba, bb;
        const int bits = pfc_sort_key_bits(n_items, h->max_elem1, h->max_elem2, &ba, &bb);
        if ((e = ensure_graphed(h, h->canon_off, (size_t)n_items + 1)) != hipSuccess) return e;
        if ((e = ensure_graphed(h, h->canon_fill, (size_t)n_items)) != hipSuccess) return e;
        if ((e = ensure_graphed(h, h->canon_item, c)) != hipSuccess) return e;
        if (h->sort_tmp_for != c || h->sort_tmp_bits != bits || h->sort_tmp_items < n_items) {
            size_t bytes = 0;
            if ((e = pfc_sort_temp_bytes(c, bits > 64 ? 64 : bits, &bytes)) != hipSuccess) return e;      // (covers the index sort too)
            if ((e = ensure_graphed(h, h->sort_tmp, bytes ? bytes : 1)) != hipSuccess) return e;
            h->sort_tmp_for = c; h->sort_tmp_bits = bits; h->sort_tmp_items = n_items;
        }
    }
    if ((e = ensure_graphed(h, h->frontier[0], f)) != hipSuccess) return e;
    if ((e = ensure_graphed(h, h->frontier[1], f)) != hipSuccess) return e;
    if ((e = ensure_graphed(h, h->cand, c)) != hipSuccess) return e;
    if ((e = ensure_graphed(h, h->clip_n, c)) != hipSuccess) return e;
    if ((e = ensure_graphed(h, h->surv, c)) != hipSuccess) return e;
    {   // kept polygons: bristle items always (friction pass), every item when the clip-only narrowphase + k_integ run
        const size_t pc = poly_cap(c);
        if ((e = ensure_graphed(h, h->poly_item, pc)) != hipSuccess) return e;
        if ((e = ensure_graphed(h, h->poly, pc * 34)) != hipSuccess) return e;
        if ((e = ensure_graphed(h, h->pcnt, pc / kNpBlock + 1)) != hipSuccess) return e;
        if (list && (e = ensure_graphed(h, h->poly_cand, pc)) != hipSuccess) return e;
    }
    if ((e = ensure_graphed(h, h->trac_item, t)) != hipSuccess) return e;
    if ((e = ensure_graphed(h, h->trac_d, t * 8)) != hipSuccess) return e;
    if ((e = ensure_graphed(h, h->tail, (size_t)h->max_levels + 40)) != hipSuccess) return e;
    if ((e = h->h_tail.ensure((size_t)h->max_levels + 40)) != hipSuccess) return e;
    if (h->opt_poison) {    // every evaluation starts from lists full of entries that must never be followed
        if ((e = hipMemsetAsync(h->frontier[0].p, 0xFF, sizeof(WorkRec) * h->frontier[0].cap, h->stream)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(h->frontier[1].p, 0xFF, sizeof(WorkRec) * h->frontier[1].cap, h->stream)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(h->cand.p, 0xFF, sizeof(WorkRec) * h->cand.cap, h->stream)) != hipSuccess) return e;
        if (h->poly_item.p && (e = hipMemsetAsync(h->poly_item.p, 0xFF, sizeof(int) * h->poly_item.cap, h->stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return e;
    }
    return hipSuccess;
}

TracSoA trac_view(pfc_context *h) {
    TracSoA t;
    size_t n = h->tcap;
    double *d = h->trac_d.p;
    t.item = h->trac_item.p;
    t.nx = d; t.ny = d + n; t.nz = d + 2 * n; t.rx = d + 3 * n; t.ry = d + 4 * n; t.rz = d + 5 * n;
    t.dA = d + 6 * n; t.p = d + 7 * n;
    return t;
}

// Option "max_levels" caps the number of broadphase levels the counters / seed expansion are laid out for.  Every buffer
// (ctr, tail, h_tail) is sized from the finalized depth h->max_levels, so the effective value never exceeds it; the
// depth-first kernels' stack reserve always uses h->max_levels (a smaller reserve could overrun the LDS stack).
int eff_levels(const pfc_context *h) {
    return (h->opt_max_levels > 0 && h->opt_max_levels < h->max_levels) ? h->opt_max_levels : h->max_levels;
}

constexpr int kDualSelectMin = 512;       // items from which a Dual evaluation first selects the pairs its seeds touch
constexpr int kBpSmallBlockMin = 3072;   // items per launch from which k_bp_dfs32 runs in 128-thread workgroups (paired A/B: 2 048 per launch 2.31 vs 2.36 ms for 256 / 128 threads, 3 072 per launch 3.39 vs 3.30)

int bfs_levels_for(const pfc_context *h, int n_items, int levels, bool half) {
    int L = 0;
    if (h->opt_bfs_levels >= 0) {
        L = h->opt_bfs_levels;
    } else {
        // Level-synchronous expansion only buys parallelism for the depth-first kernel (one workgroup per seed, ~1 000
        // resident workgroups); each level is a launch (~8 us).  Measured optimum (scripts/latency.py, bench.py):
        // big trees (a traversal is ~1.5 node tests per leaf) want >= 1 024 seeds, or 4 096 when there are only a few
        // items; small trees are done in a few iterations per seed, so 64 seeds suffice (C4: 200 -> 144 us).  A large
        // batch over small trees is usually a sparse-contact pile where a few pairs carry the work: one level spreads them.
        // Round 2 re-sweep for big trees (scripts/sweep_bfs_small.sh, C3 meshes: 1 pose 139 -> 125 us, 4 poses 167 -> 155,
        // 16 poses 215 -> 202, 64 poses 367 -> 309, 200 poses 519 -> 460): the fewer the items, the more seeds pay.
        const bool big = h->max_leaves >= 8192, mid = h->max_leaves >= 1024;
        // (end of round 2, final kernels: from ~600 items a seed level only costs -- 640 poses 0.71 vs 0.74 ms without /
        // with one level, 768 0.73 vs 0.80, 1 023 0.80 vs 0.92; 512 and below are indifferent or gain)
        // (End of round 3, scripts/sweep_bp_blk_levels.py / sweep_bp_split.py: mid-sized trees want ~256 seeds, not 1 024 --
        // 512 poses of a 1 280-leaf pair 185 vs 213 us with 0 / 1 level -- and a batch of >= 1 024 items over small or mid-sized
        // trees no level at all: the level that used to be forced there, tuned on the sparse pile C5 (340 vs 370 us), cost dense
        // batches 20-30 %: 2 000 poses 381 vs 500 us, 2 500 box-on-plane scenes 343 vs 493.  The pile gets its parallelism from
        // 512-thread workgroups instead, pile_mode.)
        // (a half of a two-half evaluation shares the chip with its twin's seeds: 1 100 poses as 2 x 550, 891 vs 930 us
        // without / with the level its own 550 items would ask for)
        const int n_eff = half ? 2 * n_items : n_items;
        const double target = big ? (n_eff >= 600 ? 1.0 : (n_eff >= 256 ? 1024.0 : (n_eff >= 128 ? 2048.0 : (n_eff >= 32 ? 16384.0 : 49152.0))))
                                  : (mid ? 256.0 : 64.0);
        double seeds = (double)n_items;
        while (seeds < target && L < 9) { seeds *= 4.0; ++L; }
    }
    return L > levels ? levels : L;
}

// A sparse pile (see hints): >= 1 024 items over small or mid-sized trees of which at most a quarter were in contact the
// last time this shape was evaluated.  Evaluated in ONE launch sequence with 512-thread broadphase workgroups (C5: 318 us
// against 340 as two halves with 256-thread workgroups and a seed level; without the level 370).
bool pile_mode(const pfc_context *h, int n_items) {
    return h->max_leaves < 8192 && n_items >= 1024 && n_items < kBpSmallBlockMin && h->shape_is_sparse(n_items) && !h->is_twin;
}

// Threads per workgroup of the depth-first broadphase kernel.  128: the halves of a big batch (throughput: the finer grain
// shares the CUs with the other half's kernels).  512: launches whose time is the descent of a few big pairs -- 8 ... 1 023 items
// over big trees (16 full-size C3 poses 198 -> 183 us, 128: 386 -> 314, 256: 459 -> 399, 600: 681 -> 662; from 1 024 items
// on 256 threads win again) and sparse piles: an iteration costs ~1.7 us whatever its width, 512 pairs per iteration halve
// the chain.  (1 024 threads: no further gain, C5 105 vs 97 us of broadphase.)  256 otherwise.
int bp_block_for(const pfc_context *h, int n_items, bool half) {
    if (n_items >= kBpSmallBlockMin) return 128;
    if (half) return 256;
    if (h->max_leaves >= 8192 && n_items >= 8 && n_items < 1024) return 512;
    if (pile_mode(h, n_items)) return 512;
    return 256;
}

// The batched broadphase of an evaluation on stream st, behind k_setup_items: L level-synchronous seed expansions, then the
// depth-first kernel (record_eval; pfc_contact_surface).
void launch_broadphase(pfc_context *h, int n_items, int L, bool half, int *ccount, int *fcount, int *next_seed, int *ucount, hipStream_t st) {
    for (int lv = 0; lv < L; ++lv) {
        BpArgs b;
        b.items = h->items.p; b.fin = h->frontier[lv & 1].p; b.fout = h->frontier[(lv + 1) & 1].p;
        b.cand = h->cand.p; b.fcount = fcount; b.ccount = ccount; b.icnt = h->icnt.p; b.status = h->status.p;
        b.level = lv; b.fcap = (int)h->fcap; b.ccap = (int)h->ccap; b.n_items = n_items;
        // upper bound of this level's frontier: n_items * 4^lv, capped by the buffer
        double ub = (double)n_items * std::pow(4.0, (double)(lv < 15 ? lv : 15));
        size_t bound = ub > (double)h->fcap ? h->fcap : (size_t)ub;
        hipLaunchKernelGGL(k_bp_expand, dim3(grid_for(bound, 256, 2048)), dim3(256), 0, st, b);
    }
    {
        double ub = (double)n_items * std::pow(4.0, (double)(L < 15 ? L : 15));
        size_t bound = ub > (double)h->fcap ? h->fcap : (size_t)ub;
        DfsArgs d;
        d.items = h->items.p; d.cand = h->cand.p; d.ccount = ccount; d.ccap = (int)h->ccap; d.icnt = h->icnt.p;
        d.status = h->status.p; d.reserve = 3 * h->max_levels + 3; d.stamps = h->stamps.p; d.n_items = n_items;
        if (h->opt_no_filter) {
            // Float64-only traversal (A/B checks)
            d.seeds = h->frontier[L & 1].p; d.n_seed = fcount + L; d.seed_cap = (int)h->fcap; d.next_seed = next_seed;
            d.no_filter = 1;
            hipLaunchKernelGGL(k_bp_dfs, dim3(grid_for(bound, 1, 256 * 8)), dim3(64), 0, st, d);
        } else {
            Dfs32Args f;
            f.items = h->items.p; f.seeds = h->frontier[L & 1].p; f.n_seed = fcount + L; f.next_seed = next_seed;
            f.seed_cap = (int)h->fcap; f.cand = h->cand.p; f.ccount = ccount; f.ccap = (int)h->ccap;
            f.ucount = ucount; f.icnt = h->icnt.p; f.status = h->status.p; f.stamps = h->stamps.p;
            f.reserve = 3 * h->max_levels + 3; f.n_items = n_items;
            // Workgroups of 128 threads for the big launches (>= 3 072 items, i.e. the halves of a step of >= 6 144): the
            // kernel alone runs as fast either way (2.08 ms), but next to the other half's narrowphase the finer grain
            // shares the CUs better (8 192-pose step 4.53 -> 4.39 ms; 4 096: 2.33 vs 2.38, 2 048: 1.30 vs 1.45 -- a smaller
            // launch needs the 256 pairs per iteration; profiles/r02_sweep_bp_block.txt).  Grid = resident workgroups.
            const int blk = bp_block_for(h, n_items, half);
            if (blk == 128 && f.reserve <= 128 * 10 - 512)
                hipLaunchKernelGGL((k_bp_dfs32<128>), dim3(grid_for(bound, 1, 256 * 8)), dim3(128), 0, st, f);
            else if (blk == 512)
                hipLaunchKernelGGL((k_bp_dfs32<512>), dim3(grid_for(bound, 1, 256 * 2)), dim3(512), 0, st, f);
            else
                hipLaunchKernelGGL((k_bp_dfs32<kDfsBlock>), dim3(grid_for(bound, 1, 256 * 6)), dim3(kDfsBlock), 0, st, f);
        }
    }
}

// The launch sequence of one evaluation on stream st (eagerly, or while st is being captured into a graph).
int record_eval(pfc_context *h, int n_items, const int *d_ins_ids, const double *d_pose, const double *d_twist,
                const double *d_s, double *d_wrench, double *d_sdot, int *d_counts, hipStream_t st, bool prof, const PassOpts &o) {
    new_value_pass(h);
    h->last_dual_reused = false;
    const int levels = eff_levels(h);
    int *ccount = h->ctr.p, *tcount = h->ctr.p + 1, *next_seed = h->ctr.p + 2;   // ctr[3]: total records, filled by k_final
    int *ucount = h->ctr.p + 4, *fcount = h->ctr.p + 6;
    int *pcount = h->ctr.p + ctr_pcount(levels);
    // counters and status are zero here: k_final of the previous evaluation (or ensure_work after an allocation) left them so
#ifdef PFC_STAMPS
    HIP_TRY(h, hipMemsetAsync(h->stamps.p, 0, sizeof(unsigned long long) * 16, st));
#endif
    if (prof) HIP_TRY(h, hipEventRecord(h->ev[EV_START], st));

    EvalArgs ea;
    ea.n_items = n_items; ea.ins_ids = d_ins_ids; ea.pose = d_pose; ea.twist = d_twist; ea.s = d_s;
    ea.bp_pose = o.bp_pose;
    ea.ins = h->d_ins; ea.meshes = h->d_meshes; ea.n_ins = (int)h->ins.size(); ea.items = h->items.p;
    ea.frontier0 = h->frontier[0].p; ea.fcount = fcount; ea.acc = h->acc.p; ea.icnt = h->icnt.p;
    ea.status = h->status.p;
    hipLaunchKernelGGL(k_setup_items, dim3(grid_for(n_items, 64, 1 << 20)), dim3(64), 0, st, ea);
    if (prof) HIP_TRY(h, hipEventRecord(h->ev[EV_SETUP], st));

    // broadphase: a few level-synchronous expansions to get enough independent seed pairs, then the per-wave
    // depth-first kernel for everything below
    const int L = bfs_levels_for(h, n_items, levels, o.half);
    launch_broadphase(h, n_items, L, o.half, ccount, fcount, next_seed, ucount, st);
    if (o.bp_pose)      // the broadphase ran on a pose of its own: the item records get the evaluation's x_r1_r2 back
        hipLaunchKernelGGL(k_repose, dim3(grid_for(n_items, 64, 1 << 20)), dim3(64), 0, st, n_items, d_pose, h->items.p);
    if (h->opt_fixed_order) {
        int ba, bb;
        const int bits = pfc_sort_key_bits(n_items, h->max_elem1, h->max_elem2, &ba, &bb);
        if (bits > 64)
            return fail(h, PFC_ERR_BAD_ARG, "option fixed_order: (item, element, element) needs %d key bits for %d items, more than 64", bits, n_items);
        size_t cover = h->sort_cover ? h->sort_cover : h->ccap;
        if (cover > h->ccap) cover = h->ccap;
        h->sort_cover_used = cover;
        // by segments (the per-item counts of the broadphase give the offsets; only the segments are sorted), or -- A/B,
        // PFC_FIXED_GLOBAL_SORT=1 -- by one sort of the covered part of the list: the same order either way
        static const bool global_sort = std::getenv("PFC_FIXED_GLOBAL_SORT") != nullptr;
        if (global_sort || h->fixed_whole_list)
            HIP_TRY(h, pfc_sort_candidates(h->cand.p, ccount, cover, h->sort_keys[0].p, h->sort_keys[1].p, h->sort_tmp.p, h->sort_tmp.cap,
                                           n_items, ba, bb, bits, h->status.p, kStFixedCover, st));
        else
            HIP_TRY(h, pfc_canon_candidates(h->cand.p, ccount, cover, h->icnt.p, n_items, h->sort_keys[0].p, h->sort_keys[1].p, h->canon_off.p,
                                            h->canon_fill.p, h->canon_item.p, bb, h->status.p, kStFixedCover, kStFixedBig, st));
        hipLaunchKernelGGL(k_fixed_init, dim3(grid_for(n_items, 256, 1 << 20)), dim3(256), 0, st, n_items, h->det.p);
    }
    if (prof) HIP_TRY(h, hipEventRecord(h->ev[EV_BP], st));

    NpArgs np;
    np.items = h->items.p; np.cand = h->cand.p; np.ccount = ccount; np.ccap = (int)h->ccap; np.acc = h->acc.p;
    np.icnt = h->icnt.p; np.n_items = n_items; np.clip_n = h->opt_debug ? h->clip_n.p : nullptr; np.trac = trac_view(h);
    np.tcount = tcount; np.tcap = (int)h->tcap; np.status = h->status.p; np.debug = h->opt_debug;
    np.stamps = h->stamps.p;
    np.rec = h->rec.p; np.rgn = h->rgn.p; np.rr_cap = (int)(h->rcap / kRgn);
    np.poly_item = h->poly_item.p; np.poly = h->poly.p; np.pcap = (int)poly_cap(h->ccap);
    np.pcnt = h->pcnt.p; np.chunk_switch = kNpChunkSwitch; np.poly_cand = o.list ? h->poly_cand.p : nullptr;
    np.surv = o.list ? h->surv.p : nullptr; np.scount = pcount + 1;
    const int np_grid = grid_for(h->ccap, kNpBlock, kNpMaxBlocks);
    int bin_split = 0;      // binned fill of the kept polygons: k_clip_queue's launches below only (set there)
    np.bin_split = 0;
    // (fixed_order: always the clip-only kernel + k_integ_fixed, whose run records carry every sum)
    const int np_mode = h->opt_debug ? 1 : ((h->opt_fixed_order || (h->opt_clip_min > 0 && n_items >= h->opt_clip_min)) ? 2 : 0);
    if (np_mode == 1) {
        if (h->any_tet_tet) hipLaunchKernelGGL((k_narrow<true, 1>), dim3(np_grid), dim3(kNpBlock), 0, st, np);
        else hipLaunchKernelGGL((k_narrow<false, 1>), dim3(np_grid), dim3(kNpBlock), 0, st, np);
    } else if (np_mode == 0) {
        if (h->any_tet_tet) hipLaunchKernelGGL((k_narrow<true, 0>), dim3(np_grid), dim3(kNpBlock), 0, st, np);
        else hipLaunchKernelGGL((k_narrow<false, 0>), dim3(np_grid), dim3(kNpBlock), 0, st, np);
    } else {
        // a half of a two-half evaluation clips on the compacted ring (MODE 3, 12 KiB of LDS per wave: shares the CUs with the
        // other half's kernels), a launch that has the chip to itself on a column per lane (MODE 2)
        // (and a launch that does not quite fill the chip: 768 poses 0.72 vs 0.74 ms; 512 poses the other way, 0.63 vs 0.62)
        // (end of round 3, with the kernel's earlier gather: every clip-only tri-tet launch -- 900 poses 802 -> 767 us, 1 000:
        // 858 -> 824, 520 ... 800 poses equal within 1 %; scripts/sweep_clip_queue_min.py.  Before: from 1 024 items or as a half.)
        if (h->opt_clip_queue && !h->any_tet_tet) {
            // big tri-tet launches: survivors of the trivial reject queued in the ring, clipped 64 at a time (8 192-pose step
            // 4.17 -> 4.13 ms as two halves, 4.87 -> 4.70 ms unsplit, 2 048 poses 1.288 -> 1.278; 768 poses lose, 0.712 -> 0.721:
            // paired A/B, profiles/r03_ab_clip_queue.txt; option value 2 forces it for every clip-only launch: tests)
            // (k_integ_fixed / k_fric_fixed count on one record per (chunk, item), the Dual list on candidate order: dense fill)
            if (!o.list && !h->opt_fixed_order) bin_split = h->opt_bin_split;
            np.bin_split = bin_split;
            hipLaunchKernelGGL(k_clip_queue, dim3(np_grid), dim3(kNpBlock), 0, st, np);
        } else if (o.half || (n_items >= 640 && n_items < 1024)) {
            if (h->any_tet_tet) hipLaunchKernelGGL((k_narrow<true, 3>), dim3(np_grid), dim3(kNpBlock), 0, st, np);
            else hipLaunchKernelGGL((k_narrow<false, 3>), dim3(np_grid), dim3(kNpBlock), 0, st, np);
        } else {
            if (h->any_tet_tet) hipLaunchKernelGGL((k_narrow<true, 2>), dim3(np_grid), dim3(kNpBlock), 0, st, np);
            else hipLaunchKernelGGL((k_narrow<false, 2>), dim3(np_grid), dim3(kNpBlock), 0, st, np);
        }
        IntegArgs ig;
        ig.items = h->items.p; ig.n_items = n_items; ig.ccount = ccount; ig.ccap = (int)h->ccap; ig.chunk_switch = kNpChunkSwitch;
        ig.pcnt = h->pcnt.p; ig.bin_split = bin_split; ig.poly_item = h->poly_item.p; ig.poly = h->poly.p; ig.pcap = np.pcap;
        ig.poly_cand = np.poly_cand; ig.surv = np.surv; ig.scount = np.scount; ig.acc = h->acc.p; ig.rec = h->rec.p;
        ig.rgn = h->rgn.p; ig.rr_cap = np.rr_cap; ig.icnt = h->icnt.p; ig.status = h->status.p;
        ig.det = h->opt_fixed_order ? h->det.p : nullptr;
        // the bristle-only forms where no instruction of the scenario is regularized (a property of the scenario, as any_tet_tet)
        const int spec = h->any_regularized ? 0 : h->opt_integ_spec;
        const dim3 ig_grid(grid_for(h->ccap, 64, kNpMaxBlocks));
        const bool q3 = h->all_rule2 && h->opt_quad_const;      // (the bristle-only forms only)
        if (h->opt_fixed_order) {
            if (spec == 2) hipLaunchKernelGGL(q3 ? k_integ_br3_q3_fixed : k_integ_br3_fixed, ig_grid, dim3(64), 0, st, ig);
            else if (spec == 1) hipLaunchKernelGGL(q3 ? k_integ_br_q3_fixed : k_integ_br_fixed, ig_grid, dim3(64), 0, st, ig);
            else hipLaunchKernelGGL(k_integ_fixed, ig_grid, dim3(64), 0, st, ig);
        } else if (spec == 2) hipLaunchKernelGGL(q3 ? k_integ_br3_q3 : k_integ_br3, ig_grid, dim3(64), 0, st, ig);
        else if (spec == 1) hipLaunchKernelGGL(q3 ? k_integ_br_q3 : k_integ_br, ig_grid, dim3(64), 0, st, ig);
        else hipLaunchKernelGGL(k_integ, ig_grid, dim3(64), 0, st, ig);
    }
    if (prof) HIP_TRY(h, hipEventRecord(h->ev[EV_NP], st));

    BrArgs br;
    br.items = h->items.p; br.n_items = n_items; br.acc = h->acc.p; br.res = h->res.p; br.icnt = h->icnt.p;
    br.trac = trac_view(h); br.tcount = tcount; br.tcap = (int)h->tcap; br.wrench = d_wrench; br.sdot = d_sdot;
    br.counts = d_counts;
    br.ctr = h->ctr.p; br.n_ctr = levels + 12; br.status = h->status.p; br.tail = o.tail ? o.tail : h->tail.p;
    br.rgn = h->rgn.p; br.i_pcount = ctr_pcount(levels);
    if (h->opt_fixed_order && np_mode == 2) {
        FixedArgs fx;
        fx.rec = h->rec.p; fx.det = h->det.p; fx.n_items = n_items; fx.n_slots = (int)(h->rcap / kRgn) * kRgn; fx.items = h->items.p;
        fx.acc = h->acc.p; fx.status = h->status.p;
        hipLaunchKernelGGL(k_shift_fixed, dim3(n_items), dim3(64), 0, st, fx);      // one wave per item
    }
    if (h->any_bristle) {
        ShiftArgs sh;
        sh.rec = h->rec.p; sh.rgn = h->rgn.p; sh.rr_cap = (int)(h->rcap / kRgn); sh.acc = h->acc.p;
        if (!(h->opt_fixed_order && np_mode == 2)) hipLaunchKernelGGL(k_shift, dim3(grid_for(h->rcap, 64, 2048)), dim3(64), 0, st, sh);
        hipLaunchKernelGGL(k_eig, dim3(n_items), dim3(64), 0, st, br);   // one wave per item
        FricArgs fr;
        fr.items = h->items.p; fr.poly_item = h->poly_item.p; fr.poly = h->poly.p; fr.ccount = ccount; fr.ccap = (int)h->ccap;
        fr.chunk_switch = kNpChunkSwitch; fr.pcnt = h->pcnt.p; fr.bin_split = bin_split;
        fr.pcap = np.pcap; fr.res = h->res.p; fr.acc = h->acc.p;
        fr.n_items = n_items; fr.status = h->status.p;
        fr.sink = FixedSink{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, nullptr};
        if (h->opt_fixed_order && np_mode == 2) {
            // records of the friction sums: two direct slots per 64-polygon piece (a piece of a batch holds one item, two at a boundary),
            // an overflow area for the pieces of piles that hold more -- at most one further record per item
            const size_t n_pos = h->ccap / 64 + 1, cap = fixed_fric_cap(h->ccap, n_items);      // (allocated by ensure_work)
            HIP_TRY(h, hipMemsetAsync(h->vfx_head.p, 0xFF, sizeof(int) * (size_t)n_items, st));
            HIP_TRY(h, hipMemsetAsync(h->vfx_head.p + n_items, 0, sizeof(int) * 2, st));
            fr.sink = FixedSink{h->vfx_rec.p, h->vfx_head.p + n_items, h->vfx_head.p, 0, 2, (int)n_pos, (int)(2 * n_pos), (int)cap, h->status.p};
        }
        // "debug" keeps the per-point kernel: the friction sums are then formed at exactly the traction points the debug views hand out
        const bool vertex_fields = h->opt_vertex_fields && !h->opt_debug;
        // (grid cap 256 x 32, twice the other narrowphase kernels': paired A/B 4.32 -> 4.22 ms per 8 192-pose step; x 64 and x 128 alike)
        const bool fric_q3 = vertex_fields && h->all_rule2 && h->opt_quad_const;      // the rule as a constant (option "quad_const")
        if (fr.sink.rec) {
            if (fric_q3) hipLaunchKernelGGL(k_fric_q3_fixed, dim3(grid_for(h->ccap, 64, 256 * 32)), dim3(64), 0, st, fr);
            else if (vertex_fields) hipLaunchKernelGGL(k_fric_fixed<true>, dim3(grid_for(h->ccap, 64, 256 * 32)), dim3(64), 0, st, fr);
            else hipLaunchKernelGGL(k_fric_fixed<false>, dim3(grid_for(h->ccap, 64, 256 * 32)), dim3(64), 0, st, fr);
            hipLaunchKernelGGL(k_fixed_reduce, dim3(n_items), dim3(64), 0, st, fr.sink, n_items, h->acc.p, kAccStride, kAccFric, 6);
        } else if (fric_q3) hipLaunchKernelGGL(k_fric_q3, dim3(grid_for(h->ccap, 64, 256 * 32)), dim3(64), 0, st, fr);
        else if (vertex_fields) hipLaunchKernelGGL(k_fric<true>, dim3(grid_for(h->ccap, 64, 256 * 32)), dim3(64), 0, st, fr);
        else hipLaunchKernelGGL(k_fric<false>, dim3(grid_for(h->ccap, 64, 256 * 32)), dim3(64), 0, st, fr);
    }
    if (prof) HIP_TRY(h, hipEventRecord(h->ev[EV_BR], st));
    hipLaunchKernelGGL(k_final, dim3(grid_for(n_items, 128, 1 << 20)), dim3(128), 0, st, br);
    if (prof) HIP_TRY(h, hipEventRecord(h->ev[EV_FIN], st));
    HIP_TRY(h, hipGetLastError());
    return PFC_OK;
}

// Enqueue one evaluation.  All pointers are device pointers.  The fixed launch sequence (2 memsets + 8..20 small
// kernels) is captured into a hipGraph the first time a shape is seen and replayed afterwards: for the reference's
// own scene sizes (a handful of instructions per calcXd!) launch overhead, not kernel time, is what an evaluation
// costs.  Profiling (HIP events between stages) uses the eager path.
int enqueue_eval(pfc_context *h, int n_items, const int *d_ins_ids, const double *d_pose, const double *d_twist,
                 const double *d_s, double *d_wrench, double *d_sdot, int *d_counts, hipStream_t st, const PassOpts &o) {
    new_value_pass(h);
    h->last_dual_reused = false;
    HIP_TRY(h, ensure_work(h, n_items, o.list));
    const int levels = eff_levels(h);
    const bool prof = h->opt_profile != 0;
    if (prof && !h->ev[0])
        for (int k = 0; k < EV_COUNT; ++k) HIP_TRY(h, hipEventCreate(h->ev[k].put()));
    const int L = bfs_levels_for(h, n_items, levels, o.half);
    bool use_graph = h->opt_graph && !prof;
#ifdef PFC_STAMPS
    use_graph = false;
#endif
    if (use_graph) {
        pfc_context::GraphKey key = {};
        key.n_items = n_items; key.levels = levels; key.L = L; key.debug = (h->opt_debug ? 1 : 0) | (o.half ? 2 : 0) | (bp_block_for(h, n_items, o.half) << 4);
        if (h->opt_fixed_order) {      // (the sort's launches depend on the slots it covers: 2^k, k in the key)
            size_t cover = h->sort_cover ? h->sort_cover : h->ccap;
            int lg = 0;
            while (((size_t)1 << lg) < cover && lg < 40) ++lg;
            key.debug |= ((lg + 1) << 16) | (h->fixed_whole_list ? 1 << 24 : 0);
        }
        key.bristle = (h->any_bristle ? 1 : 0) | (h->any_tet_tet ? 2 : 0) | (h->any_regularized ? 4 : 0) | (h->all_rule2 ? 8 : 0);
        key.surv = o.list ? 1 : 0;
        key.p[0] = d_ins_ids; key.p[1] = d_pose; key.p[2] = d_twist; key.p[3] = d_s; key.p[4] = d_wrench;
        key.p[5] = d_sdot; key.p[6] = d_counts; key.p[7] = o.tail; key.p[8] = o.bp_pose; key.stream = (void *)st; key.epoch = h->epoch;
        const int gi = key.surv;   // Radau alternates value and Dual evaluations: both graphs stay instantiated
        if (!h->ghave[gi] || std::memcmp(&key, &h->gkey[gi], sizeof key) != 0) {
            h->gexec[gi].reset();
            h->ghave[gi] = false;
            hipGraph_t graph = nullptr;
            HIP_TRY(h, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            int rc = record_eval(h, n_items, d_ins_ids, d_pose, d_twist, d_s, d_wrench, d_sdot, d_counts, st, false, o);
            hipError_t e = hipStreamEndCapture(st, &graph);
            if (rc != PFC_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
            if (e != hipSuccess) return fail(h, PFC_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
            e = hipGraphInstantiate(h->gexec[gi].put(), graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (e != hipSuccess) return fail(h, PFC_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
            h->gkey[gi] = key; h->ghave[gi] = true;
        }
        HIP_TRY(h, hipGraphLaunch(h->gexec[gi], st));
    } else {
        int rc = record_eval(h, n_items, d_ins_ids, d_pose, d_twist, d_s, d_wrench, d_sdot, d_counts, st, prof, o);
        if (rc != PFC_OK) return rc;
    }
    h->last_bfs_levels = L;
    h->last_n_items = n_items; h->last_levels = levels; h->pend = {pfc_context::Pending::Batched, st};
    h->ev_valid = prof;
    return PFC_OK;
}

// Synchronise, read counters, grow on overflow.
int check_one(pfc_context *h, const int *tail) {
    const hipStream_t st = std::exchange(h->pend, {}).stream;      // (always a Batched record: this handle's, or the twin's for its half)
    const int levels = h->last_levels;
    const size_t n_tail = (size_t)levels + 12 + 12;
    if (!tail) {
        HIP_TRY(h, hipMemcpyAsync(h->h_tail.p, h->tail.p, sizeof(int) * n_tail, hipMemcpyDeviceToHost, st));
        tail = h->h_tail.p;
    }
    HIP_TRY(h, hipStreamSynchronize(st));
    const unsigned status = (unsigned)tail[0];
    const unsigned long long *tot = reinterpret_cast<const unsigned long long *>(tail + 4);
    const int *ctr = tail + 12;
    long long fpeak = 0;
    int used_levels = 0;
    for (int lv = 0; lv <= h->last_bfs_levels && lv <= levels; ++lv) {
        if (ctr[6 + lv] > fpeak) fpeak = ctr[6 + lv];
        if (ctr[6 + lv] > 0) used_levels = lv + 1;
    }
    h->stats[1] = ctr[0]; h->last_tslots = ctr[1]; h->stats[4] = used_levels; h->stats[5] = fpeak;
    h->stats[6] = status; h->stats[7] = h->last_n_items;
    if (status & kStBadIns) return fail(h, PFC_ERR_BAD_ARG, "instruction id out of range in ins_ids");
    h->last_undecided = ctr[4];
    // before the overflow branch: also the narrowphase of an overflowing (to be re-issued) evaluation must only see
    // slots that were written
    if (status & kStHole) return fail(h, PFC_ERR_STATE, "internal error: a work-list slot was read before it was written");
    if (status & (kStFrontierOvf | kStCandOvf | kStTracOvf | kStRecOvf)) {
        // VectorCache-style growth (src/obb/vector_cache.jl:13-17): at least double, at least the observed need
        if (status & kStFrontierOvf) { size_t f = h->fcap * 2; while (f < (size_t)fpeak) f *= 2; h->fcap = f; }
        if (status & kStCandOvf) { size_t c = h->ccap * 2; while (c < (size_t)ctr[0]) c *= 2; h->ccap = c; }
        if (status & kStTracOvf) { size_t t = h->tcap * 2; while (t < (size_t)ctr[1]) t *= 2; h->tcap = t; }
        if (status & kStRecOvf) { size_t r = h->rcap * 2; while (r < (size_t)ctr[3]) r *= 2; h->rcap = r; }
        // the lists are indexed by 32-bit integers (counters, slots): an evaluation that needs more is split by the caller
        if (h->fcap > ((size_t)1 << 30) || h->ccap > ((size_t)1 << 30) || h->tcap > ((size_t)1 << 30) || h->rcap > ((size_t)1 << 30))
            return fail(h, PFC_ERR_NOMEM, "work lists beyond 2^30 entries (frontier %zu, candidates %zu, tractions %zu, records %zu): evaluate the batch in parts",
                        h->fcap, h->ccap, h->tcap, h->rcap);
        return fail(h, PFC_ERR_OVERFLOW, "work list overflow (status %u): capacities grown to frontier %zu, candidates %zu, tractions %zu, records %zu",
                    status, h->fcap, h->ccap, h->tcap, h->rcap);
    }
    if (status & kStAbort) return fail(h, PFC_ERR_STATE, "broadphase aborted: iteration guard hit (corrupt tree?)");
    if (status & kStPolyOvf) return fail(h, PFC_ERR_STATE, "internal error: a kept-polygon region overflowed");
    if (h->opt_fixed_order) {
        if (status & kStFixedBig) {      // an item with more candidates than the segment sort takes: sort the whole list, evaluate again
            h->fixed_whole_list = true;
            h->ghave[0] = h->ghave[1] = false;
            return fail(h, PFC_ERR_OVERFLOW, "option fixed_order: an item has more than 4096 candidates: the whole list is sorted from now on, re-issue");
        }
        if (status & kStFixedCover) {      // more candidates than the sort covered: cover the whole list and evaluate again
            h->sort_cover = 0;
            h->ghave[0] = h->ghave[1] = false;
            return fail(h, PFC_ERR_OVERFLOW, "option fixed_order: the candidate list outgrew the part the sort covered (%zu slots): re-issue", h->sort_cover_used);
        }
        size_t want = 1024;
        while (want < 2 * (size_t)ctr[0] + 1024) want *= 2;
        if (want >= h->ccap) want = 0;
        if (want != h->sort_cover && (want == 0 || h->sort_cover == 0 || want > h->sort_cover || 4 * want <= h->sort_cover)) h->sort_cover = want;
    }
    if (status & (kStFixedSpan | kStFixedList))
        return fail(h, PFC_ERR_STATE, "option fixed_order: the candidates of one item span more than %d chunks of 512, or one key has more than %d sum records (status %u): evaluate it without the option",
                    kFixedSpan, kSinkSpan, status);

    if (status & kStNonFinite) return fail(h, PFC_ERR_NONFINITE, "Non-finite vertex likely");
    h->stats[0] = (long long)tot[0]; h->stats[2] = (long long)tot[1]; h->stats[3] = (long long)tot[2];
    h->last_active = (long long)tot[3];
    return PFC_OK;
}

// Synchronise the pending evaluation (both halves of a split one) and merge the counters.
// (tail, fout: the pinned blocks the packed tail / the fused kernel's per-item words are on their way to with the outputs, or
// were written to by the kernels; null: fetched into the handle's own mirrors h_tail / h_fout here)
int check_fused(pfc_context *h, const int *fout);
void team_release(pfc_context *h);
int check_eval(pfc_context *h, const int *tail = nullptr, const int *fout = nullptr) {
    if (h->pend.kind == pfc_context::Pending::Fused) return check_fused(h, fout);
    h->last_fused = false;
    team_release(h);
    if (!h->pend.split_n0) {
        h->last_parts = 1;
        const int rc0 = check_one(h, tail);
        if (rc0 == PFC_OK) h->note_shape(h->last_n_items, h->last_active * 4 <= (long long)h->last_n_items);
        return rc0;
    }
    h->last_parts = 2;
    pfc_context *t = h->twin;
    const int rc1 = check_one(h, tail), rc2 = check_one(t, nullptr);   // both always run: each grows its own work lists on overflow (the second half reads its own h_tail)
    if (rc1 != PFC_OK) return rc1;
    if (rc2 != PFC_OK) { h->err = t->err; return rc2; }
    for (int k = 0; k < 4; ++k) h->stats[k] += t->stats[k];
    if (t->stats[4] > h->stats[4]) h->stats[4] = t->stats[4];
    if (t->stats[5] > h->stats[5]) h->stats[5] = t->stats[5];
    h->stats[6] |= t->stats[6];
    h->stats[7] += t->stats[7];
    h->last_undecided += t->last_undecided;
    h->note_shape((int)h->stats[7], (h->last_active + t->last_active) * 4 <= h->stats[7]);
    return PFC_OK;
}

// ---- fused small-scene path (pfc_fused.h) -------------------------------------------------------------------------
constexpr int kFusedMaxItems = 256;      // one workgroup (one CU) per item
constexpr int kFusedMaxLeaves = 6144;    // n_leaf(mesh_1) + n_leaf(mesh_2): above this one workgroup's descent is the slower one

// Teams of workgroups wait for each other inside a launch, so two team launches that are each only PARTLY resident can keep
// each other's missing workgroups off the chip until the bounded spin (~65 ms, kTeamSpinMax) gives up.  Within one process
// that cannot happen any more: a device has ONE team slot, held by the handle whose team evaluation is in flight (from the
// enqueue to the check); a handle that finds the slot taken evaluates without a team at once (one workgroup per item, or the
// batched path).  Kernels that do not wait for anybody (every other kernel of the library) only delay a team, they finish.
// Across processes the bounded spin stays the safety net.
std::atomic<pfc_context *> g_team_slot[64];
bool team_acquire(pfc_context *h) {
    if (h->team_owner) return true;
    pfc_context *expect = nullptr;
    if (!g_team_slot[h->device & 63].compare_exchange_strong(expect, h)) return false;
    h->team_owner = true;
    return true;
}
void team_release(pfc_context *h) {
    if (!h->team_owner) return;
    h->team_owner = false;
    g_team_slot[h->device & 63].store(nullptr);
}
// The unchecked call, if any, is replaced or given up: nothing is pending any more, neither the twin's half nor the team slot a
// small-scene launch held.  Every entry point that starts another call, the zero-item evaluations, a failed multi-device fan-out.
void drop_pending(pfc_context *h) {
    if (h->pend.split_n0) h->twin->pend = {};
    h->pend = {};
    team_release(h);
}

bool fused_ok(const pfc_context *h, int n_items, const PassOpts &o) {
    return h->opt_fused && !h->opt_fixed_order && h->fused_skip == 0 && !h->opt_debug && !h->opt_profile && !o.list &&
           !h->is_twin && h->d_insfull && n_items <= kFusedMaxItems && h->max_leaves <= kFusedMaxLeaves;
}
// Team size for an evaluation of a few BIG pairs (more leaves than one workgroup takes: BASELINE config 3 as written is one
// 9 680-tet x 5 120-triangle pair): as many workgroups per item as keep every workgroup of the launch resident (one per CU),
// at most kTeamMaxWg; 0: not a team evaluation.
// Small scenes (fused_ok): 1 -- unless the items are few and mid-sized (a 972-tet box on the ground keeps ONE CU busy for
// 52 us, a third of it dealing 1 100 fan triangles out to 256 threads): then a small team, one workgroup per 128 leaves of
// the pair, at most 32 (C2 64 -> 48 us, four reduced C3 poses 106 -> 81 us; a team of 2 loses to its own team sum).
int fused_team(const pfc_context *h, int n_items, const PassOpts &o) {
    const int blocks = h->n_cu < kTeamMaxBlocks ? h->n_cu : kTeamMaxBlocks;      // (a partitioned device has fewer CUs)
    if (fused_ok(h, n_items, o)) {
        // (end of round 3, scripts/variants/team_cap_run.py: a workgroup per 128 leaves, at most 32 -- a 4 880-leaf pair alone
        // 94 -> 82 us, four of them 132 -> 86, sixteen 148 -> 94; 2 000-leaf pairs 84 -> 79 (x 4), 88 -> 80 (x 16); C2 unchanged)
        int nw = (h->max_leaves + 64) / 128;
        if (nw > 32) nw = 32;
        if (n_items >= 1 && nw > blocks / n_items) nw = blocks / n_items;
        if (nw > h->opt_team) nw = h->opt_team;
        return nw >= 4 ? nw : 1;
    }
    if (!(h->opt_fused && !h->opt_fixed_order && h->opt_team && h->fused_skip == 0 && !h->opt_debug && !h->opt_profile && !o.list && !h->is_twin &&
          h->d_insfull && h->max_leaves > kFusedMaxLeaves && n_items >= 1 && n_items <= kFusedMaxItems))
        return 0;
    int nw = blocks / n_items;
    if (nw > kTeamMaxWg) nw = kTeamMaxWg;
    if (nw > h->opt_team) nw = h->opt_team;
    // A team pays while each of its workgroups has at most ~1 200 leaves of the pair to descend; beyond that the batched path with
    // its 512-thread broadphase workgroups is faster (scripts/team_vs_batched.py, team_rule_sweep.py, profiles/r03_team_rules.txt;
    // full-size C3 poses, 14 800 leaves: 8 in teams of 32 109 us against 172 batched, 16 in teams of 16 166 against 200, 20 in
    // teams of 12 203 against 212, but 24 in teams of 10 283 against 230; a 10 400-leaf pair: 24 in teams of 10 136 against 210;
    // a 7 380-leaf pair: 32 in teams of 8 137 against 188).  Until the end of round 3 the rule was "teams of at least 4", which
    // ran 64 full-size poses in teams of 4: 488 us against 289.
    return (nw >= 4 && h->max_leaves <= 1200 * nw) ? nw : 0;
}

int enqueue_fused(pfc_context *h, int n_items, const int *d_ins_ids, const double *d_pose, const double *d_twist,
                  const double *d_s, double *d_wrench, double *d_sdot, int *d_counts, hipStream_t st, const PassOpts &o) {
    new_value_pass(h);
    h->last_dual_reused = false;
    FuArgs a;
    a.n_items = n_items; a.n_ins = (int)h->ins.size(); a.ins_ids = d_ins_ids; a.pose = d_pose; a.twist = d_twist; a.s = d_s;
    a.ins = h->d_insfull; a.wrench = d_wrench; a.sdot = d_sdot; a.counts = d_counts;
    if (!o.fout) {
        HIP_TRY(h, h->fout.ensure((size_t)kFusedMaxItems * 8));
        HIP_TRY(h, h->h_fout.ensure((size_t)kFusedMaxItems * 8));
    }
    a.fout = o.fout ? o.fout : h->fout.p;
    if (++h->fused_seq == 0) h->fused_seq = 1;
    a.seq = h->fused_seq;
    if (o.fout_host) {
        // polled path: the completion words live in pinned host memory that several block layouts share (offsets depend on
        // n_items and the number of levels), so a stale small integer of an earlier layout could equal this launch's
        // sequence number -- clear this launch's n words before the kernel can write them (<= 256 host stores)
        volatile int *vf = const_cast<volatile int *>(o.fout_host);
        for (int i = 0; i < n_items; ++i) vf[8 * i + 5] = 0;
        std::atomic_thread_fence(std::memory_order_release);
    }
    a.n_dir = o.n_dir; a.d_pose = o.d_pose; a.d_twist = o.d_twist; a.d_wrench = o.d_wrench; a.d_sdot = o.d_sdot;
    a.emit_items = nullptr; a.emit_cand = nullptr; a.emit_surv = nullptr; a.emit_icnt = nullptr; a.emit_ctr = nullptr; a.emit_cap = 0;
    if (o.emit) {
        a.emit_items = h->items.p; a.emit_cand = h->cand.p; a.emit_surv = h->surv.p; a.emit_icnt = h->icnt.p;
        a.emit_ctr = h->emit_ctr.p; a.emit_cap = (int)h->ccap;
    }
    a.stamps = nullptr;
#ifdef PFC_STAMPS
    HIP_TRY(h, h->stamps.ensure(16));
    a.stamps = h->stamps.p;
#endif
    a.bp_pose = o.bp_pose; a.team_fault = h->opt_team_fault; a.f32 = h->opt_fused_f32;
    a.nw = o.nw; a.team = nullptr;
    a.team_seeds = h->max_leaves > kFusedMaxLeaves ? kTeamSeedsBig : kTeamSeeds;
    h->last_fu_nw = a.nw;
    if (a.nw > 1) {
        if (!h->team.p) {
            HIP_TRY(h, h->team.ensure((size_t)kTeamMaxBlocks * 3 * 2 * kTeamSlots));
            HIP_TRY(h, hipMemsetAsync(h->team.p, 0, sizeof(unsigned long long) * h->team.cap, st));
        }
        a.team = h->team.p;
        if (h->any_tet_tet) hipLaunchKernelGGL((k_fused<true, true>), dim3(n_items * a.nw), dim3(kFuBlock), 0, st, a);
        else hipLaunchKernelGGL((k_fused<false, true>), dim3(n_items * a.nw), dim3(kFuBlock), 0, st, a);
    } else
    // a direct launch: cheaper than a graph replay
    if (h->any_tet_tet) hipLaunchKernelGGL((k_fused<true>), dim3(n_items), dim3(kFuBlock), 0, st, a);
    else hipLaunchKernelGGL((k_fused<false>), dim3(n_items), dim3(kFuBlock), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    h->last_n_items = n_items; h->pend = {pfc_context::Pending::Fused, st}; h->ev_valid = false;
    h->last_bfs_levels = 0;
    return PFC_OK;
}

int check_fused(pfc_context *h, const int *fo) {
    const int n = h->last_n_items;
    if (!fo) {
        HIP_TRY(h, hipMemcpyAsync(h->h_fout.p, h->fout.p, sizeof(int) * 8 * (size_t)n, hipMemcpyDeviceToHost, h->pend.stream));
        fo = h->h_fout.p;
        HIP_TRY(h, hipStreamSynchronize(h->pend.stream));
    } else {
        // The kernel wrote its results straight into pinned host memory; every workgroup ends with a system-scope
        // release and its completion word.  Polling those words returns ~3 us earlier than hipStreamSynchronize wakes
        // up; after 200 us without completion (a long evaluation, a stalled queue) the stream is synchronised instead.
        // (By the clock: the 200 000 spins this used to be lasted as long as the loop's code made them, ~85 us of one item's word, and a
        // single full-size C3 pose was polled or synchronised depending on how the loop compiled: 82.5 against 88.0 us, profiles/pass_opts_ab.json.)
        const volatile int *vf = fo;
        const int seq = h->fused_seq;
        bool done = false;
        static const bool no_poll = std::getenv("PFC_FUSED_SYNC") != nullptr;     // A/B knob: synchronise instead of polling
        const auto give_up = std::chrono::steady_clock::now() + std::chrono::microseconds(200);
        for (int spin = 0; !done && !no_poll; ++spin) {
            if ((spin & 63) == 63 && std::chrono::steady_clock::now() > give_up) break;
            done = true;
            for (int i = n - 1; i >= 0; --i)
                if (vf[8 * i + 5] != seq) { done = false; break; }
        }
        if (done) std::atomic_thread_fence(std::memory_order_acquire);
        else {
            if (std::getenv("PFC_LOG_POLL")) std::fprintf(stderr, "pfc: completion poll timed out, synchronising\n");
            HIP_TRY(h, hipStreamSynchronize(h->pend.stream));
        }
    }
    h->pend = {}; h->last_parts = 1; h->last_fused = true;
    team_release(h);
    unsigned status = 0;
    long long tot[4] = {0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
        status |= (unsigned)fo[8 * i];
        for (int k = 0; k < 4; ++k) tot[k] += fo[8 * i + 1 + k];
    }
    for (int k = 0; k < 4; ++k) h->stats[k] = tot[k];
    h->stats[4] = 0; h->stats[5] = 0; h->stats[6] = status; h->stats[7] = n;
    h->last_undecided = 0; h->last_tslots = 0;
    if (status & kStBadIns) return fail(h, PFC_ERR_BAD_ARG, "instruction id out of range in ins_ids");
    if (status & kStNonFinite) return fail(h, PFC_ERR_NONFINITE, "Non-finite vertex likely");
    if (status & kStAbort) return fail(h, PFC_ERR_STATE, "broadphase aborted: iteration guard hit (corrupt tree?)");
    if (status & kStFusedOvf) {
        h->fused_skip = 64;     // the batched path takes over (and the re-issue), the fused kernel is tried again later
        return fail(h, PFC_ERR_OVERFLOW, "an item has more candidate pairs than the small-scene kernel holds: re-issue (batched path)");
    }
    if (status & kStFusedDualSkip) {
        h->dual_fused_skip = 64;
        return fail(h, PFC_ERR_OVERFLOW, "an item has more (polygon, direction) pairs than the small-scene kernel's Dual passes hold: re-issue (batched Dual path)");
    }
    return PFC_OK;
}

// Do two streams run side by side?  The halves of a big evaluation only overlap if their streams sit on different hardware
// queues of the runtime, which deals its few queues (four by default) out to streams by its own bookkeeping: with an RCCL
// communicator initialised before pfc_create and no collective issued yet -- bench.py under torch.distributed.run, i.e. every
// multi-GPU run -- both streams of a handle came to sit on ONE queue and the 8 192-pose step took 4.85 instead of 3.89 ms
// (scripts/rccl_queue_probe.py; the kernel trace shows one queue).  Creation order, first-use order: neither is a guarantee.
// So the pair is TESTED once per handle: a one-wave kernel on each stream spins for ~60 us and stamps its start and end with
// the constant-rate clock; on different queues the second starts while the first still spins.
__global__ void k_queue_probe(unsigned long long ticks, unsigned long long *out) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
    if (threadIdx.x == 0) { out[0] = t0; out[1] = wall_clock64(); }
}
bool streams_overlap(pfc_context *h, hipStream_t a, hipStream_t b) {
    if (h->stamps.ensure(16) != hipSuccess) return true;      // cannot test: assume the best
    unsigned long long *d = h->stamps.p;
    unsigned long long v[4] = {0, 0, 0, 0};
    if (hipMemsetAsync(d, 0, sizeof v, a) != hipSuccess || hipStreamSynchronize(a) != hipSuccess) return true;
    hipLaunchKernelGGL(k_queue_probe, dim3(1), dim3(64), 0, a, 6000ull, d);          // 100 MHz clock: 60 us
    hipLaunchKernelGGL(k_queue_probe, dim3(1), dim3(64), 0, b, 6000ull, d + 2);
    if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return true;
    if (hipMemcpyAsync(v, d, sizeof v, hipMemcpyDeviceToHost, a) != hipSuccess || hipStreamSynchronize(a) != hipSuccess) return true;
    (void)hipMemsetAsync(d, 0, sizeof v, a); (void)hipStreamSynchronize(a);
    return v[2] < v[1] && v[0] < v[3];      // each started before the other ended
}

// the second set of work buffers: shares the (immutable) mesh / instruction records of h
int make_twin(pfc_context *h) {
    if (h->twin) return PFC_OK;
    pfc_context *t = new (std::nothrow) pfc_context();
    if (!t) return fail(h, PFC_ERR_NOMEM, "out of host memory");
    t->device = h->device; t->is_twin = true; t->finalized = true;
    t->ins = h->ins; t->d_meshes = h->d_meshes; t->d_ins = h->d_ins; t->max_levels = h->max_levels;
    t->max_leaves = h->max_leaves; t->max_elem1 = h->max_elem1; t->max_elem2 = h->max_elem2;
    t->any_bristle = h->any_bristle; t->any_tet_tet = h->any_tet_tet; t->any_regularized = h->any_regularized; t->all_rule2 = h->all_rule2;
    t->opt_split_min = 0;
    t->stream = std::move(h->twin_stream);
    if ((!t->stream && hipStreamCreateWithFlags(t->stream.put(), hipStreamNonBlocking) != hipSuccess) ||
        hipEventCreateWithFlags(h->ev_fork.put(), hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(h->ev_join.put(), hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(h->ev_join0.put(), hipEventDisableTiming) != hipSuccess) {
        delete t;
        return fail(h, PFC_ERR_HIP, "could not create the second stream");
    }
    // one queue for both streams: a stream of another priority cannot share a hardware queue with a normal one (its price where
    // the plain pair does overlap: 1 % of the step, which is why it is the fallback and not the rule)
    h->twin_queue_fallback = 0;
    if (!std::getenv("PFC_NO_QUEUE_TEST") && !streams_overlap(h, h->stream, t->stream)) {
        int lo = 0, hi = 0;
        Stream s2;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo &&
            hipStreamCreateWithPriority(s2.put(), hipStreamNonBlocking, hi) == hipSuccess) {
            t->stream = std::move(s2);
            h->twin_queue_fallback = streams_overlap(h, h->stream, t->stream) ? 1 : 2;      // 2: still serial (reported, not fatal)
        } else {
            h->twin_queue_fallback = 2;
        }
    }
    h->twin = t;
    return PFC_OK;
}

}  // namespace

// =================================================================================================================
// C ABI
// =================================================================================================================
#include "pfc_multi.h"

// The context of what runs on one device only: the handle, or the first shard of a multi-device handle.  Such an entry is
// on_shard(h, first_ctx(h), body): on a single-device handle on_shard's copy of the message assigns h->err to itself.
static pfc_context *first_ctx(pfc_context *h) { return h->multi ? h->multi->shard[0] : h; }

extern "C" {

int pfc_version(void) { return PFC_VERSION; }

int pfc_build_info(void) {
    int f = 0;
#ifdef PFC_STAMPS
    f |= 1;
#endif
    f |= (PFC_EXP & 0xFF) << 8;
#ifdef PFC_VARIANT
    f |= 1 << 16;      // built by scripts/mkvar.sh from patched sources (an A/B variant, not the product)
#endif
    return f;
}

int pfc_create(int device, pfc_handle *out) {
    if (!out) return PFC_ERR_BAD_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return PFC_ERR_HIP;
    if (hipSetDevice(device) != hipSuccess) return PFC_ERR_HIP;
    pfc_context *h = new (std::nothrow) pfc_context();
    if (!h) return PFC_ERR_NOMEM;
    h->device = device;
    if (hipStreamCreateWithFlags(h->stream.put(), hipStreamNonBlocking) != hipSuccess) { delete h; return PFC_ERR_HIP; }
    if (hipStreamCreateWithFlags(h->twin_stream.put(), hipStreamNonBlocking) != hipSuccess) h->twin_stream.reset();   // (make_twin creates one then)
    { int cu = 0; if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess) h->n_cu = cu; }
    *out = h;
    return PFC_OK;
}

int pfc_create_multi(const int *devices, int n_devices, pfc_handle *out) {
    if (!out) return PFC_ERR_BAD_ARG;
    *out = nullptr;
    if (!devices || n_devices < 1 || n_devices > 64) return PFC_ERR_BAD_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return PFC_ERR_HIP;
    for (int k = 0; k < n_devices; ++k)
        if (devices[k] < 0 || devices[k] >= n) return PFC_ERR_HIP;
    pfc_context *h = new (std::nothrow) pfc_context();
    pfc_multi *M = new (std::nothrow) pfc_multi();
    if (!h || !M) { delete h; delete M; return PFC_ERR_NOMEM; }
    h->device = devices[0];
    h->multi = M;
    M->dev.assign(devices, devices + n_devices);
    M->stage.resize((size_t)n_devices);
    int rc = PFC_OK;
    for (int k = 0; k < n_devices && rc == PFC_OK; ++k) {
        pfc_handle c = nullptr;
        rc = pfc_create(devices[k], &c);
        if (rc != PFC_OK) break;
        M->shard.push_back(c);
        if (hipEventCreateWithFlags(M->stage[k].done.put(), hipEventDisableTiming) != hipSuccess) rc = PFC_ERR_HIP;
        // direct peer copies between the first device and this one where the hardware allows it (xGMI); failures -- same device,
        // already enabled, no peer path -- leave the staged copy of hipMemcpyPeerAsync
        if (devices[k] != devices[0]) {
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, devices[k], devices[0]) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(devices[0], 0);
            (void)hipGetLastError();
        }
    }
    if (rc == PFC_OK) {
        (void)hipSetDevice(devices[0]);
        for (int k = 1; k < n_devices; ++k)
            if (devices[k] != devices[0]) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, devices[0], devices[k]) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(devices[k], 0);
                (void)hipGetLastError();
            }
        if (hipEventCreateWithFlags(M->ev_fork.put(), hipEventDisableTiming) != hipSuccess) rc = PFC_ERR_HIP;
    }
    if (rc == PFC_OK) {
        for (int k = 1; k < n_devices; ++k) {
            pfc_multi::Worker *w = new (std::nothrow) pfc_multi::Worker();
            if (!w) { rc = PFC_ERR_NOMEM; break; }
            M->workers.push_back(w);
            w->th = std::thread(multi_worker_loop, w, devices[k]);
        }
    }
    if (rc != PFC_OK) { pfc_destroy(h); return rc; }
    *out = h;
    return PFC_OK;
}

int pfc_last_shards(pfc_handle h) { return h ? (h->multi ? h->multi->n_used : 1) : 0; }

int pfc_last_shard_bounds(pfc_handle h, int *bound, int cap) {
    if (!h) return -PFC_ERR_BAD_ARG;
    if (!bound) return -fail(h, PFC_ERR_BAD_ARG, "pfc_last_shard_bounds: null buffer");
    const pfc_multi *M = h->multi;
    const bool cut = M && (int)M->bound.size() == (int)M->shard.size() + 1;      // (a multi-device handle before its first evaluation: no items, one shard)
    const int n_used = cut ? M->n_used : 1;
    if (cap < n_used + 1) return -fail(h, PFC_ERR_BAD_ARG, "pfc_last_shard_bounds: cap %d is less than the %d bounds of %d shards", cap, n_used + 1, n_used);
    if (cut) for (int k = 0; k <= n_used; ++k) bound[k] = M->bound[k];
    else { bound[0] = 0; bound[1] = M ? 0 : h->last_n_items; }
    return n_used;
}

void pfc_destroy(pfc_handle h) {
    if (!h) return;
    if (h->multi) { multi_destroy(h); delete h; return; }
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->pend.kind && h->pend.stream) (void)hipStreamSynchronize(h->pend.stream);   // an unchecked call of any kind on the caller's stream
    team_release(h);
    if (h->twin) pfc_destroy(h->twin);
    delete h;      // every buffer, event, graph and stream is a member that frees itself; the streams go last
}

const char *pfc_last_error(pfc_handle h) { return h ? h->err.c_str() : "null handle"; }

int pfc_add_mesh(pfc_handle h, int n_pt, const double *xyz, int n_tri, const int *tri, int n_tet, const int *tet,
                 const double *eps, double Ebar, int n_node, const double *node_c, const double *node_e,
                 const double *node_R, const int *node_child, const int *node_leaf) {
    if (!h) return -PFC_ERR_BAD_ARG;
    if (h->multi) {      // replicated on every shard (the ids agree: same sequence of calls)
        int id0 = -1;
        for (size_t k = 0; k < h->multi->shard.size(); ++k) {
            const int id = on_shard(h, h->multi->shard[k], [&](pfc_context *c) {
                return pfc_add_mesh(c, n_pt, xyz, n_tri, tri, n_tet, tet, eps, Ebar, n_node, node_c, node_e, node_R, node_child, node_leaf); }, true);
            if (id < 0) return id;
            if (k == 0) id0 = id;
        }
        return id0;
    }
    if (h->finalized) return -fail(h, PFC_ERR_STATE, "pfc_add_mesh after pfc_finalize");
    if (n_pt <= 0 || !xyz || n_node <= 0 || !node_c || !node_e || !node_R || !node_child || !node_leaf)
        return -fail(h, PFC_ERR_BAD_ARG, "pfc_add_mesh: null or empty argument");
    const bool has_tri = tri && n_tri > 0, has_tet = tet && n_tet > 0;
    if (has_tri == has_tet)  // verify_eMesh_ContactProperties: src/mechanism_scenario.jl:301-306
        return -fail(h, PFC_ERR_BAD_ARG, "pfc_add_mesh: exactly one of tri / tet must be given");
    if (has_tet && !eps) return -fail(h, PFC_ERR_BAD_ARG, "pfc_add_mesh: tet mesh without eps");
    HostMesh m;
    m.n_pt = n_pt; m.n_tri = has_tri ? n_tri : 0; m.n_tet = has_tet ? n_tet : 0; m.n_node = n_node; m.Ebar = Ebar;
    const int n_elem = has_tri ? n_tri : n_tet;
    for (int k = 0; k < 3 * n_pt; ++k)
        if (!std::isfinite(xyz[k])) return -fail(h, PFC_ERR_NONFINITE, "pfc_add_mesh: non-finite vertex");
    m.xyz.assign(xyz, xyz + 3 * (size_t)n_pt);
    if (has_tri) {
        for (int k = 0; k < 3 * n_tri; ++k)
            if (tri[k] < 0 || tri[k] >= n_pt) return -fail(h, PFC_ERR_BAD_ARG, "pfc_add_mesh: triangle index out of range");
        m.tri.assign(tri, tri + 3 * (size_t)n_tri);
    } else {
        for (int k = 0; k < 4 * n_tet; ++k)
            if (tet[k] < 0 || tet[k] >= n_pt) return -fail(h, PFC_ERR_BAD_ARG, "pfc_add_mesh: tet index out of range");
        m.tet.assign(tet, tet + 4 * (size_t)n_tet);
        m.eps.assign(eps, eps + n_pt);
        // (0.0 < volume(point[tet[k]])) || error("inverted tetrahedron"): src/geometry/mesh.jl:27-29,
        // volume: src/math_kernel/geometry_kernel.jl:22-38
        for (int k = 0; k < n_tet; ++k) {
            const double *a = xyz + 3 * (size_t)tet[4 * k], *b = xyz + 3 * (size_t)tet[4 * k + 1];
            const double *c = xyz + 3 * (size_t)tet[4 * k + 2], *d = xyz + 3 * (size_t)tet[4 * k + 3];
            double V = (b[0] - a[0]) * (c[1] * d[2] - c[2] * d[1]);
            V = std::fma(b[1] - a[1], c[2] * d[0] - c[0] * d[2], V);
            V = std::fma(b[2] - a[2], c[0] * d[1] - c[1] * d[0], V);
            V = std::fma(c[0] - d[0], a[2] * b[1] - a[1] * b[2], V);
            V = std::fma(c[1] - d[1], a[0] * b[2] - a[2] * b[0], V);
            V = std::fma(c[2] - d[2], a[1] * b[0] - a[0] * b[1], V);
            if (!(0.0 < V * (1.0 / 6.0))) return -fail(h, PFC_ERR_INVERTED_TET, "inverted tetrahedron %d", k);
        }
    }
    m.nodes.resize(n_node);
    int n_leaf = 0;
    for (int k = 0; k < n_node; ++k) {
        NodeRec &r = m.nodes[k];
        for (int j = 0; j < 3; ++j) { r.c[j] = node_c[3 * k + j]; r.e[j] = node_e[3 * k + j]; }
        for (int j = 0; j < 9; ++j) r.R[j] = node_R[9 * k + j];
        r.child0 = node_child[2 * k]; r.child1 = node_child[2 * k + 1]; r.leaf = node_leaf[k]; r.pad = 0.0;
        static const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        r.aabb = std::memcmp(r.R, I9, sizeof I9) == 0 ? 1 : 0;
        if (r.leaf == kInternal) {
            if (r.child0 <= 0 || r.child0 >= n_node || r.child1 <= 0 || r.child1 >= n_node)
                return -fail(h, PFC_ERR_BAD_ARG, "pfc_add_mesh: node %d has a bad child index", k);
        } else {
            if (r.leaf < 0 || r.leaf >= n_elem) return -fail(h, PFC_ERR_BAD_ARG, "pfc_add_mesh: node %d has a bad leaf id", k);
            ++n_leaf;
        }
    }
    m.n_leaf = n_leaf;
    m.depth = tree_depth(m.nodes);
    if (m.depth < 0) return -fail(h, PFC_ERR_BAD_ARG, "pfc_add_mesh: the node array is not a tree");
    // Device node order: breadth-first (the host passes any order with node 0 = root; node indices never leave the
    // library, leaf ids are element indices).  The two children of a node become neighbours (one 128-byte line of
    // NodeF), and the first N nodes are the top levels of the tree, which the small-scene kernel keeps in LDS.
    {
        std::vector<int> order;          // order[new] = old
        order.reserve(n_node);
        order.push_back(0);
        for (size_t q = 0; q < order.size(); ++q) {
            const NodeRec &r = m.nodes[order[q]];
            if (r.leaf == kInternal) { order.push_back(r.child0); order.push_back(r.child1); }
        }
        if ((int)order.size() != n_node) return -fail(h, PFC_ERR_BAD_ARG, "pfc_add_mesh: the node array is not a tree");
        // ... and every node once: a child shared by two parents next to a node nobody points to has the right count too
        std::vector<char> seen(n_node, 0);
        for (int k : order) {
            if (seen[k]) return -fail(h, PFC_ERR_BAD_ARG, "pfc_add_mesh: the node array is not a tree");
            seen[k] = 1;
        }
        std::vector<int> inv(n_node);
        for (int k = 0; k < n_node; ++k) inv[order[k]] = k;
        std::vector<NodeRec> bfs(n_node);
        for (int k = 0; k < n_node; ++k) {
            bfs[k] = m.nodes[order[k]];
            if (bfs[k].leaf == kInternal) { bfs[k].child0 = inv[bfs[k].child0]; bfs[k].child1 = inv[bfs[k].child1]; }
        }
        m.nodes.swap(bfs);
    }
    // Device encoding: a child link to a LEAF is stored as ~index (negative), so the broadphase knows from the link
    // alone whether the child needs its rotation R (tight-fitted leaf) and can issue every load of an iteration at once.
    for (NodeRec &r : m.nodes)
        if (r.leaf == kInternal) {
            if (m.nodes[r.child0].leaf != kInternal) r.child0 = ~r.child0;
            if (m.nodes[r.child1].leaf != kInternal) r.child1 = ~r.child1;
        }
    // single-precision mirror (k_bp_dfs32): Float64 centre, Float32 extents, rotation as a unit quaternion
    m.nodesf.resize(n_node);
    for (int k = 0; k < n_node; ++k) {
        const NodeRec &r = m.nodes[k];
        NodeF f;
        std::memset(&f, 0, sizeof f);
        for (int j = 0; j < 3; ++j) { f.c[j] = (float)r.c[j]; f.e[j] = (float)r.e[j]; }
        m.cmax = std::fmax(m.cmax, (std::fabs(r.c[0]) + std::fabs(r.c[1])) + std::fabs(r.c[2]));
        const double *R = r.R;   // column-major: R(i,j) = R[i + 3 j]
        double q[4];
        const double tr = R[0] + R[4] + R[8];
        if (tr > 0.0) {
            const double sq = std::sqrt(tr + 1.0) * 2.0;
            q[0] = 0.25 * sq; q[1] = (R[5] - R[7]) / sq; q[2] = (R[6] - R[2]) / sq; q[3] = (R[1] - R[3]) / sq;
        } else if (R[0] > R[4] && R[0] > R[8]) {
            const double sq = std::sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0;
            q[0] = (R[5] - R[7]) / sq; q[1] = 0.25 * sq; q[2] = (R[3] + R[1]) / sq; q[3] = (R[6] + R[2]) / sq;
        } else if (R[4] > R[8]) {
            const double sq = std::sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0;
            q[0] = (R[6] - R[2]) / sq; q[1] = (R[3] + R[1]) / sq; q[2] = 0.25 * sq; q[3] = (R[7] + R[5]) / sq;
        } else {
            const double sq = std::sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0;
            q[0] = (R[1] - R[3]) / sq; q[1] = (R[6] + R[2]) / sq; q[2] = (R[7] + R[5]) / sq; q[3] = 0.25 * sq;
        }
        const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int j = 0; j < 4; ++j) f.q[j] = (float)(q[j] / qn);
        // host check of what the device's error bound relies on (pfc_bp.h, "Error radius E"): in Float64, the Float32
        // quaternion reproduces R to 4 u per entry and |q|^2 is within 2.25 u of 1 (u = 2^-24)
        {
            const double w = f.q[0], x = f.q[1], y = f.q[2], z = f.q[3];
            const double Rq[9] = {1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w),
                                  2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w),
                                  2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y)};
            double worst = 0.0;
            for (int j = 0; j < 9; ++j) worst = std::fmax(worst, std::fabs(Rq[j] - R[j]));
            const double n2 = w * w + x * x + y * y + z * z, u = 5.9604644775390625e-8;
            // a node that fails is never decided in single precision: NaN extent -> S = NaN -> exact test (test_pair_f32)
            if (!(std::isfinite(qn) && worst <= 4.0 * u && std::fabs(n2 - 1.0) <= 2.25 * u)) f.e[0] = std::numeric_limits<float>::quiet_NaN();
            // The 24 u radius of an internal x internal pair is derived for identity quaternions ("Error radius E", (5)); an
            // internal node with any other R (a host-supplied tree) carries the same exact-only mark, so that premise holds
            // for every pair the single-precision test decides at that radius.
            if (r.leaf == kInternal && !r.aabb) f.e[0] = std::numeric_limits<float>::quiet_NaN();
        }
        if (r.leaf == kInternal) { f.link0 = r.child0; f.link1 = r.child1; }
        else { f.link0 = r.leaf; f.link1 = -1; }
        m.nodesf[k] = f;
    }
    h->meshes.push_back(std::move(m));
    return (int)h->meshes.size() - 1;
}

int pfc_add_instruction(pfc_handle h, int id_1, int id_2, double chi, int n_quad, int model, const double *params) {
    if (!h) return -PFC_ERR_BAD_ARG;
    if (h->multi) {
        int id0 = -1;
        for (size_t k = 0; k < h->multi->shard.size(); ++k) {
            const int id = on_shard(h, h->multi->shard[k], [&](pfc_context *c) { return pfc_add_instruction(c, id_1, id_2, chi, n_quad, model, params); }, true);
            if (id < 0) return id;
            if (k == 0) id0 = id;
        }
        return id0;
    }
    if (h->finalized) return -fail(h, PFC_ERR_STATE, "pfc_add_instruction after pfc_finalize");
    const int nm = (int)h->meshes.size();
    if (id_1 < 0 || id_1 >= nm || id_2 < 0 || id_2 >= nm || !params)
        return -fail(h, PFC_ERR_BAD_ARG, "pfc_add_instruction: bad mesh id");
    if (h->meshes[id_2].n_tet == 0)  // id_2 is always a tet mesh: src/mechanism_scenario.jl:402-416
        return -fail(h, PFC_ERR_BAD_ARG, "pfc_add_instruction: id_2 must be a tet mesh");
    if (n_quad < 1 || n_quad > 2)  // src/mechanism_scenario.jl:45
        return -fail(h, PFC_ERR_BAD_ARG, "only quadrature rules 1 and 2 are currently implemented");
    if (model != PFC_REGULARIZED && model != PFC_BRISTLE) return -fail(h, PFC_ERR_BAD_ARG, "unknown friction model");
    InsDev in;
    std::memset(&in, 0, sizeof in);
    in.m1 = id_1; in.m2 = id_2; in.model = model; in.nq = n_quad; in.chi = chi;
    in.mu_s = params[0]; in.mu_d = params[1];
    if (!(in.mu_d <= in.mu_s))  // determine_μs_μd: src/mechanism_scenario.jl:353-356
        return -fail(h, PFC_ERR_BAD_ARG, "something is wrong: mu_d must be <= mu_s");
    if (model == PFC_REGULARIZED) {
        in.v_c = params[2];
    } else {
        in.tau = params[2]; in.k_bar = params[3]; in.magic = params[4];
        if (!(0.0 < in.mu_d)) return -fail(h, PFC_ERR_BAD_ARG, "mu_d cannot be 0 for bristle friction");
    }
    h->ins.push_back(in);
    return (int)h->ins.size() - 1;
}

int pfc_finalize(pfc_handle h) {
    if (!h) return PFC_ERR_BAD_ARG;
    if (h->multi) {      // every device uploads its replica at the same time
        pfc_multi *M = h->multi;
        std::vector<std::function<int()>> jobs(M->shard.size());
        for (size_t k = 0; k < M->shard.size(); ++k) { pfc_context *c = M->shard[k]; jobs[k] = [c]() { return pfc_finalize(c); }; }
        const int rc = multi_run(h, jobs);
        h->finalized = rc == PFC_OK;
        return rc;
    }
    if (h->finalized) return fail(h, PFC_ERR_STATE, "pfc_finalize called twice");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->status.ensure(4));
    HIP_TRY(h, hipMemsetAsync(h->status.p, 0, sizeof(unsigned) * 4, h->stream));   // same stream as k_prep_tet below
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<MeshDev> md(h->meshes.size());
    {   // one arena for the records of all meshes, the broadphase's single-precision nodes first (its hot set, contiguous)
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        size_t total = 0;
        for (HostMesh &m : h->meshes) total += up(sizeof(NodeF) * m.nodesf.size());
        for (HostMesh &m : h->meshes)
            total += up(sizeof(NodeRec) * m.nodes.size()) + (m.n_tri ? up(sizeof(TriRec) * m.n_tri)
                                                                      : up(sizeof(TetRec) * m.n_tet) + up(sizeof(double) * 4 * m.n_tet));
        HIP_TRY(h, h->mesh_arena.ensure(total));
        size_t off = 0;
        for (HostMesh &m : h->meshes) { m.d_nodesf = (NodeF *)(h->mesh_arena.p + off); off += up(sizeof(NodeF) * m.nodesf.size()); }
        for (HostMesh &m : h->meshes) {
            m.d_nodes = (NodeRec *)(h->mesh_arena.p + off); off += up(sizeof(NodeRec) * m.nodes.size());
            if (m.n_tri) { m.d_tri = (TriRec *)(h->mesh_arena.p + off); off += up(sizeof(TriRec) * m.n_tri); }
            else {
                m.d_tet = (TetRec *)(h->mesh_arena.p + off); off += up(sizeof(TetRec) * m.n_tet);
                m.d_tet_eps = (double *)(h->mesh_arena.p + off); off += up(sizeof(double) * 4 * m.n_tet);
            }
        }
    }
    for (size_t k = 0; k < h->meshes.size(); ++k) {
        HostMesh &m = h->meshes[k];
        DevBuf<double> d_xyz, d_eps;      // the raw vertices / pressures and the element indices: until the records are made
        DevBuf<int> d_idx;
        HIP_TRY(h, copy_sync(h, m.d_nodes, m.nodes.data(), sizeof(NodeRec) * m.nodes.size(), hipMemcpyHostToDevice));
        HIP_TRY(h, copy_sync(h, m.d_nodesf, m.nodesf.data(), sizeof(NodeF) * m.nodesf.size(), hipMemcpyHostToDevice));
        HIP_TRY(h, d_xyz.ensure(m.xyz.size()));
        HIP_TRY(h, copy_sync(h, d_xyz.p, m.xyz.data(), sizeof(double) * m.xyz.size(), hipMemcpyHostToDevice));
        if (m.n_tri) {
            HIP_TRY(h, d_idx.ensure(m.tri.size()));
            HIP_TRY(h, copy_sync(h, d_idx.p, m.tri.data(), sizeof(int) * m.tri.size(), hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_prep_tri, dim3((m.n_tri + 127) / 128), dim3(128), 0, h->stream, m.n_tri, d_xyz.p, d_idx.p, m.d_tri);
        } else {
            HIP_TRY(h, d_idx.ensure(m.tet.size()));
            HIP_TRY(h, copy_sync(h, d_idx.p, m.tet.data(), sizeof(int) * m.tet.size(), hipMemcpyHostToDevice));
            HIP_TRY(h, d_eps.ensure(m.eps.size()));
            HIP_TRY(h, copy_sync(h, d_eps.p, m.eps.data(), sizeof(double) * m.eps.size(), hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_prep_tet, dim3((m.n_tet + 127) / 128), dim3(128), 0, h->stream, m.n_tet, d_xyz.p, d_eps.p, d_idx.p,
                               m.d_tet, m.d_tet_eps, h->status.p);
        }
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        md[k].nodes = m.d_nodes; md[k].nodesf = m.d_nodesf; md[k].tri = m.d_tri; md[k].tet = m.d_tet; md[k].tet_eps = m.d_tet_eps; md[k].Ebar = m.Ebar; md[k].cmax = m.cmax;
        md[k].n_tri = m.n_tri; md[k].n_tet = m.n_tet; md[k].n_node = m.n_node; md[k].depth = m.depth;
    }
    unsigned status = 0;
    HIP_TRY(h, copy_sync(h, &status, h->status.p, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (status & kStNonFinite) return fail(h, PFC_ERR_NONFINITE, "singular tetrahedron (non-finite zeta transform)");
    if (!md.empty()) {
        HIP_TRY(h, h->own_meshes.ensure(md.size()));
        h->d_meshes = h->own_meshes.p;
        HIP_TRY(h, copy_sync(h, h->d_meshes, md.data(), sizeof(MeshDev) * md.size(), hipMemcpyHostToDevice));
    }
    h->max_levels = 1;
    h->max_leaves = 2;
    h->max_elem1 = h->max_elem2 = 1;
    h->any_bristle = h->any_regularized = false;
    h->all_rule2 = !h->ins.empty();
    for (const InsDev &in : h->ins) {
        if (in.nq == 1) h->all_rule2 = false;      // (InsDev::nq is the rule; k_setup_items gives every other rule three points)
        {   // (key widths of the candidate sort, option "fixed_order": a candidate is (element of mesh_1, tet of mesh_2))
            const HostMesh &m1 = h->meshes[in.m1], &m2 = h->meshes[in.m2];
            const int e1 = m1.n_tri ? m1.n_tri : m1.n_tet;
            if (e1 > h->max_elem1) h->max_elem1 = e1;
            if (m2.n_tet > h->max_elem2) h->max_elem2 = m2.n_tet;
        }
        int lv = h->meshes[in.m1].depth + h->meshes[in.m2].depth + 1;
        if (lv > h->max_levels) h->max_levels = lv;
        const int lf = h->meshes[in.m1].n_leaf + h->meshes[in.m2].n_leaf;
        if (lf > h->max_leaves) h->max_leaves = lf;
        if (in.model == PFC_BRISTLE) h->any_bristle = true;
        if (in.model == PFC_REGULARIZED) h->any_regularized = true;
        if (h->meshes[in.m1].n_tri == 0) h->any_tet_tet = true;
    }
    // the depth-first broadphase keeps 3 * levels + 3 stack slots in reserve (k_bp_dfs)
    if (3 * h->max_levels + 3 > kDfsStack - 128 || 3 * h->max_levels + 3 > kDfsStack32 - 1024)
        return fail(h, PFC_ERR_BAD_ARG, "OBB trees too deep (depth sum %d): rebuild them balanced", h->max_levels - 1);
    if (!h->ins.empty()) {
        HIP_TRY(h, h->own_ins.ensure(h->ins.size()));
        h->d_ins = h->own_ins.p;
        HIP_TRY(h, copy_sync(h, h->d_ins, h->ins.data(), sizeof(InsDev) * h->ins.size(), hipMemcpyHostToDevice));
        // one self-contained record per instruction for the fused small-scene kernel
        std::vector<InsFull> full(h->ins.size());
        for (size_t k = 0; k < h->ins.size(); ++k) {
            const InsDev &in = h->ins[k];
            const HostMesh &m1 = h->meshes[in.m1], &m2 = h->meshes[in.m2];
            InsFull f;
            std::memset(&f, 0, sizeof f);
            f.nodes1 = m1.d_nodes; f.nodes2 = m2.d_nodes; f.nf1 = m1.d_nodesf; f.nf2 = m2.d_nodesf;
            f.tri = m1.d_tri; f.tet = m2.d_tet; f.tet1 = m1.d_tri ? nullptr : m1.d_tet; f.eps1 = m1.d_tet_eps; f.eps2 = m2.d_tet_eps;
            f.chi = in.chi; f.Ebar = m2.Ebar; f.Ebar1 = m1.Ebar; f.mu_s = in.mu_s; f.mu_d = in.mu_d; f.v_c = in.v_c;
            f.tau = in.tau; f.k_bar = in.k_bar; f.magic = in.magic;
            f.model = in.model; f.nq = in.nq; f.n_node1 = m1.n_node; f.n_node2 = m2.n_node;
            f.reserve = 3 * (m1.depth + m2.depth + 1) + 3;
            f.cmax12 = m1.cmax + m2.cmax;
            full[k] = f;
        }
        HIP_TRY(h, h->own_insfull.ensure(full.size()));
        h->d_insfull = h->own_insfull.p;
        HIP_TRY(h, copy_sync(h, h->d_insfull, full.data(), sizeof(InsFull) * full.size(), hipMemcpyHostToDevice));
    }
    h->finalized = true;
    return PFC_OK;
}

// Argument checks shared by every evaluation entry point (host- or device-buffer, value or Dual): what the reference
// would reject with a MethodError / BoundsError before forceAllElasticIntersections! runs.
static int check_eval_args(pfc_context *h, int n_items, const void *ins_ids, const void *pose, const void *twist,
                           const void *s, const void *wrench, const void *sdot) {
    if (!h->finalized) return fail(h, PFC_ERR_STATE, "pfc_eval before pfc_finalize");
    if (n_items < 0) return fail(h, PFC_ERR_BAD_ARG, "negative n_items");
    if (n_items == 0) return PFC_OK;
    if (h->ins.empty()) return fail(h, PFC_ERR_STATE, "no contact instructions");
    if (!pose || !twist || !wrench || !sdot) return fail(h, PFC_ERR_BAD_ARG, "null buffer");
    if (!ins_ids && n_items > (int)h->ins.size())
        return fail(h, PFC_ERR_BAD_ARG, "n_items exceeds the number of instructions and no ins_ids given");
    if (h->any_bristle && !s) return fail(h, PFC_ERR_BAD_ARG, "bristle instructions need the state buffer s");
    return PFC_OK;
}

// pfc_eval_device on one device.  o: what the caller decides (pose, list, targets); nw and half are set here, with the route.
static int eval_device(pfc_context *h, int n_items, const int *d_ins_ids, const double *d_pose, const double *d_twist,
                       const double *d_s, double *d_wrench, double *d_sdot, int *d_counts, void *stream, PassOpts o) {
    { const int rc = check_eval_args(h, n_items, d_ins_ids, d_pose, d_twist, d_s, d_wrench, d_sdot); if (rc != PFC_OK) return rc; }
    drop_pending(h);
    end_kept_pass(h);
    if (n_items == 0) { h->last_n_items = 0; return PFC_OK; }
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    int team = fused_team(h, n_items, o);
    if (team > 1 && !team_acquire(h)) team = fused_ok(h, n_items, o) ? 1 : 0;     // another handle's teams are in flight on this device
    if (team) {
        o.nw = team;
        const int rc_t = enqueue_fused(h, n_items, d_ins_ids, d_pose, d_twist, d_s, d_wrench, d_sdot, d_counts, st, o);
        if (rc_t != PFC_OK) team_release(h);      // no fused evaluation pending: the slot is free again
        return rc_t;
    }
    if (h->fused_skip > 0 && n_items <= kFusedMaxItems) --h->fused_skip;
    const bool split = h->opt_split_min > 0 && n_items >= h->opt_split_min && d_ins_ids && !h->opt_debug && !h->opt_fixed_order &&
                       !o.list && !h->is_twin && !pile_mode(h, n_items);
    if (!split) return enqueue_eval(h, n_items, d_ins_ids, d_pose, d_twist, d_s, d_wrench, d_sdot, d_counts, st, o);
    int rc = make_twin(h);
    if (rc != PFC_OK) return rc;
    pfc_context *t = h->twin;
    t->opt_profile = h->opt_profile; t->opt_max_levels = h->opt_max_levels; t->opt_bfs_levels = h->opt_bfs_levels;
    t->opt_poison = h->opt_poison;
    if (t->opt_clip_min != h->opt_clip_min) { t->opt_clip_min = h->opt_clip_min; t->ghave[0] = t->ghave[1] = false; }
    if (t->opt_clip_queue != h->opt_clip_queue) { t->opt_clip_queue = h->opt_clip_queue; t->ghave[0] = t->ghave[1] = false; }
    if (t->opt_bin_split != h->opt_bin_split) { t->opt_bin_split = h->opt_bin_split; t->ghave[0] = t->ghave[1] = false; }
    if (t->opt_vertex_fields != h->opt_vertex_fields) { t->opt_vertex_fields = h->opt_vertex_fields; t->ghave[0] = t->ghave[1] = false; }
    if (t->opt_integ_spec != h->opt_integ_spec) { t->opt_integ_spec = h->opt_integ_spec; t->ghave[0] = t->ghave[1] = false; }
    if (t->opt_quad_const != h->opt_quad_const) { t->opt_quad_const = h->opt_quad_const; t->ghave[0] = t->ghave[1] = false; }
    t->opt_graph = h->opt_graph;
    if (t->opt_no_filter != h->opt_no_filter) { t->opt_no_filter = h->opt_no_filter; t->ghave[0] = t->ghave[1] = false; }
    const int n0 = n_items / 2, n1 = n_items - n0;      // (55 / 45 is the same within noise, 60 / 40 and 45 / 55 are slower: round 3)
    // Both halves run on the library's OWN two streams, which start when the caller's stream has reached this point and
    // join it again at the end.  (The first half used to run on the caller's stream.  The halves only overlap if their
    // streams sit on different hardware queues, and a stream the caller created may share one with the twin's: a torch
    // pool stream took the 8 192-pose step from 4.1 to 5.1 ms -- more than the unsplit evaluation; scripts/inflight_probe.py.)
    hipStream_t s0 = h->stream;
    HIP_TRY(h, hipEventRecord(h->ev_fork, st));
    if (s0 != st) HIP_TRY(h, hipStreamWaitEvent(s0, h->ev_fork, 0));
    HIP_TRY(h, hipStreamWaitEvent(t->stream, h->ev_fork, 0));
    o.half = true;
    rc = enqueue_eval(h, n0, d_ins_ids, d_pose, d_twist, d_s, d_wrench, d_sdot, d_counts, s0, o);
    if (rc != PFC_OK) return rc;
    if (o.bp_pose) o.bp_pose += 24 * (size_t)n0;
    o.tail = nullptr;      // the second half packs its tail into its own buffer (check_eval reads it there)
    rc = enqueue_eval(t, n1, d_ins_ids + n0, d_pose + 24 * (size_t)n0, d_twist + 6 * (size_t)n0,
                      d_s ? d_s + 6 * (size_t)n0 : nullptr, d_wrench + 6 * (size_t)n0, d_sdot + 6 * (size_t)n0,
                      d_counts ? d_counts + 4 * (size_t)n0 : nullptr, t->stream, o);
    if (rc != PFC_OK) { h->err = t->err; return rc; }
    HIP_TRY(h, hipEventRecord(h->ev_join, t->stream));
    HIP_TRY(h, hipStreamWaitEvent(st, h->ev_join, 0));
    if (s0 != st) {
        HIP_TRY(h, hipEventRecord(h->ev_join0, s0));
        HIP_TRY(h, hipStreamWaitEvent(st, h->ev_join0, 0));
    }
    h->pend = {pfc_context::Pending::Batched, s0, n0};
    return PFC_OK;
}

int pfc_eval_device(pfc_handle h, int n_items, const int *d_ins_ids, const double *d_pose, const double *d_twist,
                    const double *d_s, double *d_wrench, double *d_sdot, int *d_counts, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    if (h->multi)
        return multi_eval_device(h, n_items, 0, d_ins_ids, d_pose, nullptr, d_twist, d_s, nullptr, nullptr, nullptr, d_wrench, d_sdot,
                                 nullptr, nullptr, d_counts, stream);
    return eval_device(h, n_items, d_ins_ids, d_pose, d_twist, d_s, d_wrench, d_sdot, d_counts, stream, PassOpts());
}

namespace {

// ---- pfc_contact_surface (pfc_surface.h) ----------------------------------------------------------------------------
// The outputs of pfc_contact_surface_fric beyond the surface's (device pointers); s may be null, stiff may be null.
struct SurfFricOut {
    const double *s;
    double *fric, *fric_summary, *stiff;
};

// The whole call on stream st: item setup, the batched broadphase, the candidate list in canonical order, count, scan, item
// segments, summary and -- when both capacities suffice -- the emission; the status block goes to pinned memory for
// check_surface.  Always this launch sequence, whatever "fused", "team", "split_min", "fixed_order" or "debug" say.  With fo
// (pfc_contact_surface_fric) the same launches, the bristle state s in the item setup, and the four friction kernels of
// pfc_surface_fric.h between the emission and k_surf_final.
int surface_enqueue(pfc_context *h, int n_items, const int *d_ins_ids, const double *d_pose, const double *d_twist, long long cap_poly,
                    long long cap_trac, long long *d_poly_off, int *d_poly_idx, double *d_poly_xyz, long long *d_poly_trac,
                    double *d_trac, double *d_summary, int *d_counts, long long *d_totals, hipStream_t st, const SurfFricOut *fo = nullptr) {
    // an evaluation for the call-order rules: the candidate list and the counters a Dual evaluation could reuse are overwritten
    new_value_pass(h);
    drop_pending(h);
    forget_host_points(h);
    int ba, bb;
    const int bits = pfc_sort_key_bits(n_items, h->max_elem1, h->max_elem2, &ba, &bb);
    if (bits > 64)
        return fail(h, PFC_ERR_BAD_ARG, "pfc_contact_surface: (item, element, element) needs %d key bits for %d items, more than 64", bits, n_items);
    HIP_TRY(h, ensure_work(h, n_items, false));
    const size_t c = h->ccap;
    HIP_TRY(h, h->surf_cnt.ensure(2 * (c + 1)));
    HIP_TRY(h, h->surf_off.ensure(2 * (c + 1)));
    HIP_TRY(h, h->surf_part.ensure(c * kSurfSums));
    HIP_TRY(h, h->surf_seg.ensure((size_t)n_items + 1));
    HIP_TRY(h, h->surf_canon_off.ensure((size_t)n_items + 1));
    HIP_TRY(h, h->surf_canon_fill.ensure((size_t)n_items));
    HIP_TRY(h, h->surf_canon_item.ensure(c));
    HIP_TRY(h, h->surf_keys[0].ensure(c));
    HIP_TRY(h, h->surf_keys[1].ensure(c));
    if (fo) {
        HIP_TRY(h, h->sfric_mom.ensure((size_t)n_items * kFricSplit * kFricMom));
        HIP_TRY(h, h->sfric_sum.ensure((size_t)n_items * kFricSplit * kFricSums));
        HIP_TRY(h, h->sfric_res.ensure((size_t)n_items * kResStride));
    }
    size_t scan_bytes = 0, sort_bytes = 0;
    HIP_TRY(h, pfc_scan_pairs(nullptr, &scan_bytes, nullptr, nullptr, c + 1, st));
    if (h->surf_whole_list) HIP_TRY(h, pfc_sort_temp_bytes(c, bits, &sort_bytes));
    HIP_TRY(h, h->surf_tmp.ensure((scan_bytes > sort_bytes ? scan_bytes : sort_bytes) + 16));
    const int levels = eff_levels(h);
    const int n_ctr = levels + 12;
    HIP_TRY(h, h->surf_out.ensure((size_t)n_ctr + 3));
    HIP_TRY(h, h->h_surf.ensure((size_t)n_ctr + 3));
    int *ccount = h->ctr.p, *next_seed = h->ctr.p + 2, *ucount = h->ctr.p + 4, *fcount = h->ctr.p + 6;   // (record_eval's layout)

    EvalArgs ea;
    ea.n_items = n_items; ea.ins_ids = d_ins_ids; ea.pose = d_pose; ea.twist = d_twist; ea.s = fo ? fo->s : nullptr; ea.bp_pose = nullptr;
    ea.ins = h->d_ins; ea.meshes = h->d_meshes; ea.n_ins = (int)h->ins.size(); ea.items = h->items.p;
    ea.frontier0 = h->frontier[0].p; ea.fcount = fcount; ea.acc = h->acc.p; ea.icnt = h->icnt.p;
    ea.status = h->status.p;
    hipLaunchKernelGGL(k_setup_items, dim3(grid_for(n_items, 64, 1 << 20)), dim3(64), 0, st, ea);
    const int L = bfs_levels_for(h, n_items, levels, false);
    launch_broadphase(h, n_items, L, false, ccount, fcount, next_seed, ucount, st);
    // (item, element of mesh 1, element of mesh 2): the per-item segments sorted in LDS, or -- once an item had more candidates
    // than a segment sort takes -- one sort of the whole list
    if (h->surf_whole_list)
        HIP_TRY(h, pfc_sort_candidates(h->cand.p, ccount, c, h->surf_keys[0].p, h->surf_keys[1].p, h->surf_tmp.p, h->surf_tmp.cap, n_items,
                                       ba, bb, bits, h->status.p, kStFixedCover, st));
    else
        HIP_TRY(h, pfc_canon_candidates(h->cand.p, ccount, c, h->icnt.p, n_items, h->surf_keys[0].p, h->surf_keys[1].p, h->surf_canon_off.p,
                                        h->surf_canon_fill.p, h->surf_canon_item.p, bb, h->status.p, kStFixedCover, kStFixedBig, st));
    SurfArgs g;
    g.items = h->items.p; g.cand = h->cand.p; g.ccount = ccount; g.ccap = (int)c; g.n_items = n_items; g.icnt = h->icnt.p;
    g.status = h->status.p; g.cnt = h->surf_cnt.p; g.part = h->surf_part.p; g.off = h->surf_off.p; g.seg = h->surf_seg.p;
    g.cap_poly = cap_poly; g.cap_trac = cap_trac; g.poly_off = d_poly_off; g.poly_idx = d_poly_idx; g.poly_xyz = d_poly_xyz;
    g.poly_trac = d_poly_trac; g.trac = d_trac; g.summary = d_summary; g.counts = d_counts; g.totals = d_totals;
    const int grid = grid_for(c + 1, kSurfBlock, kNpMaxBlocks);
    if (h->any_tet_tet) hipLaunchKernelGGL((k_surf_count<true>), dim3(grid), dim3(kSurfBlock), 0, st, g);
    else hipLaunchKernelGGL((k_surf_count<false>), dim3(grid), dim3(kSurfBlock), 0, st, g);
    HIP_TRY(h, pfc_scan_pairs(h->surf_tmp.p, &scan_bytes, h->surf_cnt.p, h->surf_off.p, c + 1, st));
    HIP_TRY(h, hipMemsetAsync(h->surf_seg.p, 0, sizeof(int) * ((size_t)n_items + 1), st));
    hipLaunchKernelGGL(k_surf_seg, dim3(grid_for(c + 1, 256, 4096)), dim3(256), 0, st, g);
    hipLaunchKernelGGL(k_surf_summary, dim3(n_items < 8192 ? n_items : 8192), dim3(64), 0, st, g);
    if (h->any_tet_tet) hipLaunchKernelGGL((k_surf_emit<true>), dim3(grid), dim3(kSurfBlock), 0, st, g);
    else hipLaunchKernelGGL((k_surf_emit<false>), dim3(grid), dim3(kSurfBlock), 0, st, g);
    if (fo) {
        SurfFricArgs f;
        f.mom = h->sfric_mom.p; f.fsum = h->sfric_sum.p; f.res = h->sfric_res.p;
        f.fric = fo->fric; f.fric_summary = fo->fric_summary; f.stiff = fo->stiff;
        const int grid_w = n_items * kFricSplit;                  // one workgroup per wave of an item (n_items <= 2^27: surface_fric_args)
        const int grid_i = n_items < 8192 ? n_items : 8192;                                                  // one wave per item
        if (h->any_tet_tet) hipLaunchKernelGGL((k_sfric_mom<true>), dim3(grid_w), dim3(kSurfBlock), 0, st, g, f);
        else hipLaunchKernelGGL((k_sfric_mom<false>), dim3(grid_w), dim3(kSurfBlock), 0, st, g, f);
        hipLaunchKernelGGL(k_sfric_eig, dim3(grid_i), dim3(64), 0, st, g, f);
        if (h->any_tet_tet) hipLaunchKernelGGL((k_sfric_pass<true>), dim3(grid_w), dim3(kSurfBlock), 0, st, g, f);
        else hipLaunchKernelGGL((k_sfric_pass<false>), dim3(grid_w), dim3(kSurfBlock), 0, st, g, f);
        hipLaunchKernelGGL(k_sfric_final, dim3(grid_for(n_items, 64, 4096)), dim3(64), 0, st, g, f);
    }
    hipLaunchKernelGGL(k_surf_final, dim3(1), dim3(64), 0, st, h->ctr.p, n_ctr, h->status.p, (const long long *)h->surf_off.p, (int)c,
                       h->surf_out.p);
    HIP_TRY(h, hipMemcpyAsync(h->h_surf.p, h->surf_out.p, sizeof(long long) * ((size_t)n_ctr + 3), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipGetLastError());
    h->pend = {pfc_context::Pending::Surface, st, 0, n_ctr};
    h->surf_cap_poly = cap_poly; h->surf_cap_trac = cap_trac;
    h->last_n_items = n_items; h->last_levels = levels; h->last_bfs_levels = L;
    return PFC_OK;
}

// Synchronise the pending surface call and judge it: internal work lists grown (PFC_ERR_OVERFLOW, re-issue), or the caller's
// capacities short (PFC_ERR_OVERFLOW with surf_cap_short: totals, offsets, summary and counters are written, nothing else).
int check_surface(pfc_context *h) {
    const hipStream_t st = std::exchange(h->pend, {}).stream;
    h->surf_cap_short = false;
    HIP_TRY(h, hipStreamSynchronize(st));
    const long long *o = h->h_surf.p;
    const unsigned status = (unsigned)o[0];
    const long long *ctr = o + 3;
    long long fpeak = 0;
    for (int lv = 0; lv <= h->last_bfs_levels && lv <= h->last_levels; ++lv)
        if (ctr[6 + lv] > fpeak) fpeak = ctr[6 + lv];
    if (status & kStBadIns) return fail(h, PFC_ERR_BAD_ARG, "instruction id out of range in ins_ids");
    if (status & kStHole) return fail(h, PFC_ERR_STATE, "internal error: a work-list slot was read before it was written");
    if (status & (kStFrontierOvf | kStCandOvf)) {      // as check_one
        if (status & kStFrontierOvf) { size_t f = h->fcap * 2; while (f < (size_t)fpeak) f *= 2; h->fcap = f; }
        if (status & kStCandOvf) { size_t c = h->ccap * 2; while (c < (size_t)ctr[0]) c *= 2; h->ccap = c; }
        if (h->fcap > ((size_t)1 << 30) || h->ccap > ((size_t)1 << 30))
            return fail(h, PFC_ERR_NOMEM, "work lists beyond 2^30 entries (frontier %zu, candidates %zu): evaluate the batch in parts", h->fcap, h->ccap);
        return fail(h, PFC_ERR_OVERFLOW, "work list overflow (status %u): capacities grown to frontier %zu, candidates %zu", status, h->fcap, h->ccap);
    }
    if (status & kStAbort) return fail(h, PFC_ERR_STATE, "broadphase aborted: iteration guard hit (corrupt tree?)");
    if (status & kStFixedBig) {
        h->surf_whole_list = true;
        return fail(h, PFC_ERR_OVERFLOW, "pfc_contact_surface: an item has more than 4096 candidates: the whole list is sorted from now on, re-issue");
    }
    if (status & kStFixedCover) return fail(h, PFC_ERR_OVERFLOW, "pfc_contact_surface: the candidate list outgrew its capacity: re-issue");
    if (status & kStNonFinite) return fail(h, PFC_ERR_NONFINITE, "Non-finite vertex likely");
    if (o[1] > h->surf_cap_poly || o[2] > h->surf_cap_trac) {
        h->surf_cap_short = true;
        return fail(h, PFC_ERR_OVERFLOW, "pfc_contact_surface: %lld polygons and %lld traction points, capacities %lld and %lld: grow the buffers and call again",
                    o[1], o[2], h->surf_cap_poly, h->surf_cap_trac);
    }
    return PFC_OK;
}

int surface_args(pfc_context *h, int n_items, const void *ins_ids, const void *pose, const void *twist, long long cap_poly,
                 long long cap_trac, const void *poly_off, const void *poly_idx, const void *poly_xyz, const void *poly_trac,
                 const void *trac, const void *summary, const void *totals) {
    if (!h->finalized) return fail(h, PFC_ERR_STATE, "pfc_contact_surface before pfc_finalize");
    if (n_items < 0 || cap_poly < 0 || cap_trac < 0) return fail(h, PFC_ERR_BAD_ARG, "pfc_contact_surface: negative n_items or capacity");
    if (!poly_off || !poly_trac || !totals || (n_items > 0 && (!pose || !twist || !summary)) || (cap_poly > 0 && (!poly_idx || !poly_xyz)) ||
        (cap_trac > 0 && !trac))
        return fail(h, PFC_ERR_BAD_ARG, "pfc_contact_surface: null buffer");
    if (n_items > 0 && h->ins.empty()) return fail(h, PFC_ERR_STATE, "no contact instructions");
    if (!ins_ids && n_items > (int)h->ins.size())
        return fail(h, PFC_ERR_BAD_ARG, "n_items exceeds the number of instructions and no ins_ids given");
    return PFC_OK;
}

}  // namespace

namespace {

// The host-pointer form of both surface calls; fo (pfc_contact_surface_fric) holds host pointers here: s, fric, fric_summary, stiff.
int surface_host(pfc_context *h, int n_items, const int *ins_ids, const double *pose, const double *twist, long long cap_poly,
                 long long cap_trac, long long *poly_off, int *poly_idx, double *poly_xyz, long long *poly_trac, double *trac,
                 double *summary, int *counts, long long *totals, const SurfFricOut *fo) {
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = (size_t)n_items;
    if (n_items == 0) {
        new_value_pass(h);
        forget_host_points(h);
        poly_off[0] = 0; poly_trac[0] = 0; totals[0] = totals[1] = 0;
        return PFC_OK;
    }
    // The outputs are staged for what the last calls needed (at most the caller's capacities): a call that needs more within the
    // caller's capacities lays the block out again and runs again -- so every attempt uploads the inputs, the block may have grown.
    Stage sg(h->stage, h->stream);
    int k_off = 0, k_tot = 0, k_ptr = 0, k_idx = 0, k_xyz = 0, k_trac = 0, k_sum = 0, k_cnt = 0, k_fsum = 0, k_stiff = 0, k_fric = 0;
    int rc = PFC_OK;
    long long tot_p = 0, tot_t = 0;
    for (int attempt = 0; attempt < 40; ++attempt) {
        const size_t dp = (size_t)(cap_poly < (long long)h->surf_hcap_poly ? cap_poly : (long long)h->surf_hcap_poly);
        const size_t dt = (size_t)(cap_trac < (long long)h->surf_hcap_trac ? cap_trac : (long long)h->surf_hcap_trac);
        sg.clear();
        const int k_pose = sg.in(pose, n * 24), k_twist = sg.in(twist, n * 6), k_ids = sg.in(ins_ids, n);
        const int k_s = sg.in(fo ? fo->s : nullptr, n * 6);      // (no fo: its fields are null)
        k_off = sg.out(poly_off, n + 1); k_tot = sg.out(totals, 2); k_sum = sg.out(summary, 11 * n); k_cnt = sg.out(counts, 4 * n);
        k_fsum = sg.out(fo ? fo->fric_summary : nullptr, kFricOut * n); k_stiff = sg.out(fo ? fo->stiff : nullptr, kStiffOut * n);
        k_ptr = sg.add(Stage::Part, poly_trac, dp + 1); k_idx = sg.add(Stage::Part, poly_idx, 3 * dp);
        k_xyz = sg.add(Stage::Part, poly_xyz, 24 * dp); k_trac = sg.add(Stage::Part, trac, 8 * dt);
        k_fric = sg.add(Stage::Part, fo ? fo->fric : nullptr, 4 * dt);
        HIP_TRY(h, sg.commit());
        SurfFricOut dfo;
        dfo.s = sg.at<double>(k_s); dfo.fric_summary = sg.at<double>(k_fsum); dfo.stiff = sg.at<double>(k_stiff); dfo.fric = sg.at<double>(k_fric);
        rc = surface_enqueue(h, n_items, sg.at<int>(k_ids), sg.at<double>(k_pose), sg.at<double>(k_twist), (long long)dp, (long long)dt,
                             sg.at<long long>(k_off), sg.at<int>(k_idx), sg.at<double>(k_xyz), sg.at<long long>(k_ptr), sg.at<double>(k_trac),
                             sg.at<double>(k_sum), sg.at<int>(k_cnt), sg.at<long long>(k_tot), h->stream, fo ? &dfo : nullptr);
        if (rc == PFC_OK) rc = check_surface(h);
        if (rc == PFC_ERR_OVERFLOW && h->surf_cap_short) {
            tot_p = h->h_surf.p[1]; tot_t = h->h_surf.p[2];
            if (tot_p <= cap_poly && tot_t <= cap_trac) {      // the staging was short, not the caller's buffers
                if ((size_t)tot_p > h->surf_hcap_poly) h->surf_hcap_poly = (size_t)tot_p;
                if ((size_t)tot_t > h->surf_hcap_trac) h->surf_hcap_trac = (size_t)tot_t;
                continue;
            }
            rc = fail(h, PFC_ERR_OVERFLOW, "pfc_contact_surface: %lld polygons and %lld traction points, capacities %lld and %lld: grow the buffers and call again",
                      tot_p, tot_t, cap_poly, cap_trac);
            break;
        }
        if (rc != PFC_ERR_OVERFLOW) break;
    }
    if (rc != PFC_OK && !(rc == PFC_ERR_OVERFLOW && h->surf_cap_short)) return rc;
    if (rc == PFC_OK) {      // the lists: as long as the totals say
        tot_p = h->h_surf.p[1]; tot_t = h->h_surf.p[2];
        HIP_TRY(h, sg.fetch(k_ptr, (size_t)tot_p + 1));
        HIP_TRY(h, sg.fetch(k_idx, 3 * (size_t)tot_p));
        HIP_TRY(h, sg.fetch(k_xyz, 24 * (size_t)tot_p));
        HIP_TRY(h, sg.fetch(k_trac, 8 * (size_t)tot_t));
        HIP_TRY(h, sg.fetch(k_fric, 4 * (size_t)tot_t));
    }
    HIP_TRY(h, sg.finish());
    return rc;
}

// pfc_contact_surface_fric's buffers beyond the surface call's
int surface_fric_args(pfc_context *h, int n_items, long long cap_trac, const void *fric, const void *fric_summary) {
    if ((n_items > 0 && !fric_summary) || (cap_trac > 0 && !fric)) return fail(h, PFC_ERR_BAD_ARG, "pfc_contact_surface_fric: null buffer");
    if (n_items > (1 << 27)) return fail(h, PFC_ERR_BAD_ARG, "pfc_contact_surface_fric: more than 2^27 items: evaluate the batch in parts");
    return PFC_OK;
}

}  // namespace

int pfc_contact_surface(pfc_handle h, int n_items, const int *ins_ids, const double *pose, const double *twist, long long cap_poly,
                        long long cap_trac, long long *poly_off, int *poly_idx, double *poly_xyz, long long *poly_trac, double *trac,
                        double *summary, int *counts, long long *totals) {
    if (!h) return PFC_ERR_BAD_ARG;
    if (h->multi)
        return surface_ctx(h, [&](pfc_context *c) {
            return pfc_contact_surface(c, n_items, ins_ids, pose, twist, cap_poly, cap_trac, poly_off, poly_idx, poly_xyz, poly_trac, trac, summary,
                                       counts, totals); });
    const int rc = surface_args(h, n_items, ins_ids, pose, twist, cap_poly, cap_trac, poly_off, poly_idx, poly_xyz, poly_trac, trac, summary, totals);
    if (rc != PFC_OK) return rc;
    return surface_host(h, n_items, ins_ids, pose, twist, cap_poly, cap_trac, poly_off, poly_idx, poly_xyz, poly_trac, trac, summary, counts, totals,
                        nullptr);
}

int pfc_contact_surface_fric(pfc_handle h, int n_items, const int *ins_ids, const double *pose, const double *twist, const double *s,
                             long long cap_poly, long long cap_trac, long long *poly_off, int *poly_idx, double *poly_xyz, long long *poly_trac,
                             double *trac, double *fric, double *summary, double *fric_summary, double *stiff, int *counts, long long *totals) {
    if (!h) return PFC_ERR_BAD_ARG;
    if (h->multi)
        return surface_ctx(h, [&](pfc_context *c) {
            return pfc_contact_surface_fric(c, n_items, ins_ids, pose, twist, s, cap_poly, cap_trac, poly_off, poly_idx, poly_xyz, poly_trac, trac,
                                            fric, summary, fric_summary, stiff, counts, totals); });
    int rc = surface_args(h, n_items, ins_ids, pose, twist, cap_poly, cap_trac, poly_off, poly_idx, poly_xyz, poly_trac, trac, summary, totals);
    if (rc == PFC_OK) rc = surface_fric_args(h, n_items, cap_trac, fric, fric_summary);
    if (rc != PFC_OK) return rc;
    SurfFricOut fo;
    fo.s = s; fo.fric = fric; fo.fric_summary = fric_summary; fo.stiff = stiff;
    return surface_host(h, n_items, ins_ids, pose, twist, cap_poly, cap_trac, poly_off, poly_idx, poly_xyz, poly_trac, trac, summary, counts, totals,
                        &fo);
}

// The device-pointer form of both surface calls; fo (pfc_contact_surface_fric_device) holds device pointers.
static int surface_device(pfc_context *h, int n_items, const int *d_ins_ids, const double *d_pose, const double *d_twist, long long cap_poly,
                          long long cap_trac, long long *d_poly_off, int *d_poly_idx, double *d_poly_xyz, long long *d_poly_trac,
                          double *d_trac, double *d_summary, int *d_counts, long long *d_totals, void *stream, const SurfFricOut *fo) {
    int rc = surface_args(h, n_items, d_ins_ids, d_pose, d_twist, cap_poly, cap_trac, d_poly_off, d_poly_idx, d_poly_xyz, d_poly_trac,
                          d_trac, d_summary, d_totals);
    if (rc == PFC_OK && fo) rc = surface_fric_args(h, n_items, cap_trac, fo->fric, fo->fric_summary);
    if (rc != PFC_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if (n_items == 0) {
        new_value_pass(h);
        forget_host_points(h);
        HIP_TRY(h, hipMemsetAsync(d_poly_off, 0, sizeof(long long), st));
        HIP_TRY(h, hipMemsetAsync(d_poly_trac, 0, sizeof(long long), st));
        HIP_TRY(h, hipMemsetAsync(d_totals, 0, sizeof(long long) * 2, st));
        return PFC_OK;
    }
    return surface_enqueue(h, n_items, d_ins_ids, d_pose, d_twist, cap_poly, cap_trac, d_poly_off, d_poly_idx, d_poly_xyz, d_poly_trac,
                           d_trac, d_summary, d_counts, d_totals, st, fo);
}

int pfc_contact_surface_device(pfc_handle h, int n_items, const int *d_ins_ids, const double *d_pose, const double *d_twist,
                               long long cap_poly, long long cap_trac, long long *d_poly_off, int *d_poly_idx, double *d_poly_xyz,
                               long long *d_poly_trac, double *d_trac, double *d_summary, int *d_counts, long long *d_totals, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    auto call = [&](pfc_context *c) {
        return surface_device(c, n_items, d_ins_ids, d_pose, d_twist, cap_poly, cap_trac, d_poly_off, d_poly_idx, d_poly_xyz, d_poly_trac, d_trac,
                              d_summary, d_counts, d_totals, stream, nullptr); };
    return h->multi ? surface_ctx(h, call) : call(h);
}

int pfc_contact_surface_fric_device(pfc_handle h, int n_items, const int *d_ins_ids, const double *d_pose, const double *d_twist,
                                    const double *d_s, long long cap_poly, long long cap_trac, long long *d_poly_off, int *d_poly_idx,
                                    double *d_poly_xyz, long long *d_poly_trac, double *d_trac, double *d_fric, double *d_summary,
                                    double *d_fric_summary, double *d_stiff, int *d_counts, long long *d_totals, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    SurfFricOut fo;
    fo.s = d_s; fo.fric = d_fric; fo.fric_summary = d_fric_summary; fo.stiff = d_stiff;
    auto call = [&](pfc_context *c) {
        return surface_device(c, n_items, d_ins_ids, d_pose, d_twist, cap_poly, cap_trac, d_poly_off, d_poly_idx, d_poly_xyz, d_poly_trac, d_trac,
                              d_summary, d_counts, d_totals, stream, &fo); };
    return h->multi ? surface_ctx(h, call) : call(h);
}

// Synchronise and judge the pending call: the single-device body of pfc_check, and what the debug readers drain with.
static int drain(pfc_context *h) {
    using P = pfc_context::Pending;
    const P p = h->pend;
    switch (p.kind) {
    case P::None: return PFC_OK;
    case P::Surface: return check_surface(h);
    case P::More:        // Dual passes on a value pass that was checked before: nothing to read back
        h->pend = {};
        HIP_TRY(h, hipStreamSynchronize(p.stream));
        if (h->h_more.p && (h->h_more.p[0] & kStHole)) {
            end_kept_pass(h);
            return fail(h, PFC_ERR_STATE, "internal error: a Dual pass on a reused value pass read a work-list slot out of range");
        }
        return PFC_OK;
    case P::Batched: case P::Fused: break;
    }
    // (no kept pass here: the value pass ended it; a Dual evaluation that rides on it records its own below once it is checked)
    int rc = check_eval(h);      // (Fused: the small-scene kernel's per-item words copied down, stream synchronised)
    switch (p.dual) {
    case P::NoDual: return rc;
    case P::DualHandOver:
        if (rc != PFC_OK || (h->stats[6] & kStCandOvf)) h->dual_dev_hyb_skip = 64;
        if (rc == PFC_OK) rc = dual_handover_fit(h, p.n_dir, p.dpcap);
        break;
    case P::DualBatched:      // contributing pairs: the counter next to the polygon total in the packed tail, which check_eval has just brought over
        if (rc == PFC_OK) rc = dual_spec_fit(h, p.n_dir, h->h_tail.p[tail_pairs(h->last_levels)], p.dpcap);
        break;
    }
    if (rc == PFC_OK) h->kept = {p.dual == P::DualHandOver ? pfc_context::KeptPass::HandOver : pfc_context::KeptPass::Batched, h->last_n_items, p.ids};
    return rc;
}

int pfc_check(pfc_handle h) {
    if (!h) return PFC_ERR_BAD_ARG;
    if (h->multi) {
        pfc_context *c0 = h->multi->shard[0];
        if (c0->pend.kind != pfc_context::Pending::Surface) return multi_check(h);
        (void)hipSetDevice(c0->device);
        return on_first_shard(h, check_surface);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    return drain(h);
}

// BAR-resident input blocks (pfc_context::bar_in): allocated on first use if the device has a large BAR.
constexpr size_t kBarItems = 4096;     // items whose value inputs go there: every evaluation whose kernels read them in place (kInPlaceItems)
constexpr size_t kBarKeys = 4096;      // (item, direction) pairs whose Dual seeds go there; the Dual kernels then read the seeds and write the partials in place
                                       // (48 box-on-plane scenes x 6 directions: a chunk 96 -> 82 us; 256 scenes 278 -> 250, 100 reduced blob/tool poses 318 -> 288:
                                       // scripts/variants/bar_keys_run.py, dual_in_place_limit_run.py); without a BAR block the in-place limit is 512 pairs
static bool bar_ready(pfc_context *h) {
    if (h->bar_state == 0) {
        h->bar_state = -1;
#if defined(__x86_64__)      // the ordering argument (a locked instruction drains the write-combining buffers) is x86's
        int large_bar = 0;
        if (!std::getenv("PFC_NO_BAR_INPUTS") && hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, h->device) == hipSuccess &&
            large_bar && h->bar_in.ensure_fine_grained(kBarItems * (36 * sizeof(double) + sizeof(int))) == hipSuccess &&
            h->bar_din.ensure_fine_grained(kBarKeys * 36 * sizeof(double)) == hipSuccess)
            h->bar_state = 1;
#endif
    }
    return h->bar_state == 1;
}
// After the host has filled a BAR-resident block: drain the core's write-combining buffers, so that the stores are posted
// before the doorbell write of the launch that reads them (PCIe keeps posted writes in order).  The runtime's locked
// queue-index update does the same; this makes the ordering independent of it.
static inline void bar_publish() {
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
    asm volatile("sfence" ::: "memory");
#endif
}
// The device-visible address of a pinned input block the host has just filled: its copy in BAR-resident device memory if it
// fits there (slot 0: value inputs, slot 1: Dual seeds), else the pinned block itself.  The pinned block stays the host's copy
// (the Dual paths compare the next call's inputs with it).  The caller ends its mirrors with one bar_publish().
static void bar_mirror(pfc_context *h, void **dev, const void *pinned, size_t bytes, int slot) {
    if (!bar_ready(h)) return;
    void *dst = slot == 0 ? h->bar_in.p : h->bar_din.p;
    const size_t cap = slot == 0 ? kBarItems * (36 * sizeof(double) + sizeof(int)) : kBarKeys * 36 * sizeof(double);
    if (bytes > cap) return;
    std::memcpy(dst, pinned, bytes);
    *dev = dst;
}

// Device-visible addresses of the four pinned blocks of a small-scene Dual evaluation the host has just filled, the input blocks
// through their BAR mirrors where they fit (bar_mirror), then one bar_publish.
struct PinnedDev { void *in = nullptr, *out = nullptr, *din = nullptr, *dout = nullptr; };
static int map_pinned(pfc_context *h, PinnedDev *v, size_t in_bytes, size_t din_bytes) {
    HIP_TRY(h, hipHostGetDevicePointer(&v->in, h->pin_in.p, 0));
    HIP_TRY(h, hipHostGetDevicePointer(&v->out, h->pin_out.p, 0));
    HIP_TRY(h, hipHostGetDevicePointer(&v->din, h->pin_din.p, 0));
    HIP_TRY(h, hipHostGetDevicePointer(&v->dout, h->pin_dout.p, 0));
    bar_mirror(h, &v->in, h->pin_in.p, in_bytes, 0);
    bar_mirror(h, &v->din, h->pin_din.p, din_bytes, 1);
    bar_publish();
    return PFC_OK;
}
// Seeds and partials of up to kBarKeys (item, direction) pairs (512 without a BAR block) are read and written in place by the
// Dual kernels; larger blocks are staged.
static bool dual_in_place(const pfc_context *h, size_t nk) { return nk <= (h->bar_state == 1 ? kBarKeys : (size_t)512); }

// pfc_eval on one device.  o: pose and list flag of a Dual evaluation's value pass (two-stage path); the pinned targets are set here.
static int eval_host(pfc_context *h, int n_items, const int *ins_ids, const double *pose, const double *twist,
                     const double *s, double *wrench, double *sdot, int *counts, PassOpts o) {
    if (!h->finalized) return fail(h, PFC_ERR_STATE, "pfc_eval before pfc_finalize");
    if (n_items < 0) return fail(h, PFC_ERR_BAD_ARG, "negative n_items");
    if (n_items == 0) return PFC_OK;
    if (!pose || !twist || !wrench || !sdot) return fail(h, PFC_ERR_BAD_ARG, "null buffer");
    HIP_TRY(h, hipSetDevice(h->device));
    forget_host_points(h);      // the pinned blocks are about to be overwritten
    const size_t n = (size_t)n_items;
    // one pinned block in (a value block), one pinned block out (tail | result block): two async copies around the launch
    // sequence and a single synchronisation.  The device side of the output block lives behind the packed tail in the same
    // buffer, so that the status / counters and the results come back together.
    const ValueBlock vs(nullptr, n); const ResultBlock rs(nullptr, n);      // (for their sizes)
    const size_t t0 = tail_prefix(h), back_bytes = t0 * sizeof(int) + rs.bytes();
    HIP_TRY(h, h->pin_in.ensure(vs.bytes(true)));
    // behind the outputs: the per-item words of the fused small-scene kernel
    HIP_TRY(h, h->pin_out.ensure(t0 * sizeof(int) + rs.bytes(n <= (size_t)kFusedMaxItems)));
    HIP_TRY(h, h->h_pose.ensure(doubles_for(vs.bytes(true))));      // device mirror of the input block
    HIP_TRY(h, ensure_graphed(h, h->tail, t0 + rs.bytes() / sizeof(int) + 4));   // only ever grows; ensure_work asks for less
    // (every evaluation whose kernels read the inputs in place, i.e. up to 512 items: 64 box-on-plane scenes 52.2 -> 48.7 us, C4's
    // 256 66.5 -> 64.5, 128 full-size poses on the batched path 333 -> 328; scripts/variants/bar_items_run.py)
    const bool bar = n <= kBarItems && !o.list && bar_ready(h);
    const ValueBlock pi(bar ? h->bar_in.p : h->pin_in.p, n);
    pack_values(pi, ins_ids, pose, twist, s);
    if (bar) bar_publish();
    hipStream_t st = h->stream;
    // A small scene (what a Radau stage evaluates) pays ~5 us per staging copy, more than the kernels spend on the data:
    // there the kernels read the inputs from, and write the results and the tail to, the pinned blocks directly.
    // (Up to 512 items while the inputs sat in host memory -- a kernel's reads over PCIe stop paying beyond that; with BAR-resident
    // inputs up to 4 096: C5 through host buffers 307 -> 282 us, 1 000 box-on-plane scenes 198 -> 178, 600 full-size poses
    // 635 -> 619, 2 048 unchanged; scripts/variants/zero_copy_limit_run.py.)
    const bool zero_copy = n_items <= (bar ? (int)kBarItems : 512) && !o.list;
    ValueBlock di(h->h_pose.p, n); ResultBlock dout(h->tail.p + t0, n);
    const ResultBlock po((int *)h->pin_out.p + t0, n);      // where the host reads the results
    if (zero_copy) {
        void *dpi = h->bar_in.p, *dpo = nullptr;
        if (!bar) HIP_TRY(h, hipHostGetDevicePointer(&dpi, h->pin_in.p, 0));
        HIP_TRY(h, hipHostGetDevicePointer(&dpo, h->pin_out.p, 0));
        di = ValueBlock(dpi, n);
        dout = ResultBlock((int *)dpo + t0, n);
        o.tail = (int *)dpo;      // k_final packs the tail, the small-scene kernel its per-item words, straight into the pinned block
        if (n <= (size_t)kFusedMaxItems) { o.fout = dout.fused_words(); o.fout_host = po.fused_words(); }
    } else {
        HIP_TRY(h, hipMemcpyAsync(di.p, pi.p, pi.bytes(ins_ids != nullptr), hipMemcpyHostToDevice, st));
    }
    int rc = PFC_OK;
    for (int attempt = 0; attempt < 40; ++attempt) {
        rc = eval_device(h, n_items, ins_ids ? di.ids() : nullptr, di.pose(), di.twist(), s ? di.s() : nullptr, dout.wrench(), dout.sdot(),
                         dout.counts(), st, o);
        if (rc != PFC_OK) return rc;
        if (!zero_copy && h->pend.kind != pfc_context::Pending::Fused) HIP_TRY(h, hipMemcpyAsync(h->pin_out.p, h->tail.p, back_bytes, hipMemcpyDeviceToHost, st));
        rc = check_eval(h, (const int *)h->pin_out.p, o.fout_host);      // one D2H copy carries the tail and the outputs
        if (rc != PFC_ERR_OVERFLOW) break;
    }
    if (rc != PFC_OK) return rc;
    copy_out(po, wrench, sdot, counts);
    return PFC_OK;
}

int pfc_eval(pfc_handle h, int n_items, const int *ins_ids, const double *pose, const double *twist,
             const double *s, double *wrench, double *sdot, int *counts) {
    if (!h) return PFC_ERR_BAD_ARG;
    if (h->multi) return multi_eval(h, n_items, ins_ids, pose, twist, s, wrench, sdot, counts);
    return eval_host(h, n_items, ins_ids, pose, twist, s, wrench, sdot, counts, PassOpts());
}

namespace {

// The Dual passes of one evaluation on stream st.  tail: the packed tail of the value pass (device-visible), dp/dt/dsd
// and dw/dsdot: seeds and results (device-visible), n_pairs_bound: upper bound of the contributing pairs used to size
// the kept Dual polygons (the kernels take the actual count from the tail and guard against the capacity).
int launch_dual(pfc_context *h, int n_items, int n_dir, const int *tail, const double *dp, const double *dt,
                const double *dsd, double *dw, double *dsdot, size_t n_pairs_bound, hipStream_t st, size_t *dpcap_out,
                bool acc_cleared = false, const int *pair_count = nullptr, unsigned *status_word = nullptr) {
    const size_t nk = (size_t)n_items * n_dir;
    HIP_TRY(h, ensure_graphed(h, h->dual_acc, nk * kDaStride));
    HIP_TRY(h, ensure_graphed(h, h->dual_res, nk * kDrStride));
    if (!acc_cleared) HIP_TRY(h, hipMemsetAsync(h->dual_acc.p, 0, sizeof(double) * nk * kDaStride, st));
    DualArgs a;
    a.items = h->items.p; a.cand = h->cand.p; a.ccount = tail + 12; a.ccap = (int)h->ccap;   // packed copy of the counters
    a.surv = h->surv.p; a.scount = tail + tail_pairs(h->last_levels);
    if (pair_count) a.ccount = a.scount = pair_count;       // hand-over from the fused small-scene kernel: one list, one count
    a.n_items = n_items; a.n_dir = n_dir; a.d_pose = dp; a.d_twist = dt; a.d_s = dsd; a.icnt = h->icnt.p;
    a.dacc = h->dual_acc.p; a.dres = h->dual_res.p; a.d_wrench = dw; a.d_sdot = dsdot;
    a.status = h->status.p;
    // Hand-over: the passes report into the word behind the pair count (cleared and read back with it).  The status word
    // of the batched value pass is read by its k_final only, so a flag raised here would surface in a later evaluation.
    if (pair_count) a.status = reinterpret_cast<unsigned *>(h->emit_ctr.p) + 2;
    if (status_word) a.status = status_word;       // the passes of a reused value pass: a word pfc_check reads back
    const int cpw = 64 / n_dir;
    const int grid = grid_for((n_pairs_bound + cpw - 1) / cpw, 1, 256 * 16);
    const int kgrid = grid_for(nk, 64, 1 << 20);
    const bool tt = h->any_tet_tet;
    // Dual polygons kept between the passes: a wave of k_narrow_dual owns 64 consecutive slots (no slot counter)
    // (option fixed_order: the bound also sizes the record list of the passes' sums, for every model -- the callers compare the pair count
    // with this capacity after their synchronisation and re-issue the passes when it was exceeded)
    const size_t dpcap = dual_poly_cap(h, n_dir, n_pairs_bound);
    HIP_TRY(h, ensure_graphed(h, h->dual_poly, dpcap * kDpFields));
    HIP_TRY(h, ensure_graphed(h, h->dual_pkey, dpcap));
    a.dpoly = h->dual_poly.p; a.dpoly_key = h->dual_pkey.p; a.dpcap = (long long)dpcap;
    if (dpcap_out) *dpcap_out = dpcap;
    // Scenes of many items: the passes walk only the contributing pairs of items this chunk seeds (pfc_dual.h, k_dual_select).
    // Two short launches; a small scene's chunk is a handful of waves either way and keeps its few launches.
    // (not while the stream is being captured -- the one-graph path of up to 512 items records these launches, and the
    // lists below may have to be allocated; a captured chunk keeps the per-key skip only)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap);
    // (nor under option fixed_order: the selected list is compacted block by block in the order the blocks come by)
    if (!pair_count && n_items >= kDualSelectMin && cap == hipStreamCaptureStatusNone && !h->opt_fixed_order && std::getenv("PFC_NO_SELECT") == nullptr) {
        HIP_TRY(h, ensure_graphed(h, h->dual_sel, h->ccap));
        HIP_TRY(h, ensure_graphed(h, h->dual_flag, (size_t)n_items + 1));
        int *selcount = h->dual_flag.p + n_items;
        hipLaunchKernelGGL(k_dual_flags, dim3(n_items), dim3(64), 0, st, a, h->dual_flag.p, selcount);
        // (grid from the list's capacity, not from n_pairs_bound: the first evaluation of a handle has no pair count to go by)
        hipLaunchKernelGGL(k_dual_select, dim3(grid_for(h->ccap, 256 * kSelRounds, 256 * 8)), dim3(256), 0, st, a, h->dual_flag.p,
                           h->dual_sel.p, selcount);
        a.surv = h->dual_sel.p; a.scount = selcount;
    }
    // Pass B folded into pass A wherever the value pass was the batched one (its cop is in h->res; DualArgs::vres) and the scene
    // is tri-tet: one read of the kept polygons less.  (Option "dual_fold", default 1; PFC_NO_DUAL_FOLD=1 for A/B runs.)
    static const bool no_fold = std::getenv("PFC_NO_DUAL_FOLD") != nullptr;
    a.vres = (h->any_bristle && !pair_count && !no_fold && !tt && h->opt_dual_fold) ? h->res.p : nullptr;
    // fixed_order: every key of an item decomposes the K of the VALUE pass (one clamp decision per item and evaluation)
    // (PFC_DUAL_VALUE_K=1: the same without the option, A/B.  It was the default for a day: the same six directions as first and as
    // further chunk of one value pass differ by O(1) on the four flat-patch pairs of config 5 without it and by 1e-2 .. 2e-1 with it,
    // and k_dual_eig saves its Jacobi iteration -- C5 further chunk 355 -> 346 us.  But the value pass forms K by two parallel-axis
    // shifts, the Dual passes sum about the cop directly as the reference does, and on flat patches the value pass's noise
    // eigenvalue lands on the other side of the clamp from the Dual oracle's often enough to fail an oracle comparison of d_sdot
    // in one run of four; the Dual sums' never did in some fifty suite runs.  Both are rounding noise; the default stays with
    // the arithmetic that is closer to the reference's.)
    static const bool value_k = std::getenv("PFC_DUAL_VALUE_K") != nullptr;
    a.vres_k = ((h->opt_fixed_order || value_k) && h->any_bristle && !pair_count) ? h->res.p : nullptr;
    static const bool no_stored_v = std::getenv("PFC_NO_DUAL_STORED_V") != nullptr;
    a.stored_v = no_stored_v ? 0 : 1;
    const bool fx = h->opt_fixed_order && !pair_count;
    a.sink_a = FixedSink{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, nullptr};
    a.sink_b = a.sink_a; a.sink_c = a.sink_a;
    if (fx) {
        // the contributing pairs in candidate order (k_integ_fixed appended them piece by piece as its workgroups came by) ...
        if (h->surv_sorted_serial != h->value_serial) {
            // (as many slots as the candidate sort covered: the contributing pairs are a subset of the candidates)
            HIP_TRY(h, pfc_sort_indices(h->surv.p, a.scount, (h->sort_cover_used && h->sort_cover_used < h->ccap) ? h->sort_cover_used : h->ccap,
                                        reinterpret_cast<unsigned *>(h->sort_keys[0].p),
                                        reinterpret_cast<unsigned *>(h->sort_keys[1].p), h->sort_tmp.p, h->sort_tmp.cap, st));
            h->surv_sorted_serial = h->value_serial;
        }
        // ... and the records of passes A and B: per accumulator block at most one per (wave, item, direction), and since an item's
        // pairs are consecutive in the sorted list the (wave, item) incidences are fewer than waves + items
        const size_t n_grp = (n_pairs_bound + cpw - 1) / cpw;
        // Three blocks (passes A, B, C), each with n_dir direct slots per wave position and a shared overflow area for the waves that
        // straddle items: (items - 1) n_dir records at most per block.
        const size_t n_pos = n_grp + 1, direct = n_pos * (size_t)n_dir;
        const size_t cap = 3 * direct + 3 * (size_t)n_dir * (size_t)n_items + 64;
        if (cap > ((size_t)1 << 30)) return fail(h, PFC_ERR_NOMEM, "option fixed_order: %zu Dual sum records: evaluate the batch in parts", cap);
        HIP_TRY(h, ensure_graphed(h, h->fx_rec, cap * kSinkStride));
        HIP_TRY(h, ensure_graphed(h, h->fx_head, 3 * nk + 2));
        HIP_TRY(h, hipMemsetAsync(h->fx_head.p, 0xFF, sizeof(int) * 3 * nk, st));
        HIP_TRY(h, hipMemsetAsync(h->fx_head.p + 3 * nk, 0, sizeof(int) * 2, st));
        a.sink_a = FixedSink{h->fx_rec.p, h->fx_head.p + 3 * nk, h->fx_head.p, 0, n_dir, (int)n_pos, (int)(3 * direct), (int)cap, a.status};
        a.sink_b = FixedSink{h->fx_rec.p, h->fx_head.p + 3 * nk, h->fx_head.p + nk, (int)direct, n_dir, (int)n_pos, (int)(3 * direct), (int)cap, a.status};
        a.sink_c = FixedSink{h->fx_rec.p, h->fx_head.p + 3 * nk, h->fx_head.p + 2 * nk, (int)(2 * direct), n_dir, (int)n_pos, (int)(3 * direct), (int)cap, a.status};
        if (!tt) a.vres = h->res.p;      // tri-tet: always the folded pass (one kernel carries both blocks)
    }
    if (fx) {
        if (tt) {
            if (dual_pv_stride(n_dir) == 16) hipLaunchKernelGGL((k_narrow_dual<true, 16, false, true>), dim3(grid), dim3(64), dual_lds_bytes(n_dir), st, a);
            else hipLaunchKernelGGL((k_narrow_dual<true, 64, false, true>), dim3(grid), dim3(64), dual_lds_bytes(n_dir), st, a);
        } else {
            if (dual_pv_stride(n_dir) == 16) hipLaunchKernelGGL((k_narrow_dual<false, 16, true, true>), dim3(grid), dim3(64), dual_lds_bytes(n_dir), st, a);
            else hipLaunchKernelGGL((k_narrow_dual<false, 64, true, true>), dim3(grid), dim3(64), dual_lds_bytes(n_dir), st, a);
        }
        hipLaunchKernelGGL(k_fixed_reduce, dim3((unsigned)nk), dim3(64), 0, st, a.sink_a, (int)nk, h->dual_acc.p, kDaStride, kDaA, 20);
        if (!tt) hipLaunchKernelGGL(k_fixed_reduce, dim3((unsigned)nk), dim3(64), 0, st, a.sink_b, (int)nk, h->dual_acc.p, kDaStride, kDaB, 42);
    } else if (a.vres) {
        if (dual_pv_stride(n_dir) == 16) hipLaunchKernelGGL((k_narrow_dual<false, 16, true>), dim3(grid), dim3(64), dual_lds_bytes(n_dir), st, a);
        else hipLaunchKernelGGL((k_narrow_dual<false, 64, true>), dim3(grid), dim3(64), dual_lds_bytes(n_dir), st, a);
    } else if (dual_pv_stride(n_dir) == 16) {
        if (tt) hipLaunchKernelGGL((k_narrow_dual<true, 16>), dim3(grid), dim3(64), dual_lds_bytes(n_dir), st, a);
        else hipLaunchKernelGGL((k_narrow_dual<false, 16>), dim3(grid), dim3(64), dual_lds_bytes(n_dir), st, a);
    } else {
        if (tt) hipLaunchKernelGGL((k_narrow_dual<true, 64>), dim3(grid), dim3(64), dual_lds_bytes(n_dir), st, a);
        else hipLaunchKernelGGL((k_narrow_dual<false, 64>), dim3(grid), dim3(64), dual_lds_bytes(n_dir), st, a);
    }
    // a few dozen kept polygons only (pencil-scale pair: 116 -> 103 us per chunk): with more, the eightfold number of
    // waves costs more in per-key atomics on the same few rows than the shorter walk saves (single C3 pose: 97 -> 113 us)
    a.tri_split = (h->any_bristle && dpcap * 8 <= 16384 && !fx) ? 1 : 0;
    if (h->any_bristle) {
        const int pgrid = grid_for(dpcap * (a.tri_split ? 8 : 1), 64, 256 * 16);
        if (fx && !a.vres) {
            hipLaunchKernelGGL((k_dual_poly<1, true>), dim3(pgrid), dim3(64), 0, st, a);
            hipLaunchKernelGGL(k_fixed_reduce, dim3((unsigned)nk), dim3(64), 0, st, a.sink_b, (int)nk, h->dual_acc.p, kDaStride, kDaB, 42);
        } else if (!a.vres) hipLaunchKernelGGL((k_dual_poly<1>), dim3(pgrid), dim3(64), 0, st, a);
        hipLaunchKernelGGL(k_dual_eig, dim3((unsigned)nk), dim3(64), 0, st, a);   // one wave per (item, direction)
        if (fx) {
            hipLaunchKernelGGL((k_dual_poly<2, true>), dim3(pgrid), dim3(64), 0, st, a);
            hipLaunchKernelGGL(k_fixed_reduce, dim3((unsigned)nk), dim3(64), 0, st, a.sink_c, (int)nk, h->dual_acc.p, kDaStride, kDaC, 12);
        } else hipLaunchKernelGGL((k_dual_poly<2>), dim3(pgrid), dim3(64), 0, st, a);
    }
    hipLaunchKernelGGL(k_dual_final, dim3(kgrid), dim3(64), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    return PFC_OK;
}

// A null d_ds of nk (item, direction) pairs becomes the handle's block of zeros (cleared on st when it is new).
hipError_t zero_ds(pfc_context *h, size_t nk, const double **d_ds, hipStream_t st) {
    if (*d_ds) return hipSuccess;
    bool moved = false;
    hipError_t e = h->dual_zero.ensure(nk * 6, &moved);
    if (e == hipSuccess && moved) e = hipMemsetAsync(h->dual_zero.p, 0, sizeof(double) * h->dual_zero.cap, st);
    *d_ds = h->dual_zero.p;
    return e;
}

// A host-pointer Dual call: the arguments of pfc_eval_dual_bp, checked; bp_pose is the device-visible pinned block (or null).
struct DualCall {
    int n_items, n_dir;
    const int *ins_ids;
    const double *pose, *twist, *s, *d_pose, *d_twist, *d_s;
    double *wrench, *sdot, *d_wrench, *d_sdot;
    int *counts;
    const double *bp_pose;
    size_t n() const { return (size_t)n_items; }
    size_t nk() const { return (size_t)n_items * n_dir; }
    void deliver(ResultBlock res, PartialBlock part) const { copy_out(res, wrench, sdot, counts); copy_out_dual(part, d_wrench, d_sdot); }
};

// The Dual passes alone, on the value pass a host route kept (its lists and item records on the device, its results in the
// pinned block `res`): tail and pair_count as launch_dual takes them, levels locates the pair counter in the tail.  The pair
// count is known exactly, so there is no speculation to check.  dev_seeds / dev_part: where the kernels read and write; when
// not in_place they are staged from pin_din and to pin_dout.
int dual_on_kept_pass(pfc_context *h, const DualCall &c, const int *tail, const int *pair_count, int levels, bool in_place,
                      SeedBlock dev_seeds, PartialBlock dev_part, ResultBlock res) {
    const size_t nk = c.nk();
    hipStream_t st = h->stream;
    HIP_TRY(h, ensure_graphed(h, h->dual_acc, nk * kDaStride));
    HIP_TRY(h, hipMemsetAsync(h->dual_acc.p, 0, sizeof(double) * nk * kDaStride, st));
    if (!in_place) HIP_TRY(h, hipMemcpyAsync(dev_seeds.p, h->pin_din.p, dev_seeds.bytes(), hipMemcpyHostToDevice, st));
    h->last_levels = levels;
    const int rc = launch_dual(h, c.n_items, c.n_dir, tail, dev_seeds.d_pose(), dev_seeds.d_twist(), dev_seeds.d_s(), dev_part.d_wrench(),
                               dev_part.d_sdot(), dual_exact_bound(h), st, nullptr, true, pair_count);
    if (rc != PFC_OK) return rc;
    if (!in_place) HIP_TRY(h, hipMemcpyAsync(h->pin_dout.p, dev_part.p, dev_part.bytes(), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    c.deliver(res, PartialBlock(h->pin_dout.p, nk));
    h->last_dual_reused = true;
    return PFC_OK;
}

// Smallest scenes, all instructions regularized (test/boxes.jl and the like): value AND Dual passes inside the fused
// small-scene kernel -- one launch, results polled from pinned memory.  Returns PFC_ERR_OVERFLOW when an item does not fit
// (too many candidates / polygons): the caller takes the batched Dual path and this one stays off for a while.
int eval_dual_fused(pfc_context *h, const DualCall &c) {
    h->pin_din_pt = {};    // these pinned blocks are about to be reused
    const size_t n = c.n(), nk = c.nk();
    const ValueBlock vs(nullptr, n); const ResultBlock rs(nullptr, n); const SeedBlock ss(nullptr, nk); const PartialBlock ps(nullptr, nk);
    HIP_TRY(h, h->pin_in.ensure(vs.bytes(true))); HIP_TRY(h, h->pin_out.ensure(rs.bytes(true) + 64));
    HIP_TRY(h, h->pin_din.ensure(ss.bytes(false))); HIP_TRY(h, h->pin_dout.ensure(ps.bytes()));
    const ValueBlock pi(h->pin_in.p, n); const ResultBlock po(h->pin_out.p, n);
    pack_values(pi, c.ins_ids, c.pose, c.twist, c.s);
    pack_seeds(SeedBlock(h->pin_din.p, nk), c.d_pose, c.d_twist, nullptr, false);
    PinnedDev v;
    { const int rc = map_pinned(h, &v, vs.bytes(true), ss.bytes(false)); if (rc != PFC_OK) return rc; }
    const ValueBlock di(v.in, n); const ResultBlock dout(v.out, n); const SeedBlock ddi(v.din, nk); const PartialBlock ddo(v.dout, nk);
    PassOpts o = {c.bp_pose};
    o.fout = dout.fused_words(); o.fout_host = po.fused_words();
    o.n_dir = c.n_dir; o.d_pose = ddi.d_pose(); o.d_twist = ddi.d_twist(); o.d_wrench = ddo.d_wrench(); o.d_sdot = ddo.d_sdot();
    int rc = enqueue_fused(h, c.n_items, c.ins_ids ? di.ids() : nullptr, di.pose(), di.twist(), c.s ? di.s() : nullptr,
                           dout.wrench(), dout.sdot(), dout.counts(), h->stream, o);
    if (rc == PFC_OK) rc = check_eval(h, nullptr, o.fout_host);
    if (rc != PFC_OK) return rc;
    c.deliver(po, PartialBlock(h->pin_dout.p, nk));
    h->pin_in_pt = {c.n_items, c.ins_ids != nullptr, h->value_serial, pi.ids_at};     // a repeat of this point goes to the hybrid path
    return PFC_OK;
}

// What the hybrid and the one-graph route share.  prepare(): their four pinned blocks sized (the results res_at ints into pin_out,
// out_bytes in all); the reuse test -- the chunks of one Jacobian: value inputs bitwise equal to those still in the pinned input
// block, and the pass `kind` kept -> only the Dual passes run; values (unless reused) and seeds packed; the device-visible views,
// seeds and partials in place (dual_in_place) or through dual_in / dual_out.
struct SmallDual {
    bool same = false, in_place = true;
    PinnedDev v;
    ValueBlock di{nullptr, 0};
    ResultBlock dout{nullptr, 0}, po{nullptr, 0};      // the results as the device and as the host see them
    SeedBlock ddi{nullptr, 0};
    PartialBlock ddo{nullptr, 0};
    int prepare(pfc_context *h, const DualCall &c, pfc_context::KeptPass::Kind kind, size_t res_at, size_t out_bytes, bool list) {
        const size_t n = c.n(), nk = c.nk();
        const ValueBlock vs(nullptr, n); const SeedBlock ss(nullptr, nk); const PartialBlock ps(nullptr, nk);
        bool in_moved, out_moved;
        HIP_TRY(h, h->pin_in.ensure(vs.bytes(true), &in_moved)); HIP_TRY(h, h->pin_out.ensure(out_bytes, &out_moved));
        if (in_moved || out_moved) end_kept_pass(h);      // reallocated: the cached blocks are gone
        HIP_TRY(h, h->pin_din.ensure(ss.bytes())); HIP_TRY(h, h->pin_dout.ensure(ps.bytes()));
        const ValueBlock pi(h->pin_in.p, n);
        po = ResultBlock((int *)h->pin_out.p + res_at, n);
        same = h->opt_dual_reuse && h->kept.kind == kind && h->kept.n == c.n_items && h->kept.ids == (c.ins_ids != nullptr) &&
               same_point(pi, c.ins_ids, c.pose, c.twist, c.s, true);
        if (!same) {
            end_kept_pass(h);
            HIP_TRY(h, ensure_work(h, c.n_items, list));      // (not before a reuse: option poison refills the work lists there)
            pack_values(pi, c.ins_ids, c.pose, c.twist, c.s);
        }
        pack_seeds(SeedBlock(h->pin_din.p, nk), c.d_pose, c.d_twist, c.d_s, true);
        { const int rc = map_pinned(h, &v, vs.bytes(true), ss.bytes()); if (rc != PFC_OK) return rc; }
        di = ValueBlock(v.in, n);
        dout = ResultBlock((int *)v.out + res_at, n);
        in_place = dual_in_place(h, nk);
        if (!in_place) { HIP_TRY(h, ensure_graphed(h, h->dual_in, ss.doubles())); HIP_TRY(h, ensure_graphed(h, h->dual_out, ps.doubles())); }
        ddi = SeedBlock(in_place ? v.din : h->dual_in.p, nk);
        ddo = PartialBlock(in_place ? v.dout : h->dual_out.p, nk);
        return PFC_OK;
    }
};

// Small scenes the in-kernel Dual passes do not take (bristle items, many polygons per item): the fused kernel evaluates
// the values and hands the item records, counters and the list of candidates with a polygon to the batched Dual passes
// (k_narrow_dual ..., many workgroups), enqueued right behind it; one synchronisation.  Returns PFC_ERR_OVERFLOW when an
// item does not fit the fused kernel or the speculative size of the kept Dual polygons fell short (the caller then takes
// the batched paths).
int eval_dual_hybrid(pfc_context *h, const DualCall &c) {
    h->pin_din_pt = {};    // these pinned blocks are about to be reused
    const int n_items = c.n_items, n_dir = c.n_dir;
    const size_t nk = c.nk();
    SmallDual b;
    { const int rc = b.prepare(h, c, pfc_context::KeptPass::Hybrid, 0, ResultBlock(nullptr, c.n()).bytes(true) + 64, false); if (rc != PFC_OK) return rc; }
    HIP_TRY(h, h->emit_ctr.ensure(4)); HIP_TRY(h, h->h_emit.ensure(4));
    hipStream_t st = h->stream;
    // a repeat: the lists and item records the fused kernel handed over are still there
    if (b.same) return dual_on_kept_pass(h, c, h->tail.p, h->emit_ctr.p, h->last_levels, b.in_place, b.ddi, b.ddo, b.po);
    if (!b.in_place) HIP_TRY(h, hipMemcpyAsync(b.ddi.p, h->pin_din.p, b.ddi.bytes(), hipMemcpyHostToDevice, st));
    const size_t bound = dual_spec_bound(h->dual_hint, 64);
    HIP_TRY(h, ensure_graphed(h, h->dual_acc, nk * kDaStride));
    HIP_TRY(h, hipMemsetAsync(h->dual_acc.p, 0, sizeof(double) * nk * kDaStride, st));
    HIP_TRY(h, hipMemsetAsync(h->emit_ctr.p, 0, sizeof(int) * 4, st));
    PassOpts o = {c.bp_pose};
    o.emit = true; o.fout = b.dout.fused_words();      // (no words to poll: this path synchronises, the Dual kernels run behind the fused one)
    int rc = enqueue_fused(h, n_items, c.ins_ids ? b.di.ids() : nullptr, b.di.pose(), b.di.twist(), c.s ? b.di.s() : nullptr,
                           b.dout.wrench(), b.dout.sdot(), b.dout.counts(), st, o);
    if (rc != PFC_OK) return rc;
    size_t dpcap = 0;
    h->last_levels = eff_levels(h);
    rc = launch_dual(h, n_items, n_dir, h->tail.p, b.ddi.d_pose(), b.ddi.d_twist(), b.ddi.d_s(), b.ddo.d_wrench(), b.ddo.d_sdot(), bound, st, &dpcap,
                     true, h->emit_ctr.p);
    if (rc != PFC_OK) return rc;
    if (!b.in_place) HIP_TRY(h, hipMemcpyAsync(h->pin_dout.p, b.ddo.p, b.ddo.bytes(), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(h->h_emit.p, h->emit_ctr.p, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
    // check_fused would poll; here the stream is synchronised (the completion words of the fused kernel are long written)
    HIP_TRY(h, hipStreamSynchronize(st));
    rc = check_eval(h, nullptr, b.po.fused_words());
    if (rc == PFC_OK) rc = dual_handover_fit(h, n_dir, dpcap);
    if (rc != PFC_OK) return rc;
    c.deliver(b.po, PartialBlock(h->pin_dout.p, nk));
    h->kept = {pfc_context::KeptPass::Hybrid, n_items, c.ins_ids != nullptr};
    h->pin_in_pt = {n_items, c.ins_ids != nullptr, h->value_serial, b.di.ids_at};
    return PFC_OK;
}

// Small scenes (what Radau evaluates): value pass and Dual passes enqueued back to back, ONE synchronisation, no
// staging copies (the kernels read and write the pinned blocks), the kept Dual polygons sized from the previous Dual
// evaluation's pair count.  Returns PFC_ERR_OVERFLOW when the speculation or a work list fell short: the caller then
// takes the two-stage path, which sizes everything from the value pass.
int eval_dual_small(pfc_context *h, const DualCall &c) {
    forget_host_points(h);    // these pinned blocks are about to be reused
    const int n_items = c.n_items, n_dir = c.n_dir;
    const size_t nk = c.nk(), t0 = tail_prefix(h);      // the results sit behind the packed tail
    SmallDual b;
    { const int rc = b.prepare(h, c, pfc_context::KeptPass::OneGraph, t0, t0 * sizeof(int) + ResultBlock(nullptr, c.n()).bytes(), true); if (rc != PFC_OK) return rc; }
    hipStream_t st = h->stream;
    // One captured graph: accumulator fill, the value pass, the Dual passes.  (Launched eagerly behind the replayed value
    // graph, the Dual kernels started 9 us late.)  The capacity of the kept Dual polygons is a power of two above twice
    // the previous pair count, so that the graph survives the small changes from one evaluation to the next.
    const size_t bound = dual_spec_bound(h->dual_hint, 64);
    const PassOpts o = {c.bp_pose, true, (int *)b.v.out};      // the value pass lists the contributing candidates and packs its tail into the pinned output block
    HIP_TRY(h, ensure_graphed(h, h->dual_acc, nk * kDaStride));
    HIP_TRY(h, ensure_graphed(h, h->dual_res, nk * kDrStride));
    const size_t dpcap = dual_poly_cap(h, n_dir, bound);
    HIP_TRY(h, ensure_graphed(h, h->dual_poly, dpcap * kDpFields));
    HIP_TRY(h, ensure_graphed(h, h->dual_pkey, dpcap));
    const int levels = eff_levels(h);
    const int L = bfs_levels_for(h, n_items, levels, o.half);
    // a repeat: eager launches of the Dual passes on the value pass the last graph replay left (lists, item records, the packed
    // tail in the pinned output block)
    if (b.same) return dual_on_kept_pass(h, c, (const int *)b.v.out, nullptr, levels, b.in_place, b.ddi, b.ddo, b.po);
    // (seed and partial blocks larger than the kernels take in place are copied by memcpy nodes of the graph: reading 288 B per
    // pair over PCIe from inside k_narrow_dual stops paying)
    const ValueBlock &di = b.di; const ResultBlock &dout = b.dout; const SeedBlock &ddi = b.ddi; const PartialBlock &ddo = b.ddo;
    const int *d_ins = c.ins_ids ? di.ids() : nullptr;
    const double *d_sv = c.s ? di.s() : nullptr;
    pfc_context::DualGraphKey key = {};
    key.v.n_items = n_items; key.v.levels = levels; key.v.L = L; key.v.debug = 0;
    key.v.bristle = (h->any_bristle ? 1 : 0) | (h->any_tet_tet ? 2 : 0) | (h->any_regularized ? 4 : 0) | (h->all_rule2 ? 8 : 0); key.v.surv = 1;
    key.v.p[0] = d_ins; key.v.p[1] = di.pose(); key.v.p[2] = di.twist(); key.v.p[3] = d_sv; key.v.p[4] = dout.wrench();
    key.v.p[5] = dout.sdot(); key.v.p[6] = dout.counts(); key.v.p[7] = o.tail; key.v.p[8] = o.bp_pose; key.v.stream = (void *)st; key.v.epoch = h->epoch;
    key.n_dir = n_dir; key.bound = bound; key.din = ddi.p; key.dout = ddo.p;
    h->last_levels = levels;      // launch_dual locates the pair counter in the tail by it
    int rc = PFC_OK;
    if (!h->dghave || std::memcmp(&key, &h->dgkey, sizeof key) != 0) {
        h->dgexec.reset();
        h->dghave = false;
        hipGraph_t graph = nullptr;
        hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
        if (e == hipSuccess) {
            e = hipMemsetAsync(h->dual_acc.p, 0, sizeof(double) * nk * kDaStride, st);
            if (!b.in_place && e == hipSuccess) e = hipMemcpyAsync(ddi.p, h->pin_din.p, ddi.bytes(), hipMemcpyHostToDevice, st);
            rc = record_eval(h, n_items, d_ins, di.pose(), di.twist(), d_sv, dout.wrench(), dout.sdot(), dout.counts(), st, false, o);
            if (rc == PFC_OK)
                rc = launch_dual(h, n_items, n_dir, (const int *)b.v.out, ddi.d_pose(), ddi.d_twist(), ddi.d_s(), ddo.d_wrench(), ddo.d_sdot(), bound,
                                 st, nullptr, true);
            if (!b.in_place && rc == PFC_OK && e == hipSuccess)
                e = hipMemcpyAsync(h->pin_dout.p, ddo.p, ddo.bytes(), hipMemcpyDeviceToHost, st);
            const hipError_t e2 = hipStreamEndCapture(st, &graph);
            if (e == hipSuccess) e = e2;
        }
        if (rc == PFC_OK && e == hipSuccess) e = hipGraphInstantiate(h->dgexec.put(), graph, nullptr, nullptr, 0);
        if (graph) (void)hipGraphDestroy(graph);
        if (rc != PFC_OK) return rc;
        if (e != hipSuccess) return fail(h, PFC_ERR_HIP, "Dual graph capture failed: %s", hipGetErrorString(e));
        h->dgkey = key; h->dghave = true;
    }
    new_value_pass(h);      // the replay overwrites the device state
    h->last_dual_reused = false;
    HIP_TRY(h, hipGraphLaunch(h->dgexec, st));
    h->last_bfs_levels = L; h->last_n_items = n_items; h->pend = {pfc_context::Pending::Batched, st}; h->ev_valid = false;
    const int *tail = (const int *)h->pin_out.p;
    rc = check_eval(h, tail);           // the one synchronisation; grows the work lists on overflow
    // did the kept Dual polygons fit?  (contributing pairs: the counter next to the polygon total in the packed tail)
    if (rc == PFC_OK) rc = dual_spec_fit(h, n_dir, tail[tail_pairs(h->last_levels)], dpcap);
    if (rc != PFC_OK) return rc;
    c.deliver(b.po, PartialBlock(h->pin_dout.p, nk));
    h->kept = {pfc_context::KeptPass::OneGraph, n_items, c.ins_ids != nullptr};
    return PFC_OK;
}

// Larger batches.  One synchronisation: inputs up in one pinned block, pfc_eval_dual_device (value pass + Dual passes back to
// back, kept Dual polygons sized from the previous evaluation), results down in one pinned block, pfc_check.  A work list
// that overflowed or a speculation that fell short re-issues the evaluation (buffers have grown).
int eval_dual_one_sync(pfc_context *h, const DualCall &c) {
    const int n_items = c.n_items, n_dir = c.n_dir;
    const size_t n = c.n(), nk = c.nk();
    const bool ids = c.ins_ids != nullptr;
    hipStream_t st = h->stream;
    const OneSyncIn is(nullptr, n, nk); const OneSyncOut os(nullptr, n, nk);      // (for their sizes)
    {
        bool in_moved, out_moved;
        HIP_TRY(h, h->pin_din.ensure(is.bytes(true), &in_moved));
        HIP_TRY(h, h->pin_dout.ensure(os.bytes(), &out_moved));
        if (in_moved || out_moved) h->pin_din_pt = {};      // reallocated: the cached blocks are gone
    }
    HIP_TRY(h, ensure_graphed(h, h->dual_in, doubles_for(is.bytes(true))));
    HIP_TRY(h, ensure_graphed(h, h->dual_out, doubles_for(os.bytes())));
    const OneSyncIn pin(h->pin_din.p, n, nk), din(h->dual_in.p, n, nk);
    const OneSyncOut pout(h->pin_dout.p, n, nk), dout(h->dual_out.p, n, nk);
    const SeedBlock dd = din.seeds(); const PartialBlock ddo = dout.partials();
    // Further seed directions at the point of the previous Dual evaluation (the chunks of one Jacobian: Radau calls
    // the path ceil(NX / N_chunk) times with the same values and different partials, src/radau/radau_functions.jl:2-14):
    // if the value inputs equal, bit for bit, those still sitting in the pinned input block, the value pass on the
    // device is reused -- candidates, contributing pairs, per-item results -- and only the Dual passes run.
    // (the device lists must be those of the evaluation the pinned block belongs to: a pfc_eval_dual_device + pfc_check of
    // the caller's own in between keeps a pass of ITS point -- the serial tells the two apart)
    const auto &pt = h->pin_din_pt;
    const bool same = h->opt_dual_reuse && h->device_kept() && h->kept.n == n_items && pt.n == n_items && pt.serial == h->value_serial &&
                      pt.ids == ids && h->dual_counts_cache.size() == n * 4 &&
                      same_point(ValueBlock(pin.p, n, pt.ids_at), c.ins_ids, c.pose, c.twist, c.s, true);
    if (same) {
        // the seeds go behind the value block as before; the ids move behind them (another n_dir: another place), the results
        // stay in front of the output block and the counters, whose place moves too, come from the cache
        pack_seeds(pin.seeds(), c.d_pose, c.d_twist, c.d_s, true);
        if (ids) std::memcpy(pin.values().ids(), c.ins_ids, sizeof(int) * n);
        h->pin_din_pt.ids_at = pin.values().ids_at;
        HIP_TRY(h, hipMemcpyAsync(dd.p, pin.seeds().p, dd.bytes(), hipMemcpyHostToDevice, st));
        int rc = pfc_eval_dual_device_more(h, n_dir, dd.d_pose(), dd.d_twist(), dd.d_s(), ddo.d_wrench(), ddo.d_sdot(), st);
        if (rc != PFC_OK) return rc;
        HIP_TRY(h, hipMemcpyAsync(pout.partials().p, ddo.p, ddo.bytes(), hipMemcpyDeviceToHost, st));
        rc = pfc_check(h);
        if (rc != PFC_OK) return rc;
        copy_out(ResultBlock(pout.p, n), c.wrench, c.sdot, nullptr);
        if (c.counts) std::memcpy(c.counts, h->dual_counts_cache.data(), sizeof(int) * h->dual_counts_cache.size());
        copy_out_dual(pout.partials(), c.d_wrench, c.d_sdot);
        return PFC_OK;
    }
    h->pin_din_pt = {};
    pack_values(pin.values(), c.ins_ids, c.pose, c.twist, c.s);
    pack_seeds(pin.seeds(), c.d_pose, c.d_twist, c.d_s, true);
    HIP_TRY(h, hipMemcpyAsync(din.p, pin.p, pin.bytes(ids), hipMemcpyHostToDevice, st));
    const ValueBlock di = din.values(); const ResultBlock dr = dout.results();
    int rc = PFC_OK;
    for (int attempt = 0; attempt < 40; ++attempt) {
        rc = pfc_eval_dual_device_bp(h, n_items, n_dir, ids ? di.ids() : nullptr, di.pose(), c.bp_pose, di.twist(), c.s ? di.s() : nullptr,
                                     dd.d_pose(), dd.d_twist(), dd.d_s(), dr.wrench(), dr.sdot(), ddo.d_wrench(), ddo.d_sdot(), dr.counts(), st);
        if (rc != PFC_OK) return rc;
        HIP_TRY(h, hipMemcpyAsync(pout.p, dout.p, pout.bytes(), hipMemcpyDeviceToHost, st));
        rc = pfc_check(h);
        if (rc != PFC_ERR_OVERFLOW) break;
    }
    if (rc != PFC_OK) return rc;
    c.deliver(pout.results(), pout.partials());
    // what a following call at the same point needs: the counters (the pinned blocks keep the rest)
    const int *pc = pout.results().counts();
    h->dual_counts_cache.assign(pc, pc + n * 4);
    h->pin_din_pt = {n_items, ids, h->value_serial, pin.values().ids_at};
    return PFC_OK;
}

// Option debug, or PFC_DUAL_TWO_STAGE set for A/B runs: values, candidate list and per-item counters by the ordinary evaluation
// (the broadphase ignores partials, src/contact_algorithms_non_friction.jl:95), read the contributing-pair count, then the
// Dual passes: one pinned seed block up, one partial block down, as in pfc_eval (whose staging buffers are free again by then).
int eval_dual_two_stage(pfc_context *h, const DualCall &c) {
    const size_t nk = c.nk();
    hipStream_t st = h->stream;
    PassOpts o = {c.bp_pose, true};      // the value pass lists the contributing candidates
    int rc = eval_host(h, c.n_items, c.ins_ids, c.pose, c.twist, c.s, c.wrench, c.sdot, c.counts, o);
    if (rc != PFC_OK) return rc;
    const SeedBlock ss(nullptr, nk); const PartialBlock ps(nullptr, nk);
    HIP_TRY(h, ensure_graphed(h, h->dual_in, ss.doubles()));
    HIP_TRY(h, ensure_graphed(h, h->dual_acc, nk * kDaStride));
    HIP_TRY(h, ensure_graphed(h, h->dual_res, nk * kDrStride));
    HIP_TRY(h, ensure_graphed(h, h->dual_out, ps.doubles()));
    HIP_TRY(h, h->pin_in.ensure(ss.bytes())); HIP_TRY(h, h->pin_out.ensure(ps.bytes()));
    const SeedBlock dd(h->dual_in.p, nk); const PartialBlock ddo(h->dual_out.p, nk);
    pack_seeds(SeedBlock(h->pin_in.p, nk), c.d_pose, c.d_twist, c.d_s, true);
    HIP_TRY(h, hipMemcpyAsync(dd.p, h->pin_in.p, ss.bytes(), hipMemcpyHostToDevice, st));
    rc = launch_dual(h, c.n_items, c.n_dir, h->tail.p, dd.d_pose(), dd.d_twist(), dd.d_s(), ddo.d_wrench(), ddo.d_sdot(), (size_t)h->stats[2], st, nullptr);
    if (rc != PFC_OK) return rc;
    h->dual_hint = h->stats[2];
    HIP_TRY(h, hipMemcpyAsync(h->pin_out.p, ddo.p, ps.bytes(), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    copy_out_dual(PartialBlock(h->pin_out.p, nk), c.d_wrench, c.d_sdot);
    return PFC_OK;
}

// Which route takes a call, asked in this order; a route that returns PFC_ERR_OVERFLOW hands the call to the next.  The
// environment variables are read on every call (tests and A/B runs flip them in a running process).
// Fused: no bristle item, and not a repeat of the previous small-scene point (the all-in-one kernel keeps nothing; the hybrid
// route hands lists over that the chunks after it reuse).
bool takes_fused(const pfc_context *h, const DualCall &c, bool repeat) {
    return !h->any_bristle && fused_ok(h, c.n_items, PassOpts{c.bp_pose}) && !repeat;
}
// Hybrid: also the first choice of pfc_eval_dual_device, for device buffers.
bool takes_hybrid(const pfc_context *h, int n_items, size_t nk, const PassOpts &o) {
    return fused_ok(h, n_items, o) && nk <= 4096 && (h->dual_hint >= 0 || !h->any_bristle) && std::getenv("PFC_NO_HYBRID") == nullptr;
}
// One graph: up to 512 items once a Dual evaluation has left a pair count to size the kept polygons from.
bool takes_small(const pfc_context *h, const DualCall &c) {
    return c.n_items <= 512 && c.nk() <= 4096 && h->dual_hint >= 0 && !h->opt_debug && !h->opt_fixed_order &&
           !(h->opt_split_min > 0 && c.n_items >= h->opt_split_min);
}
bool takes_one_sync(const pfc_context *h) { return !h->opt_debug && std::getenv("PFC_DUAL_TWO_STAGE") == nullptr; }
}  // namespace

int pfc_eval_dual_device_bp(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const double *d_pose, const double *d_bp_pose,
                            const double *d_twist, const double *d_s, const double *d_dpose, const double *d_dtwist,
                            const double *d_ds, double *d_wrench, double *d_sdot, double *d_dwrench, double *d_dsdot,
                            int *d_counts, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    if (h->multi)
        return multi_eval_device(h, n_items, n_dir, d_ins_ids, d_pose, d_bp_pose, d_twist, d_s, d_dpose, d_dtwist, d_ds, d_wrench, d_sdot,
                                 d_dwrench, d_dsdot, d_counts, stream);
    if (n_dir < 1 || n_dir > 16) return fail(h, PFC_ERR_BAD_ARG, "pfc_eval_dual_device: n_dir must be in 1..16");
    { const int rc = check_eval_args(h, n_items, d_ins_ids, d_pose, d_twist, d_s, d_wrench, d_sdot); if (rc != PFC_OK) return rc; }
    drop_pending(h);
    end_kept_pass(h);
    if (n_items == 0) { h->last_n_items = 0; return PFC_OK; }
    if (!d_dpose || !d_dtwist || !d_dwrench || !d_dsdot) return fail(h, PFC_ERR_BAD_ARG, "pfc_eval_dual_device: null buffer");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const size_t nk = (size_t)n_items * n_dir;
    // Kept Dual polygons are sized WITHOUT reading the value pass back: twice the contributing pairs of the previous Dual
    // evaluation (a power of two, so that the buffers settle), a guess the first time.  pfc_check compares the actual
    // count with the capacity after the one synchronisation and asks for a re-issue if it fell short.
    size_t bound = dual_spec_bound(h->dual_hint, 4096);
    while (bound < (size_t)n_items * 8) bound *= 2;
    HIP_TRY(h, ensure_graphed(h, h->dual_acc, nk * kDaStride));
    HIP_TRY(h, ensure_graphed(h, h->dual_res, nk * kDrStride));
    HIP_TRY(h, zero_ds(h, nk, &d_ds, st));
    HIP_TRY(h, hipMemsetAsync(h->dual_acc.p, 0, sizeof(double) * nk * kDaStride, st));
    // Small scenes: the value pass in the one-workgroup-per-item kernel, which hands item records and lists to the batched
    // Dual passes (what pfc_eval_dual does for host buffers, eval_dual_hybrid).  A miss (an item that does not fit, a
    // hand-over list or a speculation that fell short) is reported by pfc_check as PFC_ERR_OVERFLOW and the re-issue takes
    // the batched value pass below.
    PassOpts o = {d_bp_pose};
    if (takes_hybrid(h, n_items, nk, o)) {
        if (h->dual_dev_hyb_skip > 0) {
            --h->dual_dev_hyb_skip;
        } else {
            HIP_TRY(h, ensure_work(h, n_items, false));
            HIP_TRY(h, h->emit_ctr.ensure(4));
            HIP_TRY(h, h->h_emit.ensure(4));
            const size_t bh = dual_spec_bound(h->dual_hint, 64);
            HIP_TRY(h, hipMemsetAsync(h->emit_ctr.p, 0, sizeof(int) * 4, st));
            o.emit = true;
            int rcf = enqueue_fused(h, n_items, d_ins_ids, d_pose, d_twist, d_s, d_wrench, d_sdot, d_counts, st, o);
            if (rcf != PFC_OK) return rcf;
            h->last_levels = eff_levels(h);
            size_t dpcap_h = 0;
            rcf = launch_dual(h, n_items, n_dir, h->tail.p, d_dpose, d_dtwist, d_ds, d_dwrench, d_dsdot, bh, st, &dpcap_h, true, h->emit_ctr.p);
            if (rcf != PFC_OK) return rcf;
            HIP_TRY(h, hipMemcpyAsync(h->h_emit.p, h->emit_ctr.p, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
            h->pend = {pfc_context::Pending::Fused, st, 0, 0, pfc_context::Pending::DualHandOver, n_dir, dpcap_h, d_ins_ids != nullptr};
            return PFC_OK;
        }
    }
    o.list = true;         // the value pass also lists the contributing candidates; batched path, one part
    int rc = enqueue_eval(h, n_items, d_ins_ids, d_pose, d_twist, d_s, d_wrench, d_sdot, d_counts, st, o);
    if (rc != PFC_OK) return rc;
    size_t dpcap = 0;
    rc = launch_dual(h, n_items, n_dir, h->tail.p, d_dpose, d_dtwist, d_ds, d_dwrench, d_dsdot, bound, st, &dpcap, true);
    if (rc != PFC_OK) return rc;
    h->pend = {pfc_context::Pending::Batched, st, 0, 0, pfc_context::Pending::DualBatched, n_dir, dpcap, d_ins_ids != nullptr};
    return PFC_OK;
}

int pfc_eval_dual_device(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const double *d_pose,
                         const double *d_twist, const double *d_s, const double *d_dpose, const double *d_dtwist,
                         const double *d_ds, double *d_wrench, double *d_sdot, double *d_dwrench, double *d_dsdot,
                         int *d_counts, void *stream) {
    return pfc_eval_dual_device_bp(h, n_items, n_dir, d_ins_ids, d_pose, nullptr, d_twist, d_s, d_dpose, d_dtwist, d_ds, d_wrench, d_sdot,
                                   d_dwrench, d_dsdot, d_counts, stream);
}

int pfc_eval_dual_device_more(pfc_handle h, int n_dir, const double *d_dpose, const double *d_dtwist, const double *d_ds,
                              double *d_dwrench, double *d_dsdot, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    if (h->multi) return multi_eval_dual_device_more(h, n_dir, d_dpose, d_dtwist, d_ds, d_dwrench, d_dsdot, stream);
    if (n_dir < 1 || n_dir > 16) return fail(h, PFC_ERR_BAD_ARG, "pfc_eval_dual_device_more: n_dir must be in 1..16");
    if (!h->device_kept())
        return fail(h, PFC_ERR_STATE, "pfc_eval_dual_device_more: no checked pfc_eval_dual_device evaluation on this handle to extend");
    if (!d_dpose || !d_dtwist || !d_dwrench || !d_dsdot) return fail(h, PFC_ERR_BAD_ARG, "pfc_eval_dual_device_more: null buffer");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const int n_items = h->kept.n;
    const size_t nk = (size_t)n_items * n_dir;
    HIP_TRY(h, ensure_graphed(h, h->dual_acc, nk * kDaStride));
    HIP_TRY(h, ensure_graphed(h, h->dual_res, nk * kDrStride));
    HIP_TRY(h, zero_ds(h, nk, &d_ds, st));
    HIP_TRY(h, hipMemsetAsync(h->dual_acc.p, 0, sizeof(double) * nk * kDaStride, st));
    // the contributing pairs are known exactly (dual_hint, from the value pass pfc_check has seen): no speculation
    const size_t bound = dual_exact_bound(h);
    // The passes report (kStHole: a list entry out of range, capacity guards) into a word of their own, cleared here and read
    // back by pfc_check in front of its synchronisation: neither the value pass's status word (read by ITS k_final only) nor
    // the hand-over block (read with the pair count of a first chunk only) is looked at again on this path.
    HIP_TRY(h, h->h_more.ensure(4));
    unsigned *more_status = h->status.p + 1;
    HIP_TRY(h, hipMemsetAsync(more_status, 0, sizeof(unsigned), st));
    const int rc = launch_dual(h, n_items, n_dir, h->tail.p, d_dpose, d_dtwist, d_ds, d_dwrench, d_dsdot, bound, st, nullptr, true,
                               h->kept.kind == pfc_context::KeptPass::HandOver ? h->emit_ctr.p : nullptr, more_status);
    if (rc != PFC_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->h_more.p, more_status, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    h->pend = {pfc_context::Pending::More, st}; h->last_dual_reused = true;
    return PFC_OK;
}

// The contact Jacobian L of every item at the point of the last checked Dual evaluation: the Dual passes of
// pfc_eval_dual_device_more, run three times on the kept value pass with unit seeds (16 + 16 + 4 directions), then packed.
int pfc_local_jacobian_device(pfc_handle h, double *d_L, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    if (h->multi) return multi_local_jacobian_device(h, d_L, stream);
    if (!h->device_kept())
        return fail(h, PFC_ERR_STATE, "pfc_local_jacobian_device: no checked pfc_eval_dual_device evaluation on this handle");
    if (!d_L) return fail(h, PFC_ERR_BAD_ARG, "pfc_local_jacobian_device: null buffer");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const int n_items = h->kept.n;
    const size_t n = (size_t)n_items;
    if (h->ljac_seed.cap < n * kLjacSeedDoubles) {      // the constant seeds: written once per capacity (a power of two of items)
        size_t cap = 64;
        while (cap < n) cap *= 2;
        HIP_TRY(h, h->ljac_seed.ensure(cap * kLjacSeedDoubles));
        hipLaunchKernelGGL(k_ljac_seeds, dim3((unsigned)((cap * kLjacCols + 255) / 256)), dim3(256), 0, st, (int)cap, h->ljac_seed.p);
        HIP_TRY(h, hipGetLastError());
    }
    const size_t cap = h->ljac_seed.cap / kLjacSeedDoubles;
    HIP_TRY(h, h->ljac_out.ensure(n * kLjacSize));
    // as pfc_eval_dual_device_more: the exact pair count, and a status word of the passes' own that pfc_check reads back
    const size_t bound = dual_exact_bound(h);
    HIP_TRY(h, h->h_more.ensure(4));
    unsigned *more_status = h->status.p + 1;
    HIP_TRY(h, hipMemsetAsync(more_status, 0, sizeof(unsigned), st));
    for (int p = 0; p < kLjacPasses; ++p) {
        const int nd = ljac_pass_dirs(p);
        const SeedBlock sd(h->ljac_seed.p + cap * 576 * p, cap * nd);
        const PartialBlock pd(h->ljac_out.p + n * 192 * p, n * nd);
        const int rc = launch_dual(h, n_items, nd, h->tail.p, sd.d_pose(), sd.d_twist(), sd.d_s(), pd.d_wrench(), pd.d_sdot(), bound, st, nullptr, false,
                                   h->kept.kind == pfc_context::KeptPass::HandOver ? h->emit_ctr.p : nullptr, more_status);
        if (rc != PFC_OK) return rc;
    }
    hipLaunchKernelGGL(k_ljac_pack, dim3((unsigned)((n * kLjacSize + 255) / 256)), dim3(256), 0, st, n_items, h->ljac_out.p, d_L);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(h->h_more.p, more_status, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    h->pend = {pfc_context::Pending::More, st}; h->last_dual_reused = true;
    return PFC_OK;
}

// Value pass (a Dual evaluation whose keys all have zero seeds: they cost nothing) and L, through the device entry points on staging
// buffers of the first device; re-issued on PFC_ERR_OVERFLOW as pfc_eval_dual does.
int pfc_local_jacobian(pfc_handle h, int n_items, const int *ins_ids, const double *pose, const double *twist, const double *s,
                       double *wrench, double *sdot, double *L, int *counts) {
    if (!h) return PFC_ERR_BAD_ARG;
    if (n_items < 0) return fail(h, PFC_ERR_BAD_ARG, "pfc_local_jacobian: negative n_items");
    if (n_items == 0) return PFC_OK;
    if (!pose || !twist || !wrench || !sdot || !L) return fail(h, PFC_ERR_BAD_ARG, "pfc_local_jacobian: null buffer");
    pfc_context *c = first_ctx(h);
    HIP_TRY(h, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t n = (size_t)n_items;
    Stage sg(c->stage, st);
    const int k_pose = sg.in(pose, n * 24), k_twist = sg.in(twist, n * 6), k_s = sg.in(s, n * 6), k_ids = sg.in(ins_ids, n);
    const int k_zero = sg.scratch<double>(SeedBlock(nullptr, n).doubles()), k_dw = sg.scratch<double>(n * 6), k_dsd = sg.scratch<double>(n * 6);      // one direction of zero seeds and its partials
    const int k_wr = sg.out(wrench, n * 6), k_sd = sg.out(sdot, n * 6), k_L = sg.out(L, n * kLjacSize), k_cnt = sg.out(counts, n * 4);
    HIP_TRY(h, sg.commit());
    const SeedBlock dz(sg.at<double>(k_zero), n);
    HIP_TRY(h, hipMemsetAsync(dz.p, 0, dz.bytes(), st));
    int rc = PFC_OK;
    for (int attempt = 0; attempt < 40; ++attempt) {
        rc = pfc_eval_dual_device(h, n_items, 1, sg.at<int>(k_ids), sg.at<double>(k_pose), sg.at<double>(k_twist), sg.at<double>(k_s), dz.d_pose(),
                                  dz.d_twist(), dz.d_s(), sg.at<double>(k_wr), sg.at<double>(k_sd), sg.at<double>(k_dw), sg.at<double>(k_dsd),
                                  sg.at<int>(k_cnt), st);
        if (rc != PFC_OK) return rc;
        rc = pfc_check(h);
        if (rc != PFC_ERR_OVERFLOW) break;
    }
    if (rc != PFC_OK) return rc;
    rc = pfc_local_jacobian_device(h, sg.at<double>(k_L), st);
    if (rc != PFC_OK) return rc;
    rc = pfc_check(h);
    if (rc != PFC_OK) return rc;
    HIP_TRY(h, hipSetDevice(c->device));
    HIP_TRY(h, sg.finish());
    return PFC_OK;
}

// [d_wrench; d_sdot] = L . seeds for every (item, direction): no handle state is read or changed, only the device and its stream.
int pfc_apply_local_jacobian_device(pfc_handle h, int n_items, int n_dir, const double *d_L, const double *d_dpose, const double *d_dtwist,
                                    const double *d_ds, double *d_dwrench, double *d_dsdot, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    // L and the seeds of a multi-device evaluation are on the first device: so is this
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        if (n_items < 0 || n_dir < 1 || n_dir > 16)
            return fail(c, PFC_ERR_BAD_ARG, "pfc_apply_local_jacobian_device: n_items >= 0 and n_dir in 1..16");
        if (n_items == 0) return PFC_OK;
        if (!d_L || !d_dpose || !d_dtwist || !d_dwrench || !d_dsdot)
            return fail(c, PFC_ERR_BAD_ARG, "pfc_apply_local_jacobian_device: null buffer");
        if (reinterpret_cast<uintptr_t>(d_L) % 16 != 0) return fail(c, PFC_ERR_BAD_ARG, "pfc_apply_local_jacobian_device: d_L must be 16-byte aligned");
        HIP_TRY(c, hipSetDevice(c->device));
        hipStream_t st = stream ? (hipStream_t)stream : c->stream;
        hipLaunchKernelGGL(k_ljac_apply, dim3((unsigned)n_items), dim3(64), 0, st, n_dir, d_L, d_dpose, d_dtwist, d_ds, d_dwrench, d_dsdot);
        HIP_TRY(c, hipGetLastError());
        return PFC_OK; });
}

int pfc_apply_local_jacobian(pfc_handle h, int n_items, int n_dir, const double *L, const double *d_pose, const double *d_twist,
                             const double *d_s, double *d_wrench, double *d_sdot) {
    if (!h) return PFC_ERR_BAD_ARG;
    pfc_context *c = first_ctx(h);
    if (n_items < 0 || n_dir < 1 || n_dir > 16) return fail(h, PFC_ERR_BAD_ARG, "pfc_apply_local_jacobian: n_items >= 0 and n_dir in 1..16");
    if (n_items == 0) return PFC_OK;
    if (!L || !d_pose || !d_twist || !d_wrench || !d_sdot) return fail(h, PFC_ERR_BAD_ARG, "pfc_apply_local_jacobian: null buffer");
    HIP_TRY(h, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t n = (size_t)n_items, nk = n * n_dir;
    Stage sg(c->stage, st);
    const int k_L = sg.in(L, n * kLjacSize), k_dp = sg.in(d_pose, nk * 24), k_dt = sg.in(d_twist, nk * 6), k_ds = sg.in(d_s, nk * 6);
    const int k_dw = sg.out(d_wrench, nk * 6), k_dsd = sg.out(d_sdot, nk * 6);
    HIP_TRY(h, sg.commit());
    const int rc = on_shard(h, c, [&](pfc_context *c1) {
        return pfc_apply_local_jacobian_device(c1, n_items, n_dir, sg.at<double>(k_L), sg.at<double>(k_dp), sg.at<double>(k_dt), sg.at<double>(k_ds),
                                               sg.at<double>(k_dw), sg.at<double>(k_dsd), st); });
    if (rc != PFC_OK) return rc;
    HIP_TRY(h, sg.finish());
    return PFC_OK;
}

// ---- contact items from body states (pfc_bodies.h) ------------------------------------------------------------------------
int pfc_set_instruction_bodies(pfc_handle h, int ins, int body_1, int body_2) {
    if (!h) return PFC_ERR_BAD_ARG;
    // the table lives with the first device, where the items are formed
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        if (ins < 0 || body_1 < -1 || body_2 < -1)
            return fail(c, PFC_ERR_BAD_ARG, "pfc_set_instruction_bodies: instruction id >= 0 and body ids >= -1 (-1: the world)");
        if (c->finalized && ins >= (int)c->ins.size())
            return fail(c, PFC_ERR_BAD_ARG, "pfc_set_instruction_bodies: the scenario has no instruction %d", ins);
        if (c->ins_bodies.size() < 2 * ((size_t)ins + 1)) c->ins_bodies.resize(2 * ((size_t)ins + 1), kBodiesUnbound);
        c->ins_bodies[2 * (size_t)ins] = body_1; c->ins_bodies[2 * (size_t)ins + 1] = body_2;
        c->bodies_stale = true;
        return PFC_OK; });
}

// The binding of instruction `ins` checked against n_body: PFC_ERR_STATE if it was never bound.
static int bodies_check_ins(pfc_context *h, const char *who, int ins, int n_body) {
    const size_t k = 2 * (size_t)ins;
    if (k + 1 >= h->ins_bodies.size() || h->ins_bodies[k] == kBodiesUnbound)
        return fail(h, PFC_ERR_STATE, "%s: instruction %d has no bodies (pfc_set_instruction_bodies)", who, ins);
    if (h->ins_bodies[k] >= n_body || h->ins_bodies[k + 1] >= n_body)
        return fail(h, PFC_ERR_BAD_ARG, "%s: instruction %d is bound to bodies (%d, %d), n_body is %d", who, ins, h->ins_bodies[k],
                    h->ins_bodies[k + 1], n_body);
    return PFC_OK;
}

// Argument checks of both forms (the ids are checked by the callers: they are device data for one of them).
static int bodies_check_args(pfc_context *h, const char *who, int n_items, const int *ins_ids, int n_scene, int n_body, const double *x_w_b,
                             const double *twist_w_b) {
    if (!h->finalized) return fail(h, PFC_ERR_STATE, "%s before pfc_finalize", who);
    if (n_items < 0 || n_scene < 1 || n_body < 0) return fail(h, PFC_ERR_BAD_ARG, "%s: n_items >= 0, n_scene >= 1, n_body >= 0", who);
    if (n_items == 0) return PFC_OK;
    if (n_body > 0 && (!x_w_b || !twist_w_b)) return fail(h, PFC_ERR_BAD_ARG, "%s: null body-state buffer", who);
    if (!ins_ids && n_items > (int)h->ins.size())
        return fail(h, PFC_ERR_BAD_ARG, "%s: n_items exceeds the number of instructions and no ins_ids given", who);
    return PFC_OK;
}

// The host forms' ids: every item's instruction and scene id in range, its instruction bound.
static int bodies_check_ids_host(pfc_context *h, const char *who, int n_items, const int *ins_ids, const int *scene, int n_scene, int n_body) {
    for (int i = 0; i < n_items; ++i) {
        const int ins = ins_ids ? ins_ids[i] : i;
        if (ins < 0 || ins >= (int)h->ins.size() || (scene && (scene[i] < 0 || scene[i] >= n_scene)))
            return fail(h, PFC_ERR_BAD_ARG, "%s: instruction / scene id out of range (item %d)", who, i);
        const int rc = bodies_check_ins(h, who, ins, n_body);
        if (rc != PFC_OK) return rc;
    }
    return PFC_OK;
}

// The device forms' ids are device data: without d_ins_ids the instructions 0 .. n_items - 1 must be bound, with them every instruction.
static int bodies_check_bound_device(pfc_context *h, const char *who, int n_items, const int *d_ins_ids, int n_body) {
    const int n_used = d_ins_ids ? (int)h->ins.size() : n_items;
    for (int k = 0; k < n_used; ++k) {
        const int rc = bodies_check_ins(h, who, k, n_body);
        if (rc != PFC_OK) return rc;
    }
    return PFC_OK;
}

// What pfc_items_from_bodies_device checks, for the entry itself and for the chains that form items (they pass its name).
static int bodies_check_device(pfc_context *h, const char *who, int n_items, const int *d_ins_ids, int n_scene, int n_body,
                               const double *d_x_w_b, const double *d_twist_w_b) {
    const int rc = bodies_check_args(h, who, n_items, d_ins_ids, n_scene, n_body, d_x_w_b, d_twist_w_b);
    return rc != PFC_OK || n_items == 0 ? rc : bodies_check_bound_device(h, who, n_items, d_ins_ids, n_body);
}

// The bind table's upload on st if it is stale (the one synchronisation of this path: once per binding, ordered behind st's
// earlier work).
static int bodies_upload_bind(pfc_context *h, hipStream_t st) {
    const int n_ins = (int)h->ins.size();
    HIP_TRY(h, hipSetDevice(h->device));
    if (!h->bodies_stale) return PFC_OK;
    h->ins_bodies.resize(2 * (size_t)n_ins, kBodiesUnbound);
    HIP_TRY(h, h->bodies_bind.ensure(2 * (size_t)n_ins));
    HIP_TRY(h, hipMemcpyAsync(h->bodies_bind.p, h->ins_bodies.data(), sizeof(int) * 2 * (size_t)n_ins, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    h->bodies_stale = false;
    return PFC_OK;
}

// The table's upload if it is stale, and the kernel, on st.  Every pointer is a device pointer.
static int bodies_launch(pfc_context *h, int n_items, const int *ins_ids, const int *scene, int n_scene, int n_body, const double *x_w_b,
                         const double *twist_w_b, double *pose, double *twist, double *x_w_r2, int *body_1, int *body_2, hipStream_t st) {
    const int n_ins = (int)h->ins.size();
    { const int rc = bodies_upload_bind(h, st); if (rc != PFC_OK) return rc; }
    BodiesArgs a;
    a.n_items = n_items; a.n_ins = n_ins; a.n_scene = n_scene; a.n_body = n_body; a.ins_ids = ins_ids; a.scene = scene;
    a.bind = h->bodies_bind.p; a.x_w_b = x_w_b; a.twist_w_b = twist_w_b; a.pose = pose; a.twist = twist; a.x_w_r2 = x_w_r2;
    a.body_1 = body_1; a.body_2 = body_2;
    hipLaunchKernelGGL(k_items_from_bodies, dim3((unsigned)((n_items + kBodiesWave - 1) / kBodiesWave)),
                       dim3(kBodiesWave), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    return PFC_OK;
}

int pfc_items_from_bodies_device(pfc_handle h, int n_items, const int *d_ins_ids, const int *d_scene, int n_scene, int n_body,
                                 const double *d_x_w_b, const double *d_twist_w_b, double *d_pose, double *d_twist, double *d_x_w_r2,
                                 int *d_body_1, int *d_body_2, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) {
        const int rc = bodies_check_device(c, "pfc_items_from_bodies_device", n_items, d_ins_ids, n_scene, n_body, d_x_w_b, d_twist_w_b);
        if (rc != PFC_OK || n_items == 0) return rc;
        return bodies_launch(c, n_items, d_ins_ids, d_scene, n_scene, n_body, d_x_w_b, d_twist_w_b, d_pose, d_twist, d_x_w_r2, d_body_1,
                             d_body_2, stream ? (hipStream_t)stream : c->stream); });
}

int pfc_items_from_bodies(pfc_handle h, int n_items, const int *ins_ids, const int *scene, int n_scene, int n_body, const double *x_w_b,
                          const double *twist_w_b, double *pose, double *twist, double *x_w_r2, int *body_1, int *body_2) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        const char *who = "pfc_items_from_bodies";
        int rc = bodies_check_args(c, who, n_items, ins_ids, n_scene, n_body, x_w_b, twist_w_b);
        if (rc != PFC_OK || n_items == 0) return rc;
        if ((rc = bodies_check_ids_host(c, who, n_items, ins_ids, scene, n_scene, n_body)) != PFC_OK) return rc;
        HIP_TRY(c, hipSetDevice(c->device));
        const size_t n = (size_t)n_items, nb = (size_t)n_scene * n_body;
        Stage sg(c->stage, c->stream);
        const int k_x = sg.in(x_w_b, nb * 12), k_tw = sg.in(twist_w_b, nb * 6), k_ids = sg.in(ins_ids, n), k_sc = sg.in(scene, n);
        const int k_pose = sg.out(pose, n * 24), k_twist = sg.out(twist, n * 6), k_xr = sg.out(x_w_r2, n * 12);
        const int k_b1 = sg.out(body_1, n), k_b2 = sg.out(body_2, n);
        HIP_TRY(c, sg.commit());
        rc = bodies_launch(c, n_items, sg.at<int>(k_ids), sg.at<int>(k_sc), n_scene, n_body, sg.at<double>(k_x), sg.at<double>(k_tw),
                           sg.at<double>(k_pose), sg.at<double>(k_twist), sg.at<double>(k_xr), sg.at<int>(k_b1), sg.at<int>(k_b2), sg.st);
        if (rc != PFC_OK) return rc;
        HIP_TRY(c, sg.finish());
        return PFC_OK; });
}

// ---- the chained state calls, over one record of their buffers (pfc_statecall.h) -----------------------------------------------------
// Each chain is the body of its extern "C" entry (and of its `_more` twin, `more` set): the entry fills a StateCall and calls it.  The
// kernels of a chain run on the first shard -- its stream unless the caller gave one -- and the evaluation between them is the
// handle's own, sharded on a multi-device handle.  A chain's own checks carry its entry's name, as when that entry is called from
// the entry above it.
static hipStream_t call_stream(const pfc_context *c, const StateCall &S) { return S.stream ? (hipStream_t)S.stream : c->stream; }

static StateCall state_call_head(int n_items, int n_dir, const int *d_ins_ids, const int *d_scene, int n_scene, void *stream) {
    StateCall S;
    S.n_items = n_items; S.n_dir = n_dir; S.ins_ids = d_ins_ids; S.scene = d_scene; S.n_scene = n_scene; S.stream = stream;
    return S;
}

// k_items_from_bodies, then exactly pfc_eval_device on the pose and twist it wrote, on the same stream.
static int eval_bodies(pfc_context *h, const StateCall &S, int n_body) {
    const StateBufs &V = S.val;
    if (S.n_items > 0 && (!V.pose || !V.twist))
        return fail(h, PFC_ERR_BAD_ARG, "pfc_eval_bodies_device: d_pose and d_twist are the evaluation's inputs");
    const int rc = on_shard(h, first_ctx(h), [&](pfc_context *c) {
        const int r = bodies_check_device(c, "pfc_items_from_bodies_device", S.n_items, S.ins_ids, S.n_scene, n_body, V.x_w_b, V.twist_w_b);
        if (r != PFC_OK || S.n_items == 0) return r;
        return bodies_launch(c, S.n_items, S.ins_ids, S.scene, S.n_scene, n_body, V.x_w_b, V.twist_w_b, V.pose, V.twist, V.x_w_r2, V.body_1,
                             V.body_2, call_stream(c, S)); });
    if (rc != PFC_OK) return rc;
    return pfc_eval_device(h, S.n_items, S.ins_ids, V.pose, V.twist, V.s, V.wrench, V.sdot, V.counts, S.stream);
}

int pfc_eval_bodies_device(pfc_handle h, int n_items, const int *d_ins_ids, const int *d_scene, int n_scene, int n_body,
                           const double *d_x_w_b, const double *d_twist_w_b, const double *d_s, double *d_pose, double *d_twist,
                           double *d_x_w_r2, int *d_body_1, int *d_body_2, double *d_wrench, double *d_sdot, int *d_counts, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    StateCall S = state_call_head(n_items, 0, d_ins_ids, d_scene, n_scene, stream);
    StateBufs &V = S.val;
    V.x_w_b = kept_value(d_x_w_b); V.twist_w_b = kept_value(d_twist_w_b); V.s = d_s;
    V.pose = d_pose; V.twist = d_twist; V.x_w_r2 = d_x_w_r2; V.body_1 = d_body_1; V.body_2 = d_body_2;
    V.wrench = d_wrench; V.sdot = d_sdot; V.counts = d_counts;
    return eval_bodies(h, S, n_body);
}

int pfc_eval_bodies(pfc_handle h, int n_items, const int *ins_ids, const int *scene, int n_scene, int n_body, const double *x_w_b,
                    const double *twist_w_b, const double *s, double *pose, double *twist, double *x_w_r2, int *body_1, int *body_2,
                    double *wrench, double *sdot, int *counts) {
    if (!h) return PFC_ERR_BAD_ARG;
    std::vector<double> tmp;
    if (n_items > 0 && (!pose || !twist)) {
        tmp.resize((size_t)n_items * 30);
        if (!pose) pose = tmp.data();
        if (!twist) twist = tmp.data() + (size_t)n_items * 24;
    }
    const int rc = pfc_items_from_bodies(h, n_items, ins_ids, scene, n_scene, n_body, x_w_b, twist_w_b, pose, twist, x_w_r2, body_1, body_2);
    if (rc != PFC_OK) return rc;
    return pfc_eval(h, n_items, ins_ids, pose, twist, s, wrench, sdot, counts);
}

// ---- Dual seeds of the items from body states and their partials (pfc_bodies.h) -------------------------------------------------
// Argument, state and binding checks of the device forms: those of pfc_items_from_bodies_device, and n_dir.
static int bodies_seeds_check_device(pfc_context *h, const char *who, int n_items, int n_dir, const int *d_ins_ids, int n_scene, int n_body,
                                     const double *d_x_w_b, const double *d_twist_w_b) {
    int rc = bodies_check_args(h, who, n_items, d_ins_ids, n_scene, n_body, d_x_w_b, d_twist_w_b);
    if (rc != PFC_OK) return rc;
    if (n_dir < 1 || n_dir > 16) return fail(h, PFC_ERR_BAD_ARG, "%s: n_dir must be in 1..16", who);
    return n_items == 0 ? PFC_OK : bodies_check_bound_device(h, who, n_items, d_ins_ids, n_body);
}

// The table's upload if it is stale, and k_dual_seeds_from_bodies, on st.  Every pointer is a device pointer.
static int bodies_seeds_launch(pfc_context *h, int n_items, int n_dir, const int *ins_ids, const int *scene, int n_scene, int n_body,
                               const double *x_w_b, const double *twist_w_b, const double *dx_w_b, const double *dtwist_w_b, double *dpose,
                               double *dtwist, double *dx_w_r2, hipStream_t st) {
    { const int rc = bodies_upload_bind(h, st); if (rc != PFC_OK) return rc; }
    if (!dpose && !dtwist && !dx_w_r2) return PFC_OK;
    BodiesSeedArgs a;
    a.n_items = n_items; a.n_dir = n_dir; a.n_ins = (int)h->ins.size(); a.n_scene = n_scene; a.n_body = n_body;
    a.ins_ids = ins_ids; a.scene = scene; a.bind = h->bodies_bind.p; a.x_w_b = x_w_b; a.twist_w_b = twist_w_b;
    a.dx_w_b = dx_w_b; a.dtwist_w_b = dtwist_w_b; a.dpose = dpose; a.dtwist = dtwist; a.dx_w_r2 = dx_w_r2;
    const size_t nk = (size_t)n_items * n_dir;
    hipLaunchKernelGGL(k_dual_seeds_from_bodies, dim3((unsigned)((nk + kBodiesWave - 1) / kBodiesWave)), dim3(kBodiesWave), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    return PFC_OK;
}

int pfc_dual_seeds_from_bodies_device(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const int *d_scene, int n_scene,
                                      int n_body, const double *d_x_w_b, const double *d_twist_w_b, const double *d_dx_w_b,
                                      const double *d_dtwist_w_b, double *d_dpose, double *d_dtwist, double *d_dx_w_r2, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) {
        const int rc = bodies_seeds_check_device(c, "pfc_dual_seeds_from_bodies_device", n_items, n_dir, d_ins_ids, n_scene, n_body, d_x_w_b,
                                                 d_twist_w_b);
        if (rc != PFC_OK || n_items == 0) return rc;
        return bodies_seeds_launch(c, n_items, n_dir, d_ins_ids, d_scene, n_scene, n_body, d_x_w_b, d_twist_w_b, d_dx_w_b, d_dtwist_w_b,
                                   d_dpose, d_dtwist, d_dx_w_r2, stream ? (hipStream_t)stream : c->stream); });
}

int pfc_dual_seeds_from_bodies(pfc_handle h, int n_items, int n_dir, const int *ins_ids, const int *scene, int n_scene, int n_body,
                               const double *x_w_b, const double *twist_w_b, const double *d_x_w_b, const double *d_twist_w_b,
                               double *d_pose, double *d_twist, double *d_x_w_r2) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        const char *who = "pfc_dual_seeds_from_bodies";
        int rc = bodies_check_args(c, who, n_items, ins_ids, n_scene, n_body, x_w_b, twist_w_b);
        if (rc != PFC_OK) return rc;
        if (n_dir < 1 || n_dir > 16) return fail(c, PFC_ERR_BAD_ARG, "%s: n_dir must be in 1..16", who);
        if (n_items == 0) return PFC_OK;
        if ((rc = bodies_check_ids_host(c, who, n_items, ins_ids, scene, n_scene, n_body)) != PFC_OK) return rc;
        HIP_TRY(c, hipSetDevice(c->device));
        const size_t n = (size_t)n_items, nb = (size_t)n_scene * n_body, nk = n * n_dir, nbk = nb * n_dir;
        Stage sg(c->stage, c->stream);
        const int k_x = sg.in(x_w_b, nb * 12), k_tw = sg.in(twist_w_b, nb * 6), k_dx = sg.in(d_x_w_b, nbk * 12), k_dtw = sg.in(d_twist_w_b, nbk * 6);
        const int k_ids = sg.in(ins_ids, n), k_sc = sg.in(scene, n);
        const int k_dpose = sg.out(d_pose, nk * 24), k_dtwist = sg.out(d_twist, nk * 6), k_dxr = sg.out(d_x_w_r2, nk * 12);
        HIP_TRY(c, sg.commit());
        rc = bodies_seeds_launch(c, n_items, n_dir, sg.at<int>(k_ids), sg.at<int>(k_sc), n_scene, n_body, sg.at<double>(k_x), sg.at<double>(k_tw),
                                 sg.at<double>(k_dx), sg.at<double>(k_dtw), sg.at<double>(k_dpose), sg.at<double>(k_dtwist), sg.at<double>(k_dxr), sg.st);
        if (rc != PFC_OK) return rc;
        HIP_TRY(c, sg.finish());
        return PFC_OK; });
}

// First call: k_items_from_bodies, k_dual_seeds_from_bodies, then exactly pfc_eval_dual_device on the buffers they wrote, on the same
// stream.  `more`: k_dual_seeds_from_bodies, then exactly pfc_eval_dual_device_more on the seeds it wrote.
static int eval_dual_bodies(pfc_context *h, const StateCall &S, int n_body, bool more) {
    const StateBufs &V = S.val, &P = S.par;
    const char *who = more ? "pfc_eval_dual_bodies_device_more" : "pfc_eval_dual_bodies_device";
    if (!more) {
        if (S.n_dir < 1 || S.n_dir > 16) return fail(h, PFC_ERR_BAD_ARG, "%s: n_dir must be in 1..16", who);
        if (S.n_items > 0 && (!V.pose || !V.twist || !P.pose || !P.twist))
            return fail(h, PFC_ERR_BAD_ARG, "%s: d_pose, d_twist, d_dpose and d_dtwist are the evaluation's inputs", who);
    } else if (!h->multi) {      // _more's own preconditions, before the seeds are written
        const int rc = bodies_seeds_check_device(h, who, S.n_items, S.n_dir, S.ins_ids, S.n_scene, n_body, V.x_w_b, V.twist_w_b);
        if (rc != PFC_OK) return rc;
        if (!h->device_kept())
            return fail(h, PFC_ERR_STATE, "%s: no checked pfc_eval_dual_device evaluation on this handle to extend", who);
        if (S.n_items != h->kept.n)
            return fail(h, PFC_ERR_BAD_ARG, "%s: n_items is %d, the kept evaluation has %d items", who, S.n_items, h->kept.n);
        if (!P.pose || !P.twist || !P.wrench || !P.sdot) return fail(h, PFC_ERR_BAD_ARG, "%s: null buffer", who);
    }
    const int rc = on_shard(h, first_ctx(h), [&](pfc_context *c) {
        const hipStream_t st = call_stream(c, S);
        int r = PFC_OK;
        if (!more) {
            r = bodies_check_device(c, "pfc_items_from_bodies_device", S.n_items, S.ins_ids, S.n_scene, n_body, V.x_w_b, V.twist_w_b);
            if (r == PFC_OK && S.n_items > 0)
                r = bodies_launch(c, S.n_items, S.ins_ids, S.scene, S.n_scene, n_body, V.x_w_b, V.twist_w_b, V.pose, V.twist, V.x_w_r2,
                                  V.body_1, V.body_2, st);
            if (r != PFC_OK) return r;
        }
        r = bodies_seeds_check_device(c, "pfc_dual_seeds_from_bodies_device", S.n_items, S.n_dir, S.ins_ids, S.n_scene, n_body, V.x_w_b,
                                      V.twist_w_b);
        if (r != PFC_OK || S.n_items == 0) return r;
        return bodies_seeds_launch(c, S.n_items, S.n_dir, S.ins_ids, S.scene, S.n_scene, n_body, V.x_w_b, V.twist_w_b, P.x_w_b, P.twist_w_b,
                                   P.pose, P.twist, P.x_w_r2, st); });
    if (rc != PFC_OK) return rc;
    if (more) return pfc_eval_dual_device_more(h, S.n_dir, P.pose, P.twist, P.s, P.wrench, P.sdot, S.stream);
    return pfc_eval_dual_device(h, S.n_items, S.n_dir, S.ins_ids, V.pose, V.twist, V.s, P.pose, P.twist, P.s, V.wrench, V.sdot, P.wrench,
                                P.sdot, V.counts, S.stream);
}

int pfc_eval_dual_bodies_device(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const int *d_scene, int n_scene, int n_body,
                                const double *d_x_w_b, const double *d_twist_w_b, const double *d_dx_w_b, const double *d_dtwist_w_b,
                                const double *d_s, const double *d_ds, double *d_pose, double *d_twist, double *d_x_w_r2, int *d_body_1,
                                int *d_body_2, double *d_dpose, double *d_dtwist, double *d_dx_w_r2, double *d_wrench, double *d_sdot,
                                double *d_dwrench, double *d_dsdot, int *d_counts, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    StateCall S = state_call_head(n_items, n_dir, d_ins_ids, d_scene, n_scene, stream);
    StateBufs &V = S.val, &P = S.par;
    V.x_w_b = kept_value(d_x_w_b); V.twist_w_b = kept_value(d_twist_w_b); P.x_w_b = kept_value(d_dx_w_b); P.twist_w_b = kept_value(d_dtwist_w_b);
    V.s = d_s; P.s = d_ds;
    V.pose = d_pose; V.twist = d_twist; V.x_w_r2 = d_x_w_r2; V.body_1 = d_body_1; V.body_2 = d_body_2;
    P.pose = d_dpose; P.twist = d_dtwist; P.x_w_r2 = d_dx_w_r2;
    V.wrench = d_wrench; V.sdot = d_sdot; P.wrench = d_dwrench; P.sdot = d_dsdot; V.counts = d_counts;
    return eval_dual_bodies(h, S, n_body, false);
}

int pfc_eval_dual_bodies_device_more(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const int *d_scene, int n_scene, int n_body,
                                     const double *d_x_w_b, const double *d_twist_w_b, const double *d_dx_w_b, const double *d_dtwist_w_b,
                                     const double *d_ds, double *d_dpose, double *d_dtwist, double *d_dx_w_r2, double *d_dwrench,
                                     double *d_dsdot, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    StateCall S = state_call_head(n_items, n_dir, d_ins_ids, d_scene, n_scene, stream);
    StateBufs &V = S.val, &P = S.par;
    V.x_w_b = kept_value(d_x_w_b); V.twist_w_b = kept_value(d_twist_w_b); P.x_w_b = kept_value(d_dx_w_b); P.twist_w_b = kept_value(d_dtwist_w_b);
    P.s = d_ds; P.pose = d_dpose; P.twist = d_dtwist; P.x_w_r2 = d_dx_w_r2; P.wrench = d_dwrench; P.sdot = d_dsdot;
    return eval_dual_bodies(h, S, n_body, true);
}

// ---- kinematics from joint states (pfc_kin.h) -----------------------------------------------------------------------------------
int pfc_set_mechanism(pfc_handle h, int n_body, const int *parent, const int *joint_type, const double *x_p_j, const double *axis) {
    if (!h) return PFC_ERR_BAD_ARG;
    // the tables live with the first device, where the states are formed
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        const char *who = "pfc_set_mechanism";
        if (n_body < 1) return fail(c, PFC_ERR_BAD_ARG, "%s: n_body is %d, a mechanism has at least one body", who, n_body);
        if (!parent || !joint_type || !x_p_j || !axis) return fail(c, PFC_ERR_BAD_ARG, "%s: null table", who);
        const size_t nb = (size_t)n_body;
        std::vector<int> jtype(nb), qoff(nb), voff(nb), path_off(nb + 1, 0), path, depth(nb);
        int nv = 0;
        for (int b = 0; b < n_body; ++b) {
            if (parent[b] < -1 || parent[b] >= b)
                return fail(c, PFC_ERR_BAD_ARG, "%s: body %d has parent %d, outside [-1, %d)", who, b, parent[b], b);
            const int t = joint_type[b];
            if (t != PFC_JOINT_FIXED && t != PFC_JOINT_REVOLUTE && t != PFC_JOINT_PRISMATIC && t != PFC_JOINT_FLOATING_MRP)
                return fail(c, PFC_ERR_BAD_ARG, "%s: body %d has the unknown joint type %d", who, b, t);
            if (t == PFC_JOINT_REVOLUTE || t == PFC_JOINT_PRISMATIC) {
                const double *a = axis + 3 * (size_t)b;
                const double n2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
                if (!(std::fabs(n2 - 1.0) <= 1e-12))
                    return fail(c, PFC_ERR_BAD_ARG, "%s: body %d's joint axis is not a unit vector (|a|^2 = %.17g)", who, b, n2);
            }
            jtype[b] = t; qoff[b] = voff[b] = nv;      // nq = nv for every joint type here
            nv += kin_joint_nq(t);
            depth[b] = parent[b] < 0 ? 1 : depth[parent[b]] + 1;
            path_off[b + 1] = path_off[b] + depth[b];
        }
        path.resize((size_t)path_off[nb]);
        std::vector<unsigned char> anc(nb * (size_t)nv, 0);
        for (int b = 0; b < n_body; ++b) {
            int k = path_off[b + 1];
            for (int a = b; a >= 0; a = parent[a]) {
                path[--k] = a;
                for (int e = 0; e < kin_joint_nq(jtype[a]); ++e) anc[(size_t)b * nv + voff[a] + e] = 1;
            }
        }
        KinHost &K = c->kin;
        K.blob.clear();
        K.o_jtype = K.put(jtype); K.o_qoff = K.put(qoff); K.o_voff = K.put(voff); K.o_path_off = K.put(path_off); K.o_path = K.put(path);
        K.o_x_p_j = K.put(std::vector<double>(x_p_j, x_p_j + 12 * nb)); K.o_axis = K.put(std::vector<double>(axis, axis + 3 * nb));
        K.o_anc = K.put(anc);
        {   // the subtrees: b and its descendants in increasing body order (a descendant's path holds b)
            std::vector<int> sub_off(nb + 1, 0), sub;
            for (int b = 0; b < n_body; ++b) {
                for (int d = b; d < n_body; ++d)
                    if (std::find(path.begin() + path_off[d], path.begin() + path_off[d + 1], b) != path.begin() + path_off[d + 1]) sub.push_back(d);
                sub_off[b + 1] = (int)sub.size();
            }
            K.o_sub_off = K.put(sub_off); K.o_sub = K.put(sub);
            K.o_inertia = K.put(std::vector<double>(13 * nb, 0.0));
            K.has_inertia = false;
        }
        K.n_body = n_body; K.nq = nv; K.nv = nv;
        c->kin_stale = true;
        return PFC_OK; });
}

int pfc_mechanism_sizes(pfc_handle h, int *n_body, int *nq, int *nv) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        if (c->kin.n_body == 0) return fail(c, PFC_ERR_STATE, "pfc_mechanism_sizes before pfc_set_mechanism");
        if (n_body) *n_body = c->kin.n_body;
        if (nq) *nq = c->kin.nq;
        if (nv) *nv = c->kin.nv;
        return PFC_OK; });
}

// Argument and state checks of both forms of pfc_kinematics.
static int kin_check_args(pfc_context *h, const char *who, int n_scene, const double *q, const double *v, bool want_twist) {
    if (h->kin.n_body == 0) return fail(h, PFC_ERR_STATE, "%s before pfc_set_mechanism", who);
    if (n_scene < 0) return fail(h, PFC_ERR_BAD_ARG, "%s: negative n_scene", who);
    if (n_scene == 0) return PFC_OK;
    if (h->kin.nq > 0 && (!q || (want_twist && !v))) return fail(h, PFC_ERR_BAD_ARG, "%s: null state vector", who);
    if (((long long)n_scene * h->kin.n_body * std::max(h->kin.nv, 1) + kKinJacBlock - 1) / kKinJacBlock >= (1ll << 31))
        return fail(h, PFC_ERR_BAD_ARG, "%s: n_scene n_body nv must be below 2^39", who);
    return PFC_OK;
}

// The tables' upload on st if they are stale (one synchronisation per pfc_set_mechanism, as bodies_upload_bind), S_w grown if a
// Jacobian is wanted and too small, and the kernels, on st.  Every pointer is a device pointer; an output that is null is not
// written, and the kernel only it needs is not launched.
static int kin_upload_tables(pfc_context *h, hipStream_t st) {
    const KinHost &K = h->kin;
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->kin_stale) {
        HIP_TRY(h, h->kin_tab.ensure(K.blob.size()));
        HIP_TRY(h, hipMemcpyAsync(h->kin_tab.p, K.blob.data(), K.blob.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        h->kin_stale = false;
    }
    return PFC_OK;
}

// The sizes, the tables' device addresses and the state of both kernels' arguments; the outputs are left null.
static KinArgs kin_table_args(const pfc_context *h, int n_scene, const double *q, const double *v) {
    const KinHost &K = h->kin;
    const char *t = h->kin_tab.p;
    KinArgs a;
    a.n_scene = n_scene; a.n_body = K.n_body; a.nq = K.nq; a.nv = K.nv;
    a.jtype = (const int *)(t + K.o_jtype); a.qoff = (const int *)(t + K.o_qoff); a.voff = (const int *)(t + K.o_voff);
    a.path_off = (const int *)(t + K.o_path_off); a.path = (const int *)(t + K.o_path);
    a.x_p_j = (const double *)(t + K.o_x_p_j); a.axis = (const double *)(t + K.o_axis); a.anc = (const unsigned char *)(t + K.o_anc);
    a.q = q; a.v = v; a.x_w_b = nullptr; a.twist_w_b = nullptr; a.S_w = nullptr; a.jac = nullptr;
    return a;
}

static int kin_launch(pfc_context *h, int n_scene, const double *q, const double *v, double *x_w_b, double *twist_w_b, double *jac,
                      hipStream_t st) {
    const KinHost &K = h->kin;
    { const int rc = kin_upload_tables(h, st); if (rc != PFC_OK) return rc; }
    const bool want_jac = jac && K.nv > 0;
    if (!x_w_b && !twist_w_b && !want_jac) return PFC_OK;
    if (want_jac) HIP_TRY(h, h->kin_sw.ensure((size_t)n_scene * K.nv * 6));
    KinArgs a = kin_table_args(h, n_scene, q, v);
    a.x_w_b = x_w_b; a.twist_w_b = twist_w_b; a.S_w = want_jac ? h->kin_sw.p : nullptr; a.jac = jac;
    const long long lanes = (long long)n_scene * K.n_body;
    hipLaunchKernelGGL(k_kinematics, dim3((unsigned)((lanes + kKinWave - 1) / kKinWave)), dim3(kKinWave), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    if (want_jac) {
        const long long tot = lanes * K.nv;
        hipLaunchKernelGGL(k_kin_jacobian, dim3((unsigned)((tot + kKinJacBlock - 1) / kKinJacBlock)), dim3(kKinJacBlock), 0, st, a);
        HIP_TRY(h, hipGetLastError());
    }
    return PFC_OK;
}

int pfc_kinematics_device(pfc_handle h, int n_scene, const double *d_q, const double *d_v, double *d_x_w_b, double *d_twist_w_b,
                          double *d_jac, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) {
        const int rc = kin_check_args(c, "pfc_kinematics_device", n_scene, d_q, d_v, d_twist_w_b != nullptr);
        if (rc != PFC_OK || n_scene == 0) return rc;
        return kin_launch(c, n_scene, d_q, d_v, d_x_w_b, d_twist_w_b, d_jac, stream ? (hipStream_t)stream : c->stream); });
}

int pfc_kinematics(pfc_handle h, int n_scene, const double *q, const double *v, double *x_w_b, double *twist_w_b, double *jac) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        int rc = kin_check_args(c, "pfc_kinematics", n_scene, q, v, twist_w_b != nullptr);
        if (rc != PFC_OK || n_scene == 0) return rc;
        HIP_TRY(c, hipSetDevice(c->device));
        const size_t ns = (size_t)n_scene, nb = ns * c->kin.n_body;
        Stage sg(c->stage, c->stream);
        const int k_q = sg.in(q, ns * c->kin.nq), k_v = sg.in(v, ns * c->kin.nv);
        const int k_x = sg.out(x_w_b, nb * 12), k_tw = sg.out(twist_w_b, nb * 6), k_j = sg.out(jac, nb * c->kin.nv * 6);
        HIP_TRY(c, sg.commit());
        rc = kin_launch(c, n_scene, sg.at<double>(k_q), sg.at<double>(k_v), sg.at<double>(k_x), sg.at<double>(k_tw), sg.at<double>(k_j), sg.st);
        if (rc != PFC_OK) return rc;
        HIP_TRY(c, sg.finish());
        return PFC_OK; });
}

// What both forms of pfc_eval_state check before anything is launched or written: the mechanism, the scenario, and the bodies of the
// instructions against the mechanism's n_body (device form: bodies_check_bound_device; host form: the ids themselves).
static int eval_state_check(pfc_context *c, const char *who, int n_items, const int *ins_ids, const int *scene, int n_scene, bool host,
                            const double *q, const double *v) {
    if (c->kin.n_body == 0) return fail(c, PFC_ERR_STATE, "%s before pfc_set_mechanism", who);
    if (!c->finalized) return fail(c, PFC_ERR_STATE, "%s before pfc_finalize", who);
    if (n_items < 0 || n_scene < 1) return fail(c, PFC_ERR_BAD_ARG, "%s: n_items >= 0, n_scene >= 1", who);
    int rc = kin_check_args(c, who, n_scene, q, v, true);
    if (rc != PFC_OK) return rc;
    if (!ins_ids && n_items > (int)c->ins.size())
        return fail(c, PFC_ERR_BAD_ARG, "%s: n_items exceeds the number of instructions and no ins_ids given", who);
    if (n_items == 0) return PFC_OK;
    return host ? bodies_check_ids_host(c, who, n_items, ins_ids, scene, n_scene, c->kin.n_body)
                : bodies_check_bound_device(c, who, n_items, ins_ids, c->kin.n_body);
}

int pfc_eval_state(pfc_handle h, int n_items, const int *ins_ids, const int *scene, int n_scene,
                   const double *q, const double *v, const double *s,
                   double *x_w_b, double *twist_w_b, double *jac,
                   double *pose, double *twist, double *x_w_r2, int *body_1, int *body_2,
                   double *wrench, double *sdot, int *counts, double *f) {
    if (!h) return PFC_ERR_BAD_ARG;
    const char *who = "pfc_eval_state";
    pfc_context *c = first_ctx(h);
    int rc = on_shard(h, c, [&](pfc_context *c1) { return eval_state_check(c1, who, n_items, ins_ids, scene, n_scene, true, q, v); });
    if (rc != PFC_OK) return rc;
    if (n_items > 0 && (!wrench || !sdot)) return fail(h, PFC_ERR_BAD_ARG, "%s: null buffer", who);
    const int n_body = c->kin.n_body, nv = c->kin.nv;
    const bool scatter = f && nv > 0;
    const size_t n = (size_t)n_items, nb = (size_t)n_scene * n_body;
    std::vector<double> tmp;      // the intermediate buffers the caller did not ask for
    std::vector<int> itmp;
    {
        size_t need = (x_w_b ? 0 : nb * 12) + (twist_w_b ? 0 : nb * 6);
        if (scatter) need += (jac ? 0 : nb * nv * 6) + (x_w_r2 ? 0 : n * 12);
        tmp.resize(need);
        double *p = tmp.data();
        if (!x_w_b) { x_w_b = p; p += nb * 12; }
        if (!twist_w_b) { twist_w_b = p; p += nb * 6; }
        if (scatter && !jac) { jac = p; p += nb * nv * 6; }
        if (scatter && !x_w_r2) { x_w_r2 = p; p += n * 12; }
        if (scatter && (!body_1 || !body_2)) {
            itmp.resize(2 * n);
            if (!body_1) body_1 = itmp.data();
            if (!body_2) body_2 = itmp.data() + n;
        }
    }
    if ((rc = pfc_kinematics(h, n_scene, q, v, x_w_b, twist_w_b, jac)) != PFC_OK) return rc;
    rc = pfc_eval_bodies(h, n_items, ins_ids, scene, n_scene, n_body, x_w_b, twist_w_b, s, pose, twist, x_w_r2, body_1, body_2, wrench, sdot,
                         counts);
    if (rc != PFC_OK || !scatter) return rc;
    return pfc_scatter_generalized(h, n_items, wrench, x_w_r2, body_1, body_2, scene, n_scene, n_scene * n_body, nv, jac, f);
}

// ---- forward dynamics from joint states (pfc_dyn.h) -------------------------------------------------------------------------------
static_assert(PFC_MAX_NV_SOLVE == kDynWave, "k_accel runs one lane per row");

int pfc_set_inertia(pfc_handle h, int n_body, const double *inertia, const double *gravity) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        const char *who = "pfc_set_inertia";
        KinHost &K = c->kin;
        if (K.n_body == 0) return fail(c, PFC_ERR_STATE, "%s before pfc_set_mechanism", who);
        if (n_body != K.n_body) return fail(c, PFC_ERR_BAD_ARG, "%s: n_body is %d, the mechanism has %d bodies", who, n_body, K.n_body);
        if (!inertia || !gravity) return fail(c, PFC_ERR_BAD_ARG, "%s: null table", who);
        for (int r = 0; r < 3; ++r)
            if (!std::isfinite(gravity[r])) return fail(c, PFC_ERR_BAD_ARG, "%s: gravity is not finite", who);
        for (int b = 0; b < n_body; ++b) {
            const double *in = inertia + 13 * (size_t)b;
            if (!std::isfinite(in[12]) || in[12] < 0.0) return fail(c, PFC_ERR_BAD_ARG, "%s: body %d has the mass %.17g", who, b, in[12]);
            double big = 0.0;
            for (int e = 0; e < 12; ++e) {
                if (!std::isfinite(in[e])) return fail(c, PFC_ERR_BAD_ARG, "%s: body %d's inertia is not finite", who, b);
                if (e < 9) big = std::max(big, std::fabs(in[e]));
            }
            for (int r = 0; r < 3; ++r)
                for (int k = r + 1; k < 3; ++k)
                    if (std::fabs(in[3 * k + r] - in[3 * r + k]) > 1e-12 * big)
                        return fail(c, PFC_ERR_BAD_ARG, "%s: body %d's moment is not symmetric (M%d%d = %.17g, M%d%d = %.17g)", who, b, r, k,
                                    in[3 * k + r], k, r, in[3 * r + k]);
        }
        std::memcpy(K.blob.data() + K.o_inertia, inertia, sizeof(double) * 13 * (size_t)n_body);
        for (int r = 0; r < 3; ++r) K.gravity[r] = gravity[r];
        K.has_inertia = true;
        c->kin_stale = true;
        return PFC_OK; });
}

// What every dynamics call needs of the handle: a mechanism, its inertias, and a scene whose tables fit k_dynamics' LDS.
static int dyn_check_state(pfc_context *h, const char *who) {
    const KinHost &K = h->kin;
    if (K.n_body == 0) return fail(h, PFC_ERR_STATE, "%s before pfc_set_mechanism", who);
    if (!K.has_inertia) return fail(h, PFC_ERR_STATE, "%s before pfc_set_inertia", who);
    if (dyn_lds_bytes(K.n_body, K.nv) > kDynMaxLds)
        return fail(h, PFC_ERR_BAD_ARG, "%s: 44 n_body + 12.5 nv doubles must fit 64 KiB of LDS (n_body = %d, nv = %d)", who, K.n_body, K.nv);
    return PFC_OK;
}

static int dyn_check_args(pfc_context *h, const char *who, int n_scene, const double *q, const double *v, const double *x_w_b,
                          const double *twist_w_b, const double *qdot, const double *H, const double *c) {
    const int rc = dyn_check_state(h, who);
    if (rc != PFC_OK) return rc;
    if (n_scene < 0) return fail(h, PFC_ERR_BAD_ARG, "%s: negative n_scene", who);
    if (n_scene == 0 || h->kin.nv == 0) return PFC_OK;
    if ((qdot && (!q || !v)) || ((H || c) && !x_w_b) || (c && (!twist_w_b || !v)))
        return fail(h, PFC_ERR_BAD_ARG, "%s: null input (qdot needs q and v, H the poses, c the poses, the twists and v)", who);
    return PFC_OK;
}

// The tables' upload on st if they are stale, then k_dynamics on st.  Every pointer is a device pointer.
static int dyn_launch(pfc_context *h, int n_scene, const double *q, const double *v, const double *x_w_b, const double *twist_w_b,
                      double *qdot, double *H, double *c, hipStream_t st) {
    const KinHost &K = h->kin;
    if (K.nv == 0 || (!qdot && !H && !c)) return PFC_OK;
    { const int rc = kin_upload_tables(h, st); if (rc != PFC_OK) return rc; }
    DynArgs a;
    a.k = kin_table_args(h, n_scene, q, v);
    const char *t = h->kin_tab.p;
    a.inertia = (const double *)(t + K.o_inertia); a.sub_off = (const int *)(t + K.o_sub_off); a.sub = (const int *)(t + K.o_sub);
    for (int r = 0; r < 3; ++r) a.g[r] = K.gravity[r];
    a.x_w_b = x_w_b; a.twist_w_b = twist_w_b; a.qdot = qdot; a.H = H; a.c = c;
    hipLaunchKernelGGL(k_dynamics, dim3((unsigned)n_scene), dim3(kDynWave), dyn_lds_bytes(K.n_body, K.nv), st, a);
    HIP_TRY(h, hipGetLastError());
    return PFC_OK;
}

int pfc_dynamics_device(pfc_handle h, int n_scene, const double *d_q, const double *d_v, const double *d_x_w_b, const double *d_twist_w_b,
                        double *d_qdot, double *d_H, double *d_c, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) {
        const int rc = dyn_check_args(c, "pfc_dynamics_device", n_scene, d_q, d_v, d_x_w_b, d_twist_w_b, d_qdot, d_H, d_c);
        if (rc != PFC_OK || n_scene == 0) return rc;
        return dyn_launch(c, n_scene, d_q, d_v, d_x_w_b, d_twist_w_b, d_qdot, d_H, d_c, stream ? (hipStream_t)stream : c->stream); });
}

int pfc_dynamics(pfc_handle h, int n_scene, const double *q, const double *v, const double *x_w_b, const double *twist_w_b,
                 double *qdot, double *H, double *c) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c1) -> int {
        int rc = dyn_check_args(c1, "pfc_dynamics", n_scene, q, v, x_w_b, twist_w_b, qdot, H, c);
        if (rc != PFC_OK || n_scene == 0) return rc;
        HIP_TRY(c1, hipSetDevice(c1->device));
        const size_t ns = (size_t)n_scene, nb = ns * c1->kin.n_body, nv = (size_t)c1->kin.nv;
        Stage sg(c1->stage, c1->stream);
        const int k_q = sg.in(q, ns * c1->kin.nq), k_v = sg.in(v, ns * nv), k_x = sg.in(x_w_b, nb * 12), k_tw = sg.in(twist_w_b, nb * 6);
        const int k_qd = sg.out(qdot, ns * c1->kin.nq), k_H = sg.out(H, ns * nv * nv), k_c = sg.out(c, ns * nv);
        HIP_TRY(c1, sg.commit());
        rc = dyn_launch(c1, n_scene, sg.at<double>(k_q), sg.at<double>(k_v), sg.at<double>(k_x), sg.at<double>(k_tw), sg.at<double>(k_qd),
                        sg.at<double>(k_H), sg.at<double>(k_c), sg.st);
        if (rc != PFC_OK) return rc;
        HIP_TRY(c1, sg.finish());
        return PFC_OK; });
}

// The solve needs the mechanism's nv only; its cap is checked before anything is launched.
static int accel_check_state(pfc_context *h, const char *who) {
    if (h->kin.n_body == 0) return fail(h, PFC_ERR_STATE, "%s before pfc_set_mechanism", who);
    if (h->kin.nv > PFC_MAX_NV_SOLVE)
        return fail(h, PFC_ERR_BAD_ARG, "%s: nv is %d, the solve takes at most PFC_MAX_NV_SOLVE = %d", who, h->kin.nv, PFC_MAX_NV_SOLVE);
    return PFC_OK;
}

static int accel_check_args(pfc_context *h, const char *who, int n_scene, const double *H, const double *c, const double *f,
                            const double *vdot) {
    const int rc = accel_check_state(h, who);
    if (rc != PFC_OK) return rc;
    if (n_scene < 0) return fail(h, PFC_ERR_BAD_ARG, "%s: negative n_scene", who);
    if (n_scene > 0 && h->kin.nv > 0 && (!H || !c || !f || !vdot)) return fail(h, PFC_ERR_BAD_ARG, "%s: null buffer", who);
    return PFC_OK;
}

static int accel_launch(pfc_context *h, int n_scene, const double *H, const double *c, const double *f, const double *tau, double *vdot,
                        int *info, hipStream_t st) {
    HIP_TRY(h, hipSetDevice(h->device));
    const int nv = h->kin.nv;
    if (nv == 0) {      // nothing to solve: every scene's flag is 0
        if (info) HIP_TRY(h, hipMemsetAsync(info, 0, sizeof(int) * (size_t)n_scene, st));
        return PFC_OK;
    }
    AccelArgs a;
    a.n_scene = n_scene; a.nv = nv; a.H = H; a.c = c; a.f = f; a.tau = tau; a.vdot = vdot; a.info = info;
    hipLaunchKernelGGL(k_accel, dim3((unsigned)n_scene), dim3(kDynWave), accel_lds_bytes(nv), st, a);
    HIP_TRY(h, hipGetLastError());
    return PFC_OK;
}

int pfc_accelerations_device(pfc_handle h, int n_scene, const double *d_H, const double *d_c, const double *d_f, const double *d_tau,
                             double *d_vdot, int *d_info, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) {
        const int rc = accel_check_args(c, "pfc_accelerations_device", n_scene, d_H, d_c, d_f, d_vdot);
        if (rc != PFC_OK || n_scene == 0) return rc;
        return accel_launch(c, n_scene, d_H, d_c, d_f, d_tau, d_vdot, d_info, stream ? (hipStream_t)stream : c->stream); });
}

int pfc_accelerations(pfc_handle h, int n_scene, const double *H, const double *c, const double *f, const double *tau, double *vdot,
                      int *info) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c1) -> int {
        int rc = accel_check_args(c1, "pfc_accelerations", n_scene, H, c, f, vdot);
        if (rc != PFC_OK || n_scene == 0) return rc;
        HIP_TRY(c1, hipSetDevice(c1->device));
        const size_t ns = (size_t)n_scene, nv = (size_t)c1->kin.nv;
        Stage sg(c1->stage, c1->stream);
        const int k_H = sg.in(H, ns * nv * nv), k_c = sg.in(c, ns * nv), k_f = sg.in(f, ns * nv), k_t = sg.in(tau, ns * nv);
        const int k_vd = sg.out(vdot, ns * nv), k_i = sg.out(info, ns);
        HIP_TRY(c1, sg.commit());
        rc = accel_launch(c1, n_scene, sg.at<double>(k_H), sg.at<double>(k_c), sg.at<double>(k_f), sg.at<double>(k_t), sg.at<double>(k_vd),
                          sg.at<int>(k_i), sg.st);
        if (rc != PFC_OK) return rc;
        HIP_TRY(c1, sg.finish());
        return PFC_OK; });
}

int pfc_state_derivative(pfc_handle h, int n_items, const int *ins_ids, const int *scene, int n_scene,
                         const double *q, const double *v, const double *s, const double *tau,
                         double *x_w_b, double *twist_w_b, double *jac,
                         double *pose, double *twist, double *x_w_r2, int *body_1, int *body_2,
                         double *wrench, double *sdot, int *counts, double *f,
                         double *qdot, double *H, double *c, double *vdot, int *info) {
    if (!h) return PFC_ERR_BAD_ARG;
    const char *who = "pfc_state_derivative";
    pfc_context *c0 = first_ctx(h);
    int rc = on_shard(h, c0, [&](pfc_context *c1) {
        const int r = dyn_check_state(c1, who);
        return r != PFC_OK ? r : accel_check_state(c1, who); });
    if (rc != PFC_OK) return rc;
    if (!f || !qdot || !H || !c || !vdot) return fail(h, PFC_ERR_BAD_ARG, "%s: null buffer", who);
    std::vector<double> tmp;      // the body states, where the caller did not ask for them
    if (n_scene > 0 && (!x_w_b || !twist_w_b)) {
        const size_t nb = (size_t)n_scene * c0->kin.n_body;
        tmp.resize(nb * 18);
        if (!x_w_b) x_w_b = tmp.data();
        if (!twist_w_b) twist_w_b = tmp.data() + nb * 12;
    }
    rc = pfc_eval_state(h, n_items, ins_ids, scene, n_scene, q, v, s, x_w_b, twist_w_b, jac, pose, twist, x_w_r2, body_1, body_2, wrench, sdot,
                        counts, f);
    if (rc != PFC_OK) return rc;
    if ((rc = pfc_dynamics(h, n_scene, q, v, x_w_b, twist_w_b, qdot, H, c)) != PFC_OK) return rc;
    return pfc_accelerations(h, n_scene, H, c, f, tau, vdot, info);
}

// ---- Dual kinematics: partials of the body states and Jacobians (the second half of pfc_kin.h) ----------------------------------
// Argument and state checks of every form: those of pfc_kinematics, n_dir, and the grids of the two Dual kernels.
static int kin_dual_check_args(pfc_context *h, const char *who, int n_scene, int n_dir, const double *q, const double *v, bool want_twist) {
    const int rc = kin_check_args(h, who, n_scene, q, v, want_twist);
    if (rc != PFC_OK) return rc;
    if (n_dir < 1 || n_dir > 16) return fail(h, PFC_ERR_BAD_ARG, "%s: n_dir must be in 1..16", who);
    if (((long long)n_scene * h->kin.n_body * n_dir * std::max(h->kin.nv, 1) + kKinWave - 1) / kKinWave >= (1ll << 31))
        return fail(h, PFC_ERR_BAD_ARG, "%s: n_scene n_body n_dir nv must be below 2^37", who);
    return PFC_OK;
}

// The tables' upload if they are stale, dS_w grown if Jacobian partials are wanted and it is too small, and the kernels, on st.
// Every pointer is a device pointer; an output that is null is not written, and the kernel only it needs is not launched.
static int kin_dual_launch(pfc_context *h, int n_scene, int n_dir, const double *q, const double *v, const double *dq, const double *dv,
                           double *dx_w_b, double *dtwist_w_b, double *djac, hipStream_t st) {
    const KinHost &K = h->kin;
    { const int rc = kin_upload_tables(h, st); if (rc != PFC_OK) return rc; }
    const bool want_jac = djac && K.nv > 0;
    if (!dx_w_b && !dtwist_w_b && !want_jac) return PFC_OK;
    if (want_jac) HIP_TRY(h, h->kin_dsw.ensure((size_t)n_scene * n_dir * K.nv * 6));
    KinDualArgs a;
    a.k = kin_table_args(h, n_scene, q, v);
    a.n_dir = n_dir; a.dq = dq; a.dv = dv; a.dx_w_b = dx_w_b; a.dtwist_w_b = dtwist_w_b;
    a.dS_w = want_jac ? h->kin_dsw.p : nullptr; a.djac = djac;
    const long long lanes = (long long)n_scene * K.n_body * n_dir;
    hipLaunchKernelGGL(k_kinematics_dual, dim3((unsigned)((lanes + kKinWave - 1) / kKinWave)), dim3(kKinWave), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    if (want_jac) {
        const long long tot = lanes * K.nv;
        hipLaunchKernelGGL(k_kin_jacobian_dual, dim3((unsigned)((tot + kKinJacBlock - 1) / kKinJacBlock)), dim3(kKinJacBlock), 0, st, a);
        HIP_TRY(h, hipGetLastError());
    }
    return PFC_OK;
}

int pfc_kinematics_dual_device(pfc_handle h, int n_scene, int n_dir, const double *d_q, const double *d_v, const double *d_dq,
                               const double *d_dv, double *d_dx_w_b, double *d_dtwist_w_b, double *d_djac, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) {
        const int rc = kin_dual_check_args(c, "pfc_kinematics_dual_device", n_scene, n_dir, d_q, d_v, d_dtwist_w_b != nullptr);
        if (rc != PFC_OK || n_scene == 0) return rc;
        return kin_dual_launch(c, n_scene, n_dir, d_q, d_v, d_dq, d_dv, d_dx_w_b, d_dtwist_w_b, d_djac,
                               stream ? (hipStream_t)stream : c->stream); });
}

int pfc_kinematics_dual(pfc_handle h, int n_scene, int n_dir, const double *q, const double *v, const double *dq, const double *dv,
                        double *dx_w_b, double *dtwist_w_b, double *djac) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        int rc = kin_dual_check_args(c, "pfc_kinematics_dual", n_scene, n_dir, q, v, dtwist_w_b != nullptr);
        if (rc != PFC_OK || n_scene == 0) return rc;
        HIP_TRY(c, hipSetDevice(c->device));
        const size_t ns = (size_t)n_scene, nk = ns * n_dir, nbk = ns * c->kin.n_body * n_dir;
        Stage sg(c->stage, c->stream);
        const int k_q = sg.in(q, ns * c->kin.nq), k_v = sg.in(v, ns * c->kin.nv), k_dq = sg.in(dq, nk * c->kin.nq), k_dv = sg.in(dv, nk * c->kin.nv);
        const int k_x = sg.out(dx_w_b, nbk * 12), k_tw = sg.out(dtwist_w_b, nbk * 6), k_j = sg.out(djac, nbk * c->kin.nv * 6);
        HIP_TRY(c, sg.commit());
        rc = kin_dual_launch(c, n_scene, n_dir, sg.at<double>(k_q), sg.at<double>(k_v), sg.at<double>(k_dq), sg.at<double>(k_dv),
                             sg.at<double>(k_x), sg.at<double>(k_tw), sg.at<double>(k_j), sg.st);
        if (rc != PFC_OK) return rc;
        HIP_TRY(c, sg.finish());
        return PFC_OK; });
}

// What both chained Dual calls check before anything is launched or written: eval_state_check, n_dir and the Dual grids, and what the
// Dual scatter would refuse.
static int eval_dual_state_check(pfc_context *c, const char *who, int n_items, int n_dir, const int *ins_ids, const int *scene, int n_scene,
                                 const double *q, const double *v, bool scatter) {
    int rc = eval_state_check(c, who, n_items, ins_ids, scene, n_scene, false, q, v);
    if (rc != PFC_OK) return rc;
    if ((rc = kin_dual_check_args(c, who, n_scene, n_dir, q, v, true)) != PFC_OK) return rc;
    if (scatter && (long long)n_scene * n_items >= (1ll << 31)) return fail(c, PFC_ERR_BAD_ARG, "%s: n_scene * n_items must be below 2^31", who);
    return PFC_OK;
}

// ---- Dual forward dynamics: partials of qdot, H, c and vdot (the ScatDual instantiation and k_accel_dual of pfc_dyn.h) ------------
// What every Dual dynamics call needs of the handle: what the value call needs, and Dual tables -- twice the value tables -- that fit.
static int dyn_dual_check_state(pfc_context *h, const char *who) {
    const int rc = dyn_check_state(h, who);
    if (rc != PFC_OK) return rc;
    const KinHost &K = h->kin;
    if (dyn_lds_bytes(K.n_body, K.nv, sizeof(ScatDual)) > kDynMaxLds)
        return fail(h, PFC_ERR_BAD_ARG, "%s: the Dual tables, 88 n_body + 24.5 nv doubles, must fit 64 KiB of LDS (n_body = %d, nv = %d)", who,
                    K.n_body, K.nv);
    return PFC_OK;
}

static int dual_dir_check(pfc_context *h, const char *who, int n_scene, int n_dir) {
    if (n_scene < 0) return fail(h, PFC_ERR_BAD_ARG, "%s: negative n_scene", who);
    if (n_dir < 1 || n_dir > 16) return fail(h, PFC_ERR_BAD_ARG, "%s: n_dir must be in 1..16", who);
    if ((long long)n_scene * n_dir >= (1ll << 31)) return fail(h, PFC_ERR_BAD_ARG, "%s: n_scene n_dir must be below 2^31", who);
    return PFC_OK;
}

static int dyn_dual_check_args(pfc_context *h, const char *who, int n_scene, int n_dir, const double *q, const double *v,
                               const double *x_w_b, const double *twist_w_b, const double *dx_w_b, const double *dtwist_w_b,
                               const double *dqdot, const double *dH, const double *dc) {
    int rc = dyn_dual_check_state(h, who);
    if (rc != PFC_OK) return rc;
    if ((rc = dual_dir_check(h, who, n_scene, n_dir)) != PFC_OK) return rc;
    if (n_scene == 0 || h->kin.nv == 0) return PFC_OK;
    if ((dqdot && (!q || !v)) || ((dH || dc) && (!x_w_b || !dx_w_b)) || (dc && (!twist_w_b || !dtwist_w_b || !v)))
        return fail(h, PFC_ERR_BAD_ARG, "%s: null input (dqdot needs q and v, dH the poses and their partials, dc the poses, the twists, "
                    "their partials and v)", who);
    return PFC_OK;
}

// The tables' upload on st if they are stale, then k_dynamics_dual on st.  Every pointer is a device pointer.
static int dyn_dual_launch(pfc_context *h, int n_scene, int n_dir, const double *q, const double *v, const double *dq, const double *dv,
                           const double *x_w_b, const double *twist_w_b, const double *dx_w_b, const double *dtwist_w_b,
                           double *dqdot, double *dH, double *dc, hipStream_t st) {
    const KinHost &K = h->kin;
    if (K.nv == 0 || (!dqdot && !dH && !dc)) return PFC_OK;
    { const int rc = kin_upload_tables(h, st); if (rc != PFC_OK) return rc; }
    DynDualArgs a;
    a.d.k = kin_table_args(h, n_scene, q, v);
    const char *t = h->kin_tab.p;
    a.d.inertia = (const double *)(t + K.o_inertia); a.d.sub_off = (const int *)(t + K.o_sub_off); a.d.sub = (const int *)(t + K.o_sub);
    for (int r = 0; r < 3; ++r) a.d.g[r] = K.gravity[r];
    a.d.x_w_b = x_w_b; a.d.twist_w_b = twist_w_b; a.d.qdot = nullptr; a.d.H = nullptr; a.d.c = nullptr;
    a.n_dir = n_dir; a.dq = dq; a.dv = dv; a.dx_w_b = dx_w_b; a.dtwist_w_b = dtwist_w_b; a.dqdot = dqdot; a.dH = dH; a.dc = dc;
    hipLaunchKernelGGL(k_dynamics_dual, dim3((unsigned)n_scene * (unsigned)n_dir), dim3(kDynWave),
                       dyn_lds_bytes(K.n_body, K.nv, sizeof(ScatDual)), st, a);
    HIP_TRY(h, hipGetLastError());
    return PFC_OK;
}

int pfc_dynamics_dual_device(pfc_handle h, int n_scene, int n_dir, const double *d_q, const double *d_v, const double *d_dq,
                             const double *d_dv, const double *d_x_w_b, const double *d_twist_w_b, const double *d_dx_w_b,
                             const double *d_dtwist_w_b, double *d_dqdot, double *d_dH, double *d_dc, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) {
        const int rc = dyn_dual_check_args(c, "pfc_dynamics_dual_device", n_scene, n_dir, d_q, d_v, d_x_w_b, d_twist_w_b, d_dx_w_b,
                                           d_dtwist_w_b, d_dqdot, d_dH, d_dc);
        if (rc != PFC_OK || n_scene == 0) return rc;
        return dyn_dual_launch(c, n_scene, n_dir, d_q, d_v, d_dq, d_dv, d_x_w_b, d_twist_w_b, d_dx_w_b, d_dtwist_w_b, d_dqdot, d_dH, d_dc,
                               stream ? (hipStream_t)stream : c->stream); });
}

int pfc_dynamics_dual(pfc_handle h, int n_scene, int n_dir, const double *q, const double *v, const double *dq, const double *dv,
                      const double *x_w_b, const double *twist_w_b, const double *dx_w_b, const double *dtwist_w_b,
                      double *dqdot, double *dH, double *dc) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        int rc = dyn_dual_check_args(c, "pfc_dynamics_dual", n_scene, n_dir, q, v, x_w_b, twist_w_b, dx_w_b, dtwist_w_b, dqdot, dH, dc);
        if (rc != PFC_OK || n_scene == 0) return rc;
        HIP_TRY(c, hipSetDevice(c->device));
        const size_t ns = (size_t)n_scene, nk = ns * n_dir, nb = ns * c->kin.n_body, nv = (size_t)c->kin.nv, nq = (size_t)c->kin.nq;
        Stage sg(c->stage, c->stream);
        const int k_q = sg.in(q, ns * nq), k_v = sg.in(v, ns * nv), k_dq = sg.in(dq, nk * nq), k_dv = sg.in(dv, nk * nv);
        const int k_x = sg.in(x_w_b, nb * 12), k_tw = sg.in(twist_w_b, nb * 6), k_dx = sg.in(dx_w_b, nb * n_dir * 12),
                  k_dtw = sg.in(dtwist_w_b, nb * n_dir * 6);
        const int k_qd = sg.out(dqdot, nk * nq), k_H = sg.out(dH, nk * nv * nv), k_c = sg.out(dc, nk * nv);
        HIP_TRY(c, sg.commit());
        rc = dyn_dual_launch(c, n_scene, n_dir, sg.at<double>(k_q), sg.at<double>(k_v), sg.at<double>(k_dq), sg.at<double>(k_dv),
                             sg.at<double>(k_x), sg.at<double>(k_tw), sg.at<double>(k_dx), sg.at<double>(k_dtw), sg.at<double>(k_qd),
                             sg.at<double>(k_H), sg.at<double>(k_c), sg.st);
        if (rc != PFC_OK) return rc;
        HIP_TRY(c, sg.finish());
        return PFC_OK; });
}

static int accel_dual_check_args(pfc_context *h, const char *who, int n_scene, int n_dir, const double *H, const double *c, const double *f,
                                 const double *dH, const double *dc, const double *df, const double *dvdot) {
    int rc = accel_check_state(h, who);
    if (rc != PFC_OK) return rc;
    if ((rc = dual_dir_check(h, who, n_scene, n_dir)) != PFC_OK) return rc;
    if (n_scene > 0 && h->kin.nv > 0 && (!H || !c || !f || !dH || !dc || !df || !dvdot)) return fail(h, PFC_ERR_BAD_ARG, "%s: null buffer", who);
    return PFC_OK;
}

static int accel_dual_launch(pfc_context *h, int n_scene, int n_dir, const double *H, const double *c, const double *f, const double *tau,
                             const double *dH, const double *dc, const double *df, const double *dtau, double *vdot, double *dvdot,
                             int *info, hipStream_t st) {
    HIP_TRY(h, hipSetDevice(h->device));
    const int nv = h->kin.nv;
    if (nv == 0) {      // nothing to solve: every scene's flag is 0
        if (info) HIP_TRY(h, hipMemsetAsync(info, 0, sizeof(int) * (size_t)n_scene, st));
        return PFC_OK;
    }
    AccelDualArgs a;
    a.a.n_scene = n_scene; a.a.nv = nv; a.a.H = H; a.a.c = c; a.a.f = f; a.a.tau = tau; a.a.vdot = vdot; a.a.info = info;
    a.n_dir = n_dir; a.dH = dH; a.dc = dc; a.df = df; a.dtau = dtau; a.dvdot = dvdot;
    const int slots = accel_dual_slots(n_dir);
    const dim3 grid((unsigned)n_scene), block(kDynWave);
    const size_t lds = accel_lds_bytes(nv, 1 + slots);
    switch (slots) {
        case 1: hipLaunchKernelGGL(k_accel_dual<1>, grid, block, lds, st, a); break;
        case 2: hipLaunchKernelGGL(k_accel_dual<2>, grid, block, lds, st, a); break;
        case 4: hipLaunchKernelGGL(k_accel_dual<4>, grid, block, lds, st, a); break;
        case 8: hipLaunchKernelGGL(k_accel_dual<8>, grid, block, lds, st, a); break;
        default: hipLaunchKernelGGL(k_accel_dual<16>, grid, block, lds, st, a); break;
    }
    HIP_TRY(h, hipGetLastError());
    return PFC_OK;
}

int pfc_accelerations_dual_device(pfc_handle h, int n_scene, int n_dir, const double *d_H, const double *d_c, const double *d_f,
                                  const double *d_tau, const double *d_dH, const double *d_dc, const double *d_df, const double *d_dtau,
                                  double *d_vdot, double *d_dvdot, int *d_info, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) {
        const int rc = accel_dual_check_args(c, "pfc_accelerations_dual_device", n_scene, n_dir, d_H, d_c, d_f, d_dH, d_dc, d_df, d_dvdot);
        if (rc != PFC_OK || n_scene == 0) return rc;
        return accel_dual_launch(c, n_scene, n_dir, d_H, d_c, d_f, d_tau, d_dH, d_dc, d_df, d_dtau, d_vdot, d_dvdot, d_info,
                                 stream ? (hipStream_t)stream : c->stream); });
}

int pfc_accelerations_dual(pfc_handle h, int n_scene, int n_dir, const double *H, const double *c, const double *f, const double *tau,
                           const double *dH, const double *dc, const double *df, const double *dtau, double *vdot, double *dvdot,
                           int *info) {
    if (!h) return PFC_ERR_BAD_ARG;
    return on_shard(h, first_ctx(h), [&](pfc_context *c1) -> int {
        int rc = accel_dual_check_args(c1, "pfc_accelerations_dual", n_scene, n_dir, H, c, f, dH, dc, df, dvdot);
        if (rc != PFC_OK || n_scene == 0) return rc;
        HIP_TRY(c1, hipSetDevice(c1->device));
        const size_t ns = (size_t)n_scene, nk = ns * n_dir, nv = (size_t)c1->kin.nv;
        Stage sg(c1->stage, c1->stream);
        const int k_H = sg.in(H, ns * nv * nv), k_c = sg.in(c, ns * nv), k_f = sg.in(f, ns * nv), k_t = sg.in(tau, ns * nv);
        const int k_dH = sg.in(dH, nk * nv * nv), k_dc = sg.in(dc, nk * nv), k_df = sg.in(df, nk * nv), k_dt = sg.in(dtau, nk * nv);
        const int k_vd = sg.out(vdot, ns * nv), k_dvd = sg.out(dvdot, nk * nv), k_i = sg.out(info, ns);
        HIP_TRY(c1, sg.commit());
        rc = accel_dual_launch(c1, n_scene, n_dir, sg.at<double>(k_H), sg.at<double>(k_c), sg.at<double>(k_f), sg.at<double>(k_t),
                               sg.at<double>(k_dH), sg.at<double>(k_dc), sg.at<double>(k_df), sg.at<double>(k_dt), sg.at<double>(k_vd),
                               sg.at<double>(k_dvd), sg.at<int>(k_i), sg.st);
        if (rc != PFC_OK) return rc;
        HIP_TRY(c1, sg.finish());
        return PFC_OK; });
}

// ---- the continuous feedback law (k_feedback, k_feedback_dual: pfc_feedback.h; the statements: include/pfc.h) -------------------------
// What both parts check of the law's sizes and tables before any launch.
static int feedback_check_law(pfc_context *h, const char *who, int nv, const FeedbackLaw &w) {
    if (nv < 1 || nv > PFC_MAX_NV_SOLVE)
        return fail(h, PFC_ERR_BAD_ARG, "%s: nv is %d, the law takes 1 .. PFC_MAX_NV_SOLVE = %d coordinates", who, nv, PFC_MAX_NV_SOLVE);
    if (w.n_act < 0 || w.n_act > nv) return fail(h, PFC_ERR_BAD_ARG, "%s: n_act is %d, 0 .. nv = %d", who, w.n_act, nv);
    if (w.n_seg < 1) return fail(h, PFC_ERR_BAD_ARG, "%s: n_seg is %d, at least one segment", who, w.n_seg);
    if (w.n_sched < 1) return fail(h, PFC_ERR_BAD_ARG, "%s: n_scene is %d, at least one scene's schedule", who, w.n_sched);
    return PFC_OK;
}

static bool feedback_law_null(const FeedbackLaw &w) {
    return (w.n_act > 0 && (!w.act || !w.kp || !w.kd || !w.seg_q)) || (w.n_seg > 1 && !w.seg_t) || !w.t;
}

static int feedback_launch(pfc_context *h, const FeedbackArgs &a, hipStream_t st) {
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_feedback, dim3((unsigned)a.n_rows), dim3(kFbWave), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    return PFC_OK;
}

static int feedback_dual_launch(pfc_context *h, const FeedbackDualArgs &a, hipStream_t st) {
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_feedback_dual, dim3((unsigned)a.n_scene * (unsigned)a.n_dir), dim3(kFbWave), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    return PFC_OK;
}

// The parts behind the public entries and the chains: sizes and buffers checked, then the launcher.
static int feedback_checked(pfc_context *h, const char *who, const FeedbackArgs &a, hipStream_t st) {
    const int rc = feedback_check_law(h, who, a.nv, a.w);
    if (rc != PFC_OK) return rc;
    if (a.n_rows < 0 || a.n_rows % a.w.n_sched != 0)
        return fail(h, PFC_ERR_BAD_ARG, "%s: n_rows is %d, a multiple >= 0 of n_scene = %d", who, a.n_rows, a.w.n_sched);
    if (a.n_rows == 0) return PFC_OK;
    if (feedback_law_null(a.w) || !a.q || !a.v || !a.H || !a.c || !a.w.tau) return fail(h, PFC_ERR_BAD_ARG, "%s: null buffer", who);
    return feedback_launch(h, a, st);
}

static int feedback_dual_checked(pfc_context *h, const char *who, const FeedbackDualArgs &a, hipStream_t st) {
    int rc = feedback_check_law(h, who, a.nv, a.w);
    if (rc != PFC_OK || (rc = dual_dir_check(h, who, a.n_scene, a.n_dir)) != PFC_OK) return rc;
    if (a.n_scene % a.w.n_sched != 0)
        return fail(h, PFC_ERR_BAD_ARG, "%s: n_rows is %d, a multiple of n_scene = %d", who, a.n_scene, a.w.n_sched);
    if (a.n_scene == 0) return PFC_OK;
    if (feedback_law_null(a.w) || !a.q || !a.v || (a.w.n_act > 0 && (!a.H || !a.dH || !a.dc)) || !a.w.dtau) return fail(h, PFC_ERR_BAD_ARG, "%s: null buffer", who);
    return feedback_dual_launch(h, a, st);
}

// The law of a chained call on its value buffers: tau = law + V.tau into law->tau.
static int feedback_of_call(pfc_context *h, const char *who, const StateCall &S, hipStream_t st) {
    FeedbackArgs a{};
    a.w = *S.law; a.n_rows = S.n_scene; a.nv = h->kin.nv;
    a.q = S.val.q; a.v = S.val.v; a.H = S.val.H; a.c = S.val.c; a.tau_in = S.val.tau;
    return feedback_checked(h, who, a, st);
}

static int feedback_dual_of_call(pfc_context *h, const char *who, const StateCall &S, hipStream_t st) {
    FeedbackDualArgs a{};
    a.w = *S.law; a.n_scene = S.n_scene; a.n_dir = S.n_dir; a.nv = h->kin.nv;
    a.q = S.val.q; a.v = S.val.v; a.H = S.val.H; a.dq = S.par.q; a.dv = S.par.v; a.dH = S.par.H; a.dc = S.par.c;
    return feedback_dual_checked(h, who, a, st);
}

int pfc_feedback_device(pfc_handle h, int n_rows, int n_scene, int nv, int n_act, int n_seg, const int *d_act, const double *d_kp,
                        const double *d_kd, const double *d_a_max, const double *d_seg_t, const double *d_seg_q, const double *d_seg_ff,
                        const double *d_t, const double *d_q, const double *d_v, const double *d_H, const double *d_c,
                        const double *d_tau_in, double *d_tau_out, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    FeedbackArgs a{};
    a.w.n_sched = n_scene; a.w.n_act = n_act; a.w.n_seg = n_seg; a.w.act = d_act; a.w.kp = d_kp; a.w.kd = d_kd; a.w.a_max = d_a_max;
    a.w.seg_t = d_seg_t; a.w.seg_q = d_seg_q; a.w.seg_ff = d_seg_ff; a.w.t = d_t; a.w.tau = d_tau_out;
    a.n_rows = n_rows; a.nv = nv; a.q = d_q; a.v = d_v; a.H = d_H; a.c = d_c; a.tau_in = d_tau_in;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) {
        return feedback_checked(c, "pfc_feedback_device", a, stream ? (hipStream_t)stream : c->stream); });
}

int pfc_feedback_dual_device(pfc_handle h, int n_rows, int n_dir, int n_scene, int nv, int n_act, int n_seg, const int *d_act,
                             const double *d_kp, const double *d_kd, const double *d_a_max, const double *d_seg_t, const double *d_seg_q,
                             const double *d_t, const double *d_q, const double *d_v, const double *d_H, const double *d_dq,
                             const double *d_dv, const double *d_dH, const double *d_dc, double *d_dtau, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    FeedbackDualArgs a{};
    a.w.n_sched = n_scene; a.w.n_act = n_act; a.w.n_seg = n_seg; a.w.act = d_act; a.w.kp = d_kp; a.w.kd = d_kd; a.w.a_max = d_a_max;
    a.w.seg_t = d_seg_t; a.w.seg_q = d_seg_q; a.w.t = d_t; a.w.dtau = d_dtau;
    a.n_scene = n_rows; a.n_dir = n_dir; a.nv = nv; a.q = d_q; a.v = d_v; a.H = d_H; a.dq = d_dq; a.dv = d_dv; a.dH = d_dH; a.dc = d_dc;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) {
        return feedback_dual_checked(c, "pfc_feedback_dual_device", a, stream ? (hipStream_t)stream : c->stream); });
}

// ---- applied body wrenches (k_body_wrench, k_body_wrench_dual: pfc_body_wrench.h; the statements: include/pfc.h) ------------------------
// What both parts check of the sizes and tables before any launch.
static int body_wrench_check(pfc_context *h, const char *who, int nv, const BodyWrenches &w) {
    if (nv < 1 || nv > PFC_MAX_NV_SOLVE)
        return fail(h, PFC_ERR_BAD_ARG, "%s: nv is %d, the wrenches take 1 .. PFC_MAX_NV_SOLVE = %d coordinates", who, nv, PFC_MAX_NV_SOLVE);
    if (w.n_body < 1) return fail(h, PFC_ERR_BAD_ARG, "%s: n_body is %d, at least one body", who, w.n_body);
    if (w.n_w < 0) return fail(h, PFC_ERR_BAD_ARG, "%s: n_w is %d, not negative", who, w.n_w);
    if (w.n_seg < 1) return fail(h, PFC_ERR_BAD_ARG, "%s: n_seg is %d, at least one segment", who, w.n_seg);
    if (w.n_sched < 1) return fail(h, PFC_ERR_BAD_ARG, "%s: n_scene is %d, at least one scene's schedule", who, w.n_sched);
    return PFC_OK;
}

static bool body_wrench_null(const BodyWrenches &w) {
    return (w.n_w > 0 && (!w.body || !w.frame || !w.point || !w.seg_w)) || (w.n_seg > 1 && !w.seg_t) || !w.t;
}

static int body_wrench_launch(pfc_context *h, const BodyWrenchArgs &a, hipStream_t st) {
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_body_wrench, dim3((unsigned)a.n_rows), dim3(kBwWave), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    return PFC_OK;
}

static int body_wrench_dual_launch(pfc_context *h, const BodyWrenchDualArgs &a, hipStream_t st) {
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_body_wrench_dual, dim3((unsigned)a.n_scene * (unsigned)a.n_dir), dim3(kBwWave), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    return PFC_OK;
}

// The parts behind the public entries and the chains: sizes and buffers checked, then the launcher.
static int body_wrench_checked(pfc_context *h, const char *who, const BodyWrenchArgs &a, hipStream_t st) {
    const int rc = body_wrench_check(h, who, a.nv, a.w);
    if (rc != PFC_OK) return rc;
    if (a.n_rows < 0 || a.n_rows % a.w.n_sched != 0)
        return fail(h, PFC_ERR_BAD_ARG, "%s: n_rows is %d, a multiple >= 0 of n_scene = %d", who, a.n_rows, a.w.n_sched);
    if (a.n_rows == 0) return PFC_OK;
    if (body_wrench_null(a.w) || (a.w.n_w > 0 && (!a.x_w_b || !a.jac)) || !a.w.tau) return fail(h, PFC_ERR_BAD_ARG, "%s: null buffer", who);
    return body_wrench_launch(h, a, st);
}

static int body_wrench_dual_checked(pfc_context *h, const char *who, const BodyWrenchDualArgs &a, hipStream_t st) {
    int rc = body_wrench_check(h, who, a.nv, a.w);
    if (rc != PFC_OK || (rc = dual_dir_check(h, who, a.n_scene, a.n_dir)) != PFC_OK) return rc;
    if (a.n_scene % a.w.n_sched != 0)
        return fail(h, PFC_ERR_BAD_ARG, "%s: n_rows is %d, a multiple of n_scene = %d", who, a.n_scene, a.w.n_sched);
    if (a.n_scene == 0) return PFC_OK;
    if (body_wrench_null(a.w) || (a.w.n_w > 0 && (!a.x_w_b || !a.jac || !a.dx_w_b || !a.djac)) || !a.w.dtau)
        return fail(h, PFC_ERR_BAD_ARG, "%s: null buffer", who);
    return body_wrench_dual_launch(h, a, st);
}

// The wrenches of a chained call on its value buffers, behind the law: tau = (law->tau or V.tau) + the wrenches into push->tau.
static int body_wrench_of_call(pfc_context *h, const char *who, const StateCall &S, hipStream_t st) {
    BodyWrenchArgs a{};
    a.w = *S.push; a.n_rows = S.n_scene; a.nv = h->kin.nv;
    a.x_w_b = S.val.x_w_b; a.jac = S.val.jac; a.tau_in = S.law ? S.law->tau : S.val.tau;
    return body_wrench_checked(h, who, a, st);
}

static int body_wrench_dual_of_call(pfc_context *h, const char *who, const StateCall &S, hipStream_t st) {
    BodyWrenchDualArgs a{};
    a.w = *S.push; a.n_scene = S.n_scene; a.n_dir = S.n_dir; a.nv = h->kin.nv;
    a.x_w_b = S.val.x_w_b; a.jac = S.val.jac; a.dx_w_b = S.par.x_w_b; a.djac = S.par.jac; a.dtau_in = S.law ? S.law->dtau : S.par.tau;
    return body_wrench_dual_checked(h, who, a, st);
}

// The tau and dtau the solve of a chained call reads: the wrenches' sums, else the law's, else the call's own.
static const double *solve_tau(const StateCall &S) { return S.push ? S.push->tau : S.law ? S.law->tau : S.val.tau; }
static const double *solve_dtau(const StateCall &S) { return S.push ? S.push->dtau : S.law ? S.law->dtau : S.par.tau; }

int pfc_body_wrench_device(pfc_handle h, int n_rows, int n_scene, int n_body, int nv, int n_w, int n_seg, const int *d_body,
                           const int *d_frame, const double *d_point, const double *d_seg_t, const double *d_seg_w, const double *d_t,
                           const double *d_x_w_b, const double *d_jac, const double *d_tau_in, double *d_tau_out, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    BodyWrenchArgs a{};
    a.w.n_sched = n_scene; a.w.n_body = n_body; a.w.n_w = n_w; a.w.n_seg = n_seg; a.w.body = d_body; a.w.frame = d_frame;
    a.w.point = d_point; a.w.seg_t = d_seg_t; a.w.seg_w = d_seg_w; a.w.t = d_t; a.w.tau = d_tau_out;
    a.n_rows = n_rows; a.nv = nv; a.x_w_b = d_x_w_b; a.jac = d_jac; a.tau_in = d_tau_in;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) {
        return body_wrench_checked(c, "pfc_body_wrench_device", a, stream ? (hipStream_t)stream : c->stream); });
}

int pfc_body_wrench_dual_device(pfc_handle h, int n_rows, int n_dir, int n_scene, int n_body, int nv, int n_w, int n_seg,
                                const int *d_body, const int *d_frame, const double *d_point, const double *d_seg_t,
                                const double *d_seg_w, const double *d_t, const double *d_x_w_b, const double *d_jac,
                                const double *d_dx_w_b, const double *d_djac, const double *d_dtau_in, double *d_dtau, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    BodyWrenchDualArgs a{};
    a.w.n_sched = n_scene; a.w.n_body = n_body; a.w.n_w = n_w; a.w.n_seg = n_seg; a.w.body = d_body; a.w.frame = d_frame;
    a.w.point = d_point; a.w.seg_t = d_seg_t; a.w.seg_w = d_seg_w; a.w.t = d_t; a.w.dtau = d_dtau;
    a.n_scene = n_rows; a.n_dir = n_dir; a.nv = nv; a.x_w_b = d_x_w_b; a.jac = d_jac; a.dx_w_b = d_dx_w_b; a.djac = d_djac;
    a.dtau_in = d_dtau_in;
    return on_shard(h, first_ctx(h), [&](pfc_context *c) {
        return body_wrench_dual_checked(c, "pfc_body_wrench_dual_device", a, stream ? (hipStream_t)stream : c->stream); });
}

// What both Dual chains check before the first launch, beyond what the Dual evaluation checks itself: the inertias, the Dual LDS
// limit, the nv cap and n_dir.
static int state_derivative_dual_check(pfc_context *c, const char *who, int n_scene, int n_dir) {
    int rc = dyn_dual_check_state(c, who);
    if (rc != PFC_OK) return rc;
    if ((rc = accel_check_state(c, who)) != PFC_OK) return rc;
    return dual_dir_check(c, who, n_scene, n_dir);
}

// The broadphase pose of a host Dual call (m.float's state: calcTriTetIntersections!, non_friction.jl:94-101) is kept in pinned
// host memory, which the value pass reads in place (96 bytes per item, once): *bp_pose becomes that block's device-visible
// address.  A pose other than the previous call's -- or none after one -- ends everything a previous evaluation left to reuse.
static int keep_bp_pose(pfc_context *h, int n_items, const double **bp_pose) {
    if (n_items <= 0) *bp_pose = nullptr;
    if (!*bp_pose) {
        if (h->pin_bp_n == 0) return PFC_OK;
        // the previous host-buffer Dual evaluation culled with a pose of its own: its lists are not this evaluation's
        end_kept_pass(h);
        forget_host_points(h);
        h->pin_bp_n = 0;
        return PFC_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t bytes = sizeof(double) * 24 * (size_t)n_items;
    bool moved;
    HIP_TRY(h, h->pin_bp.ensure(bytes, &moved));
    if (moved) h->pin_bp_n = -1;
    if (h->pin_bp_n != n_items || std::memcmp(h->pin_bp.p, *bp_pose, bytes) != 0) {
        // another broadphase pose: nothing a previous Dual evaluation left can be reused (the candidate lists differ)
        end_kept_pass(h);
        forget_host_points(h);
        std::memcpy(h->pin_bp.p, *bp_pose, bytes);
        h->pin_bp_n = n_items;
    }
    void *dev = nullptr;
    HIP_TRY(h, hipHostGetDevicePointer(&dev, h->pin_bp.p, 0));
    *bp_pose = (const double *)dev;
    return PFC_OK;
}

// The host-pointer Dual evaluation: argument checks, the broadphase pose, then the first route that takes the call (DESIGN.md
// "Host Dual routes").
int pfc_eval_dual_bp(pfc_handle h, int n_items, int n_dir, const int *ins_ids, const double *pose, const double *bp_pose,
                     const double *twist, const double *s, const double *d_pose, const double *d_twist, const double *d_s,
                     double *wrench, double *sdot, double *d_wrench, double *d_sdot, int *counts) {
    if (!h) return PFC_ERR_BAD_ARG;
    if (h->multi)
        return multi_eval_dual(h, n_items, n_dir, ins_ids, pose, bp_pose, twist, s, d_pose, d_twist, d_s, wrench, sdot, d_wrench, d_sdot, counts);
    { const int rc = keep_bp_pose(h, n_items, &bp_pose); if (rc != PFC_OK) return rc; }
    if (n_dir < 1 || n_dir > 16) return fail(h, PFC_ERR_BAD_ARG, "pfc_eval_dual: n_dir must be in 1..16");
    if (n_items > 0 && (!d_pose || !d_twist || !d_wrench || !d_sdot))
        return fail(h, PFC_ERR_BAD_ARG, "pfc_eval_dual: null buffer");
    { const int rc = check_eval_args(h, n_items, ins_ids, pose, twist, s, wrench, sdot); if (rc != PFC_OK) return rc; }
    // A repeat of the previous small-scene Dual evaluation's point (the next chunk of a Jacobian)?
    const bool repeat = n_items > 0 && h->opt_dual_reuse && h->pin_in_pt.n == n_items && h->pin_in.p && h->pin_in_pt.ids == (ins_ids != nullptr) &&
                        same_point(ValueBlock(h->pin_in.p, (size_t)n_items, h->pin_in_pt.ids_at), ins_ids, pose, twist, s, false);
    if (!repeat) h->pin_in_pt = {};
    if (n_items == 0) return PFC_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const DualCall c = {n_items, n_dir, ins_ids, pose, twist, s, d_pose, d_twist, d_s, wrench, sdot, d_wrench, d_sdot, counts, bp_pose};
    int rc;
    if (takes_fused(h, c, repeat)) {
        if (h->dual_fused_skip > 0) --h->dual_fused_skip;
        else if ((rc = eval_dual_fused(h, c)) != PFC_ERR_OVERFLOW) return rc;      // else: an item did not fit
    }
    if (takes_hybrid(h, n_items, c.nk(), PassOpts{bp_pose})) {
        if ((rc = eval_dual_hybrid(h, c)) != PFC_ERR_OVERFLOW) return rc;          // else: lists grown / speculation short
        if (h->dual_dev_hyb_skip < 1) h->dual_dev_hyb_skip = 1;   // (not the same sequence again inside pfc_eval_dual_device)
    }
    if (takes_small(h, c) && (rc = eval_dual_small(h, c)) != PFC_ERR_OVERFLOW) return rc;      // else: as above
    return takes_one_sync(h) ? eval_dual_one_sync(h, c) : eval_dual_two_stage(h, c);
}

int pfc_eval_dual(pfc_handle h, int n_items, int n_dir, const int *ins_ids, const double *pose, const double *twist,
                  const double *s, const double *d_pose, const double *d_twist, const double *d_s, double *wrench,
                  double *sdot, double *d_wrench, double *d_sdot, int *counts) {
    return pfc_eval_dual_bp(h, n_items, n_dir, ins_ids, pose, nullptr, twist, s, d_pose, d_twist, d_s, wrench, sdot, d_wrench, d_sdot, counts);
}

int pfc_set_option(pfc_handle h, const char *name, long long value) {
    if (!h || !name) return PFC_ERR_BAD_ARG;
    if (h->multi) {
        if (!std::strcmp(name, "multi_min")) { h->multi->opt_min_items = value < 1 ? 1 : (int)value; h->multi->part_n = 0; return PFC_OK; }
        h->multi->dev_kept = false;      // (as every shard's kept pass below)
        for (pfc_context *c : h->multi->shard) {
            const int rc = on_shard(h, c, [&](pfc_context *c1) { return pfc_set_option(c1, name, value); });
            if (rc != PFC_OK) return rc;
        }
        return PFC_OK;
    }
    end_kept_pass(h);      // every option change ends the kept pass, also one that sets an option to what it is
    if (!std::strcmp(name, "debug")) h->opt_debug = value != 0;
    else if (!std::strcmp(name, "profile")) h->opt_profile = value != 0;
    else if (!std::strcmp(name, "max_levels")) {
        if (value < 0 || value > (1 << 20) || (h->finalized && value > h->max_levels))
            return fail(h, PFC_ERR_BAD_ARG, "max_levels must be 0 (automatic) or 1..%d (depth of the finalized trees + 1)", h->max_levels);
        h->opt_max_levels = (int)value; h->ghave[0] = h->ghave[1] = false; h->dghave = false;
    }
    else if (!std::strcmp(name, "bfs_levels")) h->opt_bfs_levels = (int)value;
    else if (!std::strcmp(name, "graph")) h->opt_graph = value != 0;
    else if (!std::strcmp(name, "split_min")) h->opt_split_min = (int)value;
    else if (!std::strcmp(name, "dual_reuse")) h->opt_dual_reuse = (int)value;
    else if (!std::strcmp(name, "clip_min")) { h->opt_clip_min = (int)value; h->ghave[0] = h->ghave[1] = false; h->dghave = false; }
    else if (!std::strcmp(name, "clip_queue")) { h->opt_clip_queue = (int)value; h->ghave[0] = h->ghave[1] = false; h->dghave = false; }
    else if (!std::strcmp(name, "vertex_fields")) {
        if (value != 0 && value != 1) return fail(h, PFC_ERR_BAD_ARG, "vertex_fields must be 0 (per-point k_fric) or 1 (per-corner fields)");
        h->opt_vertex_fields = (int)value; h->ghave[0] = h->ghave[1] = false; h->dghave = false;
    }
    else if (!std::strcmp(name, "bin_split")) {
        const long long sp = value < 0 ? -value : value;
        if (value != 0 && (sp < 3 || sp > 9))
            return fail(h, PFC_ERR_BAD_ARG, "bin_split must be 0 (dense fill), 3..9 (polygons of fewer vertices fill a 512-candidate chunk from its front) or -9..-3 (chunks of every size)");
        h->opt_bin_split = (int)value; h->ghave[0] = h->ghave[1] = false; h->dghave = false;
    }
    else if (!std::strcmp(name, "integ_spec")) {
        if (value < 0 || value > 2)
            return fail(h, PFC_ERR_BAD_ARG, "integ_spec must be 0 (general k_integ), 1 (bristle-only form, two waves per SIMD) or 2 (the same at three waves)");
        h->opt_integ_spec = (int)value; h->ghave[0] = h->ghave[1] = false; h->dghave = false;
    }
    else if (!std::strcmp(name, "quad_const")) {
        if (value != 0 && value != 1) return fail(h, PFC_ERR_BAD_ARG, "quad_const must be 0 (the kernels read the item's quadrature rule) or 1 (rule 2 as a constant where every instruction has it)");
        h->opt_quad_const = (int)value; h->ghave[0] = h->ghave[1] = false; h->dghave = false;
    }
    else if (!std::strcmp(name, "poison")) h->opt_poison = value != 0;
    else if (!std::strcmp(name, "fused")) { h->opt_fused = value != 0; h->fused_skip = 0; }
    else if (!std::strcmp(name, "team")) h->opt_team = value < 0 ? 0 : (value > kTeamMaxWg ? kTeamMaxWg : (int)value);
    else if (!std::strcmp(name, "team_fault")) h->opt_team_fault = (int)value;
    else if (!std::strcmp(name, "fused_f32")) h->opt_fused_f32 = value != 0;
    else if (!std::strcmp(name, "dual_fold")) { h->opt_dual_fold = value != 0; h->dghave = false; }
    else if (!std::strcmp(name, "fixed_order")) {
        // the batched path only while it is on, whatever "fused" / "team" / "split_min" / "graph" say (fused_ok, fused_team, the split
        // rule and use_graph look at it): no one-launch kernel, no two-half split, eager launches (the sort is library code)
        const int on = value != 0;
        if (on != h->opt_fixed_order) {      // (setting it to what it is keeps the graphs and the record list)
            h->opt_fixed_order = on; h->fused_skip = 0;
            h->ghave[0] = h->ghave[1] = false; h->dghave = false;
            h->rec.release();      // (the records change their stride)
        }
    }
    else if (!std::strcmp(name, "no_filter")) { h->opt_no_filter = (int)value; h->ghave[0] = h->ghave[1] = false; h->dghave = false; }
    else return fail(h, PFC_ERR_BAD_ARG, "unknown option %s", name);
    return PFC_OK;
}

int pfc_get_stats(pfc_handle h, long long *out8) {
    if (!h || !out8) return PFC_ERR_BAD_ARG;
    if (h->multi) { for (int k = 0; k < 8; ++k) out8[k] = h->multi->stats[k]; return PFC_OK; }
    for (int k = 0; k < 8; ++k) out8[k] = h->stats[k];
    return PFC_OK;
}

int pfc_get_stage_ms(pfc_handle h, float *out6) {
    if (!h || !out6) return PFC_ERR_BAD_ARG;
    // the first shard's stages (every shard runs the same sequence on its range)
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        if (!c->ev_valid) return fail(c, PFC_ERR_STATE, "profile option was off for the last evaluation");
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipEventSynchronize(c->ev[EV_FIN]));
        for (int k = 0; k < 5; ++k) HIP_TRY(c, hipEventElapsedTime(&out6[k], c->ev[k], c->ev[k + 1]));
        HIP_TRY(c, hipEventElapsedTime(&out6[5], c->ev[EV_START], c->ev[EV_FIN]));
        if (c->last_parts == 2 && c->twin && c->twin->ev_valid) {
            // two concurrent halves: mean duration of a stage over the two half-launches, total = the longer half
            pfc_context *t = c->twin;
            float b[6];
            HIP_TRY(c, hipEventSynchronize(t->ev[EV_FIN]));
            for (int k = 0; k < 5; ++k) HIP_TRY(c, hipEventElapsedTime(&b[k], t->ev[k], t->ev[k + 1]));
            HIP_TRY(c, hipEventElapsedTime(&b[5], t->ev[EV_START], t->ev[EV_FIN]));
            for (int k = 0; k < 5; ++k) out6[k] = 0.5f * (out6[k] + b[k]);
            if (b[5] > out6[5]) out6[5] = b[5];
        }
        return PFC_OK; });
}

int pfc_last_parts(pfc_handle h) { return h ? (h->multi ? pfc_last_parts(h->multi->shard[0]) : (h->last_fused ? 0 : h->last_parts)) : 0; }
int pfc_last_team(pfc_handle h) { return h ? (h->multi ? pfc_last_team(h->multi->shard[0]) : (h->last_fused ? h->last_fu_nw : 0)) : 0; }
int pfc_last_dual_reused(pfc_handle h) {
    if (!h) return 0;
    if (h->multi) {      // 1 only if every shard that took part reused its value pass
        for (int k = 0; k < h->multi->n_used; ++k)
            if (h->multi->bound[k + 1] > h->multi->bound[k] && !h->multi->shard[k]->last_dual_reused) return 0;
        return 1;
    }
    return h->last_dual_reused ? 1 : 0;
}

int pfc_debug_pairs(pfc_handle h, int item, int *pairs, int *clip_n, int cap) {
    if (!h) return -PFC_ERR_BAD_ARG;
    if (h->multi) {
        int local = 0;
        pfc_context *c = multi_locate(h, item, &local);
        if (!c) return -fail(h, PFC_ERR_BAD_ARG, "bad item");
        return on_shard(h, c, [&](pfc_context *c1) { return pfc_debug_pairs(c1, local, pairs, clip_n, cap); }, true);
    }
    if (!h->opt_debug) return -fail(h, PFC_ERR_STATE, "debug option is off");
    { int rc = drain(h); if (rc) return -rc; }
    if (item < 0 || item >= h->last_n_items) return -fail(h, PFC_ERR_BAD_ARG, "bad item");
    size_t nc = (size_t)h->stats[1];
    std::vector<WorkRec> c(nc);
    std::vector<int> cn(nc);
    if (nc) {
        if (copy_sync(h, c.data(), h->cand.p, sizeof(WorkRec) * nc, hipMemcpyDeviceToHost) != hipSuccess ||
            copy_sync(h, cn.data(), h->clip_n.p, sizeof(int) * nc, hipMemcpyDeviceToHost) != hipSuccess)
            return -fail(h, PFC_ERR_HIP, "copy failed");
    }
    int n = 0;
    for (size_t k = 0; k < nc; ++k)
        if (c[k].item == item) {
            if (n < cap) {
                if (pairs) { pairs[2 * n] = c[k].a; pairs[2 * n + 1] = c[k].b; }
                if (clip_n) clip_n[n] = cn[k];
            }
            ++n;
        }
    return n;
}

int pfc_debug_tractions(pfc_handle h, int item, double *buf, int cap) {
    if (!h) return -PFC_ERR_BAD_ARG;
    if (h->multi) {
        int local = 0;
        pfc_context *c = multi_locate(h, item, &local);
        if (!c) return -fail(h, PFC_ERR_BAD_ARG, "bad item");
        return on_shard(h, c, [&](pfc_context *c1) { return pfc_debug_tractions(c1, local, buf, cap); }, true);
    }
    if (!h->opt_debug) return -fail(h, PFC_ERR_STATE, "debug option is off");
    { int rc = drain(h); if (rc) return -rc; }
    if (item < 0 || item >= h->last_n_items) return -fail(h, PFC_ERR_BAD_ARG, "bad item");
    size_t nt = (size_t)h->last_tslots;
    std::vector<int> ti(nt);
    std::vector<double> td(nt * 8);
    if (nt) {
        if (copy_sync(h, ti.data(), h->trac_item.p, sizeof(int) * nt, hipMemcpyDeviceToHost) != hipSuccess)
            return -fail(h, PFC_ERR_HIP, "copy failed");
        for (int a = 0; a < 8; ++a)
            if (copy_sync(h, td.data() + a * nt, h->trac_d.p + a * h->tcap, sizeof(double) * nt, hipMemcpyDeviceToHost) != hipSuccess)
                return -fail(h, PFC_ERR_HIP, "copy failed");
    }
    int n = 0;
    for (size_t k = 0; k < nt; ++k)
        if (ti[k] == item) {
            if (n < cap && buf)
                for (int a = 0; a < 8; ++a) buf[8 * (size_t)n + a] = td[a * nt + k];
            ++n;
        }
    return n;
}

int pfc_debug_stiffness(pfc_handle h, int item, double *K36, double *Kis36, double *Sinv6, double *cop3) {
    if (!h) return -PFC_ERR_BAD_ARG;
    if (h->multi) {
        int local = 0;
        pfc_context *c = multi_locate(h, item, &local);
        if (!c) return -fail(h, PFC_ERR_BAD_ARG, "bad item");
        return on_shard(h, c, [&](pfc_context *c1) { return pfc_debug_stiffness(c1, local, K36, Kis36, Sinv6, cop3); }, true);
    }
    { int rc = drain(h); if (rc) return -rc; }
    if (h->last_fused)      // the fused small-scene kernel keeps K in LDS only
        return -fail(h, PFC_ERR_STATE, "pfc_debug_stiffness: set option debug (or fused = 0) before the evaluation");
    if (item < 0 || item >= h->last_n_items) return -fail(h, PFC_ERR_BAD_ARG, "bad item");
    std::vector<double> r(kResStride);
    int ic[4];
    if (copy_sync(h, r.data(), h->res.p + (size_t)item * kResStride, sizeof(double) * kResStride, hipMemcpyDeviceToHost) != hipSuccess ||
        copy_sync(h, ic, h->icnt.p + 4 * (size_t)item, sizeof ic, hipMemcpyDeviceToHost) != hipSuccess)
        return -fail(h, PFC_ERR_HIP, "copy failed");
    if (ic[3] == 0) return 0;
    if (K36) std::memcpy(K36, r.data() + kResK, sizeof(double) * 36);
    if (Kis36) std::memcpy(Kis36, r.data() + kResKis, sizeof(double) * 36);
    if (Sinv6) std::memcpy(Sinv6, r.data() + kResSinv, sizeof(double) * 6);
    if (cop3) std::memcpy(cop3, r.data() + kResCop, sizeof(double) * 3);
    return 1;
}

// Both forms of pfc_scatter_generalized behind their checks: f zeroed unless it accumulates, then k_scatter, enqueued on st.
static int scatter_launch(pfc_context *h, int n_items, int nv, const double *wrench, const double *x_w_r2, const int *body_1, const int *body_2,
                          const int *scene, int n_scene, const double *jac, double *f, int accumulate, hipStream_t st) {
    HIP_TRY(h, hipSetDevice(h->device));
    if (!accumulate) HIP_TRY(h, hipMemsetAsync(f, 0, sizeof(double) * (size_t)n_scene * nv, st));
    if (n_items > 0) {
        ScatterArgs a;
        a.n_items = n_items; a.nv = nv; a.wrench = wrench; a.x_w_r2 = x_w_r2; a.body_1 = body_1; a.body_2 = body_2;
        a.scene = scene; a.jac = jac; a.f = f;
        const long long tot = (long long)n_items * nv;
        hipLaunchKernelGGL(k_scatter, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, a);
        HIP_TRY(h, hipGetLastError());
    }
    return PFC_OK;
}

int pfc_scatter_generalized(pfc_handle h, int n_items, const double *wrench, const double *x_w_r2, const int *body_1,
                            const int *body_2, const int *scene, int n_scene, int n_body, int nv, const double *jac,
                            double *f_out) {
    if (!h) return PFC_ERR_BAD_ARG;
    // a few microseconds of work: the first device does it
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        if (n_items < 0 || nv <= 0 || n_scene <= 0 || n_body < 0 || !f_out)
            return fail(c, PFC_ERR_BAD_ARG, "pfc_scatter_generalized: bad argument");
        if (n_items > 0 && (!wrench || !x_w_r2 || !body_1 || !body_2 || (n_body > 0 && !jac)))
            return fail(c, PFC_ERR_BAD_ARG, "pfc_scatter_generalized: null buffer");
        for (int i = 0; i < n_items; ++i) {
            if (body_1[i] >= n_body || body_2[i] >= n_body || (scene && (scene[i] < 0 || scene[i] >= n_scene)))
                return fail(c, PFC_ERR_BAD_ARG, "pfc_scatter_generalized: body / scene id out of range (item %d)", i);
        }
        HIP_TRY(c, hipSetDevice(c->device));
        const size_t n = (size_t)n_items, nf = (size_t)n_scene * nv, nj = n ? (size_t)n_body * 6 * nv : 0;
        Stage sg(c->stage, c->stream);
        const int k_w = sg.in(wrench, n * 6), k_x = sg.in(x_w_r2, n * 12), k_j = sg.in(jac, nj);
        const int k_b1 = sg.in(body_1, n), k_b2 = sg.in(body_2, n), k_sc = sg.in(scene, n), k_f = sg.out(f_out, nf);
        HIP_TRY(c, sg.commit());
        const int rc = scatter_launch(c, n_items, nv, sg.at<double>(k_w), sg.at<double>(k_x), sg.at<int>(k_b1), sg.at<int>(k_b2),
                                      sg.at<int>(k_sc), n_scene, sg.at<double>(k_j), sg.at<double>(k_f), 0, sg.st);
        if (rc != PFC_OK) return rc;
        HIP_TRY(c, sg.finish());
        return PFC_OK; });
}

int pfc_scatter_generalized_device(pfc_handle h, int n_items, const double *d_wrench, const double *d_x_w_r2, const int *d_body_1,
                                   const int *d_body_2, const int *d_scene, int n_scene, int nv, const double *d_jac, double *d_f,
                                   int accumulate, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    // the wrenches of a multi-device evaluation end up on the first device: so does this
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        if (n_items < 0 || nv <= 0 || n_scene <= 0 || !d_f) return fail(c, PFC_ERR_BAD_ARG, "pfc_scatter_generalized_device: bad argument");
        if (n_items > 0 && (!d_wrench || !d_x_w_r2 || !d_body_1 || !d_body_2 || !d_jac))
            return fail(c, PFC_ERR_BAD_ARG, "pfc_scatter_generalized_device: null buffer");
        return scatter_launch(c, n_items, nv, d_wrench, d_x_w_r2, d_body_1, d_body_2, d_scene, n_scene, d_jac, d_f, accumulate,
                              stream ? (hipStream_t)stream : c->stream); });
}

// pfc_scatter_generalized_dual[_device] behind the scene CSR (keys / off, or NULL: one segment): the world wrenches and the ordered
// projection (pfc_scatter.h), enqueued on st.
static int scatter_dual_launch(pfc_handle h, int n_items, int n_dir, const double *wrench, const double *dwrench, const double *x_w_r2,
                               const double *dx_w_r2, const int *body_1, const int *body_2, const int *keys, const int *off, int n_scene,
                               int nv, const double *jac, const double *djac, double *f, double *df, int accumulate, hipStream_t st) {
    const size_t n = (size_t)n_items, nc = 1 + (size_t)n_dir;
    HIP_TRY(h, h->sdual_w.ensure(n * nc * 6 + 1));
    if (n_items > 0) {
        const long long lanes = (long long)n * nc;
        const long long g = std::min<long long>((lanes + 255) / 256, 1 << 16);
        hipLaunchKernelGGL(k_scat_world, dim3((unsigned)g), dim3(256), 0, st, n_items, n_dir, wrench, dwrench, x_w_r2, dx_w_r2,
                           h->sdual_w.p);
        HIP_TRY(h, hipGetLastError());
    }
    ScatDualArgs a;
    a.n_items = n_items; a.n_dir = n_dir; a.nv = nv; a.n_scene = n_scene; a.n_jb = (nv + kScatJB - 1) / kScatJB;
    a.accumulate = accumulate ? 1 : 0; a.W = h->sdual_w.p; a.jac = jac; a.djac = djac; a.body_1 = body_1; a.body_2 = body_2;
    a.keys = keys; a.off = off; a.f = f; a.df = df;
    const long long blocks = (long long)n_scene * (long long)nc * a.n_jb;
    hipLaunchKernelGGL(k_scat_proj, dim3((unsigned)std::min<long long>(blocks, 1 << 16)), dim3(256), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    return PFC_OK;
}

int pfc_scatter_generalized_dual(pfc_handle h, int n_items, int n_dir, const double *wrench, const double *d_wrench,
                                 const double *x_w_r2, const double *d_x_w_r2, const int *body_1, const int *body_2,
                                 const int *scene, int n_scene, int n_body, int nv, const double *jac, const double *d_jac,
                                 double *f_out, double *d_f_out) {
    if (!h) return PFC_ERR_BAD_ARG;
    // as pfc_scatter_generalized: the first device does it
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        if (n_items < 0 || n_dir < 1 || n_dir > kScatMaxDir || nv <= 0 || n_scene <= 0 || n_body < 0 || !d_f_out)
            return fail(c, PFC_ERR_BAD_ARG, "pfc_scatter_generalized_dual: bad argument");
        if ((long long)n_scene * n_items >= (1ll << 31))
            return fail(c, PFC_ERR_BAD_ARG, "pfc_scatter_generalized_dual: n_scene * n_items must be below 2^31");
        if (n_items > 0 && (!wrench || !d_wrench || !x_w_r2 || !body_1 || !body_2 || (n_body > 0 && !jac)))
            return fail(c, PFC_ERR_BAD_ARG, "pfc_scatter_generalized_dual: null buffer");
        for (int i = 0; i < n_items; ++i) {
            if (body_1[i] >= n_body || body_2[i] >= n_body || (scene && (scene[i] < 0 || scene[i] >= n_scene)))
                return fail(c, PFC_ERR_BAD_ARG, "pfc_scatter_generalized_dual: body / scene id out of range (item %d)", i);
        }
        HIP_TRY(c, hipSetDevice(c->device));
        const size_t n = (size_t)n_items, nd = (size_t)n_dir, nf = (size_t)n_scene * nv, nj = n ? (size_t)n_body * nv * 6 : 0;
        std::vector<int> keys, off;
        if (scene && n_items > 0) {      // the items by scene in ascending item order: a counting sort
            off.assign((size_t)n_scene + 1, 0);
            for (int i = 0; i < n_items; ++i) ++off[(size_t)scene[i] + 1];
            for (int s = 0; s < n_scene; ++s) off[(size_t)s + 1] += off[(size_t)s];
            std::vector<int> fill(off.begin(), off.end() - 1);
            keys.resize(n);
            for (int i = 0; i < n_items; ++i) keys[(size_t)fill[(size_t)scene[i]]++] = scene[i] * n_items + i;
        }
        Stage sg(c->stage, c->stream);
        const int k_w = sg.in(wrench, n * 6), k_dw = sg.in(d_wrench, n * nd * 6), k_x = sg.in(x_w_r2, n * 12), k_dx = sg.in(d_x_w_r2, n * nd * 12);
        const int k_j = sg.in(jac, nj), k_dj = sg.in(d_jac, nj * nd), k_b1 = sg.in(body_1, n), k_b2 = sg.in(body_2, n);
        const int k_keys = sg.in(keys.empty() ? nullptr : keys.data(), keys.size()), k_off = sg.in(off.empty() ? nullptr : off.data(), off.size());
        const int k_f = sg.out(f_out, nf), k_df = sg.out(d_f_out, nf * nd);
        HIP_TRY(c, sg.commit());
        const int rc = scatter_dual_launch(c, n_items, n_dir, sg.at<double>(k_w), sg.at<double>(k_dw), sg.at<double>(k_x), sg.at<double>(k_dx),
                                           sg.at<int>(k_b1), sg.at<int>(k_b2), sg.at<int>(k_keys), sg.at<int>(k_off), n_scene, nv,
                                           sg.at<double>(k_j), sg.at<double>(k_dj), sg.at<double>(k_f), sg.at<double>(k_df), 0, sg.st);
        if (rc != PFC_OK) return rc;
        HIP_TRY(c, sg.finish());
        return PFC_OK; });
}

// The scene CSR of the device form on st, in the context's own buffers: the items by scene in ascending item order -- sorted keys
// scene * n_items + item, offsets per scene -- or both null (no d_scene, or no items: one segment).
static int scatter_dual_csr(pfc_context *h, int n_items, const int *d_scene, int n_scene, hipStream_t st, int **keys, int **off) {
    HIP_TRY(h, hipSetDevice(h->device));
    *keys = *off = nullptr;
    if (!d_scene || n_items <= 0) return PFC_OK;
    const size_t n = (size_t)n_items;
    size_t bytes = 0;
    HIP_TRY(h, h->sdual_i.ensure(n * 3 + (size_t)n_scene + 2));
    HIP_TRY(h, pfc_sort_temp_bytes(n, 32, &bytes));
    HIP_TRY(h, h->sdual_tmp.ensure(bytes ? bytes : 1));
    *keys = h->sdual_i.p; *off = *keys + n;
    int *count = *off + n_scene + 1;
    unsigned *kin = reinterpret_cast<unsigned *>(count + 1), *kout = kin + n;
    hipLaunchKernelGGL(k_scat_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n_items, n_scene, d_scene, *keys, count);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, pfc_sort_indices(*keys, count, n, kin, kout, h->sdual_tmp.p, h->sdual_tmp.cap, st));
    hipLaunchKernelGGL(k_scat_off, dim3((unsigned)(((size_t)n_scene + 256) / 256)), dim3(256), 0, st, n_items, n_scene, *keys, *off);
    HIP_TRY(h, hipGetLastError());
    return PFC_OK;
}

int pfc_scatter_generalized_dual_device(pfc_handle h, int n_items, int n_dir, const double *d_wrench_val, const double *d_dwrench,
                                        const double *d_x_w_r2, const double *d_dx_w_r2, const int *d_body_1, const int *d_body_2,
                                        const int *d_scene, int n_scene, int nv, const double *d_jac, const double *d_djac,
                                        double *d_f, double *d_df, int accumulate, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    // the wrenches of a multi-device evaluation end up on the first device: so does this
    return on_shard(h, first_ctx(h), [&](pfc_context *c) -> int {
        if (n_items < 0 || n_dir < 1 || n_dir > kScatMaxDir || nv <= 0 || n_scene <= 0 || !d_df)
            return fail(c, PFC_ERR_BAD_ARG, "pfc_scatter_generalized_dual_device: bad argument");
        if ((long long)n_scene * n_items >= (1ll << 31))
            return fail(c, PFC_ERR_BAD_ARG, "pfc_scatter_generalized_dual_device: n_scene * n_items must be below 2^31");
        if (n_items > 0 && (!d_wrench_val || !d_dwrench || !d_x_w_r2 || !d_body_1 || !d_body_2 || !d_jac))
            return fail(c, PFC_ERR_BAD_ARG, "pfc_scatter_generalized_dual_device: null buffer");
        hipStream_t st = stream ? (hipStream_t)stream : c->stream;
        int *keys, *off;
        const int rc = scatter_dual_csr(c, n_items, d_scene, n_scene, st, &keys, &off);
        if (rc != PFC_OK) return rc;
        return scatter_dual_launch(c, n_items, n_dir, d_wrench_val, d_dwrench, d_x_w_r2, d_dx_w_r2, d_body_1, d_body_2, keys, off, n_scene,
                                   nv, d_jac, d_djac, d_f, d_df, accumulate, st); });
}

// ---- the chains from joint states: kinematics, the items and their evaluation, the third-law scatter, dynamics and the solve -----
// What the stages' own entries would check again has been checked by the chain (eval_state_check, eval_dual_state_check, the
// state checks of the dynamics and the null-buffer lists): the stage launches are called directly, with the record's fields.
static int eval_state(pfc_context *h, const StateCall &S) {
    const char *who = "pfc_eval_state_device";
    const StateBufs &V = S.val;
    pfc_context *c = first_ctx(h);
    int rc = on_shard(h, c, [&](pfc_context *c1) { return eval_state_check(c1, who, S.n_items, S.ins_ids, S.scene, S.n_scene, false, V.q, V.v); });
    if (rc != PFC_OK) return rc;
    const int nv = c->kin.nv;
    const bool scatter = V.f && nv > 0;
    if (!V.x_w_b || !V.twist_w_b || !V.pose || !V.twist || !V.wrench || !V.sdot || (scatter && (!V.jac || !V.x_w_r2 || !V.body_1 || !V.body_2)))
        return fail(h, PFC_ERR_BAD_ARG, "%s: null buffer", who);
    rc = on_shard(h, c, [&](pfc_context *c1) { return kin_launch(c1, S.n_scene, V.q, V.v, V.x_w_b, V.twist_w_b, V.jac, call_stream(c1, S)); });
    if (rc != PFC_OK || (rc = eval_bodies(h, S, c->kin.n_body)) != PFC_OK || !scatter) return rc;
    return on_shard(h, c, [&](pfc_context *c1) {
        return scatter_launch(c1, S.n_items, nv, V.wrench, V.x_w_r2, V.body_1, V.body_2, S.scene, S.n_scene, V.jac, V.f, 0, call_stream(c1, S)); });
}

static int state_derivative(pfc_context *h, const StateCall &S) {
    const char *who = "pfc_state_derivative_device";
    const StateBufs &V = S.val;
    pfc_context *c = first_ctx(h);
    int rc = on_shard(h, c, [&](pfc_context *c1) {
        const int r = dyn_check_state(c1, who);
        return r != PFC_OK ? r : accel_check_state(c1, who); });
    if (rc != PFC_OK) return rc;
    if (!V.f || !V.qdot || !V.H || !V.c || !V.vdot) return fail(h, PFC_ERR_BAD_ARG, "%s: null buffer", who);
    if ((rc = eval_state(h, S)) != PFC_OK) return rc;
    return on_shard(h, c, [&](pfc_context *c1) {
        const hipStream_t st = call_stream(c1, S);
        int r = dyn_launch(c1, S.n_scene, V.q, V.v, V.x_w_b, V.twist_w_b, V.qdot, V.H, V.c, st);
        if (r == PFC_OK && S.law) r = feedback_of_call(c1, who, S, st);
        if (r == PFC_OK && S.push) r = body_wrench_of_call(c1, who, S, st);
        return r != PFC_OK ? r : accel_launch(c1, S.n_scene, V.H, V.c, V.f, solve_tau(S), V.vdot, V.info, st); });
}

// `more`: another chunk of directions at the point of the last checked first call -- only partials are written, the values are read.
static int eval_dual_state(pfc_context *h, const StateCall &S, bool more) {
    const char *who = more ? "pfc_eval_dual_state_device_more" : "pfc_eval_dual_state_device";
    const StateBufs &V = S.val, &P = S.par;
    pfc_context *c = first_ctx(h);
    const int nv = c->kin.nv;
    const bool scatter = P.f && nv > 0;
    int rc = on_shard(h, c, [&](pfc_context *c1) {
        return eval_dual_state_check(c1, who, S.n_items, S.n_dir, S.ins_ids, S.scene, S.n_scene, V.q, V.v, scatter); });
    if (rc != PFC_OK) return rc;
    if (more && !h->multi) {      // _more's own preconditions, before the partials are written
        if (!h->device_kept())
            return fail(h, PFC_ERR_STATE, "%s: no checked pfc_eval_dual_device evaluation on this handle to extend", who);
        if (S.n_items != h->kept.n)
            return fail(h, PFC_ERR_BAD_ARG, "%s: n_items is %d, the kept evaluation has %d items", who, S.n_items, h->kept.n);
    }
    if (!V.x_w_b || !V.twist_w_b || !P.x_w_b || !P.twist_w_b || !P.pose || !P.twist || !P.wrench || !P.sdot ||
        (!more && (!V.pose || !V.twist || !V.wrench || !V.sdot)) ||
        (scatter && (!V.jac || !P.jac || !V.x_w_r2 || !P.x_w_r2 || !V.body_1 || !V.body_2 || (more && !V.wrench))))
        return fail(h, PFC_ERR_BAD_ARG, "%s: null buffer", who);
    rc = on_shard(h, c, [&](pfc_context *c1) {
        const hipStream_t st = call_stream(c1, S);
        const int r = more ? PFC_OK : kin_launch(c1, S.n_scene, V.q, V.v, V.x_w_b, V.twist_w_b, V.jac, st);
        return r != PFC_OK ? r : kin_dual_launch(c1, S.n_scene, S.n_dir, V.q, V.v, P.q, P.v, P.x_w_b, P.twist_w_b, P.jac, st); });
    if (rc != PFC_OK || (rc = eval_dual_bodies(h, S, c->kin.n_body, more)) != PFC_OK || !scatter) return rc;
    return on_shard(h, c, [&](pfc_context *c1) {
        const hipStream_t st = call_stream(c1, S);
        int *keys, *off;
        const int r = scatter_dual_csr(c1, S.n_items, S.scene, S.n_scene, st, &keys, &off);
        if (r != PFC_OK) return r;
        return scatter_dual_launch(c1, S.n_items, S.n_dir, V.wrench, P.wrench, V.x_w_r2, P.x_w_r2, V.body_1, V.body_2, keys, off, S.n_scene, nv,
                                   V.jac, P.jac, more ? nullptr : V.f, P.f, 0, st); });
}

static int state_derivative_dual(pfc_context *h, const StateCall &S, bool more) {
    const char *who = more ? "pfc_state_derivative_dual_device_more" : "pfc_state_derivative_dual_device";
    const StateBufs &V = S.val, &P = S.par;
    pfc_context *c = first_ctx(h);
    int rc = on_shard(h, c, [&](pfc_context *c1) { return state_derivative_dual_check(c1, who, S.n_scene, S.n_dir); });
    if (rc != PFC_OK) return rc;
    if (!V.f || !P.f || !V.H || !V.c || !P.qdot || !P.H || !P.c || !P.vdot || (!more && (!V.qdot || !V.vdot)))
        return fail(h, PFC_ERR_BAD_ARG, "%s: null buffer", who);
    if ((rc = eval_dual_state(h, S, more)) != PFC_OK) return rc;
    return on_shard(h, c, [&](pfc_context *c1) {
        const hipStream_t st = call_stream(c1, S);
        int r = more ? PFC_OK : dyn_launch(c1, S.n_scene, V.q, V.v, V.x_w_b, V.twist_w_b, V.qdot, V.H, V.c, st);
        if (r != PFC_OK) return r;
        r = dyn_dual_launch(c1, S.n_scene, S.n_dir, V.q, V.v, P.q, P.v, V.x_w_b, V.twist_w_b, P.x_w_b, P.twist_w_b, P.qdot, P.H, P.c, st);
        if (r != PFC_OK) return r;
        if (S.law) {      // the law's value on a first chunk only (a `more` chunk reads what it left), its partials on every chunk
            if (!more && (r = feedback_of_call(c1, who, S, st)) != PFC_OK) return r;
            if ((r = feedback_dual_of_call(c1, who, S, st)) != PFC_OK) return r;
        }
        if (S.push) {     // the wrenches behind the law, likewise
            if (!more && (r = body_wrench_of_call(c1, who, S, st)) != PFC_OK) return r;
            if ((r = body_wrench_dual_of_call(c1, who, S, st)) != PFC_OK) return r;
        }
        return accel_dual_launch(c1, S.n_scene, S.n_dir, V.H, V.c, V.f, solve_tau(S), P.H, P.c, P.f, solve_dtau(S),
                                 more ? nullptr : V.vdot, P.vdot, more ? nullptr : V.info, st); });
}

// The six entries: one fill of the record each -- the only place a parameter position meets a field name -- and one call.
int pfc_eval_state_device(pfc_handle h, int n_items, const int *d_ins_ids, const int *d_scene, int n_scene,
                          const double *d_q, const double *d_v, const double *d_s,
                          double *d_x_w_b, double *d_twist_w_b, double *d_jac,
                          double *d_pose, double *d_twist, double *d_x_w_r2, int *d_body_1, int *d_body_2,
                          double *d_wrench, double *d_sdot, int *d_counts, double *d_f, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    StateCall S = state_call_head(n_items, 0, d_ins_ids, d_scene, n_scene, stream);
    StateBufs &V = S.val;
    V.q = d_q; V.v = d_v; V.s = d_s;
    V.x_w_b = d_x_w_b; V.twist_w_b = d_twist_w_b; V.jac = d_jac;
    V.pose = d_pose; V.twist = d_twist; V.x_w_r2 = d_x_w_r2; V.body_1 = d_body_1; V.body_2 = d_body_2;
    V.wrench = d_wrench; V.sdot = d_sdot; V.counts = d_counts; V.f = d_f;
    return eval_state(h, S);
}

int pfc_state_derivative_device(pfc_handle h, int n_items, const int *d_ins_ids, const int *d_scene, int n_scene,
                                const double *d_q, const double *d_v, const double *d_s, const double *d_tau,
                                double *d_x_w_b, double *d_twist_w_b, double *d_jac,
                                double *d_pose, double *d_twist, double *d_x_w_r2, int *d_body_1, int *d_body_2,
                                double *d_wrench, double *d_sdot, int *d_counts, double *d_f,
                                double *d_qdot, double *d_H, double *d_c, double *d_vdot, int *d_info, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    StateCall S = state_call_head(n_items, 0, d_ins_ids, d_scene, n_scene, stream);
    StateBufs &V = S.val;
    V.q = d_q; V.v = d_v; V.s = d_s; V.tau = d_tau;
    V.x_w_b = d_x_w_b; V.twist_w_b = d_twist_w_b; V.jac = d_jac;
    V.pose = d_pose; V.twist = d_twist; V.x_w_r2 = d_x_w_r2; V.body_1 = d_body_1; V.body_2 = d_body_2;
    V.wrench = d_wrench; V.sdot = d_sdot; V.counts = d_counts; V.f = d_f;
    V.qdot = d_qdot; V.H = d_H; V.c = d_c; V.vdot = d_vdot; V.info = d_info;
    return state_derivative(h, S);
}

int pfc_eval_dual_state_device(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const int *d_scene, int n_scene,
                               const double *d_q, const double *d_v, const double *d_dq, const double *d_dv,
                               const double *d_s, const double *d_ds,
                               double *d_x_w_b, double *d_twist_w_b, double *d_jac,
                               double *d_dx_w_b, double *d_dtwist_w_b, double *d_djac,
                               double *d_pose, double *d_twist, double *d_x_w_r2, int *d_body_1, int *d_body_2,
                               double *d_dpose, double *d_dtwist, double *d_dx_w_r2,
                               double *d_wrench, double *d_sdot, double *d_dwrench, double *d_dsdot, int *d_counts,
                               double *d_f, double *d_df, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    StateCall S = state_call_head(n_items, n_dir, d_ins_ids, d_scene, n_scene, stream);
    StateBufs &V = S.val, &P = S.par;
    V.q = d_q; V.v = d_v; V.s = d_s; P.q = d_dq; P.v = d_dv; P.s = d_ds;
    V.x_w_b = d_x_w_b; V.twist_w_b = d_twist_w_b; V.jac = d_jac; P.x_w_b = d_dx_w_b; P.twist_w_b = d_dtwist_w_b; P.jac = d_djac;
    V.pose = d_pose; V.twist = d_twist; V.x_w_r2 = d_x_w_r2; V.body_1 = d_body_1; V.body_2 = d_body_2;
    P.pose = d_dpose; P.twist = d_dtwist; P.x_w_r2 = d_dx_w_r2;
    V.wrench = d_wrench; V.sdot = d_sdot; P.wrench = d_dwrench; P.sdot = d_dsdot; V.counts = d_counts; V.f = d_f; P.f = d_df;
    return eval_dual_state(h, S, false);
}

int pfc_eval_dual_state_device_more(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const int *d_scene, int n_scene,
                                    const double *d_q, const double *d_v, const double *d_dq, const double *d_dv, const double *d_ds,
                                    const double *d_x_w_b, const double *d_twist_w_b, const double *d_jac,
                                    double *d_dx_w_b, double *d_dtwist_w_b, double *d_djac,
                                    const double *d_x_w_r2, const int *d_body_1, const int *d_body_2, const double *d_wrench,
                                    double *d_dpose, double *d_dtwist, double *d_dx_w_r2, double *d_dwrench, double *d_dsdot,
                                    double *d_df, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    StateCall S = state_call_head(n_items, n_dir, d_ins_ids, d_scene, n_scene, stream);
    StateBufs &V = S.val, &P = S.par;
    V.q = d_q; V.v = d_v; P.q = d_dq; P.v = d_dv; P.s = d_ds;
    V.x_w_b = kept_value(d_x_w_b); V.twist_w_b = kept_value(d_twist_w_b); V.jac = kept_value(d_jac);
    P.x_w_b = d_dx_w_b; P.twist_w_b = d_dtwist_w_b; P.jac = d_djac;
    V.x_w_r2 = kept_value(d_x_w_r2); V.body_1 = kept_value(d_body_1); V.body_2 = kept_value(d_body_2); V.wrench = kept_value(d_wrench);
    P.pose = d_dpose; P.twist = d_dtwist; P.x_w_r2 = d_dx_w_r2; P.wrench = d_dwrench; P.sdot = d_dsdot; P.f = d_df;
    return eval_dual_state(h, S, true);
}

int pfc_state_derivative_dual_device(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const int *d_scene, int n_scene,
                                     const double *d_q, const double *d_v, const double *d_dq, const double *d_dv,
                                     const double *d_s, const double *d_ds, const double *d_tau, const double *d_dtau,
                                     double *d_x_w_b, double *d_twist_w_b, double *d_jac,
                                     double *d_dx_w_b, double *d_dtwist_w_b, double *d_djac,
                                     double *d_pose, double *d_twist, double *d_x_w_r2, int *d_body_1, int *d_body_2,
                                     double *d_dpose, double *d_dtwist, double *d_dx_w_r2,
                                     double *d_wrench, double *d_sdot, double *d_dwrench, double *d_dsdot, int *d_counts,
                                     double *d_f, double *d_df,
                                     double *d_qdot, double *d_H, double *d_c, double *d_vdot, int *d_info,
                                     double *d_dqdot, double *d_dH, double *d_dc, double *d_dvdot, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    StateCall S = state_call_head(n_items, n_dir, d_ins_ids, d_scene, n_scene, stream);
    StateBufs &V = S.val, &P = S.par;
    V.q = d_q; V.v = d_v; V.s = d_s; V.tau = d_tau; P.q = d_dq; P.v = d_dv; P.s = d_ds; P.tau = d_dtau;
    V.x_w_b = d_x_w_b; V.twist_w_b = d_twist_w_b; V.jac = d_jac; P.x_w_b = d_dx_w_b; P.twist_w_b = d_dtwist_w_b; P.jac = d_djac;
    V.pose = d_pose; V.twist = d_twist; V.x_w_r2 = d_x_w_r2; V.body_1 = d_body_1; V.body_2 = d_body_2;
    P.pose = d_dpose; P.twist = d_dtwist; P.x_w_r2 = d_dx_w_r2;
    V.wrench = d_wrench; V.sdot = d_sdot; P.wrench = d_dwrench; P.sdot = d_dsdot; V.counts = d_counts; V.f = d_f; P.f = d_df;
    V.qdot = d_qdot; V.H = d_H; V.c = d_c; V.vdot = d_vdot; V.info = d_info; P.qdot = d_dqdot; P.H = d_dH; P.c = d_dc; P.vdot = d_dvdot;
    return state_derivative_dual(h, S, false);
}

int pfc_state_derivative_dual_device_more(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const int *d_scene, int n_scene,
                                          const double *d_q, const double *d_v, const double *d_dq, const double *d_dv, const double *d_ds,
                                          const double *d_tau, const double *d_dtau,
                                          const double *d_x_w_b, const double *d_twist_w_b, const double *d_jac,
                                          double *d_dx_w_b, double *d_dtwist_w_b, double *d_djac,
                                          const double *d_x_w_r2, const int *d_body_1, const int *d_body_2, const double *d_wrench,
                                          double *d_dpose, double *d_dtwist, double *d_dx_w_r2, double *d_dwrench, double *d_dsdot,
                                          double *d_df, const double *d_H, const double *d_c, const double *d_f,
                                          double *d_dqdot, double *d_dH, double *d_dc, double *d_dvdot, void *stream) {
    if (!h) return PFC_ERR_BAD_ARG;
    StateCall S = state_call_head(n_items, n_dir, d_ins_ids, d_scene, n_scene, stream);
    StateBufs &V = S.val, &P = S.par;
    V.q = d_q; V.v = d_v; V.tau = d_tau; P.q = d_dq; P.v = d_dv; P.s = d_ds; P.tau = d_dtau;
    V.x_w_b = kept_value(d_x_w_b); V.twist_w_b = kept_value(d_twist_w_b); V.jac = kept_value(d_jac);
    P.x_w_b = d_dx_w_b; P.twist_w_b = d_dtwist_w_b; P.jac = d_djac;
    V.x_w_r2 = kept_value(d_x_w_r2); V.body_1 = kept_value(d_body_1); V.body_2 = kept_value(d_body_2); V.wrench = kept_value(d_wrench);
    P.pose = d_dpose; P.twist = d_dtwist; P.x_w_r2 = d_dx_w_r2; P.wrench = d_dwrench; P.sdot = d_dsdot; P.f = d_df;
    V.H = kept_value(d_H); V.c = kept_value(d_c); V.f = kept_value(d_f); P.qdot = d_dqdot; P.H = d_dH; P.c = d_dc; P.vdot = d_dvdot;
    return state_derivative_dual(h, S, true);
}

int pfc_debug_stamps(pfc_handle h, long long *out16) {
    if (!h || !out16) return PFC_ERR_BAD_ARG;
    if (h->multi) return pfc_debug_stamps(h->multi->shard[0], out16);
    { int rc = drain(h); if (rc) return rc; }
    unsigned long long v[16] = {0};
    if (h->stamps.p) HIP_TRY(h, copy_sync(h, v, h->stamps.p, sizeof v, hipMemcpyDeviceToHost));
    for (int k = 0; k < 16; ++k) out16[k] = (long long)v[k];
    out16[7] = h->last_undecided;
#ifndef PFC_STAMPS
    out16[6] = h->twin_queue_fallback;      // make_twin's finding about the two streams (statistics view of the product build)
#endif
    return PFC_OK;
}

int pfc_selftest_math(pfc_handle h, int n, const double *x, const double *y, double *out3n) {
    if (!h || n <= 0 || !x || !y || !out3n) return PFC_ERR_BAD_ARG;
    if (h->multi) return pfc_selftest_math(h->multi->shard[0], n, x, y, out3n);
    HIP_TRY(h, hipSetDevice(h->device));
    DevBuf<double> dx, dy, dout;
    HIP_TRY(h, dx.ensure(n));
    HIP_TRY(h, dy.ensure(n));
    HIP_TRY(h, dout.ensure(3 * (size_t)n));
    HIP_TRY(h, copy_sync(h, dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_TRY(h, copy_sync(h, dy.p, y, sizeof(double) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_selftest, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, dx.p, dy.p, dout.p);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, copy_sync(h, out3n, dout.p, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost));
    return PFC_OK;
}

int pfc_selftest_kis(pfc_handle h, int n, const double *Kbar36, const double *dKbar36, const double *Vlam42, double *out72) {
    if (!h || n <= 0 || !Kbar36 || !dKbar36 || !out72) return PFC_ERR_BAD_ARG;
    if (h->multi) return pfc_selftest_kis(h->multi->shard[0], n, Kbar36, dKbar36, Vlam42, out72);
    HIP_TRY(h, hipSetDevice(h->device));
    DevBuf<double> dk, ddk, dvl, dout;
    HIP_TRY(h, dk.ensure(36 * (size_t)n));
    HIP_TRY(h, ddk.ensure(36 * (size_t)n));
    HIP_TRY(h, dout.ensure(72 * (size_t)n));
    if (Vlam42) HIP_TRY(h, dvl.ensure(42 * (size_t)n));
    HIP_TRY(h, copy_sync(h, dk.p, Kbar36, sizeof(double) * 36 * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(h, copy_sync(h, ddk.p, dKbar36, sizeof(double) * 36 * (size_t)n, hipMemcpyHostToDevice));
    if (Vlam42) HIP_TRY(h, copy_sync(h, dvl.p, Vlam42, sizeof(double) * 42 * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_selftest_kis, dim3(n), dim3(64), 0, h->stream, n, dk.p, ddk.p, dvl.p, dout.p);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, copy_sync(h, out72, dout.p, sizeof(double) * 72 * (size_t)n, hipMemcpyDeviceToHost));
    return PFC_OK;
}

// ---- the Radau IIA host driver: the parts, configuration and state, controller, gripper program, batch step, integration -------------
#include "pfc_radau_host.h"

}  // extern "C"
