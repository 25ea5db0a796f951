// pfc_scatter.h -- the third-law scatter on Dual numbers (pfc_scatter_generalized_dual[_device]): addGeneralizedForcesThirdLaw!
// (src/contact_algorithms_non_friction.jl:267-286) as the reference runs it on the Dual state of a Jacobian chunk, where the
// wrench, x_rw_r2 and the geometric Jacobians (refreshJacobians!, :86-92) all carry partials.  Included by pfc_hip.hip inside
// namespace pfc (device code only).
//
// Order: every output entry (scene s, value or direction k, coordinate j) is one sum over the items of s in ascending item order,
// +tau(body_2) then -tau(body_1), as the reference loops over its instructions -- so f is the C oracle's value scatter to the bit and
// the partials are a fixed function of the inputs.  No atomics.  The kernels:
//   k_scat_keys / k_scat_off  a CSR of the items by scene: key scene * n_items + item (sorted by pfc_sort_indices), offsets by a
//                             binary search per scene; not run without scene ids (one segment) or by the host form (host CSR);
//   k_scat_world              one lane per (item, value-or-direction): transform(wrench, x_rw_r2) on the Dual numbers;
//   k_scat_proj               one workgroup per (scene, value-or-direction, kScatJB coordinates): the 256 lanes evaluate
//                             torque!'s J' w terms of kScatTile items at once into LDS, then kScatJB lanes add them in item order.
// scat_world and scat_tau are templates: the value (double) and the Dual (ScatDual) instantiations are the same statements.
#pragma once

constexpr int kScatJB = 16;        // velocity coordinates per projection workgroup (consecutive: the Jacobian reads are contiguous)
constexpr int kScatTile = 64;      // items per LDS tile of k_scat_proj
constexpr int kScatMaxDir = 16;

// One partial of a ForwardDiff.Dual: value and the partial of one seed direction, with ForwardDiff's rules (the product in the
// order of _mul_partials: d(a b) = da b + a db).  pfc_bodies.h evaluates the item expressions on the same type.
struct ScatDual { double v, d; };
__device__ inline ScatDual operator+(ScatDual a, ScatDual b) { return {a.v + b.v, a.d + b.d}; }
__device__ inline ScatDual operator-(ScatDual a, ScatDual b) { return {a.v - b.v, a.d - b.d}; }
__device__ inline ScatDual operator-(ScatDual a) { return {-a.v, -a.d}; }
__device__ inline ScatDual operator*(ScatDual a, ScatDual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
// The quotient in the order of _div_partials through _mul_partials: d(a / b) = da (1 / b) + db (-(a / b^2)).  (Written as recalled:
// bit parity with ForwardDiff for this rule is unpinned)  Used by the Dual kinematics (pfc_kin.h).
__device__ inline ScatDual operator/(ScatDual a, ScatDual b) {
    return {a.v / b.v, a.d * (1.0 / b.v) + b.d * (-(a.v / (b.v * b.v)))};
}

// RigidBodyDynamics transform(wrench, x_rw_r2) (the C oracle's statements): w [ang; lin], x = R (9, column-major), t (3);
// o = [R ang + t x lin; R lin].
template <class T> __device__ inline void scat_world(const T *w, const T *x, T *o) {
    const T lx = (x[0] * w[3] + x[3] * w[4]) + x[6] * w[5];
    const T ly = (x[1] * w[3] + x[4] * w[4]) + x[7] * w[5];
    const T lz = (x[2] * w[3] + x[5] * w[4]) + x[8] * w[5];
    o[0] = ((x[0] * w[0] + x[3] * w[1]) + x[6] * w[2]) + (x[10] * lz - x[11] * ly);
    o[1] = ((x[1] * w[0] + x[4] * w[1]) + x[7] * w[2]) + (x[11] * lx - x[9] * lz);
    o[2] = ((x[2] * w[0] + x[5] * w[1]) + x[8] * w[2]) + (x[9] * ly - x[10] * lx);
    o[3] = lx; o[4] = ly; o[5] = lz;
}

// torque!(tau, jac, wrench) for one coordinate: J_ang[:, j] . ang + J_lin[:, j] . lin.
template <class T> __device__ inline T scat_tau(const T *J, const T *o) {
    return ((J[0] * o[0] + J[1] * o[1]) + J[2] * o[2]) + ((J[3] * o[3] + J[4] * o[4]) + J[5] * o[5]);
}

// keys[i] = scene[i] * n_items + i (an id outside [0, n_scene) gets -1: sorted last, in no segment); *count = n_items.
__global__ void __launch_bounds__(256) k_scat_keys(int n_items, int n_scene, const int *scene, int *keys, int *count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *count = n_items;
    if (i >= n_items) return;
    const int s = scene[i];
    keys[i] = (s >= 0 && s < n_scene) ? s * n_items + i : -1;
}

// off[s] = first position of the sorted keys at or above s * n_items (s = 0 .. n_scene), unsigned (the -1 keys lie above all).
__global__ void __launch_bounds__(256) k_scat_off(int n_items, int n_scene, const int *keys, int *off) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > n_scene) return;
    const unsigned target = (unsigned)s * (unsigned)n_items;
    int lo = 0, hi = n_items;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((unsigned)keys[mid] < target) lo = mid + 1; else hi = mid;
    }
    off[s] = lo;
}

// W[i][c] (c = 0: value, c = 1 + k: partial of direction k) = transform(wrench, x_rw_r2) of item i.  dwrench n_items x n_dir x 6,
// dx n_items x n_dir x 12 (NULL: zero partials, read as zeros so that the bytes are those of a zero array).
__device__ inline void scat_world_lane(long long t, int n_dir, const double *wrench, const double *dwrench, const double *x_w_r2,
                                       const double *dx_w_r2, double *W) {
    const int i = (int)(t / (1 + n_dir)), c = (int)(t % (1 + n_dir));
    const double *w = wrench + 6 * (size_t)i, *x = x_w_r2 + 12 * (size_t)i;
    double *o = W + 6 * (size_t)t;
    if (c == 0) {
        double wv[6], xv[12], ov[6];
        for (int e = 0; e < 6; ++e) wv[e] = w[e];
        for (int e = 0; e < 12; ++e) xv[e] = x[e];
        scat_world<double>(wv, xv, ov);
        for (int e = 0; e < 6; ++e) o[e] = ov[e];
        return;
    }
    const size_t ik = (size_t)i * n_dir + (c - 1);
    ScatDual wd[6], xd[12], od[6];
    for (int e = 0; e < 6; ++e) wd[e] = ScatDual{w[e], dwrench[6 * ik + e]};
    for (int e = 0; e < 12; ++e) xd[e] = ScatDual{x[e], dx_w_r2 ? dx_w_r2[12 * ik + e] : 0.0};
    scat_world<ScatDual>(wd, xd, od);
    for (int e = 0; e < 6; ++e) o[e] = od[e].d;
}

__global__ void __launch_bounds__(256) k_scat_world(int n_items, int n_dir, const double *wrench, const double *dwrench,
                                                    const double *x_w_r2, const double *dx_w_r2, double *W) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < (long long)n_items * (1 + n_dir);
         t += (long long)gridDim.x * blockDim.x)
        scat_world_lane(t, n_dir, wrench, dwrench, x_w_r2, dx_w_r2, W);
}

struct ScatDualArgs {
    int n_items, n_dir, nv, n_scene, n_jb, accumulate;
    const double *W;               // n_items x (1 + n_dir) x 6 (k_scat_world)
    const double *jac;             // n_body x nv x 6
    const double *djac;            // n_body x n_dir x nv x 6, or NULL (zero partials)
    const int *body_1, *body_2;
    const int *keys, *off;         // CSR by scene (keys: scene * n_items + item); keys NULL: every item in scene 0, in order
    double *f;                     // n_scene x nv, or NULL (the value workgroups return)
    double *df;                    // n_scene x n_dir x nv
};

// One block of k_scat_proj: scene sc, c (0: value, 1 + k: direction k), coordinates j0 = kScatJB jb .. j0 + kScatJB.  Lane (r, jl)
// evaluates the terms of the tile's items r, r + 16, ... at coordinate j0 + jl; lanes 0 .. kScatJB - 1 then add them in item order.
// (The workgroups of k_scat_proj stride over the blocks, so the grid does not bound n_scene.)
__device__ inline void scat_proj_block(const ScatDualArgs &g, int jb, int sc, int c, double (*s_t)[kScatTile][kScatJB],
                                       int (*s_on)[kScatTile]) {
    if (c == 0 && !g.f) return;
    const int nc = 1 + g.n_dir;
    const int tid = threadIdx.x, jl = tid % kScatJB, r0 = tid / kScatJB;
    const int j = jb * kScatJB + jl;
    const bool jok = j < g.nv;
    int p0 = 0, p1 = 0;
    if (g.keys) { p0 = g.off[sc]; p1 = g.off[sc + 1]; }
    else if (sc == 0) p1 = g.n_items;
    const int kbase = sc * g.n_items;
    double *out = c == 0 ? g.f + (size_t)sc * g.nv + j : g.df + ((size_t)sc * g.n_dir + (c - 1)) * g.nv + j;
    const bool summer = tid < kScatJB && jok;
    double acc = 0.0;
    if (summer && g.accumulate) acc = *out;
    for (int t0 = p0; t0 < p1; t0 += kScatTile) {
        const int nt = min(kScatTile, p1 - t0);
        for (int r = r0; r < nt; r += 256 / kScatJB) {
            const int i = g.keys ? g.keys[t0 + r] - kbase : t0 + r;
            const int bb[2] = {g.body_2[i], g.body_1[i]};
            if (jl == 0) { s_on[0][r] = bb[0] >= 0; s_on[1][r] = bb[1] >= 0; }
            if (!jok) continue;
            const double *W0 = g.W + (size_t)i * nc * 6;
            for (int q = 0; q < 2; ++q) {
                const int b = bb[q];
                double t = 0.0;
                if (b >= 0) {
                    const double *J = g.jac + ((size_t)b * g.nv + j) * 6;
                    if (c == 0) {
                        double Jv[6], ov[6];
                        for (int e = 0; e < 6; ++e) { Jv[e] = J[e]; ov[e] = W0[e]; }
                        t = scat_tau<double>(Jv, ov);
                    } else {
                        const double *Wc = W0 + 6 * c;
                        const double *dJ = g.djac ? g.djac + (((size_t)b * g.n_dir + (c - 1)) * g.nv + j) * 6 : nullptr;
                        ScatDual Jd[6], od[6];
                        for (int e = 0; e < 6; ++e) { Jd[e] = ScatDual{J[e], dJ ? dJ[e] : 0.0}; od[e] = ScatDual{W0[e], Wc[e]}; }
                        t = scat_tau<ScatDual>(Jd, od).d;
                    }
                }
                s_t[q][r][jl] = t;
            }
        }
        __syncthreads();
        if (summer) {
            for (int r = 0; r < nt; ++r) {      // f += 1.0 * tau_2, then f += -1.0 * tau_1 (:271-272)
                if (s_on[0][r]) acc = acc + s_t[0][r][jl];
                if (s_on[1][r]) acc = acc - s_t[1][r][jl];
            }
        }
        __syncthreads();
    }
    if (summer) *out = acc;
}

__global__ void __launch_bounds__(256) k_scat_proj(ScatDualArgs g) {
    __shared__ double s_t[2][kScatTile][kScatJB];
    __shared__ int s_on[2][kScatTile];
    const int nc = 1 + g.n_dir;
    for (long long blk = blockIdx.x; blk < (long long)g.n_scene * nc * g.n_jb; blk += gridDim.x)      // (uniform over the workgroup)
        scat_proj_block(g, (int)(blk % g.n_jb), (int)(blk / g.n_jb / nc), (int)(blk / g.n_jb % nc), s_t, s_on);
}
