// pfc_surface_fric.h -- the friction half of the contact surface (pfc_contact_surface_fric): per traction point the friction force
// T_c that traction() returns (src/contact_algorithms_friction.jl:12-48) and its branch, per item the friction wrench, ṡ and the
// bristle patch state (K, K̄^{-1/2}, S⁻¹, Δ²; :85-201).  Included by pfc_hip.hip inside namespace pfc after pfc_surface.h (device
// code only).
//
// The kernels run behind k_surf_summary, on the same canonical candidate list, offsets and segments (pfc_surface.h):
//   k_sfric_mom    bristle items with points: calc_patch_spatial_stiffness!'s moments about the cop of the summary (:147-169);
//   k_sfric_eig    one wave per item: kAccIp / kAccIpc summed as k_surf_summary sums them (the same statements, so the cop that
//                  eig_item forms is the summary's, bit for bit), the moments of k_sfric_mom, then eig_item (pfc_br.h) unchanged;
//   k_sfric_pass   every item with points: T̄s or vel_t, traction(), the friction sums about the cop and the first-branch sums;
//                  the rows of fric at the points' offsets when both caller capacities suffice;
//   k_sfric_final  per item: the friction wrench about the r2 origin, the total wrench, ṡ.
// k_sfric_mom and k_sfric_pass give each item kFricSplit waves: lane l of wave b takes the candidates c0 + 64 b + l,
// c0 + 64 (b + kFricSplit) + l, ... of the item's segment in order, a fixed butterfly sums the wave, and the kFricSplit records
// are added in order.  Every sum is a function of the candidate list alone: no grid, timing or option enters, and no atomics.
// The points are re-derived with surf_polygon / surf_fan, the statements k_surf_emit writes trac with.
#pragma once

constexpr int kFricSplit = 8;      // waves per item in k_sfric_mom and k_sfric_pass (part of the summation order: fixed)
constexpr int kFricMom = 27;       // Snn 6, San 9, Saa 6, Srr 6 about the cop: the kAccSnn .. kAccSrr slots of eig_item's block
constexpr int kFricSums = 8;       // friction wrench about the cop [ang 3; lin 3], first-branch sum p dA, first-branch count
constexpr int kFricOut = 20;       // fric_summary row
constexpr int kStiffOut = 84;      // stiff row: K 36, K̄^{-1/2} 36, diag S⁻¹ 6, Δ² 6

struct SurfFricArgs {
    double *mom;                   // n_items x kFricSplit x kFricMom (bristle items with points)
    double *fsum;                  // n_items x kFricSplit x kFricSums (items with points)
    double *res;                   // n_items x kResStride: eig_item's result block (bristle items with points)
    double *fric;                  // 4 per traction point: T_c (3), branch
    double *fric_summary;          // kFricOut per item
    double *stiff;                 // kStiffOut per item, or null
};

// The candidates [c0, c1) of item i and its number of traction points (k_surf_summary's clamps).
__device__ __forceinline__ long long sfric_range(const SurfArgs &g, int i, int n_c, int &c0, int &c1) {
    c0 = g.seg[i]; c1 = g.seg[i + 1];
    c0 = c0 < 0 ? 0 : (c0 > n_c ? n_c : c0);
    c1 = c1 < c0 ? c0 : (c1 > n_c ? n_c : c1);
    return g.off[2 * (size_t)c1 + 1] - g.off[2 * (size_t)c0 + 1];
}

template <bool TT>
__global__ void __launch_bounds__(kSurfBlock) k_sfric_mom(SurfArgs g, SurfFricArgs f) {
    __shared__ double ring_lds[8 * 4 * kSurfBlock];
    const int lane = threadIdx.x;
    const int n_c = surf_n_c(g);
    const long long b = blockIdx.x;      // one workgroup per (item, wave of the item): a grid-stride loop here spilled SGPRs
    if (b >= (long long)g.n_items * kFricSplit) return;
    const int i = (int)(b / kFricSplit), sp = (int)(b % kFricSplit);
    const ItemRec *it = g.items + i;
    int c0, c1;
    if (it->model != PFC_BRISTLE || sfric_range(g, i, n_c, c0, c1) <= 0) return;
    double m[kFricMom];
#pragma unroll
    for (int k = 0; k < kFricMom; ++k) m[k] = 0.0;
    for (int c = c0 + sp * 64 + lane; c < c1; c += 64 * kFricSplit) {
        if (g.cnt[2 * (size_t)c + 1] <= 0) continue;
        const WorkRec cw = g.cand[c];
        // the item's record through the candidate (cw.item == i): per-lane loads, as in k_surf_emit -- the same values held
        // in scalar registers ran the kernel out of them
        const ItemRec *ic = g.items + cw.item;
        const GTetRec *tp = (const GTetRec *)(ic->tet + cw.b);
        RingCol<kSurfBlock> ring{ring_lds, lane, 0};
        V3 nh = mk3(0.0, 0.0, 0.0), cen = mk3(0.0, 0.0, 0.0);
        const int n = surf_polygon<TT>(ic, cw, tp, ring, nh, cen, g.status, false);
        if (n < 3) continue;
        const V3 cop = ld3(g.summary + (size_t)cw.item * kSurfSums + 6);
        // calc_patch_spatial_stiffness! (friction.jl:147-169), x = r - cop, a = x x n̂: sum w n̂ n̂', sum w a n̂' (column-major),
        // sum w a a', sum w x x'
        surf_fan(surf_point_params(ic, tp), ring, n, cen, nh, [&](const V3 &r, const V3 &, double p, double dA) {
            const double w = p * dA;
            const V3 x = r - cop;
            const V3 a = cross(x, nh);
            m[0] += w * (nh.x * nh.x); m[1] += w * (nh.x * nh.y); m[2] += w * (nh.x * nh.z);
            m[3] += w * (nh.y * nh.y); m[4] += w * (nh.y * nh.z); m[5] += w * (nh.z * nh.z);
            m[6] += w * (a.x * nh.x); m[7] += w * (a.y * nh.x); m[8] += w * (a.z * nh.x);
            m[9] += w * (a.x * nh.y); m[10] += w * (a.y * nh.y); m[11] += w * (a.z * nh.y);
            m[12] += w * (a.x * nh.z); m[13] += w * (a.y * nh.z); m[14] += w * (a.z * nh.z);
            m[15] += w * (a.x * a.x); m[16] += w * (a.x * a.y); m[17] += w * (a.x * a.z);
            m[18] += w * (a.y * a.y); m[19] += w * (a.y * a.z); m[20] += w * (a.z * a.z);
            m[21] += w * (x.x * x.x); m[22] += w * (x.x * x.y); m[23] += w * (x.x * x.z);
            m[24] += w * (x.y * x.y); m[25] += w * (x.y * x.z); m[26] += w * (x.z * x.z);
        });
    }
#pragma unroll
    for (int k = 0; k < kFricMom; ++k) m[k] = surf_wave_sum(m[k]);
    if (lane < kFricMom) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < kFricMom; ++k) if (lane == k) v = m[k];
        f.mom[(size_t)b * kFricMom + lane] = v;
    }
}

// decompose_K! / calc_K̄_sqrt_inv / Δ² (friction.jl:85-132) per bristle item with points; the stiff row of every item.
__global__ void __launch_bounds__(64) k_sfric_eig(SurfArgs g, SurfFricArgs f) {
    __shared__ EigScratch E;
    __shared__ double acc[kAccStride];
    __shared__ double res[kResStride];
    const int lane = threadIdx.x;
    const int n_c = surf_n_c(g);
    for (int i = blockIdx.x; i < g.n_items; i += gridDim.x) {
        const ItemRec *it = g.items + i;
        int c0, c1;
        const long long pts = sfric_range(g, i, n_c, c0, c1);
        double *so = f.stiff ? f.stiff + (size_t)i * kStiffOut : nullptr;
        if (it->model != PFC_BRISTLE || pts <= 0) {
            if (so)
                for (int k = lane; k < kStiffOut; k += 64) so[k] = 0.0;
            continue;
        }
        // sum w and sum w r: k_surf_summary's statements over the same partials (its s[9] and s[6..8])
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int c = c0 + lane; c < c1; c += 64) {
            if (g.cnt[2 * (size_t)c + 1] <= 0) continue;
            const double *p = g.part + (size_t)c * kSurfSums;
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] += p[6 + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = surf_wave_sum(s[k]);
        double mv = 0.0;
        if (lane < kFricMom)
            for (int sp = 0; sp < kFricSplit; ++sp) mv += f.mom[((size_t)i * kFricSplit + sp) * kFricMom + lane];
        wave_lds_sync();      // (the previous item's readers of acc / res are through)
        if (lane == 0) {
            acc[kAccIp] = s[3];
            acc[kAccIpc] = s[0]; acc[kAccIpc + 1] = s[1]; acc[kAccIpc + 2] = s[2];
        }
        if (lane < kFricMom) acc[kAccSnn + lane] = mv;
        wave_lds_sync();
        eig_item(acc, it->k_bar, it->magic, it->s, res, E, lane);
        wave_lds_sync();
        double *ro = f.res + (size_t)i * kResStride;
        for (int k = lane; k < kResStride; k += 64) ro[k] = res[k];
        if (so) {
            if (lane < 36) { so[lane] = res[kResK + lane]; so[36 + lane] = res[kResKis + lane]; }
            if (lane < 6) { so[72 + lane] = res[kResSinv + lane]; so[78 + lane] = res[kResDelta + lane]; }
        }
    }
}

template <bool TT>
__global__ void __launch_bounds__(kSurfBlock) k_sfric_pass(SurfArgs g, SurfFricArgs f) {
    __shared__ double ring_lds[8 * 4 * kSurfBlock];
    const int lane = threadIdx.x;
    const int n_c = surf_n_c(g);
    const long long tot_p = g.off[2 * (size_t)g.ccap], tot_t = g.off[2 * (size_t)g.ccap + 1];
    const bool emit = tot_p <= g.cap_poly && tot_t <= g.cap_trac;      // else no byte of fric is written (as k_surf_emit)
    const long long b = blockIdx.x;      // one workgroup per (item, wave of the item): a grid-stride loop here spilled SGPRs
    if (b >= (long long)g.n_items * kFricSplit) return;
    const int i = (int)(b / kFricSplit), sp = (int)(b % kFricSplit);
    const ItemRec *it = g.items + i;
    int c0, c1;
    if (sfric_range(g, i, n_c, c0, c1) <= 0) return;
    const bool br = it->model == PFC_BRISTLE;
    double s[kFricSums];
#pragma unroll
    for (int k = 0; k < kFricSums; ++k) s[k] = 0.0;
    for (int c = c0 + sp * 64 + lane; c < c1; c += 64 * kFricSplit) {
        const long long npts = g.cnt[2 * (size_t)c + 1];
        if (npts <= 0) continue;
        const long long t0 = g.off[2 * (size_t)c + 1], tend = t0 + npts;
        const bool store = emit && tend <= g.cap_trac;
        const WorkRec cw = g.cand[c];
        const ItemRec *ic = g.items + cw.item;      // (per-lane loads: see k_sfric_mom)
        const GTetRec *tp = (const GTetRec *)(ic->tet + cw.b);
        RingCol<kSurfBlock> ring{ring_lds, lane, 0};
        V3 nh = mk3(0.0, 0.0, 0.0), cen = mk3(0.0, 0.0, 0.0);
        const int n = surf_polygon<TT>(ic, cw, tp, ring, nh, cen, g.status, false);
        if (n < 3) continue;
        const V3 cop = ld3(g.summary + (size_t)cw.item * kSurfSums + 6);
        const double mu_s = ic->mu_s, mu_d = ic->mu_d, v_c = ic->v_c, tau = ic->tau, k_bar = ic->k_bar;
        V3 Da = mk3(0.0, 0.0, 0.0), Dl = mk3(0.0, 0.0, 0.0);
        if (br) {
            const double *r = f.res + (size_t)cw.item * kResStride;
            Da = ld3(r + kResDelta); Dl = ld3(r + kResDelta + 3);
        }
        long long tpos = t0;
        surf_fan(surf_point_params(ic, tp), ring, n, cen, nh, [&](const V3 &r, const V3 &rdot, double p, double dA) {
            const double p_dA = p * dA;
            const V3 x = r - cop;
            V3 T;
            bool first;
            if (br) {
                // calc_spatial_bristle_force (friction.jl:182-193): T̄s = -k̄ (δ² + τ ṙ), δ² = Δ²_lin + Δ²_ang x (r - cop)
                V3 Ts = ((Dl + cross(Da, x)) + rdot * tau) * (-k_bar);
                Ts = vec_sub_vec_proj(Ts, nh);
                // traction(::Bristle) (:32-48)
                const double m2 = dot(Ts, Ts);
                first = m2 < mu_s * mu_s;
                if (first) {
                    T = Ts;
                } else {
                    const double mg = __builtin_sqrt(m2);
                    const double mu = clamped_piecewise(mg, 2 * mu_s, 3 * mu_s, mu_s, mu_d);
                    T = (Ts * mu) / mg;
                }
            } else {
                // yes_contact!(::Regularized) (:57-63) and traction(::Regularized) (:12-29)
                const V3 vt = vec_sub_vec_proj(rdot, nh);
                const double m2 = dot(vt, vt);
                first = m2 < v_c * v_c;
                if (first) {
                    T = (vt * (-mu_s)) / v_c;
                } else {
                    const double mg = __builtin_sqrt(m2);
                    const double mu = clamped_piecewise(mg, 2 * v_c, 3 * v_c, mu_s, mu_d);
                    T = (vt * (-mu)) / mg;
                }
            }
            const V3 Tc = T * p_dA;
            const V3 ta = cross(x, Tc);
            s[0] += ta.x; s[1] += ta.y; s[2] += ta.z;
            s[3] += Tc.x; s[4] += Tc.y; s[5] += Tc.z;
            if (first) { s[6] += p_dA; s[7] += 1.0; }
            if (store && tpos < tend) {
                double *o = f.fric + 4 * (size_t)tpos;
                o[0] = Tc.x; o[1] = Tc.y; o[2] = Tc.z; o[3] = first ? 0.0 : 1.0;
            }
            ++tpos;
        });
    }
#pragma unroll
    for (int k = 0; k < kFricSums; ++k) s[k] = surf_wave_sum(s[k]);
    if (lane < kFricSums) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < kFricSums; ++k) if (lane == k) v = s[k];
        f.fsum[(size_t)b * kFricSums + lane] = v;
    }
}

// bristle_wrench_in_world / no_contact! epilogue (friction.jl:76-81, 119-143), one lane per item: the records of k_sfric_pass
// in order, the friction wrench moved from the cop to the r2 origin, total = normal (summary) + friction, ṡ as final_item forms it.
__global__ void __launch_bounds__(64) k_sfric_final(SurfArgs g, SurfFricArgs f) {
    const int n_c = surf_n_c(g);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < g.n_items; i += gridDim.x * blockDim.x) {
        const ItemRec *it = g.items + i;
        int c0, c1;
        const long long pts = sfric_range(g, i, n_c, c0, c1);
        double fs[kFricSums];
#pragma unroll
        for (int k = 0; k < kFricSums; ++k) fs[k] = 0.0;
        if (pts > 0)
            for (int sp = 0; sp < kFricSplit; ++sp) {
                const double *q = f.fsum + ((size_t)i * kFricSplit + sp) * kFricSums;
#pragma unroll
                for (int k = 0; k < kFricSums; ++k) fs[k] += q[k];
            }
        const double *sm = g.summary + (size_t)i * kSurfSums;
        const V3 cop = ld3(sm + 6);
        const V3 fang = mk3(fs[0], fs[1], fs[2]), flin = mk3(fs[3], fs[4], fs[5]);
        const V3 fang2 = fang + cross(cop, flin);
        const double wf[6] = {fang2.x, fang2.y, fang2.z, flin.x, flin.y, flin.z};
        double *o = f.fric_summary + (size_t)i * kFricOut;
#pragma unroll
        for (int k = 0; k < 6; ++k) { o[k] = sm[k] + wf[k]; o[6 + k] = wf[k]; }
        double sd[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (it->model == PFC_BRISTLE) {
            const double tau_inv = 1.0 / it->tau;
            double s0[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) s0[k] = it->s[k];
            if (pts <= 0) {
#pragma unroll
                for (int k = 0; k < 6; ++k) sd[k] = -tau_inv * s0[k];
            } else {
                const double *r = f.res + (size_t)i * kResStride;
                double sw[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) sw[k] = r[kResSinv + k] * fs[k];
#pragma unroll
                for (int ii = 0; ii < 6; ++ii) {
                    double acc = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; ++k) acc += r[kResKis + ii + 6 * k] * sw[k];
                    sd[ii] = -tau_inv * (acc + s0[ii]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) o[12 + k] = sd[k];
        o[18] = fs[6];
        o[19] = fs[7];
    }
}
