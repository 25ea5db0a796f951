// pfc_surface.h -- the contact surface of an evaluation (pfc_contact_surface): per item the clipped polygons, the traction points
// (the reference's TractionCache: n̂, r_cart, dA, p; src/structs.jl) and normal_wrench / normal_wrench_cop
// (src/contact_algorithms_normal.jl:2-34), in one canonical order whatever the handle's options.  Included by pfc_hip.hip inside
// namespace pfc (device code only).
//
// The candidate list comes from the batched broadphase and is put in (item, element of mesh 1, element of mesh 2) order by
// pfc_canon_candidates / pfc_sort_candidates (pfc_sort.hip).  Then, one lane per candidate:
//   k_surf_count    gather + trivial reject (np_front), clip (pfc_clip.h), polygon set-up, fan quadrature (fan_triangle_points):
//                   {kept polygon 0 / 1, traction points} per list slot, and the candidate's partial sums in point order;
//   pfc_scan_pairs  exclusive scan of those pairs (rocPRIM, pfc_sort.hip): every candidate's polygon and point offset, the totals;
//   k_surf_seg      the item segments of the sorted list;
//   k_surf_summary  one wave per item: counters, polygon CSR, and the item's sums over its candidates' partials -- lane l adds the
//                   candidates l, l + 64, ... of the segment in order, then a fixed butterfly; the same bits in every run;
//   k_surf_emit     when both caller capacities suffice: the same clip again, vertices and traction points written at their offsets.
// The traction points are those of k_narrow bit for bit: the same front, clip, set-up and quadrature statements in the same
// order (the library is compiled with -ffp-contract=off).
#pragma once

constexpr int kSurfBlock = 64;     // one wave per workgroup: the polygon ring takes 16 KiB of LDS
constexpr int kSurfSums = 11;      // normal wrench [ang 3; lin 3], sum p dA r (3), sum p dA, sum dA

struct SurfArgs {
    const ItemRec *items;
    const WorkRec *cand;           // the candidate list, canonical order
    const int *ccount;
    int ccap, n_items;
    const int *icnt;               // per item: node tests, candidates (broadphase)
    unsigned *status;
    long long *cnt;                // 2 per list slot 0 .. ccap: {kept polygon 0 / 1, traction points}; zeros behind the list
    double *part;                  // kSurfSums per candidate with traction points
    const long long *off;          // exclusive scan of cnt: polygon and point offset per slot; slot ccap holds the totals
    int *seg;                      // n_items + 1: the candidates of item i are [seg[i], seg[i + 1])
    long long cap_poly, cap_trac;  // the caller's capacities (polygons, traction points)
    long long *poly_off;           // n_items + 1
    int *poly_idx;                 // 3 per polygon: element of mesh 1, element of mesh 2, vertex count
    double *poly_xyz;              // 24 per polygon: 8 vertices in frame r2, unused slots 0
    long long *poly_trac;          // polygons + 1: first traction point of every polygon
    double *trac;                  // 8 per point: n̂ 3, r 3, dA, p
    double *summary;               // kSurfSums per item (sum p dA r replaced by the cop)
    int *counts;                   // 4 per item, or null
    long long *totals;             // polygons, traction points
};

__device__ __forceinline__ int surf_n_c(const SurfArgs &g) {
    const int n = *g.ccount;
    return n < 0 ? 0 : (n > g.ccap ? g.ccap : n);
}

// The polygon of candidate cw in frame r2: np_front, the clip in the lane's ring column, then k_narrow's polygon set-up --
// poly_r2 = mul_then_un_pad(x_r2_ζ2, poly_ζ2) (poly_eight.jl:83-98) converted in place, centroid(poly_r2, n̂2)
// (poly_eight.jl:35-52).  Returns the vertex count, 0 if the clip left fewer than 3 vertices.
template <bool TT>
__device__ __forceinline__ int surf_polygon(const ItemRec *it, const WorkRec &cw, const GTetRec *tp, RingCol<kSurfBlock> &ring, V3 &nh,
                                            V3 &cen, unsigned *status, bool report) {
    double z[4][4];
    int n_in = 0;
    V3 nh_in = mk3(0.0, 0.0, 0.0);
    if (!np_front<TT>(it, cw, tp, z, n_in, nh_in, status, report)) return 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < n_in) {
#pragma unroll
            for (int i = 0; i < 4; ++i) ring.set(k, i, z[k][i]);
        }
    bool err = false;
    const int n = clip_ring_in_tet_coordinates(ring, n_in, err);     // pfc_clip.h
    if (err && report) atomicOr(status, kStNonFinite);
    if (n < 3) return 0;
    nh = nh_in;
    double V[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) V[k] = tp->xrz[k];
    auto conv = [&](int k) {
        const double z0 = ring.get(k, 0), z1 = ring.get(k, 1), z2 = ring.get(k, 2), z3 = ring.get(k, 3);
        const V3 x = mk3(((V[0] * z0 + V[3] * z1) + V[6] * z2) + V[9] * z3,
                         ((V[1] * z0 + V[4] * z1) + V[7] * z2) + V[10] * z3,
                         ((V[2] * z0 + V[5] * z1) + V[8] * z2) + V[11] * z3);
        ring.set(k, 0, x.x); ring.set(k, 1, x.y); ring.set(k, 2, x.z);
        return x;
    };
    const V3 a = conv(0);
    V3 cc = conv(1);
    double cum_sum = 0.0;
    V3 cum_prod = mk3(0.0, 0.0, 0.0);
    for (int k = 2; k < n; ++k) {
        const V3 b = cc;
        cc = conv(k);
        const double ar = triangle_area(a, b, cc, nh);
        cum_prod = cum_prod + ((a + b) + cc) * (1.0 / 3.0) * ar;
        cum_sum += ar;
    }
    cen = (cum_sum == 0.0) ? a : cum_prod / cum_sum;
    return n;
}

__device__ __forceinline__ PointParams surf_point_params(const ItemRec *it, const GTetRec *tp) {
    PointParams pp;
    pp.w = ld3(it->w); pp.vl = ld3(it->v); pp.chi = it->chi; pp.Ebar = it->Ebar;
    pp.er0 = tp->epsr[0]; pp.er1 = tp->epsr[1]; pp.er2 = tp->epsr[2]; pp.er3 = tp->epsr[3]; pp.nq = it->nq;
    return pp;
}

// The fan of the reference (integrate_patch: triangles (v_{n-1}, v_0, c), (v_0, v_1, c), ...) over the polygon in the ring.
template <class F>
__device__ __forceinline__ int surf_fan(const PointParams &pp, const RingCol<kSurfBlock> &ring, int n, const V3 &cen, const V3 &nh, F &&body) {
    int n_pt = 0;
    V3 v2 = mk3(ring.get(n - 1, 0), ring.get(n - 1, 1), ring.get(n - 1, 2));
    for (int k = 0; k < n; ++k) {
        const V3 v1 = v2;
        v2 = mk3(ring.get(k, 0), ring.get(k, 1), ring.get(k, 2));
        n_pt += fan_triangle_points(pp, v1, v2, cen, nh, body);
    }
    return n_pt;
}

template <bool TT>
__global__ void __launch_bounds__(kSurfBlock) k_surf_count(SurfArgs g) {
    __shared__ double ring_lds[8 * 4 * kSurfBlock];
    const int lane = threadIdx.x;
    const int n_c = surf_n_c(g);
    for (long long base = (long long)blockIdx.x * kSurfBlock; base <= g.ccap; base += (long long)gridDim.x * kSurfBlock) {
        const long long idx = base + lane;
        if (idx > g.ccap) continue;
        long long npoly = 0, npts = 0;
        if (idx < n_c) {
            const WorkRec cw = g.cand[idx];
            if ((unsigned)cw.item >= (unsigned)g.n_items) {      // an unwritten slot is reported, never followed
                atomicOr(g.status, kStHole);
            } else {
                const ItemRec *it = g.items + cw.item;
                const GTetRec *tp = (const GTetRec *)(it->tet + cw.b);
                RingCol<kSurfBlock> ring{ring_lds, lane, 0};
                V3 nh = mk3(0.0, 0.0, 0.0), cen = mk3(0.0, 0.0, 0.0);
                const int n = surf_polygon<TT>(it, cw, tp, ring, nh, cen, g.status, true);
                if (n >= 3) {
                    npoly = 1;
                    double s[kSurfSums];
#pragma unroll
                    for (int k = 0; k < kSurfSums; ++k) s[k] = 0.0;
                    // normal_wrench_cop (normal.jl:17-34): λ = p dA n̂, lin += λ, ang += r x λ, sum p dA r, sum p dA; and sum dA
                    npts = surf_fan(surf_point_params(it, tp), ring, n, cen, nh, [&](const V3 &r, const V3 &, double p, double dA) {
                        const double p_dA = p * dA;
                        const V3 lam = nh * p_dA;
                        const V3 ta = cross(r, lam);
                        s[0] += ta.x; s[1] += ta.y; s[2] += ta.z;
                        s[3] += lam.x; s[4] += lam.y; s[5] += lam.z;
                        s[6] += p_dA * r.x; s[7] += p_dA * r.y; s[8] += p_dA * r.z;
                        s[9] += p_dA; s[10] += dA;
                    });
                    if (npts > 0) {
                        double *o = g.part + (size_t)idx * kSurfSums;
#pragma unroll
                        for (int k = 0; k < kSurfSums; ++k) o[k] = s[k];
                    }
                }
            }
        }
        g.cnt[2 * idx] = npoly;
        g.cnt[2 * idx + 1] = npts;
    }
}

// seg[i] = first list slot of item i (the list is sorted by item): the slots where the item changes fill every index between.
__global__ void __launch_bounds__(256) k_surf_seg(SurfArgs g) {
    const int n_c = surf_n_c(g);
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j <= n_c; j += (long long)gridDim.x * blockDim.x) {
        int prev = j > 0 ? g.cand[j - 1].item : -1;
        int cur = j < n_c ? g.cand[j].item : g.n_items;
        prev = prev < -1 ? -1 : (prev > g.n_items ? g.n_items : prev);
        cur = cur < -1 ? -1 : (cur > g.n_items ? g.n_items : cur);
        for (int i = prev + 1; i <= cur; ++i) g.seg[i] = (int)j;
    }
}

__device__ __forceinline__ double surf_wave_sum(double v) {      // butterfly: every lane ends with the same bits
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ void __launch_bounds__(64) k_surf_summary(SurfArgs g) {
    const int lane = threadIdx.x;
    const int n_c = surf_n_c(g);
    for (int i = blockIdx.x; i < g.n_items; i += gridDim.x) {
        int c0 = g.seg[i], c1 = g.seg[i + 1];
        c0 = c0 < 0 ? 0 : (c0 > n_c ? n_c : c0);
        c1 = c1 < c0 ? c0 : (c1 > n_c ? n_c : c1);
        double s[kSurfSums];
#pragma unroll
        for (int k = 0; k < kSurfSums; ++k) s[k] = 0.0;
        for (int c = c0 + lane; c < c1; c += 64) {
            if (g.cnt[2 * (size_t)c + 1] <= 0) continue;
            const double *p = g.part + (size_t)c * kSurfSums;
#pragma unroll
            for (int k = 0; k < kSurfSums; ++k) s[k] += p[k];
        }
#pragma unroll
        for (int k = 0; k < kSurfSums; ++k) s[k] = surf_wave_sum(s[k]);
        const long long polys = g.off[2 * (size_t)c1] - g.off[2 * (size_t)c0];
        const long long pts = g.off[2 * (size_t)c1 + 1] - g.off[2 * (size_t)c0 + 1];
        if (lane < kSurfSums) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < kSurfSums; ++k) if (lane == k) v = s[k];
            if (lane >= 6 && lane < 9) {      // cop = sum p dA r / sum p dA (no point: 0, where the reference divides 0 by 0)
                v = pts > 0 ? v / s[9] : 0.0;
            }
            if (pts == 0) v = 0.0;
            g.summary[(size_t)i * kSurfSums + lane] = v;
        }
        if (lane == 0) {
            g.poly_off[i] = g.off[2 * (size_t)c0];
            if (g.counts) {
                int *co = g.counts + 4 * (size_t)i;
                co[0] = g.icnt[4 * (size_t)i]; co[1] = g.icnt[4 * (size_t)i + 1]; co[2] = (int)polys; co[3] = (int)pts;
            }
        }
    }
    if (blockIdx.x == 0 && lane == 0) {
        g.poly_off[g.n_items] = g.off[2 * (size_t)g.ccap];
        g.totals[0] = g.off[2 * (size_t)g.ccap];
        g.totals[1] = g.off[2 * (size_t)g.ccap + 1];
    }
}

template <bool TT>
__global__ void __launch_bounds__(kSurfBlock) k_surf_emit(SurfArgs g) {
    __shared__ double ring_lds[8 * 4 * kSurfBlock];
    const long long tot_p = g.off[2 * (size_t)g.ccap], tot_t = g.off[2 * (size_t)g.ccap + 1];
    if (tot_p > g.cap_poly || tot_t > g.cap_trac) return;      // the caller grows its buffers: none of them is touched
    const int lane = threadIdx.x;
    if (blockIdx.x == 0 && lane == 0) g.poly_trac[tot_p] = tot_t;
    const int n_c = surf_n_c(g);
    for (long long base = (long long)blockIdx.x * kSurfBlock; base < n_c; base += (long long)gridDim.x * kSurfBlock) {
        const long long idx = base + lane;
        if (idx >= n_c || g.cnt[2 * idx] == 0) continue;
        const long long kp = g.off[2 * idx], t0 = g.off[2 * idx + 1], npts = g.cnt[2 * idx + 1];
        if (kp >= g.cap_poly || t0 + npts > g.cap_trac) continue;      // (cannot happen: offsets + counts <= totals <= capacities)
        const WorkRec cw = g.cand[idx];
        const ItemRec *it = g.items + cw.item;
        const GTetRec *tp = (const GTetRec *)(it->tet + cw.b);
        RingCol<kSurfBlock> ring{ring_lds, lane, 0};
        V3 nh = mk3(0.0, 0.0, 0.0), cen = mk3(0.0, 0.0, 0.0);
        const int n = surf_polygon<TT>(it, cw, tp, ring, nh, cen, g.status, false);
        int *pi = g.poly_idx + 3 * (size_t)kp;
        pi[0] = cw.a; pi[1] = cw.b; pi[2] = n;
        double *px = g.poly_xyz + 24 * (size_t)kp;
        for (int k = 0; k < 8; ++k) {
            const bool v = k < n;
            px[3 * k] = v ? ring.get(k, 0) : 0.0;
            px[3 * k + 1] = v ? ring.get(k, 1) : 0.0;
            px[3 * k + 2] = v ? ring.get(k, 2) : 0.0;
        }
        g.poly_trac[kp] = t0;
        if (n < 3) continue;
        long long tpos = t0;
        const long long tend = t0 + npts;
        surf_fan(surf_point_params(it, tp), ring, n, cen, nh, [&](const V3 &r, const V3 &, double p, double dA) {
            if (tpos < tend) {
                double *o = g.trac + 8 * (size_t)tpos;
                o[0] = nh.x; o[1] = nh.y; o[2] = nh.z; o[3] = r.x; o[4] = r.y; o[5] = r.z; o[6] = dA; o[7] = p;
            }
            ++tpos;
        });
    }
}

// The counters and the status word of the evaluation go to out (status, polygons, points, counters[0 .. n_ctr)) and are left zeroed
// for the next evaluation, as k_final leaves them.
__global__ void __launch_bounds__(64) k_surf_final(int *ctr, int n_ctr, unsigned *status, const long long *off, int ccap, long long *out) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        out[0] = (long long)status[0];
        out[1] = off[2 * (size_t)ccap];
        out[2] = off[2 * (size_t)ccap + 1];
    }
    __syncthreads();
    if (tid < 4) status[tid] = 0u;
    for (int k = tid; k < n_ctr; k += blockDim.x) { out[3 + k] = ctr[k]; ctr[k] = 0; }
}
