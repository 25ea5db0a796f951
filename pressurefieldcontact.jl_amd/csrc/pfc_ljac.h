// pfc_ljac.h -- per-item contact Jacobians (pfc_local_jacobian[_device], pfc_apply_local_jacobian[_device]).  Included by pfc_hip.hip
// inside namespace pfc (device code only).
//
// Every branch of a Dual pass compares values only, so at one value point the partials of an item are linear in its seeds:
//   [d_wrench; d_sdot] (12 x n_dir) = L (12 x 36) . [d_pose 24; d_twist 6; d_s 6] (36 x n_dir).
// L is built by three Dual passes on the kept value pass with unit seeds (columns 0..15, 16..31, 32..35) and applied to further
// seed chunks as a batched product.  Layout of L: n_items x 12 x 36 doubles, row-major per item; row r = output r (wrench [ang; lin],
// then ṡ), column k = input k (the 24 pose numbers, twist 6, s 6).  The kernels:
//   k_ljac_seeds  the unit seeds of the three passes, written once per capacity (the blocks are laid out by capacity, not by item
//                 count, so the content does not depend on the evaluation);
//   k_ljac_pack   the passes' (item, direction, 6) partials into L's columns;
//   k_ljac_apply  one wave per item: seeds into LDS, zero keys skipped before any read of L, L into LDS, one lane per output.
#pragma once

constexpr int kLjacRows = 12, kLjacCols = 36, kLjacSize = kLjacRows * kLjacCols;
constexpr int kLjacPasses = 3;
constexpr int kLjacSeedDoubles = kLjacCols * kLjacCols;     // unit-seed doubles per item over the three passes
__host__ __device__ constexpr int ljac_pass_dirs(int p) { return p < 2 ? 16 : kLjacCols - 32; }
constexpr int kLjacSeedStride = kLjacCols + 1;      // LDS row of one direction's seeds (odd in doubles: rows start on different banks)

// Unit seeds for `cap` items.  Pass p (nd directions, column 16 p + d for direction d) starts at cap * 576 p: d_pose cap x nd x 24,
// then d_twist cap x nd x 6, then d_s cap x nd x 6 (1 296 cap doubles in all).  One lane per (item, column).
__global__ void __launch_bounds__(256) k_ljac_seeds(int cap, double *seed) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)cap * kLjacCols) return;
    const int i = (int)(t / kLjacCols), col = (int)(t % kLjacCols);
    const int p = col / 16, d = col % 16, nd = ljac_pass_dirs(p);
    const size_t c = (size_t)cap, key = (size_t)i * nd + d;
    double *pose = seed + c * 576 * p, *tw = pose + c * nd * 24, *s = tw + c * nd * 6;
    for (int k = 0; k < 24; ++k) pose[key * 24 + k] = k == col ? 1.0 : 0.0;
    for (int k = 0; k < 6; ++k) tw[key * 6 + k] = 24 + k == col ? 1.0 : 0.0;
    for (int k = 0; k < 6; ++k) s[key * 6 + k] = 30 + k == col ? 1.0 : 0.0;
}

// L[i][r][k] from the partials of pass p = k / 16, which wrote d_wrench n x nd x 6 then d_sdot n x nd x 6 from out + n 192 p.
// One lane per entry of L (coalesced stores).
__global__ void __launch_bounds__(256) k_ljac_pack(int n_items, const double *out, double *L) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n_items * kLjacSize) return;
    const int i = (int)(t / kLjacSize), e = (int)(t % kLjacSize), r = e / kLjacCols, k = e % kLjacCols;
    const int p = k / 16, d = k % 16, nd = ljac_pass_dirs(p);
    const size_t n = (size_t)n_items, key = (size_t)i * nd + d;
    const double *region = out + n * 192 * p;
    L[t] = r < 6 ? region[key * 6 + r] : region[n * nd * 6 + key * 6 + (r - 6)];
}

// [d_wrench; d_sdot] of every (item, direction) = L_item . seeds.  One 64-lane workgroup per item.  A key whose 36 seeds are all
// zero gets exact zeros (the Dual passes' seed_nonzero skip); an item without a nonzero key does not read L.  ds may be NULL.
__global__ void __launch_bounds__(64) k_ljac_apply(int n_dir, const double *L, const double *dp, const double *dt, const double *ds,
                                                   double *dw, double *dsd) {
    __shared__ double sL[kLjacSize];
    __shared__ double sS[16 * kLjacSeedStride];
    const int item = blockIdx.x, lane = threadIdx.x;
    const size_t k0 = (size_t)item * n_dir;
    for (int e = lane; e < n_dir * 24; e += 64) sS[(e / 24) * kLjacSeedStride + e % 24] = dp[k0 * 24 + e];
    for (int e = lane; e < n_dir * 6; e += 64) {
        sS[(e / 6) * kLjacSeedStride + 24 + e % 6] = dt[k0 * 6 + e];
        sS[(e / 6) * kLjacSeedStride + 30 + e % 6] = ds ? ds[k0 * 6 + e] : 0.0;
    }
    __syncthreads();
    bool nz = false;
    if (lane < n_dir)
        for (int k = 0; k < kLjacCols; ++k) nz |= sS[lane * kLjacSeedStride + k] != 0.0;     // (NaN != 0: a NaN seed is a live key)
    const unsigned long long live = __ballot(nz);
    const int n_out = 6 * n_dir;
    if (live == 0ull) {
        for (int o = lane; o < n_out; o += 64) { dw[k0 * 6 + o] = 0.0; dsd[k0 * 6 + o] = 0.0; }
        return;
    }
    const double2 *Lg = reinterpret_cast<const double2 *>(L + (size_t)item * kLjacSize);
    for (int e = lane; e < kLjacSize / 2; e += 64) {
        const double2 v = Lg[e];
        sL[2 * e] = v.x; sL[2 * e + 1] = v.y;
    }
    __syncthreads();
    for (int o = lane; o < 2 * n_out; o += 64) {
        const bool sd = o >= n_out;
        const int q = sd ? o - n_out : o, d = q / 6, r = q % 6 + (sd ? 6 : 0);
        double acc = 0.0;
        if ((live >> d) & 1ull) {
            const double *l = sL + r * kLjacCols, *s = sS + d * kLjacSeedStride;
#pragma unroll 12
            for (int k = 0; k < kLjacCols; ++k) acc = fma(l[k], s[k], acc);
        }
        (sd ? dsd : dw)[k0 * 6 + q] = acc;
    }
}
