// pfc_multi.h -- multi-device handles (pfc_create_multi, SURVEY section 8(b) "pfc_create(device_mask)").  Host code only;
// included by pfc_hip.hip in front of the C ABI.
//
// The reference host is ONE Julia process whose calcXd! loops over the contact instructions
// (src/contact_algorithms_non_friction.jl:60-68); it cannot be launched once per GPU.  A multi-device handle lets that one
// process use every GPU of the node through the same entry points: the handle owns one ordinary handle ("shard") per entry
// of the device list -- meshes, trees and instructions replicated at pfc_add_mesh / pfc_add_instruction / pfc_finalize
// (a few MB) -- and every evaluation cuts its items into CONTIGUOUS ranges, one per shard, balanced by cost (the node tests and
// candidates each item had in the previous evaluation of the same item list; the leaf-count product of its two meshes the first
// time: SURVEY 8(e)).  Items are independent (each force_single_elastic_intersection!, :70-84, reads immutable meshes and its
// own pose / twist / state), so there is no collective in the data path:
//   * host-pointer entry points (pfc_eval, pfc_eval_dual[_bp]): one host thread per shard (persistent workers; the caller's
//     thread takes shard 0) calls the ordinary entry point on its range of the CALLER's arrays -- every device copies its rows
//     from / to the caller's memory itself, nothing is gathered;
//   * device-pointer entry points (pfc_eval_device, pfc_eval_dual_device[_more]): the buffers live on the FIRST device of the
//     list; ranges of shards 1.. are copied to staging buffers on their device (peer copies over xGMI), evaluated there on the
//     shard's own stream and copied back into the caller's buffers; events order everything against the caller's stream, one
//     host thread enqueues it all; pfc_check synchronises every shard.
// A contiguous range keeps the candidate lists grouped the way the single-device path has them, needs no index lists and no
// gather / scatter; what it gives up against a longest-first assignment is balance when single items dominate (they do not in
// the configurations of BASELINE.json: 256 equal scenes, 2 016 pile pairs, batches of poses).
#pragma once
#include "pfc_partition.h"

struct pfc_multi {
    std::vector<pfc_context *> shard;
    std::vector<int> dev;
    int opt_min_items = 8;                 // option "multi_min": items per shard below which fewer shards are used
    // partition of the last evaluation
    std::vector<int> bound;                // items [bound[k], bound[k + 1]) on shard k
    int n_used = 1;
    int part_n = 0;
    bool part_ids = false, part_dev = false;   // ... made for an evaluation with ins_ids / through the device-pointer entry points
    std::vector<int> part_ins;             // the ins_ids the partition (and the costs) belong to (host-pointer entry points)
    std::vector<double> cost;
    bool counts_valid = false;
    PinBuf<int, 2> h_counts;               // pinned: n x 4 counters of the last evaluation
    std::vector<int> iota;
    long long stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // ---- worker threads (host-pointer entry points) ----
    struct Worker {
        std::thread th;
        std::mutex m;
        std::condition_variable cv;
        std::function<int()> job;
        std::atomic<int> state{0};         // 0 idle, 1 job posted, 2 done (result not collected yet), 3 quit
        int rc = 0;
    };
    std::vector<Worker *> workers;         // workers[k - 1] serves shard k
    // ---- device-pointer entry points ----
    struct Stage {
        DevBuf<double> in, out, din, dout;
        DevBuf<int> ids, cnt, iota;
        Event done;
    };
    std::vector<Stage> stage;
    Event ev_fork;
    bool dev_pending = false;              // a device-pointer evaluation is enqueued and not checked yet
    const int *dev_counts = nullptr;       // where shard k's counters lie on ITS device: stage[k].cnt (k = 0: the caller's array or stage[0].cnt)
    hipStream_t dev_stream = nullptr;
    bool dev_kept = false;                 // every shard keeps its pass: pfc_eval_dual_device_more may follow (same partition)
    int dev_reuse_ndir = 0;
};

namespace {

void multi_worker_loop(pfc_multi::Worker *w, int device) {
    (void)hipSetDevice(device);
    for (;;) {
        int st = w->state.load(std::memory_order_acquire);
        // a simulation evaluates back to back: stay awake for a moment after a job before going to sleep on the condition variable
        for (int spin = 0; spin < 20000 && st != 1 && st != 3; ++spin) {
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
            st = w->state.load(std::memory_order_acquire);
        }
        if (st != 1 && st != 3) {
            std::unique_lock<std::mutex> lk(w->m);
            w->cv.wait(lk, [&] { const int s2 = w->state.load(std::memory_order_acquire); return s2 == 1 || s2 == 3; });
            st = w->state.load(std::memory_order_acquire);
        }
        if (st == 3) return;
        w->rc = w->job();
        w->state.store(2, std::memory_order_release);
    }
}

void multi_post(pfc_multi::Worker *w, std::function<int()> f) {
    w->job = std::move(f);
    { std::lock_guard<std::mutex> lk(w->m); w->state.store(1, std::memory_order_release); }
    w->cv.notify_one();
}

int multi_collect(pfc_multi::Worker *w) {
    for (long spin = 0; w->state.load(std::memory_order_acquire) != 2; ++spin) {
        if (spin > 4000) std::this_thread::yield();
#if defined(__x86_64__)
        else __builtin_ia32_pause();
#endif
    }
    const int rc = w->rc;
    w->state.store(0, std::memory_order_release);
    return rc;
}

// jobs[k] for the shards k < n_used (empty function: nothing to do); the caller's thread runs jobs[0].  Returns the first
// non-zero status in shard order and copies that shard's message.
int multi_run(pfc_context *h, std::vector<std::function<int()>> &jobs) {
    pfc_multi *M = h->multi;
    for (size_t k = 1; k < jobs.size(); ++k)
        if (jobs[k]) multi_post(M->workers[k - 1], jobs[k]);
    int rc = jobs[0] ? jobs[0]() : PFC_OK;
    if (rc != PFC_OK) h->err = M->shard[0]->err;
    for (size_t k = 1; k < jobs.size(); ++k)
        if (jobs[k]) {
            const int rk = multi_collect(M->workers[k - 1]);
            if (rk != PFC_OK && rc == PFC_OK) { rc = rk; h->err = M->shard[k]->err; }
        }
    (void)hipSetDevice(M->dev[0]);
    return rc;
}

// Contiguous ranges balanced by cost.  The partition of the previous evaluation is kept while the item list is the same and
// the ranges stay within 15 % of balance under the new costs: the chunks of one Jacobian (same values, other partials,
// src/radau/radau_functions.jl:2-14) must see the same ranges for the shards to reuse their value pass.
// ins_ids: the item list if the host can read it (host-pointer entry points; null = item i is instruction i); on the
// device-pointer path the list is device data: has_ids tells whether there is one, is_dev that its content is not compared (the
// caller re-evaluating the same buffers is the case the cost feedback is for).
void multi_partition(pfc_context *h, int n, const int *ins_ids, bool has_ids, bool is_dev) {
    pfc_multi *M = h->multi;
    const int K = (int)M->shard.size();
    const int k_use = partition_k_use(n, K, M->opt_min_items);
    const bool same_list = M->part_n == n && M->part_ids == has_ids && M->part_dev == is_dev && (int)M->bound.size() == K + 1 &&
                           (is_dev || !ins_ids || std::memcmp(M->part_ins.data(), ins_ids, sizeof(int) * (size_t)n) == 0);
    M->cost.resize((size_t)n);
    if (same_list && M->counts_valid) {
        for (int i = 0; i < n; ++i) M->cost[i] = partition_cost_counters(M->h_counts.p[4 * (size_t)i], M->h_counts.p[4 * (size_t)i + 1]);
    } else {
        const pfc_context *c0 = M->shard[0];
        for (int i = 0; i < n; ++i) {
            double c = partition_cost_leaves(0.0, 0.0);
            if (!(is_dev && has_ids)) {      // (a device-resident item list cannot be read here: equal costs until the counters are known)
                const int id = ins_ids ? ins_ids[i] : i;
                if (id >= 0 && id < (int)c0->ins.size())
                    c = partition_cost_leaves((double)c0->meshes[c0->ins[id].m1].n_leaf, (double)c0->meshes[c0->ins[id].m2].n_leaf);
            }
            M->cost[i] = c;
        }
    }
    if (same_list && M->n_used == k_use && partition_keeps(M->cost.data(), n, M->bound.data(), k_use)) return;      // still balanced: keep the ranges
    M->bound.resize((size_t)K + 1);
    partition_cut(M->cost.data(), n, k_use, K, M->bound.data());
    M->n_used = k_use;
    M->part_n = n; M->part_ids = has_ids; M->part_dev = is_dev;
    if (ins_ids && !is_dev) M->part_ins.assign(ins_ids, ins_ids + n); else M->part_ins.clear();
    M->dev_kept = false;
}

int multi_ensure_host(pfc_context *h, int n) {
    pfc_multi *M = h->multi;
    bool moved = false;
    const hipError_t e = M->h_counts.ensure((size_t)n * 4, &moved);
    if (moved) M->counts_valid = false;
    HIP_TRY(h, e);
    if ((int)M->iota.size() < n) {
        const int n0 = (int)M->iota.size();
        M->iota.resize((size_t)n * 2);
        for (int i = n0; i < (int)M->iota.size(); ++i) M->iota[i] = i;
    }
    return PFC_OK;
}

void multi_merge_stats(pfc_context *h) {
    pfc_multi *M = h->multi;
    for (int k = 0; k < 8; ++k) M->stats[k] = 0;
    for (int k = 0; k < M->n_used; ++k) {
        const long long *s = M->shard[k]->stats;
        for (int j = 0; j < 4; ++j) M->stats[j] += s[j];
        if (s[4] > M->stats[4]) M->stats[4] = s[4];
        if (s[5] > M->stats[5]) M->stats[5] = s[5];
        M->stats[6] |= s[6];
        M->stats[7] += s[7];
    }
}

int multi_check_args(pfc_context *h, int n_items, const void *ins_ids, const void *pose, const void *twist, const void *wrench,
                     const void *sdot) {
    pfc_context *c0 = h->multi->shard[0];
    if (!c0->finalized) return fail(h, PFC_ERR_STATE, "pfc_eval before pfc_finalize");
    if (n_items < 0) return fail(h, PFC_ERR_BAD_ARG, "negative n_items");
    if (n_items == 0) return PFC_OK;
    if (c0->ins.empty()) return fail(h, PFC_ERR_STATE, "no contact instructions");
    if (!pose || !twist || !wrench || !sdot) return fail(h, PFC_ERR_BAD_ARG, "null buffer");
    if (!ins_ids && n_items > (int)c0->ins.size())
        return fail(h, PFC_ERR_BAD_ARG, "n_items exceeds the number of instructions and no ins_ids given");
    return PFC_OK;
}

// ---- host-pointer entry points -----------------------------------------------------------------------------------
int multi_eval(pfc_context *h, int n_items, const int *ins_ids, const double *pose, const double *twist, const double *s,
               double *wrench, double *sdot, int *counts) {
    pfc_multi *M = h->multi;
    { const int rc = multi_check_args(h, n_items, ins_ids, pose, twist, wrench, sdot); if (rc != PFC_OK || n_items == 0) return rc; }
    if (M->shard[0]->any_bristle && !s) return fail(h, PFC_ERR_BAD_ARG, "bristle instructions need the state buffer s");
    { const int rc = multi_ensure_host(h, n_items); if (rc != PFC_OK) return rc; }
    multi_partition(h, n_items, ins_ids, ins_ids != nullptr, false);
    M->dev_pending = false; M->dev_kept = false;
    const int *ids = ins_ids ? ins_ids : M->iota.data();
    int *cnt = M->h_counts.p;
    std::vector<std::function<int()>> jobs((size_t)M->n_used);
    for (int k = 0; k < M->n_used; ++k) {
        const int b0 = M->bound[k], nk = M->bound[k + 1] - b0;
        if (nk <= 0) continue;
        pfc_context *c = M->shard[k];
        const int *idk = (k == 0 && !ins_ids) ? nullptr : ids + b0;
        jobs[k] = [=]() {
            return pfc_eval(c, nk, idk, pose + 24 * (size_t)b0, twist + 6 * (size_t)b0, s ? s + 6 * (size_t)b0 : nullptr,
                            wrench + 6 * (size_t)b0, sdot + 6 * (size_t)b0, cnt + 4 * (size_t)b0);
        };
    }
    const int rc = multi_run(h, jobs);
    M->counts_valid = rc == PFC_OK;
    if (rc != PFC_OK) return rc;
    if (counts) std::memcpy(counts, cnt, sizeof(int) * (size_t)n_items * 4);
    multi_merge_stats(h);
    return PFC_OK;
}

int multi_eval_dual(pfc_context *h, int n_items, int n_dir, const int *ins_ids, const double *pose, const double *bp_pose,
                    const double *twist, const double *s, const double *d_pose, const double *d_twist, const double *d_s,
                    double *wrench, double *sdot, double *d_wrench, double *d_sdot, int *counts) {
    pfc_multi *M = h->multi;
    if (n_dir < 1 || n_dir > 16) return fail(h, PFC_ERR_BAD_ARG, "pfc_eval_dual: n_dir must be in 1..16");
    if (n_items > 0 && (!d_pose || !d_twist || !d_wrench || !d_sdot)) return fail(h, PFC_ERR_BAD_ARG, "pfc_eval_dual: null buffer");
    { const int rc = multi_check_args(h, n_items, ins_ids, pose, twist, wrench, sdot); if (rc != PFC_OK || n_items == 0) return rc; }
    if (M->shard[0]->any_bristle && !s) return fail(h, PFC_ERR_BAD_ARG, "bristle instructions need the state buffer s");
    { const int rc = multi_ensure_host(h, n_items); if (rc != PFC_OK) return rc; }
    multi_partition(h, n_items, ins_ids, ins_ids != nullptr, false);
    M->dev_pending = false; M->dev_kept = false;
    const int *ids = ins_ids ? ins_ids : M->iota.data();
    int *cnt = M->h_counts.p;
    const size_t nd = (size_t)n_dir;
    std::vector<std::function<int()>> jobs((size_t)M->n_used);
    for (int k = 0; k < M->n_used; ++k) {
        const size_t b0 = (size_t)M->bound[k];
        const int nk = M->bound[k + 1] - (int)b0;
        if (nk <= 0) continue;
        pfc_context *c = M->shard[k];
        const int *idk = (k == 0 && !ins_ids) ? nullptr : ids + b0;
        jobs[k] = [=]() {
            return pfc_eval_dual_bp(c, nk, n_dir, idk, pose + 24 * b0, bp_pose ? bp_pose + 24 * b0 : nullptr, twist + 6 * b0,
                                    s ? s + 6 * b0 : nullptr, d_pose + 24 * nd * b0, d_twist + 6 * nd * b0,
                                    d_s ? d_s + 6 * nd * b0 : nullptr, wrench + 6 * b0, sdot + 6 * b0, d_wrench + 6 * nd * b0,
                                    d_sdot + 6 * nd * b0, cnt + 4 * b0);
        };
    }
    const int rc = multi_run(h, jobs);
    M->counts_valid = rc == PFC_OK;
    if (rc != PFC_OK) return rc;
    if (counts) std::memcpy(counts, cnt, sizeof(int) * (size_t)n_items * 4);
    multi_merge_stats(h);
    return PFC_OK;
}

// ---- device-pointer entry points ---------------------------------------------------------------------------------
hipError_t multi_copy(void *dst, int dst_dev, const void *src, int src_dev, size_t bytes, hipStream_t st) {
    if (bytes == 0) return hipSuccess;
    if (dst_dev == src_dev) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
    return hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, st);
}

// device iota of shard k covering [0, n)
int multi_dev_iota(pfc_context *h, int k, int n) {
    pfc_multi *M = h->multi;
    pfc_multi::Stage &S = M->stage[k];
    if (S.iota.cap >= (size_t)n) return PFC_OK;
    HIP_TRY(h, S.iota.ensure((size_t)n));        // (multi_ensure_host has made the host iota at least n long)
    HIP_TRY(h, hipMemcpyAsync(S.iota.p, M->iota.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, M->shard[k]->stream));
    HIP_TRY(h, hipStreamSynchronize(M->shard[k]->stream));
    return PFC_OK;
}

// The fan-out of the device-pointer entry points.  Every shard k >= 1 with items runs on its device and stream behind the caller's
// stream st0 (fork event): stage(k) makes its staging ready (nothing there waits for st0), run(k, stream) copies its range in, calls
// the shard and copies the results back into the caller's buffers; then run(0, st0) evaluates shard 0 on the caller's arrays and
// stream, which waits for every other shard.  Both return a status with its message in h->err.  One exit for errors: once shards
// have work enqueued (copies that write into the caller's buffers; staging the next call may reallocate), the streams that may
// hold some are synchronised and the shards' pending calls dropped (drop_pending) before the first error is returned.  The caller's thread is
// back on the first device -- the one its buffers and its stream live on -- whichever way this returns.
template <class StageFn, class RunFn>
int multi_fan_out(pfc_context *h, hipStream_t st0, const char *what, StageFn stage, RunFn run) {
    pfc_multi *M = h->multi;
    const int dev0 = M->dev[0];
    int rc = PFC_OK, enq = 1;      // shards [1, enq) may have work enqueued
    hipError_t e = hipSetDevice(dev0);
    if (e == hipSuccess && M->n_used > 1) e = hipEventRecord(M->ev_fork, st0);
    for (int k = 1; k < M->n_used && rc == PFC_OK && e == hipSuccess; ++k) {
        if (M->bound[k + 1] <= M->bound[k]) continue;
        hipStream_t sk = M->shard[k]->stream;
        if ((e = hipSetDevice(M->dev[k])) != hipSuccess || (rc = stage(k)) != PFC_OK || (e = hipStreamWaitEvent(sk, M->ev_fork, 0)) != hipSuccess)
            break;
        enq = k + 1;
        if ((rc = run(k, sk)) == PFC_OK) e = hipEventRecord(M->stage[k].done, sk);
    }
    if (rc == PFC_OK && e == hipSuccess && (e = hipSetDevice(dev0)) == hipSuccess) {
        rc = run(0, st0);
        for (int k = 1; k < M->n_used && rc == PFC_OK && e == hipSuccess; ++k)
            if (M->bound[k + 1] > M->bound[k]) e = hipStreamWaitEvent(st0, M->stage[k].done, 0);
    }
    if (rc == PFC_OK && e != hipSuccess) rc = fail(h, PFC_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    if (rc != PFC_OK) {
        for (int k = 1; k < enq; ++k) {
            (void)hipSetDevice(M->dev[k]);
            (void)hipStreamSynchronize(M->shard[k]->stream);
            drop_pending(M->shard[k]);
        }
        (void)hipSetDevice(dev0);
        (void)hipStreamSynchronize(st0);
        drop_pending(M->shard[0]);
    }
    return rc;
}

// value evaluation (n_dir == 0) or Dual evaluation with every buffer on device dev[0]
int multi_eval_device(pfc_context *h, int n_items, int n_dir, const int *d_ins_ids, const double *d_pose, const double *d_bp,
                      const double *d_twist, const double *d_s, const double *d_dpose, const double *d_dtwist, const double *d_ds,
                      double *d_wrench, double *d_sdot, double *d_dwrench, double *d_dsdot, int *d_counts, void *stream) {
    pfc_multi *M = h->multi;
    { const int rc = multi_check_args(h, n_items, d_ins_ids, d_pose, d_twist, d_wrench, d_sdot); if (rc != PFC_OK) return rc; }
    M->dev_pending = false; M->dev_kept = false;
    if (n_items == 0) return PFC_OK;
    if (M->shard[0]->any_bristle && !d_s) return fail(h, PFC_ERR_BAD_ARG, "bristle instructions need the state buffer s");
    if (n_dir && (n_dir < 1 || n_dir > 16)) return fail(h, PFC_ERR_BAD_ARG, "pfc_eval_dual_device: n_dir must be in 1..16");
    if (n_dir && (!d_dpose || !d_dtwist || !d_dwrench || !d_dsdot)) return fail(h, PFC_ERR_BAD_ARG, "pfc_eval_dual_device: null buffer");
    { const int rc = multi_ensure_host(h, n_items); if (rc != PFC_OK) return rc; }
    // the item list is device data: the partition is made for (n_items, ids given or not) and balanced by the counters the
    // previous check brought back
    multi_partition(h, n_items, nullptr, d_ins_ids != nullptr, true);
    const int dev0 = M->dev[0];
    hipStream_t st0 = stream ? (hipStream_t)stream : M->shard[0]->stream;
    const size_t nd = (size_t)n_dir;
    auto stage = [&](int k) -> int {
        pfc_multi::Stage &S = M->stage[k];
        const size_t n = (size_t)(M->bound[k + 1] - M->bound[k]);
        HIP_TRY(h, S.in.ensure(ValueBlock(nullptr, n).doubles() + n * 24)); HIP_TRY(h, S.out.ensure(ResultBlock(nullptr, n).doubles())); HIP_TRY(h, S.cnt.ensure(n * 4));
        if (d_ins_ids) HIP_TRY(h, S.ids.ensure(n));
        else return multi_dev_iota(h, k, n_items);
        return PFC_OK;
    };
    auto run = [&](int k, hipStream_t sk) -> int {
        pfc_context *c = M->shard[k];
        const size_t b0 = (size_t)M->bound[k];
        const int nk = M->bound[k + 1] - (int)b0;
        int rc;
        if (k == 0) {      // the caller's arrays in place
            int *cnt0 = d_counts;
            if (!cnt0) { HIP_TRY(h, M->stage[0].cnt.ensure((size_t)nk * 4)); cnt0 = M->stage[0].cnt.p; }
            M->dev_counts = cnt0;
            if (n_dir == 0) rc = pfc_eval_device(c, nk, d_ins_ids, d_pose, d_twist, d_s, d_wrench, d_sdot, cnt0, st0);
            else rc = pfc_eval_dual_device_bp(c, nk, n_dir, d_ins_ids, d_pose, d_bp, d_twist, d_s, d_dpose, d_dtwist, d_ds, d_wrench, d_sdot,
                                              d_dwrench, d_dsdot, cnt0, st0);
            if (rc != PFC_OK) h->err = c->err;
            return rc;
        }
        pfc_multi::Stage &S = M->stage[k];
        const int dk = M->dev[k];
        const size_t n = (size_t)nk;
        const int *idk = d_ins_ids ? S.ids.p : S.iota.p + b0;
        const ValueBlock vi(S.in.p, n); const ResultBlock ro(S.out.p, n);      // (ids and counts apart: S.ids, S.cnt; the broadphase pose behind the values)
        double *ip = vi.pose(), *it = vi.twist(), *is = vi.s(), *ib = vi.p + vi.doubles(), *ow = ro.wrench(), *os = ro.sdot();
        if (d_ins_ids) HIP_TRY(h, multi_copy(S.ids.p, dk, d_ins_ids + b0, dev0, sizeof(int) * n, sk));
        HIP_TRY(h, multi_copy(ip, dk, d_pose + 24 * b0, dev0, sizeof(double) * n * 24, sk));
        HIP_TRY(h, multi_copy(it, dk, d_twist + 6 * b0, dev0, sizeof(double) * n * 6, sk));
        if (d_s) HIP_TRY(h, multi_copy(is, dk, d_s + 6 * b0, dev0, sizeof(double) * n * 6, sk));
        if (d_bp) HIP_TRY(h, multi_copy(ib, dk, d_bp + 24 * b0, dev0, sizeof(double) * n * 24, sk));
        if (n_dir == 0) {
            rc = pfc_eval_device(c, nk, idk, ip, it, d_s ? is : nullptr, ow, os, S.cnt.p, sk);
        } else {
            HIP_TRY(h, S.din.ensure(SeedBlock(nullptr, n * nd).doubles())); HIP_TRY(h, S.dout.ensure(PartialBlock(nullptr, n * nd).doubles()));
            const SeedBlock sd(S.din.p, n * nd); const PartialBlock pd(S.dout.p, n * nd);
            double *dp = sd.d_pose(), *dt = sd.d_twist(), *dsd = sd.d_s(), *dw = pd.d_wrench(), *dsdot = pd.d_sdot();
            HIP_TRY(h, multi_copy(dp, dk, d_dpose + 24 * nd * b0, dev0, sizeof(double) * n * nd * 24, sk));
            HIP_TRY(h, multi_copy(dt, dk, d_dtwist + 6 * nd * b0, dev0, sizeof(double) * n * nd * 6, sk));
            if (d_ds) HIP_TRY(h, multi_copy(dsd, dk, d_ds + 6 * nd * b0, dev0, sizeof(double) * n * nd * 6, sk));
            rc = pfc_eval_dual_device_bp(c, nk, n_dir, idk, ip, d_bp ? ib : nullptr, it, d_s ? is : nullptr, dp, dt, d_ds ? dsd : nullptr,
                                         ow, os, dw, dsdot, S.cnt.p, sk);
            if (rc == PFC_OK) {
                HIP_TRY(h, multi_copy(d_dwrench + 6 * nd * b0, dev0, dw, dk, sizeof(double) * n * nd * 6, sk));
                HIP_TRY(h, multi_copy(d_dsdot + 6 * nd * b0, dev0, dsdot, dk, sizeof(double) * n * nd * 6, sk));
            }
        }
        if (rc != PFC_OK) { h->err = c->err; return rc; }
        HIP_TRY(h, multi_copy(d_wrench + 6 * b0, dev0, ow, dk, sizeof(double) * n * 6, sk));
        HIP_TRY(h, multi_copy(d_sdot + 6 * b0, dev0, os, dk, sizeof(double) * n * 6, sk));
        if (d_counts) HIP_TRY(h, multi_copy(d_counts + 4 * b0, dev0, S.cnt.p, dk, sizeof(int) * n * 4, sk));
        return PFC_OK;
    };
    const int rc = multi_fan_out(h, st0, n_dir ? "pfc_eval_dual_device" : "pfc_eval_device", stage, run);
    if (rc != PFC_OK) return rc;
    M->dev_pending = true; M->dev_stream = st0; M->dev_reuse_ndir = n_dir;
    return PFC_OK;
}

int multi_eval_dual_device_more(pfc_context *h, int n_dir, const double *d_dpose, const double *d_dtwist, const double *d_ds,
                                double *d_dwrench, double *d_dsdot, void *stream) {
    pfc_multi *M = h->multi;
    if (n_dir < 1 || n_dir > 16) return fail(h, PFC_ERR_BAD_ARG, "pfc_eval_dual_device_more: n_dir must be in 1..16");
    if (!M->dev_kept)
        return fail(h, PFC_ERR_STATE, "pfc_eval_dual_device_more: no checked pfc_eval_dual_device evaluation on this handle to extend");
    if (!d_dpose || !d_dtwist || !d_dwrench || !d_dsdot) return fail(h, PFC_ERR_BAD_ARG, "pfc_eval_dual_device_more: null buffer");
    const int dev0 = M->dev[0];
    hipStream_t st0 = stream ? (hipStream_t)stream : M->shard[0]->stream;
    const size_t nd = (size_t)n_dir;
    auto stage = [&](int k) -> int {
        pfc_multi::Stage &S = M->stage[k];
        const size_t n = (size_t)(M->bound[k + 1] - M->bound[k]);
        HIP_TRY(h, S.din.ensure(SeedBlock(nullptr, n * nd).doubles())); HIP_TRY(h, S.dout.ensure(PartialBlock(nullptr, n * nd).doubles()));
        return PFC_OK;
    };
    auto run = [&](int k, hipStream_t sk) -> int {
        pfc_context *c = M->shard[k];
        if (k == 0) {
            const int rc = pfc_eval_dual_device_more(c, n_dir, d_dpose, d_dtwist, d_ds, d_dwrench, d_dsdot, st0);
            if (rc != PFC_OK) h->err = c->err;
            return rc;
        }
        pfc_multi::Stage &S = M->stage[k];
        const int dk = M->dev[k];
        const size_t b0 = (size_t)M->bound[k], n = (size_t)M->bound[k + 1] - b0;
        const SeedBlock sd(S.din.p, n * nd); const PartialBlock pd(S.dout.p, n * nd);
        double *dp = sd.d_pose(), *dt = sd.d_twist(), *dsd = sd.d_s(), *dw = pd.d_wrench(), *dsdot = pd.d_sdot();
        HIP_TRY(h, multi_copy(dp, dk, d_dpose + 24 * nd * b0, dev0, sizeof(double) * n * nd * 24, sk));
        HIP_TRY(h, multi_copy(dt, dk, d_dtwist + 6 * nd * b0, dev0, sizeof(double) * n * nd * 6, sk));
        if (d_ds) HIP_TRY(h, multi_copy(dsd, dk, d_ds + 6 * nd * b0, dev0, sizeof(double) * n * nd * 6, sk));
        const int rc = pfc_eval_dual_device_more(c, n_dir, dp, dt, d_ds ? dsd : nullptr, dw, dsdot, sk);
        if (rc != PFC_OK) { h->err = c->err; return rc; }
        HIP_TRY(h, multi_copy(d_dwrench + 6 * nd * b0, dev0, dw, dk, sizeof(double) * n * nd * 6, sk));
        HIP_TRY(h, multi_copy(d_dsdot + 6 * nd * b0, dev0, dsdot, dk, sizeof(double) * n * nd * 6, sk));
        return PFC_OK;
    };
    const int rc = multi_fan_out(h, st0, "pfc_eval_dual_device_more", stage, run);
    if (rc != PFC_OK) return rc;
    M->dev_pending = true; M->dev_stream = st0; M->dev_reuse_ndir = -1;      // (-1: a further chunk -- the counters are not brought back again)
    return PFC_OK;
}

// pfc_local_jacobian_device over the shards: each builds the rows of L of its range on the value pass it keeps; shards 1.. write
// theirs into staging on their device and copy them into d_L on the first.
int multi_local_jacobian_device(pfc_context *h, double *d_L, void *stream) {
    pfc_multi *M = h->multi;
    if (!M->dev_kept)
        return fail(h, PFC_ERR_STATE, "pfc_local_jacobian_device: no checked pfc_eval_dual_device evaluation on this handle");
    if (!d_L) return fail(h, PFC_ERR_BAD_ARG, "pfc_local_jacobian_device: null buffer");
    const int dev0 = M->dev[0];
    hipStream_t st0 = stream ? (hipStream_t)stream : M->shard[0]->stream;
    auto stage = [&](int k) -> int {
        HIP_TRY(h, M->stage[k].dout.ensure((size_t)(M->bound[k + 1] - M->bound[k]) * kLjacSize));
        return PFC_OK;
    };
    auto run = [&](int k, hipStream_t sk) -> int {
        pfc_context *c = M->shard[k];
        double *out = k == 0 ? d_L : M->stage[k].dout.p;
        const int rc = pfc_local_jacobian_device(c, out, sk);
        if (rc != PFC_OK) { h->err = c->err; return rc; }
        const size_t b0 = (size_t)M->bound[k], n = (size_t)M->bound[k + 1] - b0;
        if (k > 0) HIP_TRY(h, multi_copy(d_L + kLjacSize * b0, dev0, out, M->dev[k], sizeof(double) * n * kLjacSize, sk));
        return PFC_OK;
    };
    const int rc = multi_fan_out(h, st0, "pfc_local_jacobian_device", stage, run);
    if (rc != PFC_OK) return rc;
    M->dev_pending = true; M->dev_stream = st0; M->dev_reuse_ndir = -1;      // pfc_check as after pfc_eval_dual_device_more
    return PFC_OK;
}

int multi_check(pfc_context *h) {
    pfc_multi *M = h->multi;
    if (!M->dev_pending) return PFC_OK;
    M->dev_pending = false;
    const bool more = M->dev_reuse_ndir < 0;
    int rc = PFC_OK;
    // every shard is checked (each grows its own lists on overflow); the first failure in shard order is reported
    for (int k = 0; k < M->n_used; ++k) {
        const int nk = M->bound[k + 1] - M->bound[k];
        if (nk <= 0) continue;
        pfc_context *c = M->shard[k];
        (void)hipSetDevice(M->dev[k]);
        if (!more) {
            const int *src = k == 0 ? M->dev_counts : M->stage[k].cnt.p;
            hipStream_t sk = k == 0 ? M->dev_stream : c->stream;
            if (hipMemcpyAsync(M->h_counts.p + 4 * (size_t)M->bound[k], src, sizeof(int) * 4 * (size_t)nk, hipMemcpyDeviceToHost, sk) != hipSuccess)
                (void)hipGetLastError();
        }
        const int rk = pfc_check(c);
        if (rk != PFC_OK && rc == PFC_OK) { rc = rk; h->err = c->err; }
    }
    (void)hipSetDevice(M->dev[0]);
    // the caller's stream has the shards' results behind their events: synchronise it too (pfc_check's contract)
    if (M->n_used > 1 && M->dev_stream) {
        const hipError_t e = hipStreamSynchronize(M->dev_stream);
        if (e != hipSuccess && rc == PFC_OK) rc = fail(h, PFC_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    }
    if (!more) M->counts_valid = rc == PFC_OK;
    if (rc == PFC_OK) {
        if (!more) multi_merge_stats(h);
        M->dev_kept = more ? true : M->dev_reuse_ndir > 0;
        if (M->dev_kept)
            for (int k = 0; k < M->n_used; ++k)
                if (M->bound[k + 1] > M->bound[k] && !M->shard[k]->device_kept()) M->dev_kept = false;
    }
    return rc;
}

// the shard that evaluated item `item` of the last evaluation and the item's index there
pfc_context *multi_locate(pfc_context *h, int item, int *local) {
    pfc_multi *M = h->multi;
    for (int k = 0; k < M->n_used && k + 1 < (int)M->bound.size(); ++k)
        if (item >= M->bound[k] && item < M->bound[k + 1]) { *local = item - M->bound[k]; return M->shard[k]; }
    return nullptr;
}

// An entry point run on shard c of a multi-device handle h: a failure -- a status other than PFC_OK, or a negative id / count
// where the entry point returns one (`count`) -- leaves the shard's message in h.
template <class F>
int on_shard(pfc_context *h, pfc_context *c, F call, bool count = false) {
    const int r = call(c);
    if (count ? r < 0 : r != PFC_OK) h->err = c->err;
    return r;
}
// ... on the first shard: what runs on one device only (the scatter calls, the contact surface, L times seeds, the stage times).
template <class F>
int on_first_shard(pfc_context *h, F call) { return on_shard(h, h->multi->shard[0], call); }

// A surface call on a multi-device handle runs on the first device's context; the handle's pending device-pointer evaluation
// and its Dual reuse end here, as with any other evaluation.
template <class F>
int surface_ctx(pfc_context *h, F call) {
    h->multi->dev_pending = false; h->multi->dev_kept = false;
    return on_first_shard(h, call);
}

void multi_destroy(pfc_context *h) {
    pfc_multi *M = h->multi;
    for (pfc_multi::Worker *w : M->workers) {
        { std::lock_guard<std::mutex> lk(w->m); w->state.store(3, std::memory_order_release); }
        w->cv.notify_one();
        if (w->th.joinable()) w->th.join();
        delete w;
    }
    for (size_t k = 0; k < M->shard.size(); ++k) {
        (void)hipSetDevice(M->dev[k]);
        if (M->shard[k]->stream) (void)hipStreamSynchronize(M->shard[k]->stream);
        if (k < M->stage.size()) M->stage[k] = pfc_multi::Stage();      // its staging goes with the shard's device current
        pfc_destroy(M->shard[k]);
    }
    (void)hipSetDevice(M->dev.empty() ? 0 : M->dev[0]);
    delete M;
    h->multi = nullptr;
}

}  // namespace
