// pfc_partition.h -- how a multi-device handle cuts the n items of an evaluation into contiguous ranges, one per shard.
// Host code only: no HIP header, no pfc_context; included by pfc_multi.h (multi_partition is the one caller in the library)
// and, alone, by tests/partition_check.cpp.  tests/partition_reference.py states the same functions in Python floats.
//
//   cost[i]   what item i is expected to take: partition_cost_leaves the first time an item list is seen, partition_cost_counters
//             once the counters of the previous evaluation of the same list are known;
//   k_use     shards that take part: n / multi_min, at least 1, at most K (partition_k_use);
//   bound     K + 1 entries; shard k evaluates the items [bound[k], bound[k + 1]); bound[k] = n for k >= k_use (partition_cut);
//   keep      the ranges of the previous evaluation stay while the most loaded shard is within 15 % of the mean under the new
//             costs (partition_keeps): the chunks of one Jacobian must see the same ranges for the shards to reuse their value pass.
#pragma once

// the first evaluation of an item list: the leaf-count product of the item's two meshes
inline double partition_cost_leaves(double n_leaf_1, double n_leaf_2) { return 64.0 + 0.02 * n_leaf_1 * n_leaf_2; }
// ... and afterwards what the item did in the previous evaluation (counters 0 and 1 of its row)
inline double partition_cost_counters(int node_tests, int candidates) { return 64.0 + (double)node_tests + 4.0 * (double)candidates; }

// shards used for n items on K shards: min_items (option "multi_min") items per shard at least
inline int partition_k_use(int n, int K, int min_items) {
    int k_use = n / (min_items > 0 ? min_items : 1);
    if (k_use > K) k_use = K;
    if (k_use < 1) k_use = 1;
    return k_use;
}

// Are the ranges bound[0..k_use] still balanced under cost[0..n)?  worst * k_use <= 1.15 * total.
inline bool partition_keeps(const double *cost, int n, const int *bound, int k_use) {
    double total = 0.0;
    for (int i = 0; i < n; ++i) total += cost[i];
    double worst = 0.0;
    for (int k = 0; k < k_use; ++k) {
        double c = 0.0;
        for (int i = bound[k]; i < bound[k + 1]; ++i) c += cost[i];
        if (c > worst) worst = c;
    }
    return worst * k_use <= 1.15 * total;
}

// Cut [0, n) into k_use contiguous ranges of about total / k_use each: boundary k goes in front of the first item whose half
// would cross k * total / k_use (so it lies within half an item of its target), then every used shard is given an item at
// least (both clamps; they need n >= k_use, which partition_k_use gives for min_items >= 1).  Writes bound[0..K].
inline void partition_cut(const double *cost, int n, int k_use, int K, int *bound) {
    double total = 0.0;
    for (int i = 0; i < n; ++i) total += cost[i];
    bound[0] = 0;
    double acc = 0.0;
    int i = 0;
    for (int k = 1; k < k_use; ++k) {
        const double target = total * (double)k / (double)k_use;
        while (i < n && acc + 0.5 * cost[i] < target) acc += cost[i++];
        int b = i;
        if (b < bound[k - 1] + 1) b = bound[k - 1] + 1;      // every used shard gets an item
        if (b > n - (k_use - k)) b = n - (k_use - k);
        while (i < b) acc += cost[i++];
        bound[k] = b;
    }
    for (int k = k_use; k <= K; ++k) bound[k] = n;
}
