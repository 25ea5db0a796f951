// Stand-alone driver of csrc/pfc_partition.h (tests/test_partition.py builds it with AddressSanitizer and UBSan and compares
// its output with tests/partition_reference.py).  Every array is allocated to the element, so a read or write of bound[K + 1],
// cost[n] or bound[-1] is a sanitizer report.
//
// stdin, one case per line:   K n min_items has_prev [prev_k_use prev_bound[0..K]] cost[0..n)
//   costs are hexadecimal floating-point literals, so they arrive bit for bit; the previous partition is optional.
//   A line "c n_leaf_1 n_leaf_2 node_tests candidates" prints the two cost formulas instead.
// stdout, one line per case:  k_use keep_prev keep_fresh | bound[0..K] | bound[0..K] of a second cut
//   keep_prev: partition_keeps of the previous partition under these costs (-1: none given, or it used another k_use);
//   keep_fresh: partition_keeps of the cut just made.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "pfc_partition.h"

static bool next_line(std::string &line) {
    line.clear();
    int c;
    while ((c = std::getchar()) != EOF && c != '\n') line.push_back((char)c);
    return c != EOF || !line.empty();
}

int main() {
    std::string line;
    long n_cases = 0;
    while (next_line(line)) {
        if (line.empty()) continue;
        const char *p = line.c_str();
        char *end = nullptr;
        if (*p == 'c') {      // "c n_leaf_1 n_leaf_2 node_tests candidates": the two cost formulas, printed bit for bit
            long a = 0, b = 0, c = 0, d = 0;
            if (std::sscanf(p + 1, "%ld %ld %ld %ld", &a, &b, &c, &d) != 4) { std::fprintf(stderr, "bad cost line\n"); return 2; }
            std::printf("c %a %a\n", partition_cost_leaves((double)a, (double)b), partition_cost_counters((int)c, (int)d));
            continue;
        }
        auto rd_int = [&]() { const long v = std::strtol(p, &end, 10); if (end == p) { std::fprintf(stderr, "case %ld: integer expected\n", n_cases); std::exit(2); } p = end; return (int)v; };
        auto rd_dbl = [&]() { const double v = std::strtod(p, &end); if (end == p) { std::fprintf(stderr, "case %ld: cost expected\n", n_cases); std::exit(2); } p = end; return v; };
        const int K = rd_int(), n = rd_int(), min_items = rd_int(), has_prev = rd_int();
        if (K < 1 || n < 1) { std::fprintf(stderr, "case %ld: K and n must be positive\n", n_cases); return 2; }
        std::unique_ptr<int[]> prev(new int[(size_t)K + 1]);
        int prev_k_use = -1;
        if (has_prev) {
            prev_k_use = rd_int();
            for (int k = 0; k <= K; ++k) prev[k] = rd_int();
        }
        std::unique_ptr<double[]> cost(new double[(size_t)n]);
        for (int i = 0; i < n; ++i) cost[i] = rd_dbl();

        const int k_use = partition_k_use(n, K, min_items);
        int keep_prev = -1;
        if (has_prev && prev_k_use == k_use) keep_prev = partition_keeps(cost.get(), n, prev.get(), k_use) ? 1 : 0;
        std::unique_ptr<int[]> bound(new int[(size_t)K + 1]), again(new int[(size_t)K + 1]);
        partition_cut(cost.get(), n, k_use, K, bound.get());
        const int keep_fresh = partition_keeps(cost.get(), n, bound.get(), k_use) ? 1 : 0;
        partition_cut(cost.get(), n, k_use, K, again.get());

        std::printf("%d %d %d |", k_use, keep_prev, keep_fresh);
        for (int k = 0; k <= K; ++k) std::printf(" %d", bound[k]);
        std::printf(" |");
        for (int k = 0; k <= K; ++k) std::printf(" %d", again[k]);
        std::printf("\n");
        ++n_cases;
    }
    std::printf("partition ok %ld\n", n_cases);
    return 0;
}
