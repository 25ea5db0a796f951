// pfc_hostblocks.h -- the blocks the host-pointer entry points move between caller arrays, pinned host memory and the device.
// Plain C++ (no HIP, no pfc_context): a view is a base pointer and a count, and the same view type addresses the pinned host
// copy of a block, its device-visible mapping or BAR mirror, and its staged device buffer.  This header is the one statement
// of the layouts (tests/hostblocks_check.cpp holds the second, with the offsets written out):
//   value block    pose n x 24 | twist n x 6 | s n x 6 | ids n ints, ids_at doubles in (n x 36 unless another block sits between)
//   seed block     d_pose nk x 24 | d_twist nk x 6 | d_s nk x 6 (the all-in-one kernel takes no d_s)
//   result block   wrench n x 6 | sdot n x 6 | counts n x 4 ints, counts_at doubles in (n x 12 ...) | fused kernel: n x 8 ints
//   partial block  d_wrench nk x 6 | d_sdot nk x 6
//   one-sync in    value block | seed block | ids          one-sync out    result block | partial block | counts
#pragma once
#include <cstddef>
#include <cstring>

namespace pfc_blocks {

// Doubles that hold `bytes` of a block whose tail is ints, and one spare (the sizes the staging buffers have always had).
inline size_t doubles_for(size_t bytes) { return (bytes + 7) / 8 + 1; }

struct ValueBlock {
    double *p; size_t n, ids_at;
    ValueBlock(void *base, size_t n_items) : p((double *)base), n(n_items), ids_at(n_items * 36) {}
    ValueBlock(void *base, size_t n_items, size_t ids_at_) : p((double *)base), n(n_items), ids_at(ids_at_) {}
    double *pose() const { return p; }           double *twist() const { return p + n * 24; }
    double *s() const { return p + n * 30; }     int *ids() const { return reinterpret_cast<int *>(p + ids_at); }
    size_t doubles() const { return n * 36; }
    size_t bytes(bool with_ids) const { return doubles() * sizeof(double) + (with_ids ? n * sizeof(int) : 0); }
};

struct SeedBlock {
    double *p; size_t nk;
    SeedBlock(void *base, size_t n_keys) : p((double *)base), nk(n_keys) {}
    double *d_pose() const { return p; }         double *d_twist() const { return p + nk * 24; }
    double *d_s() const { return p + nk * 30; }
    size_t doubles(bool with_s = true) const { return nk * (with_s ? 36 : 30); }
    size_t bytes(bool with_s = true) const { return doubles(with_s) * sizeof(double); }
};

struct ResultBlock {
    double *p; size_t n, counts_at;
    ResultBlock(void *base, size_t n_items) : p((double *)base), n(n_items), counts_at(n_items * 12) {}
    ResultBlock(void *base, size_t n_items, size_t counts_at_) : p((double *)base), n(n_items), counts_at(counts_at_) {}
    double *wrench() const { return p; }         double *sdot() const { return p + n * 6; }
    int *counts() const { return reinterpret_cast<int *>(p + counts_at); }
    int *fused_words() const { return counts() + n * 4; }      // status and counts of the fused small-scene kernel
    size_t doubles() const { return n * 12; }
    size_t bytes(bool with_fused_words = false) const { return doubles() * sizeof(double) + n * (with_fused_words ? 12 : 4) * sizeof(int); }
};

struct PartialBlock {
    double *p; size_t nk;
    PartialBlock(void *base, size_t n_keys) : p((double *)base), nk(n_keys) {}
    double *d_wrench() const { return p; }       double *d_sdot() const { return p + nk * 6; }
    size_t doubles() const { return nk * 12; }
    size_t bytes() const { return doubles() * sizeof(double); }
};

// The blocks of the one-sync route: one copy up, one copy down.
struct OneSyncIn {
    double *p; size_t n, nk;
    OneSyncIn(void *base, size_t n_items, size_t n_keys) : p((double *)base), n(n_items), nk(n_keys) {}
    size_t doubles() const { return ValueBlock(p, n).doubles() + SeedBlock(p, nk).doubles(); }
    ValueBlock values() const { return ValueBlock(p, n, doubles()); }
    SeedBlock seeds() const { return SeedBlock(p + ValueBlock(p, n).doubles(), nk); }
    size_t bytes(bool with_ids) const { return doubles() * sizeof(double) + (with_ids ? n * sizeof(int) : 0); }
};
struct OneSyncOut {
    double *p; size_t n, nk;
    OneSyncOut(void *base, size_t n_items, size_t n_keys) : p((double *)base), n(n_items), nk(n_keys) {}
    size_t doubles() const { return ResultBlock(p, n).doubles() + PartialBlock(p, nk).doubles(); }
    ResultBlock results() const { return ResultBlock(p, n, doubles()); }
    PartialBlock partials() const { return PartialBlock(p + ResultBlock(p, n).doubles(), nk); }
    size_t bytes() const { return doubles() * sizeof(double) + n * 4 * sizeof(int); }
};

// Value inputs of b.n items into a host-written block (zeros for a null s; a null ins_ids leaves the ids alone).
inline void pack_values(ValueBlock b, const int *ins_ids, const double *pose, const double *twist, const double *s) {
    std::memcpy(b.pose(), pose, sizeof(double) * b.n * 24);
    std::memcpy(b.twist(), twist, sizeof(double) * b.n * 6);
    if (s) std::memcpy(b.s(), s, sizeof(double) * b.n * 6); else std::memset(b.s(), 0, sizeof(double) * b.n * 6);
    if (ins_ids) std::memcpy(b.ids(), ins_ids, sizeof(int) * b.n);
}
// Seeds of b.nk (item, direction) pairs: d_pose | d_twist, then -- with_s -- d_s (zeros for a null d_s).
inline void pack_seeds(SeedBlock b, const double *d_pose, const double *d_twist, const double *d_s, bool with_s) {
    std::memcpy(b.d_pose(), d_pose, sizeof(double) * b.nk * 24);
    std::memcpy(b.d_twist(), d_twist, sizeof(double) * b.nk * 6);
    if (!with_s) return;
    if (d_s) std::memcpy(b.d_s(), d_s, sizeof(double) * b.nk * 6); else std::memset(b.d_s(), 0, sizeof(double) * b.nk * 6);
}
// The same-point test of the host Dual routes: are these value inputs bit for bit those the block holds?  zero_s: a null s must
// find zeros stored (without it a null s is not compared: no bristle item reads s).
inline bool same_point(ValueBlock b, const int *ins_ids, const double *pose, const double *twist, const double *s, bool zero_s) {
    if (std::memcmp(b.pose(), pose, sizeof(double) * b.n * 24) != 0 || std::memcmp(b.twist(), twist, sizeof(double) * b.n * 6) != 0) return false;
    if (s) {
        if (std::memcmp(b.s(), s, sizeof(double) * b.n * 6) != 0) return false;
    } else if (zero_s) {
        for (size_t k = 0; k < b.n * 6; ++k)
            if (std::memcmp(b.s() + k, "\0\0\0\0\0\0\0\0", 8) != 0) return false;
    }
    return !ins_ids || std::memcmp(b.ids(), ins_ids, sizeof(int) * b.n) == 0;
}
// Results out of a block the device has filled (counts may be null) ...
inline void copy_out(ResultBlock b, double *wrench, double *sdot, int *counts) {
    std::memcpy(wrench, b.wrench(), sizeof(double) * b.n * 6);
    std::memcpy(sdot, b.sdot(), sizeof(double) * b.n * 6);
    if (counts) std::memcpy(counts, b.counts(), sizeof(int) * b.n * 4);
}
// ... and the partials of b.nk (item, direction) pairs.
inline void copy_out_dual(PartialBlock b, double *d_wrench, double *d_sdot) {
    std::memcpy(d_wrench, b.d_wrench(), sizeof(double) * b.nk * 6);
    std::memcpy(d_sdot, b.d_sdot(), sizeof(double) * b.nk * 6);
}

}  // namespace pfc_blocks
