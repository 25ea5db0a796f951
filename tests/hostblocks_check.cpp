// Stand-alone check of csrc/pfc_hostblocks.h (built and run by tests/test_hostblocks.py under AddressSanitizer and UBSan).
// The offsets below are written out literally on purpose: this file is the second, independent statement of the layouts.
#include "pfc_hostblocks.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

using namespace pfc_blocks;

static int checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        ++checks;                                                                \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

static_assert(std::is_trivially_copyable<ValueBlock>::value && std::is_trivially_copyable<SeedBlock>::value &&
              std::is_trivially_copyable<ResultBlock>::value && std::is_trivially_copyable<PartialBlock>::value &&
              std::is_trivially_copyable<OneSyncIn>::value && std::is_trivially_copyable<OneSyncOut>::value, "views are plain values");

static void flip_bit(void *p) { *(unsigned char *)p ^= 1; }

// n items, n_dir directions: every accessor, pack / compare / unpack, for ids and s given or null.
static void run(size_t n, size_t n_dir, bool with_ids, bool with_s, bool with_ds) {
    const size_t nk = n * n_dir;
    std::vector<double> pose(n * 24), twist(n * 6), s(n * 6), d_pose(nk * 24), d_twist(nk * 6), d_s(nk * 6);
    std::vector<int> ids(n);
    double x = 1.0;
    for (auto *v : {&pose, &twist, &s, &d_pose, &d_twist, &d_s})
        for (double &e : *v) e = (x += 0.25);
    for (size_t k = 0; k < n; ++k) ids[k] = 7 + (int)k;
    const int *pid = with_ids ? ids.data() : nullptr;
    const double *ps = with_s ? s.data() : nullptr;

    // ---- value block: exactly bytes(true) are allocated, so a wrong offset or size is an ASan report
    std::vector<char> vbuf(n * 36 * 8 + n * 4, (char)0x5A);
    const ValueBlock v(vbuf.data(), n);
    char *vb = vbuf.data();
    CHECK((char *)v.pose() == vb && (char *)v.twist() == vb + n * 24 * 8 && (char *)v.s() == vb + n * 30 * 8);
    CHECK((char *)v.ids() == vb + n * 36 * 8);
    CHECK(v.doubles() == n * 36 && v.bytes(false) == n * 288 && v.bytes(true) == n * 288 + n * 4 && v.ids_at == n * 36);
    pack_values(v, pid, pose.data(), twist.data(), ps);
    CHECK(std::memcmp(vb, pose.data(), n * 192) == 0 && std::memcmp(vb + n * 192, twist.data(), n * 48) == 0);
    for (size_t k = 0; k < n * 6; ++k) CHECK(v.s()[k] == (with_s ? s[k] : 0.0));
    for (size_t k = 0; k < n; ++k) CHECK(((unsigned char *)v.ids())[4 * k] == (with_ids ? (unsigned char)ids[k] : 0x5A));
    CHECK(same_point(v, pid, pose.data(), twist.data(), ps, true) && same_point(v, pid, pose.data(), twist.data(), ps, false));
    // a one-bit change in each part is noticed (first and last element of the part)
    for (size_t at : {(size_t)0, n * 24 - 1}) { flip_bit(&pose[at]); CHECK(!same_point(v, pid, pose.data(), twist.data(), ps, true)); flip_bit(&pose[at]); }
    for (size_t at : {(size_t)0, n * 6 - 1}) { flip_bit(&twist[at]); CHECK(!same_point(v, pid, pose.data(), twist.data(), ps, true)); flip_bit(&twist[at]); }
    if (with_s)
        for (size_t at : {(size_t)0, n * 6 - 1}) { flip_bit(&s[at]); CHECK(!same_point(v, pid, pose.data(), twist.data(), ps, true)); flip_bit(&s[at]); }
    if (with_ids)
        for (size_t at : {(size_t)0, n - 1}) { flip_bit(&ids[at]); CHECK(!same_point(v, pid, pose.data(), twist.data(), ps, true)); flip_bit(&ids[at]); }
    // a null s against the stored s: compared (with zeros) only under zero_s
    {
        const bool stored_zero = !with_s;
        CHECK(same_point(v, pid, pose.data(), twist.data(), nullptr, true) == stored_zero);
        CHECK(same_point(v, pid, pose.data(), twist.data(), nullptr, false));
        flip_bit(v.s() + n * 6 - 1);      // one bit of the last stored s (for stored zeros: a denormal, still not "zeros")
        CHECK(!same_point(v, pid, pose.data(), twist.data(), nullptr, true) && same_point(v, pid, pose.data(), twist.data(), nullptr, false));
        flip_bit(v.s() + n * 6 - 1);
    }
    // null ids are not compared
    CHECK(same_point(v, nullptr, pose.data(), twist.data(), ps, true));

    // ---- seed block, with and without its d_s part
    std::vector<char> sbuf(with_ds ? nk * 36 * 8 : nk * 30 * 8, (char)0x5A);
    const SeedBlock sd(sbuf.data(), nk);
    CHECK((char *)sd.d_pose() == sbuf.data() && (char *)sd.d_twist() == sbuf.data() + nk * 24 * 8 && (char *)sd.d_s() == sbuf.data() + nk * 30 * 8);
    CHECK(sd.doubles(true) == nk * 36 && sd.doubles(false) == nk * 30 && sd.bytes(true) == nk * 288 && sd.bytes(false) == nk * 240 && sd.doubles() == nk * 36);
    pack_seeds(sd, d_pose.data(), d_twist.data(), with_s ? d_s.data() : nullptr, with_ds);
    CHECK(std::memcmp(sd.d_pose(), d_pose.data(), nk * 192) == 0 && std::memcmp(sd.d_twist(), d_twist.data(), nk * 48) == 0);
    if (with_ds) for (size_t k = 0; k < nk * 6; ++k) CHECK(sd.d_s()[k] == (with_s ? d_s[k] : 0.0));

    // ---- result block with the fused kernel's words, partial block
    std::vector<char> rbuf(n * 12 * 8 + n * 4 * 4 + n * 8 * 4);
    const ResultBlock r(rbuf.data(), n);
    CHECK((char *)r.wrench() == rbuf.data() && (char *)r.sdot() == rbuf.data() + n * 6 * 8 && (char *)r.counts() == rbuf.data() + n * 12 * 8);
    CHECK((char *)r.fused_words() == rbuf.data() + n * 12 * 8 + n * 4 * 4);
    CHECK(r.doubles() == n * 12 && r.bytes() == n * 96 + n * 16 && r.bytes(true) == n * 96 + n * 16 + n * 32 && r.counts_at == n * 12);
    for (size_t k = 0; k < n * 12; ++k) r.wrench()[k] = 100.0 + (double)k;
    for (size_t k = 0; k < n * 4; ++k) r.counts()[k] = 1000 + (int)k;
    std::vector<double> wr(n * 6), sdt(n * 6);
    std::vector<int> cnt(n * 4, -1);
    copy_out(r, wr.data(), sdt.data(), nullptr);
    copy_out(r, wr.data(), sdt.data(), cnt.data());
    for (size_t k = 0; k < n * 6; ++k) CHECK(wr[k] == 100.0 + (double)k && sdt[k] == 100.0 + (double)(n * 6 + k));
    for (size_t k = 0; k < n * 4; ++k) CHECK(cnt[k] == 1000 + (int)k);
    std::vector<char> pbuf(nk * 12 * 8);
    const PartialBlock pt(pbuf.data(), nk);
    CHECK((char *)pt.d_wrench() == pbuf.data() && (char *)pt.d_sdot() == pbuf.data() + nk * 6 * 8 && pt.doubles() == nk * 12 && pt.bytes() == nk * 96);
    for (size_t k = 0; k < nk * 12; ++k) pt.d_wrench()[k] = 200.0 + (double)k;
    std::vector<double> dw(nk * 6), dsd(nk * 6);
    copy_out_dual(pt, dw.data(), dsd.data());
    for (size_t k = 0; k < nk * 6; ++k) CHECK(dw[k] == 200.0 + (double)k && dsd[k] == 200.0 + (double)(nk * 6 + k));

    // ---- the one-sync blocks: values | seeds | ids and results | partials | counts, where pfc_eval_dual_device is handed them
    std::vector<char> ibuf((n * 36 + nk * 36) * 8 + n * 4, (char)0x5A), obuf((n * 12 + nk * 12) * 8 + n * 16);
    const OneSyncIn in(ibuf.data(), n, nk);
    CHECK(in.doubles() == n * 36 + nk * 36 && in.bytes(true) == ibuf.size() && in.bytes(false) == ibuf.size() - n * 4);
    CHECK((char *)in.values().pose() == ibuf.data() && (char *)in.values().twist() == ibuf.data() + n * 24 * 8 && (char *)in.values().s() == ibuf.data() + n * 30 * 8);
    CHECK((char *)in.seeds().d_pose() == ibuf.data() + n * 36 * 8 && (char *)in.seeds().d_twist() == ibuf.data() + (n * 36 + nk * 24) * 8 &&
          (char *)in.seeds().d_s() == ibuf.data() + (n * 36 + nk * 30) * 8);
    CHECK((char *)in.values().ids() == ibuf.data() + (n * 36 + nk * 36) * 8 && in.values().ids_at == n * 36 + nk * 36);
    pack_values(in.values(), pid, pose.data(), twist.data(), ps);
    pack_seeds(in.seeds(), d_pose.data(), d_twist.data(), d_s.data(), true);
    CHECK(same_point(in.values(), pid, pose.data(), twist.data(), ps, true));      // the seeds did not run into the values or the ids
    CHECK(same_point(ValueBlock(ibuf.data(), n, in.values().ids_at), pid, pose.data(), twist.data(), ps, true));
    CHECK(std::memcmp(in.seeds().d_s(), d_s.data(), nk * 48) == 0);
    const OneSyncOut out(obuf.data(), n, nk);
    CHECK(out.doubles() == n * 12 + nk * 12 && out.bytes() == obuf.size());
    CHECK((char *)out.results().wrench() == obuf.data() && (char *)out.results().sdot() == obuf.data() + n * 6 * 8);
    CHECK((char *)out.partials().d_wrench() == obuf.data() + n * 12 * 8 && (char *)out.partials().d_sdot() == obuf.data() + (n * 12 + nk * 6) * 8);
    CHECK((char *)out.results().counts() == obuf.data() + (n * 12 + nk * 12) * 8);
    for (size_t k = 0; k < n * 4; ++k) out.results().counts()[k] = 3000 + (int)k;
    copy_out(out.results(), wr.data(), sdt.data(), cnt.data());
    for (size_t k = 0; k < n * 4; ++k) CHECK(cnt[k] == 3000 + (int)k);
    // the staging buffers hold the blocks with their ints: sizes in doubles
    CHECK(doubles_for(in.bytes(true)) == n * 36 + nk * 36 + (n + 1) / 2 + 1 && doubles_for(out.bytes()) == n * 12 + nk * 12 + 2 * n + 1);
    CHECK(doubles_for(v.bytes(true)) == n * 36 + (n + 1) / 2 + 1 && doubles_for(v.bytes(true)) * 8 >= v.bytes(true));
}

int main() {
    for (size_t n : {(size_t)1, (size_t)3})
        for (size_t n_dir : {(size_t)1, (size_t)16})
            for (int ids = 0; ids < 2; ++ids)
                for (int s = 0; s < 2; ++s)
                    for (int ds = 0; ds < 2; ++ds) run(n, n_dir, ids != 0, s != 0, ds != 0);
    std::printf("hostblocks ok: %d checks\n", checks);
    return 0;
}
