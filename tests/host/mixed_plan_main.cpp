// Stand-alone checks of the mixed-length planner (rustfs_amd/csrc/rs_mixed_plan.h):
// validation, kernel ordering and sub-batch splitting on a CPU.  Built with the
// host compiler and -fsanitize=address,undefined by tests/test_mixed_plan.py
// and run as a child process; exits 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rustfs_amd/csrc/rs_mixed_plan.h"

using namespace rsg::mixed;

static int failures = 0;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// stripes of the given lengths packed into separate arenas with `gap` bytes between them
static std::vector<StripeDesc> packed(int k, int m, const std::vector<uint64_t>& lens, uint64_t gap, uint64_t d0 = 0,
                                      uint64_t p0 = 0) {
    std::vector<StripeDesc> d;
    uint64_t doff = d0, poff = p0;
    for (uint64_t len : lens) {
        d.push_back({doff, poff, len});
        doff += (uint64_t)k * len + gap;
        poff += (uint64_t)m * len + gap;
    }
    return d;
}

// the a3 layout in one arena: [k data shards][m parity shards] per stripe
static std::vector<StripeDesc> a3(int k, int m, const std::vector<uint64_t>& lens) {
    std::vector<StripeDesc> d;
    uint64_t off = 0;
    for (uint64_t len : lens) {
        d.push_back({off, off + (uint64_t)k * len, len});
        off += (uint64_t)(k + m) * len;
    }
    return d;
}

static bool ok(int k, int m, const std::vector<StripeDesc>& d, uint64_t db, uint64_t pb) {
    return validate(k, m, d.size(), d.data(), db, pb);
}

static void check_order(const std::vector<StripeDesc>& d, size_t first, size_t count, uint64_t dlo, uint64_t plo) {
    std::vector<MixedDesc> t;
    order_for_kernel(d.data(), first, count, dlo, plo, t);
    CHECK(t.size() == count);
    std::vector<int> seen(count, 0);
    for (size_t i = 0; i < t.size(); ++i) {
        CHECK(t[i].job < count);
        if (t[i].job >= count) continue;
        ++seen[t[i].job];
        const StripeDesc& s = d[first + t[i].job];
        CHECK(t[i].len == s.shard_len);
        if (s.shard_len) {
            CHECK(t[i].data_off == s.data_off - dlo);
            CHECK(t[i].parity_off == s.parity_off - plo);
        }
        if (i) CHECK(chunks_of(t[i - 1].len) >= chunks_of(t[i].len));
    }
    for (int c : seen) CHECK(c == 1);
}

static void check_split(int k, int m, const std::vector<StripeDesc>& d, bool dig, uint64_t stage, size_t want_subs) {
    std::vector<SubBatch> subs;
    split(k, m, d.size(), d.data(), dig, stage, d.size() ? d.size() : 1, subs);
    if (want_subs) CHECK(subs.size() == want_subs);
    size_t next = 0;
    for (const SubBatch& b : subs) {
        CHECK(b.first == next);
        CHECK(b.count >= 1);
        next = b.first + b.count;
        // spans cover every non-empty stripe of the run
        for (size_t i = b.first; i < b.first + b.count && i < d.size(); ++i) {
            if (!d[i].shard_len) continue;
            CHECK(b.data_lo <= d[i].data_off && d[i].data_off + (uint64_t)k * d[i].shard_len <= b.data_hi);
            if (m) CHECK(b.parity_lo <= d[i].parity_off && d[i].parity_off + (uint64_t)m * d[i].shard_len <= b.parity_hi);
        }
        // within the staging size unless it is a single stripe
        if (b.count > 1) CHECK(stage_bytes(b, k, m, dig) <= stage);
        check_order(d, b.first, b.count, b.data_lo, b.parity_lo);
    }
    CHECK(next == d.size());
}

int main() {
    const uint64_t SEP = 1ull << 40;  // a parity arena far from the data arena
    static_assert(chunks_of(0) == 0 && chunks_of(1) == 1 && chunks_of(512) == 1 && chunks_of(513) == 2 &&
                      chunks_of(0xffffffffull) == 8388608u,
                  "chunk count");
    static_assert(spw_for(6) == 4 && spw_for(12) == 4 && spw_for(16) == 1 && spw_for(8) == 2 && spw_for(20) == 4 &&
                      spw_for(19) == 2,
                  "stripes per workgroup");

    // ---- valid tables ----
    const std::vector<uint64_t> lens = {0, 1, 7, 8, 31, 32, 33, 511, 512, 513, 1023, 1024, 1025, 87382, 0};
    for (int spw : {1, 2, 4}) {
        for (size_t n : {(size_t)0, (size_t)1, (size_t)spw, (size_t)spw + 1}) {
            std::vector<uint64_t> l(lens.begin(), lens.begin() + (long)n);
            auto d = packed(8, 4, l, 3);
            CHECK(ok(8, 4, d, 0, SEP));
            check_order(d, 0, d.size(), 0, 0);
        }
    }
    {
        auto d = packed(12, 4, lens, 1, 5, 9);
        CHECK(ok(12, 4, d, 0, SEP));
        CHECK(ok(12, 0, d, 0, 0));  // m = 0: parity ranges are empty
        check_order(d, 0, d.size(), 0, 0);
        auto al = a3(12, 4, lens);
        CHECK(ok(12, 4, al, 0, 0));        // aliased, a3
        CHECK(ok(12, 4, al, 4096, 4096));  // the same arena at another address
        check_order(al, 0, al.size(), 0, 0);
        // all stripes empty: offsets are not looked at
        std::vector<StripeDesc> z = {{9, 9, 0}, {9, 9, 0}, {0, 0, 0}};
        CHECK(ok(4, 2, z, 0, 0));
        check_order(z, 0, z.size(), 0, 0);
        // a zero-length stripe between two others occupies no range
        std::vector<StripeDesc> mid = {{0, 0, 10}, {5, 5, 0}, {40, 20, 10}};
        CHECK(ok(4, 2, mid, 0, SEP));
        // touching ranges are disjoint
        std::vector<StripeDesc> touch = {{0, 0, 10}, {40, 20, 10}};
        CHECK(ok(4, 2, touch, 0, SEP));
        // the largest shard length
        std::vector<StripeDesc> big = {{0, 0, 0xffffffffull}};
        CHECK(ok(16, 4, big, 0, 1ull << 50));
    }

    // ---- rejections ----
    {
        std::vector<StripeDesc> d;
        d = {{0, 0, 10}, {0, 20, 10}};  // data_off not strictly ascending
        CHECK(!ok(4, 2, d, 0, SEP));
        d = {{40, 0, 10}, {0, 20, 10}};  // descending
        CHECK(!ok(4, 2, d, 0, SEP));
        d = {{0, 0, 10}, {39, 20, 10}};  // data ranges overlap by one byte
        CHECK(!ok(4, 2, d, 0, SEP));
        d = {{0, 20, 10}, {40, 20, 10}};  // parity_off not strictly ascending
        CHECK(!ok(4, 2, d, 0, SEP));
        d = {{0, 0, 10}, {40, 19, 10}};  // parity ranges overlap by one byte
        CHECK(!ok(4, 2, d, 0, SEP));
        d = {{0, 0, 0x100000000ull}};  // shard_len above 0xffffffff
        CHECK(!ok(4, 2, d, 0, SEP));
        d = {{UINT64_MAX - 10, 0, 10}};  // range wraps the address space
        CHECK(!ok(4, 2, d, 0, SEP));
        d = {{0, 0, 10}};
        CHECK(!ok(4, 2, d, UINT64_MAX - 20, 0));
        // aliased arenas: parity on its own stripe's data, on the next stripe's data, one byte
        d = {{0, 39, 10}};
        CHECK(!ok(4, 2, d, 0, 0));
        d = {{0, 40, 10}, {59, 100, 10}};
        CHECK(!ok(4, 2, d, 0, 0));
        d = {{100, 0, 10}, {200, 81, 10}};  // parity of stripe 1 ends inside data of stripe 0
        CHECK(!ok(4, 2, d, 0, 0));
        // ... and the same through different base addresses
        d = {{0, 0, 10}};
        CHECK(!ok(4, 2, d, 1000, 1039));
        CHECK(ok(4, 2, d, 1000, 1040));
        CHECK(ok(4, 2, d, 1000, 980));
        CHECK(!ok(4, 2, d, 1000, 981));
        CHECK(!validate(0, 2, 0, nullptr, 0, 0));
        CHECK(!validate(4, -1, 0, nullptr, 0, 0));
        CHECK(!validate(4, 2, 1, nullptr, 0, 0));
    }

    // ---- sub-batches ----
    {
        // 10 stripes of 4 KiB shards, RS(4,2): data 16 KiB, parity 8 KiB, digests 192 B per stripe
        auto d = packed(4, 2, std::vector<uint64_t>(10, 4096), 0);
        check_split(4, 2, d, true, 1ull << 30, 1);
        check_split(4, 2, d, true, 3 * (16384 + 8192) + 768, 4);  // digests of 3: 576 -> 768; 3 + 3 + 3 + 1
        check_split(4, 2, d, true, 3 * (16384 + 8192) + 767, 5);  // one byte short: 2 + 2 + 2 + 2 + 2
        check_split(4, 2, d, true, 1, 10);                        // every stripe oversized: one each
        check_split(4, 2, d, false, 2 * (16384 + 8192), 5);
        // an oversized stripe among small ones gets a sub-batch of its own
        auto o = packed(4, 2, {100, 100, 1 << 20, 100, 0, 100}, 3);
        std::vector<SubBatch> subs;
        split(4, 2, o.size(), o.data(), true, 64 << 10, o.size(), subs);
        CHECK(subs.size() == 3);
        if (subs.size() == 3) {
            CHECK(subs[0].first == 0 && subs[0].count == 2);
            CHECK(subs[1].first == 2 && subs[1].count == 1);
            CHECK(stage_bytes(subs[1], 4, 2, true) > (64u << 10));
            CHECK(subs[2].first == 3 && subs[2].count == 3);
        }
        check_split(4, 2, o, true, 64 << 10, 3);
        // gaps count: the span is first start to last end
        auto g = packed(4, 2, {100, 100}, 100000);
        check_split(4, 2, g, true, 64 << 10, 2);
        // empty list, all-empty stripes, m = 0, aliased a3
        check_split(4, 2, {}, true, 1 << 20, 0);
        std::vector<SubBatch> none;
        split(4, 2, 0, nullptr, true, 1 << 20, 1, none);
        CHECK(none.empty());
        check_split(4, 2, {{7, 7, 0}, {7, 7, 0}}, true, 1 << 20, 1);
        check_split(4, 0, packed(4, 0, lens, 2), true, 64 << 10, 0);
        check_split(12, 4, a3(12, 4, lens), true, 256 << 10, 0);
        // a count limit splits too
        split(4, 2, d.size(), d.data(), true, 1ull << 30, 4, subs);
        CHECK(subs.size() == 3 && subs[2].count == 2);
    }

    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("mixed plan ok\n");
    return 0;
}
