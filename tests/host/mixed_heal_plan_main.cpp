// Stand-alone check of the mixed-length heal's host planner
// (rustfs_amd/csrc/rs_mixed_heal_plan.h), built by the host compiler with
// AddressSanitizer + UBSan and run directly (tests/test_mixed_heal_plan.py).
#include <set>
#include <vector>

#include "../../rustfs_amd/csrc/rs_mixed_heal_plan.h"
#include "record_rounds_check.h"  // CHECK, run_rounds

using namespace rsg::mixed;

namespace {

// A valid list: source records at odd offsets with 1..3 byte gaps, target
// records at other odd offsets with the same gaps, or packed densely.
std::vector<RecordDesc> make(const std::vector<uint32_t>& lens, const std::vector<uint32_t>& present,
                             bool dense = false) {
    std::vector<RecordDesc> d(lens.size());
    uint64_t r = 1, o = 3;
    for (size_t i = 0; i < lens.size(); ++i) {
        d[i] = RecordDesc{r, o, lens[i], present[i % present.size()]};
        r += kRecHeader + lens[i] + 1 + i % 3;
        o += kRecHeader + lens[i] + (dense ? 0 : 1 + i % 3);
    }
    return d;
}

void test_validation() {
    const int k = 4, m = 2, t = k + m;
    const uint64_t A = 0x100000000ull;  // arenas far apart
    uint64_t files[6], tg[6] = {};
    for (int i = 0; i < t; ++i) files[i] = A * (uint64_t)(i + 1);
    tg[1] = 0x900000000ull;
    tg[5] = 0xa00000000ull;
    const std::vector<uint32_t> lens = {0, 1, 7, 8, 513, 0, 87382};
    std::vector<RecordDesc> d = make(lens, {0x3f});
    CHECK(validate_heal(k, m, d.size(), d.data(), files, tg));
    CHECK(validate_heal(k, m, 0, nullptr, files, tg));
    {
        auto e = make(lens, {0x3f}, true);  // densely packed target records
        CHECK(validate_heal(k, m, e.size(), e.data(), files, tg));
    }
    // no target at all
    {
        uint64_t none[6] = {};
        CHECK(!validate_heal(k, m, d.size(), d.data(), files, none));
    }
    // a present bit at or above k+m
    {
        auto e = d;
        e[2].present = 1u << t;
        CHECK(!validate_heal(k, m, e.size(), e.data(), files, tg));
        e[2].present = 0x80000000u;
        CHECK(!validate_heal(k, m, e.size(), e.data(), files, tg));
    }
    // record ranges not ascending / overlapping
    {
        auto e = d;
        e[1].rec_off = e[0].rec_off + kRecHeader - 1;
        CHECK(!validate_heal(k, m, e.size(), e.data(), files, tg));
        e = d;
        std::swap(e[3].rec_off, e[4].rec_off);
        CHECK(!validate_heal(k, m, e.size(), e.data(), files, tg));
    }
    // target ranges not ascending / overlapping: a zero-length stripe's range is its 32 header bytes
    {
        auto e = d;
        e[1].out_off = e[0].out_off + kRecHeader - 1;  // into the bare digest of stripe 0
        CHECK(!validate_heal(k, m, e.size(), e.data(), files, tg));
        e = d;
        e[6].out_off = e[5].out_off + 31;  // stripe 5 is empty too
        CHECK(!validate_heal(k, m, e.size(), e.data(), files, tg));
        e = d;
        e[5].out_off = e[4].out_off + kRecHeader + 513 - 1;  // an empty stripe's header inside a body
        CHECK(!validate_heal(k, m, e.size(), e.data(), files, tg));
        e = d;
        std::swap(e[2].out_off, e[4].out_off);
        CHECK(!validate_heal(k, m, e.size(), e.data(), files, tg));
        e = d;
        e[3].out_off = e[2].out_off;  // equal starts
        CHECK(!validate_heal(k, m, e.size(), e.data(), files, tg));
    }
    // ranges that wrap the address space
    {
        auto e = d;
        e[6].rec_off = UINT64_MAX - 40;
        CHECK(!validate_heal(k, m, e.size(), e.data(), files, tg));
        e = d;
        e[6].rec_off = UINT64_MAX - files[t - 2] - 100;  // wraps only relative to the highest arena read
        CHECK(!validate_heal(k, m, e.size(), e.data(), files, tg));
        e = d;
        e[6].out_off = UINT64_MAX - 40;
        CHECK(!validate_heal(k, m, e.size(), e.data(), files, tg));
        e = d;
        e[6].out_off = UINT64_MAX - tg[5] - 100;  // wraps only relative to the highest target
        CHECK(!validate_heal(k, m, e.size(), e.data(), files, tg));
    }
    // a target span meets the record span of an arena: only one that is read
    {
        uint64_t f2[6];
        for (int i = 0; i < t; ++i) f2[i] = files[i];
        f2[4] = tg[1] + 100;
        CHECK(!validate_heal(k, m, d.size(), d.data(), f2, tg));
        auto e = make(lens, {0x2f});  // shard 4 never read
        CHECK(validate_heal(k, m, e.size(), e.data(), f2, tg));
        f2[4] = 0;  // a NULL arena, whatever `present` says
        CHECK(validate_heal(k, m, d.size(), d.data(), f2, tg));
        // a target's own source arena is never read: it may be the target arena itself
        f2[4] = files[4];
        f2[1] = tg[1];
        CHECK(validate_heal(k, m, d.size(), d.data(), f2, tg));
        // zero-length stripes still have target ranges to protect
        auto z = make({0, 0, 0}, {0x3f});
        f2[4] = tg[5] + 40;
        CHECK(!validate_heal(k, m, z.size(), z.data(), f2, tg));
    }
    // two targets' spans meet
    {
        uint64_t t2[6] = {};
        t2[1] = tg[1];
        t2[5] = tg[1] + 1000;
        CHECK(!validate_heal(k, m, d.size(), d.data(), files, t2));
        t2[5] = tg[1] + d.back().out_off + kRecHeader + d.back().shard_len - d[0].out_off;  // end to start
        CHECK(validate_heal(k, m, d.size(), d.data(), files, t2));
    }
    CHECK(!validate_heal(0, 2, d.size(), d.data(), files, tg));
    CHECK(!validate_heal(30, 3, 0, nullptr, files, tg));  // k + m > 32
    CHECK(!validate_heal(k, m, d.size(), nullptr, files, tg));
    CHECK(!validate_heal(k, m, d.size(), d.data(), nullptr, tg));
    CHECK(!validate_heal(k, m, d.size(), d.data(), files, nullptr));
}

void test_plans() {
    MaskPlan p;
    // RS(4,2), data shard 1 the target, all others readable: sources 0 2 3 4, surplus 5
    CHECK(plan_heal_mask(4, 2, 0x3f, 1u << 1, p));  // the target's own bit is ignored
    CHECK(p.src == std::vector<int>({0, 2, 3, 4}) && p.written == std::vector<int>({1}) &&
          p.surplus == std::vector<int>({5}));
    CHECK(p.read_mask() == 0x3du && p.rows() == 2);
    // a parity target: sources are the data, the other parity is surplus
    CHECK(plan_heal_mask(4, 2, 0x3f, 1u << 5, p));
    CHECK(p.src == std::vector<int>({0, 1, 2, 3}) && p.written == std::vector<int>({5}) &&
          p.surplus == std::vector<int>({4}));
    // a data and a parity target: exactly k readable
    CHECK(plan_heal_mask(4, 2, 0x3f, (1u << 0) | (1u << 4), p));
    CHECK(p.src == std::vector<int>({1, 2, 3, 5}) && p.written == std::vector<int>({0, 4}) && p.surplus.empty());
    // one target and one shard absent besides
    CHECK(plan_heal_mask(4, 2, 0x3f & ~(1u << 3), 1u << 0, p));
    CHECK(p.src == std::vector<int>({1, 2, 4, 5}) && p.surplus.empty() && p.rows() == 1);
    // fewer than k readable non-target shards
    CHECK(!plan_heal_mask(4, 2, 0x3f & ~(1u << 3), (1u << 0) | (1u << 1), p));
    CHECK(!plan_heal_mask(4, 2, 0x3f, 0x7, p));  // more targets than m
    CHECK(!plan_heal_mask(4, 2, 0, 1u, p));
    // R = e + surplus <= m, k sources, surplus shards are parity, for every
    // mask of RS(4,2) and RS(8,4) and every target set of 1..m shards
    const int geos[2][2] = {{4, 2}, {8, 4}};
    for (const auto& g : geos) {
        const int k = g[0], m = g[1], t = k + m;
        size_t plans = 0;
        for (uint32_t targets = 1; targets < (1u << t); ++targets) {
            const int e = popcount32(targets);
            if (e > m) continue;
            for (uint32_t mask = 0; mask < (1u << t); ++mask) {
                const bool ok = plan_heal_mask(k, m, mask, targets, p);
                CHECK(ok == (popcount32(mask & ~targets) >= k));
                if (!ok) continue;
                ++plans;
                CHECK((int)p.src.size() == k && (int)p.written.size() == e);
                CHECK(p.rows() >= 1 && p.rows() <= m && heal_kernel_shape(k, p.rows()));
                CHECK((p.read_mask() & targets) == 0 && p.read_mask() == (mask & ~targets));
                for (size_t i = 1; i < p.src.size(); ++i) CHECK(p.src[i - 1] < p.src[i]);
                for (int s : p.surplus) CHECK(s >= k && s > p.src.back());
            }
        }
        CHECK(plans > 0);
    }
    CHECK(heal_kernel_geometry(16, 4) && heal_kernel_geometry(1, 1) && !heal_kernel_geometry(5, 0) &&
          !heal_kernel_geometry(10, 6) && !heal_kernel_geometry(17, 3));
    CHECK(!heal_kernel_shape(8, 0) && !heal_kernel_shape(8, 5));
}

// groups of 1, SPW and SPW+1 stripes out of three interleaved masks
void test_grouping_and_order() {
    const int k = 8, m = 4, spw = decode_spw_for(k + 4);
    const uint32_t targets = 1u << 2;
    const uint32_t A = 0xffb, B = 0xff9, C = 0x3b;  // C: fewer than k readable
    std::vector<uint32_t> masks;
    for (int i = 0; i < spw + 1; ++i) {
        masks.push_back(B);
        if (i < spw) masks.push_back(C);
        if (i == 1) masks.push_back(A);
    }
    const size_t n = masks.size();
    std::vector<uint32_t> lens(n);
    for (size_t i = 0; i < n; ++i) lens[i] = (uint32_t)((i * 700) % 2000);  // caller order != kernel order
    lens[3] = 0;
    std::vector<RecordDesc> d = make(lens, {0xfff});
    std::vector<uint32_t> todo(n);
    for (size_t i = 0; i < n; ++i) todo[i] = (uint32_t)i;
    std::vector<MaskGroup> g;
    group_by_mask(masks.data(), todo, g);
    CHECK(g.size() == 3 && g[0].mask == B && g[1].mask == C && g[2].mask == A);
    CHECK(g[0].stripes.size() == (size_t)spw + 1 && g[1].stripes.size() == (size_t)spw && g[2].stripes.size() == 1);
    std::set<uint32_t> seen;
    for (const MaskGroup& gr : g) {
        MaskPlan p;
        CHECK(plan_heal_mask(k, m, gr.mask, targets, p) == (gr.mask != C));  // fewer than k: no launch
        std::vector<DecDesc> tab;
        order_group_for_kernel(heal_out_rule(1), d.data(), gr.stripes, 0, d[0].rec_off, 3, tab);
        CHECK(tab.size() == gr.stripes.size());
        std::set<uint32_t> jobs;
        for (size_t i = 0; i < tab.size(); ++i) {
            CHECK(i == 0 || chunks_of(tab[i - 1].len) >= chunks_of(tab[i].len));
            CHECK(jobs.insert(tab[i].job).second);  // a permutation of the group
            CHECK(seen.insert(tab[i].job).second);
            const RecordDesc& s = d[tab[i].job];  // job maps back to the caller's index
            CHECK(masks[tab[i].job] == gr.mask && tab[i].len == s.shard_len);
            CHECK(tab[i].rec_off == s.rec_off - d[0].rec_off);
            CHECK(tab[i].out_off == s.out_off - 3);  // zero-length stripes keep their target offset
        }
        CHECK(jobs == std::set<uint32_t>(gr.stripes.begin(), gr.stripes.end()));
    }
    CHECK(seen.size() == n);
    // a sub-batch's jobs are relative to its first stripe
    std::vector<uint32_t> part = {0, 1, 2};
    std::vector<DecDesc> tab;
    order_group_for_kernel(heal_out_rule(1), d.data() + 5, part, 0, d[5].rec_off, d[5].out_off, tab);
    for (const DecDesc& x : tab)
        CHECK(x.job < 3 && x.len == d[5 + x.job].shard_len && x.out_off == d[5 + x.job].out_off - d[5].out_off);
}

void test_split() {
    const int files = 5, targets = 2;
    std::vector<uint32_t> lens;
    for (int i = 0; i < 40; ++i) lens.push_back(i % 7 == 0 ? 0u : 1000u * (uint32_t)(i % 5 + 1));
    lens[20] = 300000;  // larger than the stage: a sub-batch of its own
    std::vector<RecordDesc> d = make(lens, {0x3f});
    const uint64_t stage = 200000;
    const OutRule rule = heal_out_rule(targets);
    std::vector<RecSubBatch> subs;
    split_records(rule, files, d.size(), d.data(), stage, d.size(), subs);
    size_t next = 0;
    bool alone = false;
    for (const RecSubBatch& b : subs) {
        CHECK(b.first == next && b.count >= 1);  // every stripe once, in order
        next += b.count;
        CHECK(b.count == 1 || record_stage_bytes(rule, b, files) <= stage);
        if (b.first == 20) alone = b.count == 1;
        const RecordDesc& last = d[b.first + b.count - 1];
        CHECK(b.rec_lo == d[b.first].rec_off && b.rec_hi == last.rec_off + kRecHeader + last.shard_len);
        CHECK(b.out_lo == d[b.first].out_off && b.out_hi == last.out_off + kRecHeader + last.shard_len);
        // the record span once per arena, the target span once per target
        CHECK(record_stage_bytes(rule, b, files) ==
              files * stage_round(b.rec_hi - b.rec_lo) + targets * stage_round(b.out_hi - b.out_lo));
    }
    CHECK(next == d.size() && alone && subs.size() >= 3);
    split_records(rule, files, d.size(), d.data(), UINT64_MAX, d.size(), subs);
    CHECK(subs.size() == 1 && subs[0].count == d.size());
    split_records(rule, files, d.size(), d.data(), UINT64_MAX, 7, subs);  // max_count
    CHECK(subs.size() == 6 && subs.back().count == 5);
    split_records(rule, files, 0, d.data(), stage, 1, subs);
    CHECK(subs.empty());
    auto z = make({0, 0, 0}, {0x3f});  // only empty stripes: their headers are the target span
    split_records(rule, files, z.size(), z.data(), stage, z.size(), subs);
    CHECK(subs.size() == 1 && subs[0].out_hi - subs[0].out_lo >= 3 * kRecHeader);
}

// The rounds the library runs (plan_round -> launches -> shard_flags_from_rows
// -> redo_from_flags), driven by a table of records that are rotten; ends in
// at most k+m rounds with the verified sets.
void test_redo() {
    const int k = 4, m = 2, t = k + m;
    const uint32_t targets = 1u << 1;
    const size_t n = 8;
    // rotten[s]: bits of stripe s's records that fail their hash when read
    const uint32_t rotten[n] = {0, 0x04, 0x10, 0x20, 0x3d, 0x02, 0x14, 0};
    const uint32_t start[n] = {0x3d, 0x3d, 0x3d, 0x3d, 0x3d, 0x3d, 0x3d, 0x1d};
    uint32_t masks[n];
    for (size_t s = 0; s < n; ++s) masks[s] = start[s];
    const std::vector<RecordDesc> d = make({7, 0, 513, 64, 1025, 1, 0, 300}, {0x3f});
    const int rounds = rounds_check::run_rounds(k, m, heal_out_rule(1), d, rotten, masks, [&](uint32_t mask, MaskPlan& p) {
        return plan_heal_mask(k, m, mask, targets, p);
    });
    CHECK(rounds <= t);
    for (size_t s = 0; s < n; ++s) {
        MaskPlan p;
        if (plan_heal_mask(k, m, masks[s], targets, p)) CHECK((p.read_mask() & rotten[s]) == 0);
    }
    CHECK(masks[0] == 0x3d && masks[7] == 0x1d);
    CHECK(masks[1] == 0x39);  // a rotten source: parity 5 steps in
    CHECK(masks[2] == 0x2d);  // a rotten source parity
    CHECK(masks[3] == 0x1d);  // a rotten surplus parity
    CHECK(popcount32(masks[4]) < k);
    CHECK(masks[5] == 0x3d);  // rot in the target's own record is never seen: it is not read
    CHECK(popcount32(masks[6]) < k);  // data 2 and parity 4: three left
}

// A round that mixes groups with a plan and a group with fewer than k readable
// shards, which has no launch: the flags of each launch go to its own group's
// stripes.  RS(4,2) with data shard 1 the target, three masks interleaved in
// groups of SPW+1, SPW and 1 stripes, the one without a plan first met between
// the other two.
void test_rounds_beside_a_group_without_launch() {
    const int k = 4, m = 2, t = k + m, spw = decode_spw_for(t);
    const uint32_t targets = 1u << 1;
    const uint32_t A = 0x3d, B = 0x2d, C = 0x0d;  // C: three bits set
    std::vector<uint32_t> masks, rotten, lens;
    for (int i = 0; i < spw + 1; ++i) {
        masks.push_back(B);
        rotten.push_back(i == spw ? 0x20u : 0u);  // a source parity: three left
        if (i < spw) {
            masks.push_back(C);
            rotten.push_back(0x3f);  // never read
        }
        if (i == 1) {
            masks.push_back(A);
            rotten.push_back(0x10);  // joins B's mask in the second round
        }
    }
    const size_t n = masks.size();
    for (size_t i = 0; i < n; ++i) lens.push_back((uint32_t)((i * 700) % 2000));
    const std::vector<RecordDesc> d = make(lens, {0x3f});
    const std::vector<uint32_t> start = masks;
    const int rounds = rounds_check::run_rounds(
        k, m, heal_out_rule(1), d, rotten.data(), masks.data(),
        [&](uint32_t mask, MaskPlan& p) { return plan_heal_mask(k, m, mask, targets, p); });
    CHECK(rounds >= 2 && rounds <= t);
    size_t moved = 0;
    for (size_t s = 0; s < n; ++s) {
        // no launch: untouched, whatever the launches beside it wrote
        CHECK(masks[s] == (start[s] == C ? C : start[s] & ~rotten[s]));
        moved += masks[s] != start[s];
    }
    CHECK(moved == 2);
}

}  // namespace

int main() {
    test_validation();
    test_plans();
    test_grouping_and_order();
    test_split();
    test_redo();
    test_rounds_beside_a_group_without_launch();
    printf("mixed heal plan ok\n");
    return 0;
}
