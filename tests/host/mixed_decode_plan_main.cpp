// Stand-alone check of the mixed-length GET's host planner
// (rustfs_amd/csrc/rs_mixed_decode_plan.h), built by the host compiler with
// AddressSanitizer + UBSan and run directly (tests/test_mixed_decode_plan.py).
#include <set>
#include <vector>

#include "record_rounds_check.h"  // CHECK, run_rounds; the planner header

using namespace rsg::mixed;

namespace {

// A valid list: records at odd offsets with 1..3 byte gaps, out windows packed
// with the same gaps.
std::vector<RecordDesc> make(int k, const std::vector<uint32_t>& lens, const std::vector<uint32_t>& present) {
    std::vector<RecordDesc> d(lens.size());
    uint64_t r = 1, o = 3;
    for (size_t i = 0; i < lens.size(); ++i) {
        d[i] = RecordDesc{r, o, lens[i], present[i % present.size()]};
        r += kRecHeader + lens[i] + 1 + i % 3;
        o += (uint64_t)k * lens[i] + 1 + i % 3;
    }
    return d;
}

void test_validation() {
    const int k = 4, m = 2, t = k + m;
    const uint64_t A = 0x100000000ull;  // arenas far apart
    uint64_t files[6], out = 0x900000000ull;
    for (int i = 0; i < t; ++i) files[i] = A * (uint64_t)(i + 1);
    const std::vector<uint32_t> lens = {0, 1, 7, 8, 513, 0, 87382};
    std::vector<RecordDesc> d = make(k, lens, {0x3f});
    CHECK(validate_decode(k, m, d.size(), d.data(), files, out));
    CHECK(validate_decode(k, m, 0, nullptr, files, out));
    CHECK(validate_decode(k, 0, d.size(), make(k, lens, {0xf}).data(), files, out));  // m = 0
    // zero-length stripes: out offsets are not looked at
    {
        auto e = d;
        e[0].out_off = UINT64_MAX;
        e[5].out_off = 0;
        CHECK(validate_decode(k, m, e.size(), e.data(), files, out));
    }
    // a present bit at or above k+m
    {
        auto e = d;
        e[2].present = 1u << t;
        CHECK(!validate_decode(k, m, e.size(), e.data(), files, out));
        e[2].present = 0x80000000u;
        CHECK(!validate_decode(k, m, e.size(), e.data(), files, out));
    }
    // record ranges not ascending / overlapping (a bare digest still occupies 32 bytes)
    {
        auto e = d;
        e[1].rec_off = e[0].rec_off + kRecHeader - 1;
        CHECK(!validate_decode(k, m, e.size(), e.data(), files, out));
        e = d;
        std::swap(e[3].rec_off, e[4].rec_off);
        CHECK(!validate_decode(k, m, e.size(), e.data(), files, out));
        e = d;
        e[6].rec_off = e[5].rec_off;  // equal starts
        CHECK(!validate_decode(k, m, e.size(), e.data(), files, out));
    }
    // out ranges not ascending / overlapping
    {
        auto e = d;
        e[3].out_off = e[2].out_off + (uint64_t)k * e[2].shard_len - 1;
        CHECK(!validate_decode(k, m, e.size(), e.data(), files, out));
        e = d;
        std::swap(e[2].out_off, e[4].out_off);
        CHECK(!validate_decode(k, m, e.size(), e.data(), files, out));
    }
    // ranges that wrap the address space
    {
        auto e = d;
        e[6].rec_off = UINT64_MAX - 40;
        CHECK(!validate_decode(k, m, e.size(), e.data(), files, out));
        e = d;
        e[6].rec_off = UINT64_MAX - files[t - 1] - 100;  // wraps only relative to the highest arena
        CHECK(!validate_decode(k, m, e.size(), e.data(), files, out));
        e = d;
        e[6].out_off = UINT64_MAX - 8;
        CHECK(!validate_decode(k, m, e.size(), e.data(), files, out));
        e = d;
        e[6].out_off = UINT64_MAX - out - 8;
        CHECK(!validate_decode(k, m, e.size(), e.data(), files, out));
    }
    // the out span meets a source arena's record span: only one that is used
    {
        uint64_t f2[6];
        for (int i = 0; i < t; ++i) f2[i] = files[i];
        f2[5] = out + 100;
        CHECK(!validate_decode(k, m, d.size(), d.data(), f2, out));
        auto e = make(k, lens, {0x1f});  // shard 5 never read
        CHECK(validate_decode(k, m, e.size(), e.data(), f2, out));
        f2[5] = 0;  // a NULL arena, whatever `present` says
        CHECK(validate_decode(k, m, d.size(), d.data(), f2, out));
        // all stripes empty: no out span
        auto z = make(k, {0, 0, 0}, {0x3f});
        f2[5] = out;
        CHECK(validate_decode(k, m, z.size(), z.data(), f2, out));
    }
    CHECK(!validate_decode(0, 2, d.size(), d.data(), files, out));
    CHECK(!validate_decode(30, 3, 0, nullptr, files, out));  // k + m > 32
    CHECK(!validate_decode(k, m, d.size(), nullptr, files, out));
}

void test_plans() {
    MaskPlan p;
    // RS(4,2), all present: nothing rebuilt, no parity read
    CHECK(plan_mask(4, 2, 0x3f, true, p));
    CHECK(p.src == std::vector<int>({0, 1, 2, 3}) && p.written.empty() && p.surplus.empty());
    CHECK(p.read_mask() == 0xfu);
    // data shard 1 absent: sources 0 2 3 4, surplus 5 (only with verify_surplus)
    CHECK(plan_mask(4, 2, 0x3d, true, p));
    CHECK(p.src == std::vector<int>({0, 2, 3, 4}) && p.written == std::vector<int>({1}) &&
          p.surplus == std::vector<int>({5}));
    CHECK(p.read_mask() == 0x3du);
    CHECK(plan_mask(4, 2, 0x3d, false, p));
    CHECK(p.surplus.empty() && p.read_mask() == 0x1du);
    // exactly k, then k - 1
    CHECK(plan_mask(4, 2, 0x35, true, p));
    CHECK(p.src == std::vector<int>({0, 2, 4, 5}) && p.written == std::vector<int>({1, 3}) && p.surplus.empty());
    CHECK(!plan_mask(4, 2, 0x31, true, p));
    CHECK(!plan_mask(4, 2, 0, true, p));
    CHECK(plan_mask(5, 0, 0x1f, true, p));  // m = 0 only verifies
    CHECK(p.written.empty() && p.surplus.empty());
    CHECK(!plan_mask(5, 0, 0x1e, true, p));
    // the computed rows never exceed m
    for (uint32_t mask = 0; mask < (1u << 12); ++mask)
        if (plan_mask(8, 4, mask, true, p)) CHECK(p.written.size() + p.surplus.size() <= 4 && p.src.size() == 8);
    CHECK(decode_kernel_geometry(16, 4) && decode_kernel_geometry(5, 0) && !decode_kernel_geometry(10, 6) &&
          !decode_kernel_geometry(17, 3));
}

// groups of 1, SPW and SPW+1 stripes out of three interleaved masks
void test_grouping_and_order() {
    const int k = 8, m = 4, spw = decode_spw_for(k + 4);
    const uint32_t A = 0xfff, B = 0xffd, C = 0x3f;  // C: fewer than k bits
    std::vector<uint32_t> masks;
    for (int i = 0; i < spw + 1; ++i) {
        masks.push_back(B);
        if (i < spw) masks.push_back(C);
        if (i == 1) masks.push_back(A);
    }
    const size_t n = masks.size();
    std::vector<uint32_t> lens(n);
    for (size_t i = 0; i < n; ++i) lens[i] = (uint32_t)((i * 700) % 2000);  // caller order != kernel order
    std::vector<RecordDesc> d = make(k, lens, {0xfff});
    std::vector<uint32_t> todo(n);
    for (size_t i = 0; i < n; ++i) todo[i] = (uint32_t)i;
    std::vector<MaskGroup> g;
    group_by_mask(masks.data(), todo, g);
    CHECK(g.size() == 3 && g[0].mask == B && g[1].mask == C && g[2].mask == A);
    CHECK(g[0].stripes.size() == (size_t)spw + 1 && g[1].stripes.size() == (size_t)spw && g[2].stripes.size() == 1);
    std::set<uint32_t> seen;
    for (const MaskGroup& gr : g) {
        for (size_t i = 0; i < gr.stripes.size(); ++i) {
            CHECK(masks[gr.stripes[i]] == gr.mask);
            CHECK(i == 0 || gr.stripes[i - 1] < gr.stripes[i]);  // stable: caller order inside a group
            CHECK(seen.insert(gr.stripes[i]).second);
        }
        MaskPlan p;
        CHECK(plan_mask(k, m, gr.mask, true, p) == (gr.mask != C));  // fewer than k bits: no launch
        std::vector<DecDesc> tab;
        order_group_for_kernel(get_out_rule(k), d.data(), gr.stripes, 0, d[0].rec_off, 3, tab);
        CHECK(tab.size() == gr.stripes.size());
        std::set<uint32_t> jobs;
        for (size_t i = 0; i < tab.size(); ++i) {
            CHECK(i == 0 || chunks_of(tab[i - 1].len) >= chunks_of(tab[i].len));
            CHECK(jobs.insert(tab[i].job).second);
            const RecordDesc& s = d[tab[i].job];  // job maps back to the caller's index
            CHECK(masks[tab[i].job] == gr.mask && tab[i].len == s.shard_len);
            CHECK(tab[i].rec_off == s.rec_off - d[0].rec_off);
            CHECK(tab[i].out_off == (s.shard_len ? s.out_off - 3 : 0));
        }
        CHECK(jobs == std::set<uint32_t>(gr.stripes.begin(), gr.stripes.end()));
    }
    CHECK(seen.size() == n);
    // a sub-batch's jobs are relative to its first stripe
    std::vector<uint32_t> part = {5, 6, 7};
    std::vector<DecDesc> tab;
    order_group_for_kernel(get_out_rule(k), d.data(), part, 5, d[5].rec_off, 0, tab);
    for (const DecDesc& x : tab) CHECK(x.job < 3 && x.len == d[5 + x.job].shard_len);
    // an empty todo list
    group_by_mask(masks.data(), {}, g);
    CHECK(g.empty());
}

void test_split() {
    const int k = 4, t = 6;
    std::vector<uint32_t> lens;
    for (int i = 0; i < 40; ++i) lens.push_back(i % 7 == 0 ? 0u : 1000u * (uint32_t)(i % 5 + 1));
    lens[20] = 300000;  // larger than the stage: a sub-batch of its own
    std::vector<RecordDesc> d = make(k, lens, {0x3f});
    const uint64_t stage = 200000;
    const OutRule rule = get_out_rule(k);
    std::vector<RecSubBatch> subs;
    split_records(rule, t, d.size(), d.data(), stage, d.size(), subs);
    size_t next = 0;
    bool alone = false;
    for (const RecSubBatch& b : subs) {
        CHECK(b.first == next && b.count >= 1);
        next += b.count;
        CHECK(b.count == 1 || record_stage_bytes(rule, b, t) <= stage);
        if (b.first == 20) alone = b.count == 1;
        CHECK(b.rec_lo == d[b.first].rec_off);
        const RecordDesc& last = d[b.first + b.count - 1];
        CHECK(b.rec_hi == last.rec_off + kRecHeader + last.shard_len);
        for (size_t j = 0; j < b.count; ++j) {
            const RecordDesc& s = d[b.first + j];
            if (s.shard_len) CHECK(b.out_lo <= s.out_off && s.out_off + (uint64_t)k * s.shard_len <= b.out_hi);
        }
    }
    CHECK(next == d.size() && alone && subs.size() >= 3);
    split_records(rule, t, d.size(), d.data(), UINT64_MAX, d.size(), subs);
    CHECK(subs.size() == 1 && subs[0].count == d.size());
    split_records(rule, t, d.size(), d.data(), UINT64_MAX, 7, subs);  // max_count
    CHECK(subs.size() == 6 && subs.back().count == 5);
    split_records(rule, t, 0, d.data(), stage, 1, subs);
    CHECK(subs.empty());
    auto z = make(k, {0, 0, 0}, {0x3f});  // only empty stripes: no out span
    split_records(rule, t, z.size(), z.data(), stage, z.size(), subs);
    CHECK(subs.size() == 1 && subs[0].out_lo == 0 && subs[0].out_hi == 0 && subs[0].rec_hi > subs[0].rec_lo);
}

// The rounds the library runs (plan_round -> launches -> shard_flags_from_rows
// -> redo_from_flags), driven by a table of records that are rotten; ends in
// at most k+m rounds with the verified sets.
void test_redo() {
    const int k = 4, m = 2, t = k + m;
    const size_t n = 9;
    // rotten[s]: bits of stripe s's records that fail their hash when read
    const uint32_t rotten[n] = {0, 0x02, 0x10, 0x20, 0x3f, 0x0f, 0x01, 0x12, 0};
    uint32_t masks[n] = {0x3f, 0x3f, 0x3d, 0x3d, 0x3f, 0x3f, 0x07, 0x3f, 0x3e};
    const uint32_t start[n] = {0x3f, 0x3f, 0x3d, 0x3d, 0x3f, 0x3f, 0x07, 0x3f, 0x3e};
    const std::vector<RecordDesc> d = make(k, {7, 0, 513, 64, 1025, 1, 0, 300, 65}, {0x3f});
    const int rounds = rounds_check::run_rounds(k, m, get_out_rule(k), d, rotten, masks, [&](uint32_t mask, MaskPlan& p) {
        return plan_mask(k, m, mask, true, p);
    });
    CHECK(rounds <= t);
    for (size_t s = 0; s < n; ++s) {
        // no record that was read and failed stays; nothing healthy is dropped
        CHECK(masks[s] == (start[s] & ~rotten[s]) || popcount32(masks[s]) < k ||
              (masks[s] & ~rotten[s]) == masks[s]);
        MaskPlan p;
        if (plan_mask(k, m, masks[s], true, p)) CHECK((p.read_mask() & rotten[s]) == 0);
    }
    CHECK(masks[0] == 0x3f && masks[8] == 0x3e);
    CHECK(masks[1] == 0x3d);                  // rotten data shard found with all data assumed present
    CHECK(masks[2] == 0x2d && masks[3] == 0x1d);  // a rotten source parity, a rotten surplus parity
    CHECK(popcount32(masks[4]) < k && popcount32(masks[5]) < k && popcount32(masks[6]) < k);
    CHECK(masks[7] == 0x2d);  // parity 4 is found rotten only after data 1 is
}

// A round that mixes groups with a plan and a group with fewer than k readable
// shards, which has no launch: the flags of each launch go to its own group's
// stripes.  RS(4,2), three masks interleaved in groups of SPW+1, SPW and 1
// stripes, the one without a plan first met between the other two.
void test_rounds_beside_a_group_without_launch() {
    const int k = 4, m = 2, t = k + m, spw = decode_spw_for(t);
    const uint32_t A = 0x3f, B = 0x3d, C = 0x07;  // C: three bits set
    std::vector<uint32_t> masks, rotten, lens;
    for (int i = 0; i < spw + 1; ++i) {
        masks.push_back(B);
        rotten.push_back(i == 1 ? 0x10u : i == spw ? 0x01u : 0u);  // a source parity; a data source
        if (i < spw) {
            masks.push_back(C);
            rotten.push_back(0x3f);  // never read
        }
        if (i == 1) {
            masks.push_back(A);
            rotten.push_back(0x02);  // joins B's mask in the second round
        }
    }
    const size_t n = masks.size();
    for (size_t i = 0; i < n; ++i) lens.push_back((uint32_t)((i * 700) % 2000));
    const std::vector<RecordDesc> d = make(k, lens, {0x3f});
    const std::vector<uint32_t> start = masks;
    const int rounds = rounds_check::run_rounds(k, m, get_out_rule(k), d, rotten.data(), masks.data(),
                                                [&](uint32_t mask, MaskPlan& p) { return plan_mask(k, m, mask, true, p); });
    CHECK(rounds >= 2 && rounds <= t);
    size_t moved = 0;
    for (size_t s = 0; s < n; ++s) {
        // no launch: untouched, whatever the launches beside it wrote
        CHECK(masks[s] == (start[s] == C ? C : start[s] & ~rotten[s]));
        moved += masks[s] != start[s];
    }
    CHECK(moved == 3);
}

// The depth of the redo rounds, RS(5,4) with data shard 2 rotten and further
// rotten parity shards: the launching rounds of each stripe on its own, with
// and without verify_surplus, as literal figures (the ones the GPU tests'
// Python model, tests/mixed_shapes.py settle, is held to in
// tests/test_mixed_shapes.py and tests/test_gpu_mixed_decode.py); then all of
// them in one batch beside clean stripes, which runs as deep as the deepest.
void test_redo_depth() {
    const int k = 5, m = 4;
    const uint32_t all = 0x1ff, d2 = 1u << 2;
    struct Row {
        uint32_t parity;  // rotten parity shards (bits 5..8)
        int off, on;      // launching rounds without / with verify_surplus
        bool ok_off, ok_on;
        uint32_t end_off, end_on;  // the final masks
    };
    const Row rows[] = {
        {0x000, 2, 2, true, true, all & ~d2, all & ~d2},
        {0x020, 3, 3, true, true, all & ~d2 & ~0x020u, all & ~d2 & ~0x020u},
        {0x060, 4, 3, true, true, all & ~d2 & ~0x060u, all & ~d2 & ~0x060u},
        {0x0e0, 5, 3, true, true, all & ~d2 & ~0x0e0u, all & ~d2 & ~0x0e0u},
        {0x1e0, 5, 2, false, false, 0x01b, 0x01b},
        {0x1c0, 2, 3, true, true, all & ~d2, all & ~d2 & ~0x1c0u},  // without verify_surplus parity 6 onwards is never read
        {0x040, 2, 3, true, true, all & ~d2, all & ~d2 & ~0x040u},
    };
    const size_t nrows = sizeof(rows) / sizeof(rows[0]);
    for (int vs = 0; vs < 2; ++vs) {
        auto plan = [&](uint32_t mask, MaskPlan& p) { return plan_mask(k, m, mask, vs != 0, p); };
        int deepest = 0;
        for (const Row& r : rows) {
            const std::vector<RecordDesc> d = make(k, {513}, {all});
            const uint32_t rotten = d2 | r.parity;
            uint32_t mask = all;
            int launching = 0;
            const int rounds = rounds_check::run_rounds(k, m, get_out_rule(k), d, &rotten, &mask, plan, &launching);
            const bool ok = vs ? r.ok_on : r.ok_off;
            CHECK(launching == (vs ? r.on : r.off));
            CHECK(rounds == launching + (ok ? 0 : 1));  // the round that finds no plan launches nothing
            CHECK(mask == (vs ? r.end_on : r.end_off) && (popcount32(mask) >= k) == ok);
            deepest = std::max(deepest, launching);
        }
        CHECK(deepest == (vs ? 3 : 5));
        // one batch: every row between clean stripes, lengths mixed
        std::vector<uint32_t> rotten, masks, lens;
        for (size_t i = 0; i < nrows; ++i) {
            rotten.push_back(d2 | rows[i].parity);
            rotten.push_back(0);
            lens.push_back((uint32_t)(i % 2 ? 1025 : 7));
            lens.push_back(33);
        }
        masks.assign(rotten.size(), all);
        const std::vector<RecordDesc> d = make(k, lens, {all});
        int launching = 0;
        rounds_check::run_rounds(k, m, get_out_rule(k), d, rotten.data(), masks.data(), plan, &launching);
        CHECK(launching == deepest);
        for (size_t i = 0; i < nrows; ++i) {
            CHECK(masks[2 * i] == (vs ? rows[i].end_on : rows[i].end_off));
            CHECK(masks[2 * i + 1] == all);
        }
    }
}

}  // namespace

int main() {
    test_validation();
    test_plans();
    test_grouping_and_order();
    test_split();
    test_redo();
    test_rounds_beside_a_group_without_launch();
    test_redo_depth();
    printf("mixed decode plan ok\n");
    return 0;
}
