// Stand-alone check of the mixed-length deep scan's host planner
// (rustfs_amd/csrc/rs_mixed_verify_plan.h), built by the host compiler with
// AddressSanitizer + UBSan and run directly (tests/test_mixed_verify_plan.py).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../rustfs_amd/csrc/rs_mixed_verify_plan.h"

using namespace rsg::mixed;

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
            exit(1);                                                  \
        }                                                             \
    } while (0)

namespace {

constexpr uint64_t HS = 32;

uint64_t want_of(uint64_t part, uint32_t shard) {
    uint64_t w = 0;
    CHECK(verify_expect_size(part, shard, HS, w));
    return w;
}

// A complete, healthy file of `part` body bytes in records of `shard`.
FileDesc whole(uint64_t off, uint64_t part, uint32_t shard, uint32_t arena) {
    const uint64_t w = want_of(part, shard);
    return FileDesc{off, w, w, part, shard, arena};
}

// Files laid out over `n_arenas` arenas round-robin, ascending per arena with
// gaps of 0..2 bytes; returns the list, `end` the arenas' lengths.
struct Shape {
    uint64_t part;
    uint32_t shard;
    int64_t cut;  // file_len = want + cut (negative: truncated)
};

std::vector<FileDesc> layout(const std::vector<Shape>& shapes, int n_arenas, std::vector<uint64_t>& end) {
    end.assign((size_t)n_arenas, 0);
    std::vector<FileDesc> d;
    for (size_t i = 0; i < shapes.size(); ++i) {
        const uint32_t a = (uint32_t)(i % (size_t)n_arenas);
        FileDesc f = whole(end[a] + i % 3, shapes[i].part, shapes[i].shard, a);
        f.file_len = (uint64_t)((int64_t)f.want_size + shapes[i].cut);
        d.push_back(f);
        if (f.file_len) end[a] = f.off + f.file_len;
    }
    return d;
}

void test_sizes() {
    CHECK(want_of(0, 0) == 0 && want_of(0, 5) == 0);
    CHECK(want_of(1, 1) == 33 && want_of(10, 4) == 10 + 3 * 32 && want_of(8, 4) == 8 + 2 * 32);
    uint64_t w;
    CHECK(verify_expect_size(100, 7, 0, w) && w == 100);  // NONE: the part's own size
    CHECK(!verify_expect_size(UINT64_MAX - 5, 1, HS, w));  // does not fit 64 bits
    const FileDesc f{0, 100, UINT64_MAX - 5, UINT64_MAX - 5, 1, 0};  // no want_size equals it
    CHECK(!verify_size_ok(f, HS) && verify_records(f, HS) == 0);
}

void test_validation() {
    const uint64_t base[3] = {0x100000000ull, 0x200000000ull, 0x300000000ull};
    std::vector<uint64_t> end;
    const std::vector<Shape> shapes = {{10, 4, 0}, {0, 0, 0}, {87382, 87382, 0}, {3, 1, -1}, {513, 256, 5}, {0, 7, 0}};
    std::vector<FileDesc> d = layout(shapes, 3, end);
    CHECK(validate_verify(3, d.size(), d.data(), base));
    CHECK(validate_verify(3, 0, nullptr, base));
    // NULL pointers, arena counts
    CHECK(!validate_verify(3, d.size(), nullptr, base));
    CHECK(!validate_verify(3, d.size(), d.data(), nullptr));
    CHECK(!validate_verify(0, d.size(), d.data(), base));
    CHECK(!validate_verify(33, d.size(), d.data(), base));
    // arena >= n_arenas
    CHECK(!validate_verify(2, d.size(), d.data(), base));
    {
        auto e = d;
        e[0].arena = 3;
        CHECK(!validate_verify(3, e.size(), e.data(), base));
        e[0].arena = 0xffffffffu;
        CHECK(!validate_verify(3, e.size(), e.data(), base));
    }
    // shard_size == 0 with part_size > 0 (even for an empty file)
    {
        auto e = d;
        e[1].part_size = 1;
        CHECK(!validate_verify(3, e.size(), e.data(), base));
    }
    // a NULL arena holds only empty files
    {
        const uint64_t nul[3] = {base[0], 0, base[2]};
        CHECK(!validate_verify(3, d.size(), d.data(), nul));  // file 4 (arena 1) has bytes
        auto e = d;
        e[4].file_len = 0;
        CHECK(validate_verify(3, e.size(), e.data(), nul));  // arena 1: only empty files now
    }
    // a range that wraps: in its offset, against its arena's address
    {
        auto e = d;
        e[5].off = UINT64_MAX - 3;
        e[5].file_len = 4;
        CHECK(!validate_verify(3, e.size(), e.data(), base));
        e[5].off = UINT64_MAX - base[2] - 3;
        CHECK(!validate_verify(3, e.size(), e.data(), base));
        e[5].off = UINT64_MAX - base[2] - 4;  // ends at the last byte
        CHECK(validate_verify(3, e.size(), e.data(), base));
    }
    // ranges of one arena not ascending / overlapping; other arenas interleave freely
    {
        auto e = d;
        CHECK(e[3].arena == e[0].arena);
        e[3].off = e[0].off + e[0].file_len - 1;
        CHECK(!validate_verify(3, e.size(), e.data(), base));
        e[3].off = e[0].off + e[0].file_len;  // touching is disjoint
        CHECK(validate_verify(3, e.size(), e.data(), base));
        e[3].off = 0;
        e[0].off = 500;  // descending in list order
        CHECK(!validate_verify(3, e.size(), e.data(), base));
        auto g = d;
        g[4].off = 0;  // arena 1's only non-empty file: anywhere, whatever the others' offsets
        CHECK(validate_verify(3, g.size(), g.data(), base));
        g[1].off = UINT64_MAX;  // an empty file occupies nothing
        CHECK(validate_verify(3, g.size(), g.data(), base));
    }
}

// Every unit's header and body inside [off, off + min(file_len, want_size)),
// flag indices in caller order [file][record], no zero-length unit.
void check_units(const std::vector<FileDesc>& d, const std::vector<VerifyUnit>& units,
                 const std::vector<uint64_t>& flag0, const std::vector<uint64_t>& expect_recs) {
    CHECK(flag0.size() == d.size() + 1 && flag0[0] == 0 && flag0[d.size()] == units.size());
    size_t at = 0;
    for (size_t j = 0; j < d.size(); ++j) {
        const FileDesc& f = d[j];
        CHECK(flag0[j + 1] - flag0[j] == expect_recs[j]);
        const uint64_t lim = f.off + std::min(f.file_len, f.want_size);
        for (uint64_t r = 0; r < expect_recs[j]; ++r, ++at) {
            const VerifyUnit& u = units[at];
            CHECK(u.flag == flag0[j] + r);
            CHECK(u.len > 0);
            CHECK(u.addr == f.off + r * (HS + f.shard_size) + HS);
            CHECK(u.addr - HS >= f.off && u.addr + u.len <= lim);
            const uint64_t full = f.part_size / f.shard_size;
            CHECK(u.len == (r < full ? f.shard_size : f.part_size - full * f.shard_size));
        }
    }
    CHECK(at == units.size());
}

void test_expansion() {
    const uint64_t zero[kVerifyMaxArenas] = {};
    std::vector<uint64_t> end;
    // parts of 0..3 full records with tails 0, 1 and shard - 1, whole
    for (uint32_t shard : {1u, 2u, 7u, 32u, 33u, 256u, 87382u}) {
        std::vector<Shape> shapes;
        std::vector<uint64_t> recs;
        for (uint64_t full = 0; full <= 3; ++full)
            for (uint64_t tail : {(uint64_t)0, (uint64_t)1, (uint64_t)shard - 1}) {
                if (tail >= shard) continue;  // shard 1 has no tail
                shapes.push_back({full * shard + tail, shard, 0});
                recs.push_back(full + (tail ? 1 : 0));
            }
        std::vector<FileDesc> d = layout(shapes, 3, end);
        CHECK(validate_verify(3, d.size(), d.data(), end.data()));
        std::vector<VerifyUnit> units;
        std::vector<uint64_t> flag0;
        CHECK(expand_units(d.data(), 0, d.size(), HS, zero, units, flag0));
        check_units(d, units, flag0, recs);
        // with NONE nothing is a unit
        CHECK(expand_units(d.data(), 0, d.size(), 0, zero, units, flag0) && units.empty());
    }
    // cuts: mid-header, mid-body, at a record boundary; longer files; a size mismatch among healthy ones
    {
        const uint32_t S = 100;
        const uint64_t part = 3 * S + 40, rec = HS + S;  // 3 full records + a 40-byte tail
        struct Cut {
            uint64_t file_len, recs;
        };
        const uint64_t want = want_of(part, S);
        CHECK(want == 3 * rec + HS + 40);
        const std::vector<Cut> cuts = {
            {0, 0},                // empty
            {HS - 1, 0},           // mid first header
            {HS, 0},               // header only
            {HS + S - 1, 0},       // mid first body
            {rec, 1},              // at a record boundary
            {rec + 5, 1},          // mid second header
            {2 * rec + HS + 1, 2}, // mid third body
            {3 * rec, 3},          // boundary before the tail record
            {3 * rec + HS, 3},     // the tail's header only
            {want - 1, 3},         // the tail cut by one byte
            {want, 4},             // whole
            {want + 1, 4},         // trailing data
            {want + 1000, 4},
        };
        std::vector<FileDesc> d;
        std::vector<uint64_t> recs;
        uint64_t at[2] = {3, 5};
        for (size_t i = 0; i < cuts.size(); ++i) {
            const uint32_t a = (uint32_t)(i & 1);
            d.push_back(FileDesc{at[a], cuts[i].file_len, want, part, S, a});
            recs.push_back(cuts[i].recs);
            at[a] += cuts[i].file_len + i % 2;
            if (i == 6) {  // a size-mismatch file among healthy ones: no unit, whatever is there
                d.push_back(FileDesc{at[0], want, want + 1, part, S, 0});
                recs.push_back(0);
                at[0] += want;
                d.push_back(FileDesc{at[1], want, want, part, 2 * S, 1});
                recs.push_back(0);
                at[1] += want;
            }
        }
        const uint64_t ends[2] = {at[0] + 1, at[1] + 1};
        CHECK(validate_verify(2, d.size(), d.data(), ends));
        std::vector<VerifyUnit> units;
        std::vector<uint64_t> flag0;
        CHECK(expand_units(d.data(), 0, d.size(), HS, zero, units, flag0));
        check_units(d, units, flag0, recs);
        // a window of the list numbers its flags from 0, bases are added
        uint64_t base[kVerifyMaxArenas] = {};
        base[0] = 0x1000;
        base[1] = 0x200000000ull;
        std::vector<VerifyUnit> win;
        std::vector<uint64_t> f0;
        CHECK(expand_units(d.data(), 4, 5, HS, base, win, f0));
        CHECK(f0[0] == 0 && f0[5] == win.size() && win.size() == flag0[9] - flag0[4]);
        for (size_t i = 0; i < win.size(); ++i) {
            const VerifyUnit& u = units[(size_t)flag0[4] + i];
            CHECK(win[i].flag == i && win[i].len == u.len);
        }
        CHECK(win[0].addr == base[d[4].arena] + d[4].off + HS);
        // part_size == 0 with a non-empty file: no unit
        FileDesc z{0, 17, 0, 0, 0, 0};
        CHECK(verify_size_ok(z, HS) && verify_records(z, HS) == 0);
    }
}

void test_order() {
    const uint64_t zero[kVerifyMaxArenas] = {};
    std::vector<uint64_t> end;
    std::vector<Shape> shapes;
    const uint32_t lens[] = {1, 255, 256, 257, 4096, 511, 512, 87382, 7, 768, 4097, 300};
    for (int rep = 0; rep < 3; ++rep)
        for (uint32_t s : lens) shapes.push_back({(uint64_t)s * 2 + (s > 1 ? s / 2 : 0), s, 0});
    std::vector<FileDesc> d = layout(shapes, 4, end);
    std::vector<VerifyUnit> units, tab;
    std::vector<uint64_t> flag0;
    CHECK(expand_units(d.data(), 0, d.size(), HS, zero, units, flag0));
    order_units_for_kernel(units, tab);
    CHECK(tab.size() == units.size());
    std::vector<int> seen(units.size(), 0);
    for (size_t i = 0; i < tab.size(); ++i) {
        CHECK(tab[i].flag < units.size() && !seen[tab[i].flag]++);  // a permutation
        const VerifyUnit& u = units[tab[i].flag];
        CHECK(u.addr == tab[i].addr && u.len == tab[i].len);
        if (i) {
            CHECK(verify_unit_batches(tab[i - 1]) >= verify_unit_batches(tab[i]));  // non-increasing
            if (verify_unit_batches(tab[i - 1]) == verify_unit_batches(tab[i]))
                CHECK(tab[i - 1].flag < tab[i].flag);  // equal counts stay in caller order
        }
    }
    std::vector<VerifyUnit> none, out;
    order_units_for_kernel(none, out);
    CHECK(out.empty());
}

void test_split() {
    std::vector<uint64_t> end;
    std::vector<Shape> shapes;
    for (int i = 0; i < 40; ++i) shapes.push_back({(uint64_t)(1000 + 37 * i), (uint32_t)(100 + i), i % 7 == 3 ? -5 : 0});
    shapes.push_back({200000, 1000, 0});  // oversize for the limits below
    for (int i = 0; i < 10; ++i) shapes.push_back({(uint64_t)(500 + i), 64, 0});
    shapes.push_back({0, 0, 0});
    shapes.push_back({3000, 100, 500000});  // a long surplus: never read, never staged
    shapes.push_back({3000, 100, -3950});   // cut inside its first record: nothing of it is read
    shapes.push_back({700, 64, 0});
    std::vector<FileDesc> d = layout(shapes, 3, end);
    {
        // what is read of a file decides what it costs
        std::vector<VerifySubBatch> one;
        split_verify(1, &d[52], HS, (uint64_t)1 << 30, one);
        CHECK(one.size() == 1 && one[0].units == 30 && one[0].hi[d[52].arena] - one[0].lo[d[52].arena] == d[52].want_size);
        CHECK(verify_stage_bytes(one[0]) == stage_round(d[52].want_size) + stage_round(30 * 16) + stage_round(30));
        split_verify(1, &d[53], HS, (uint64_t)1 << 30, one);
        CHECK(one.size() == 1 && d[53].file_len == 10 && one[0].touched == 0 && verify_stage_bytes(one[0]) == 0);
    }
    d[5].want_size += 1;  // a size mismatch: read by nobody, costs nothing
    for (uint64_t stage : {(uint64_t)1, (uint64_t)4096, (uint64_t)20000, (uint64_t)100000, (uint64_t)1 << 30}) {
        std::vector<VerifySubBatch> subs;
        split_verify(d.size(), d.data(), HS, stage, subs);
        size_t next = 0;
        for (const VerifySubBatch& b : subs) {
            CHECK(b.first == next && b.count >= 1);  // every file once, in order
            next += b.count;
            CHECK(verify_stage_bytes(b) <= stage || b.count == 1);  // within the limit, or alone
            // the spans and the unit count are those of its files
            uint64_t units = 0, lo[kVerifyMaxArenas], hi[kVerifyMaxArenas];
            uint32_t touched = 0;
            for (size_t j = b.first; j < b.first + b.count; ++j) {
                const FileDesc& f = d[j];
                if (!verify_records(f, HS)) continue;  // never read: not staged
                if (!(touched >> f.arena & 1u)) lo[f.arena] = f.off;
                touched |= 1u << f.arena;
                hi[f.arena] = f.off + std::min(f.file_len, f.want_size);  // the surplus is not read
                units += verify_records(f, HS);
            }
            CHECK(touched == b.touched && units == b.units);
            for (int a = 0; a < kVerifyMaxArenas; ++a)
                if (touched >> a & 1u) CHECK(lo[a] == b.lo[a] && hi[a] == b.hi[a]);
        }
        CHECK(next == d.size());
        if (stage == 100000) {  // the 200000-byte part is alone, its neighbours are not
            bool alone = false;
            for (const VerifySubBatch& b : subs)
                if (b.first <= 40 && 40 < b.first + b.count) alone = b.count == 1 && verify_stage_bytes(b) > stage;
            CHECK(alone && subs.size() >= 3);
        }
        if (stage == (uint64_t)1 << 30) CHECK(subs.size() == 1);
    }
    std::vector<VerifySubBatch> subs;
    split_verify(0, nullptr, HS, 4096, subs);
    CHECK(subs.empty());
}

void test_reduce() {
    const uint32_t S = 50;
    const uint64_t part = 4 * S + 9, rec = HS + S, want = want_of(part, S);
    // whole, truncated after 2 records, longer, size mismatch, empty part, part 0 with bytes
    std::vector<FileDesc> d = {
        {0, want, want, part, S, 0},          {1000, 2 * rec + 3, want, part, S, 0}, {2000, want + 2, want, part, S, 0},
        {3000, want, want - 1, part, S, 0},   {4000, 0, 0, 0, 0, 0},                 {4000, 5, 0, 0, 0, 0},
    };
    const uint64_t zero[kVerifyMaxArenas] = {};
    std::vector<VerifyUnit> units;
    std::vector<uint64_t> flag0;
    CHECK(expand_units(d.data(), 0, d.size(), HS, zero, units, flag0));
    CHECK(units.size() == 5 + 2 + 5);
    std::vector<VerifyVerdict> v(d.size());
    std::vector<uint8_t> flags(units.size(), 1);
    reduce_verdicts(d.data(), 0, d.size(), HS, flag0, flags.data(), v.data());
    CHECK(v[0] == kVerifyOk && v[1] == kVerifyEof && v[2] == kVerifyTrailing && v[3] == kVerifySizeMismatch &&
          v[4] == kVerifyOk && v[5] == kVerifyTrailing);
    // mismatch before EOF before trailing; one or several bad records: one mismatch, the others untouched
    for (size_t bad0 : {(size_t)0, (size_t)2, (size_t)4}) {
        std::fill(flags.begin(), flags.end(), 1);
        flags[bad0] = 0;
        flags[4] = 0;
        flags[flag0[1] + 1] = 0;
        flags[flag0[2] + 4] = 0;
        reduce_verdicts(d.data(), 0, d.size(), HS, flag0, flags.data(), v.data());
        CHECK(v[0] == kVerifyBitrot && v[1] == kVerifyBitrot && v[2] == kVerifyBitrot && v[3] == kVerifySizeMismatch &&
              v[4] == kVerifyOk && v[5] == kVerifyTrailing);
    }
    // only the flags of a file's own records matter
    std::fill(flags.begin(), flags.end(), 1);
    flags[flag0[1]] = 0;
    reduce_verdicts(d.data(), 0, d.size(), HS, flag0, flags.data(), v.data());
    CHECK(v[0] == kVerifyOk && v[1] == kVerifyBitrot && v[2] == kVerifyTrailing);
    // NONE: sizes only, no flags at all
    std::vector<FileDesc> e = {{0, 100, 100, 100, 7, 0}, {0, 99, 100, 100, 7, 0}, {0, 101, 100, 100, 7, 0},
                               {0, 132, 132, 100, 100, 0}};
    std::vector<uint64_t> f0(e.size() + 1, 0);
    v.assign(e.size(), kVerifyBitrot);
    reduce_verdicts(e.data(), 0, e.size(), 0, f0, nullptr, v.data());
    CHECK(v[0] == kVerifyOk && v[1] == kVerifyEof && v[2] == kVerifyTrailing && v[3] == kVerifySizeMismatch);
}

}  // namespace

int main() {
    test_sizes();
    test_validation();
    test_expansion();
    test_order();
    test_split();
    test_reduce();
    printf("mixed verify plan ok\n");
    return 0;
}
