// blocks_plan_main.cpp — the gathered block encode's host planner
// (rustfs_amd/csrc/rs_blocks_plan.h) on a CPU: validation, tile and unit
// tables, sub-batch splits, and the copy / launch counts DESIGN.md states.
// Stand-alone (its own main); tests/test_blocks_plan.py builds it with the
// host compiler under AddressSanitizer + UBSan and runs it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../rustfs_amd/csrc/rs_blocks_plan.h"

using namespace rsg::blocks;

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            exit(1);                                              \
        }                                                         \
    } while (0)

namespace {

uint8_t* at(uint64_t a) { return reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(a)); }

// One block's pointer list, kept alive next to the Block that points at it.
struct Blk {
    std::vector<uint8_t*> ptr;
    Block b;
};

// k+m shards back to back at `base` (encode_buffer's layout)
Blk packed(int t, uint64_t base, uint64_t len, uint64_t digests = 0) {
    Blk x;
    for (int s = 0; s < t; ++s) x.ptr.push_back(at(base + (uint64_t)s * len));
    x.b = Block{nullptr, len, digests ? at(digests) : nullptr};
    return x;
}
// every shard on its own, `gap` bytes between them
Blk spread(int t, uint64_t base, uint64_t len, uint64_t gap, uint64_t digests = 0) {
    Blk x;
    for (int s = 0; s < t; ++s) x.ptr.push_back(at(base + (uint64_t)s * (len + gap)));
    x.b = Block{nullptr, len, digests ? at(digests) : nullptr};
    return x;
}
std::vector<Block> list(std::vector<Blk>& v) {
    std::vector<Block> out;
    for (Blk& x : v) {
        x.b.shards = x.ptr.data();
        out.push_back(x.b);
    }
    return out;
}

void test_validation() {
    const int k = 4, m = 2, t = 6;
    {
        std::vector<Blk> v{packed(t, 0x100000, 100), spread(t, 0x200000, 33, 7, 0x300000)};
        auto l = list(v);
        CHECK(validate(k, m, l.size(), l.data(), true) == kOk);
        CHECK(validate(k, m, 0, nullptr, true) == kOk);
        CHECK(validate(k, m, 2, nullptr, true) == kInvalid);
        l[1].shards = nullptr;
        CHECK(validate(k, m, l.size(), l.data(), true) == kInvalid);
    }
    for (int s = 0; s < t; ++s) {  // a null shard pointer, data or parity
        std::vector<Blk> v{packed(t, 0x100000, 100), packed(t, 0x200000, 100)};
        v[1].ptr[(size_t)s] = nullptr;
        auto l = list(v);
        CHECK(validate(k, m, l.size(), l.data(), false) == kInvalid);
    }
    {
        std::vector<Blk> v{packed(t, 0x100000, 100), packed(t, 0x200000, 0)};
        auto l = list(v);
        CHECK(validate(k, m, l.size(), l.data(), false) == kEmpty);
        l[1].shard_len = kMaxLen + 1;
        CHECK(validate(k, m, l.size(), l.data(), false) == kInvalid);
        std::vector<Blk> w{packed(t, 0x100000, 100), packed(t, 0x200000, kMaxLen)};  // the largest length
        auto lw = list(w);
        CHECK(validate(k, m, lw.size(), lw.data(), false) == kOk);
    }
    {  // a range that wraps the address space
        std::vector<Blk> v{packed(t, 0x100000, 100)};
        v[0].ptr[5] = at(UINT64_MAX - 50);
        auto l = list(v);
        CHECK(validate(k, m, l.size(), l.data(), false) == kInvalid);
    }
    {  // data ranges may overlap each other, inside a block and across blocks
        std::vector<Blk> v{packed(t, 0x100000, 100), packed(t, 0x200000, 100)};
        v[0].ptr[1] = v[0].ptr[0];
        v[1].ptr[2] = v[0].ptr[0] + 50;
        auto l = list(v);
        CHECK(validate(k, m, l.size(), l.data(), true) == kOk);
    }
    // a parity or digest range that meets any other range, in any list order
    for (int order = 0; order < 2; ++order) {
        for (int what = 0; what < 6; ++what) {
            Blk a = packed(t, 0x100000, 100, 0x110000), c = packed(t, 0x200000, 100, 0x210000);
            bool needs_digests = false;
            switch (what) {
                case 0: c.ptr[4] = a.ptr[0] + 99; break;            // parity over another block's data (1 byte)
                case 1: c.ptr[5] = a.ptr[5] - 99; break;            // parity over parity
                case 2: c.ptr[4] = c.ptr[1]; break;                 // parity over its own block's data
                case 3: c.b.digests = a.ptr[2] + 10; needs_digests = true; break;  // digests over data
                case 4: c.b.digests = a.b.digests + 191; needs_digests = true; break;  // digests over digests (1 byte)
                case 5: c.ptr[4] = a.b.digests - 99; needs_digests = true; break;  // parity over digests
            }
            std::vector<Blk> v;
            if (order) { v.push_back(c); v.push_back(a); } else { v.push_back(a); v.push_back(c); }
            auto l = list(v);
            CHECK(validate(k, m, l.size(), l.data(), true) == kInvalid);
            // without an algo the digest pointers do not count
            CHECK((validate(k, m, l.size(), l.data(), false) == kInvalid) == !needs_digests);
        }
    }
    {  // ranges that only touch are fine
        Blk a = packed(t, 0x100000, 100, 0x100000 + 600);
        std::vector<Blk> v{a, packed(t, 0x100000 + 600 + 192, 64)};
        auto l = list(v);
        CHECK(validate(k, m, l.size(), l.data(), true) == kOk);
    }
}

// the kernel's workgroup -> (block, tile) search and its thread -> unit map
void test_tiles() {
    const int k = 2, m = 1, t = 3;
    const uint64_t lens[] = {1, kTile - 1, kTile, kTile + 1, 3ull * kTile + 5};
    std::vector<Blk> v;
    uint64_t base = 0x1000000;
    for (uint64_t len : lens) {
        v.push_back(packed(t, base, len));
        base += 0x100000;
    }
    auto l = list(v);
    CHECK(validate(k, m, l.size(), l.data(), false) == kOk);
    BatchPlan p;
    plan_batch(k, m, l.size(), l.data(), false, nullptr, nullptr, 0x7000000000ull, p);
    const size_t n = l.size();
    CHECK(p.tile0.size() == n + 1 && p.tile0[0] == 0 && p.desc.size() == n);
    std::vector<std::vector<uint8_t>> cover;
    for (uint64_t len : lens) cover.emplace_back((size_t)len, 0);
    for (uint32_t wg = 0; wg < p.tile0[n]; ++wg) {
        uint32_t lo = 0, hi = (uint32_t)n;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (p.tile0[mid] <= wg) lo = mid;
            else hi = mid;
        }
        CHECK(p.tile0[lo] <= wg && wg < p.tile0[lo + 1]);
        const uint64_t len = p.desc[lo].len;
        CHECK(len == lens[lo]);
        for (uint32_t th = 0; th < 256; ++th) {
            const uint64_t off = (uint64_t)(wg - p.tile0[lo]) * kTile + th * 16u;
            if (off >= len) continue;
            for (uint64_t x = off; x < off + 16 && x < len; ++x) ++cover[lo][(size_t)x];
        }
    }
    for (size_t i = 0; i < n; ++i)
        for (uint8_t c : cover[i]) CHECK(c == 1);
    CHECK(p.tile0[n] == 1 + 1 + 1 + 2 + 4);
}

void test_units() {
    const int k = 3, m = 2, t = 5;
    const uint64_t lens[] = {300, 7, 70000, 300, 1, 4096};
    std::vector<Blk> v;
    uint64_t base = 0x1000000;
    for (size_t i = 0; i < 6; ++i) {
        v.push_back(packed(t, base, lens[i], i == 1 ? 0 : base + 0x80000));  // block 1: parity only
        base += 0x100000;
    }
    auto l = list(v);
    CHECK(validate(k, m, l.size(), l.data(), true) == kOk);
    const uint64_t stage = 0x7000000000ull;
    BatchPlan p;
    plan_batch(k, m, l.size(), l.data(), true, nullptr, nullptr, stage, p);
    CHECK(p.unit.size() == 5u * t);
    for (size_t j = 1; j < p.unit.size(); ++j) CHECK(p.unit[j - 1].len >= p.unit[j].len);
    // a permutation: every (hashed block, shard) once, with its own digest slot
    std::vector<int> seen(p.unit.size(), 0);
    CHECK(p.digest_bytes == 5u * t * 32 && p.moves.size() == 5);
    for (const HashUnit& u : p.unit) {
        CHECK(u.pad == 0 && u.out >= p.digest_dev && (u.out - p.digest_dev) % 32 == 0);
        const size_t slot = (size_t)((u.out - p.digest_dev) / 32);
        CHECK(slot < seen.size());
        ++seen[slot];
        // the message is the stage slot of that shard: inside the stage, below the digests
        CHECK(u.addr >= stage && u.addr + u.len <= p.digest_dev);
        const DigestMove& mv = p.moves[slot / t];
        CHECK(mv.off == (slot / t) * (uint64_t)t * 32);
        size_t blk = 0;
        while (l[blk].digests != mv.host) ++blk;
        CHECK(u.len == l[blk].shard_len);
    }
    for (int c : seen) CHECK(c == 1);
    CHECK(p.stage_bytes <= stage_round(p.digest_dev - stage + p.digest_bytes));
    // with digests everything pageable is staged: in = slot, no copy-through, out = slot, no second store
    for (size_t i = 0; i < l.size(); ++i)
        for (int c = 0; c < k; ++c) CHECK(p.desc[i].in[c] >= stage && p.desc[i].copy[c] == 0);
}

void test_split() {
    const int k = 2, m = 1, t = 3;
    const uint64_t stage = 32u << 20;
    std::vector<Blk> v;
    uint64_t base = 0x10000000;
    // 3 MiB per block staged; the fifth block alone is over the stage
    const uint64_t lens[] = {1 << 20, 1 << 20, 5 << 20, 1 << 20, 12 << 20, 1 << 20, 9 << 20, 9 << 20, 1};
    for (uint64_t len : lens) {
        v.push_back(packed(t, base, len, base + 0x3000000));
        base += 0x4000000;
    }
    auto l = list(v);
    for (int want = 0; want < 2; ++want) {
        std::vector<SubBatch> subs;
        split(k, m, l.size(), l.data(), want != 0, stage, subs);
        size_t next = 0;
        for (const SubBatch& s : subs) {
            CHECK(s.first == next && s.count >= 1);
            next += s.count;
            uint64_t bytes = 0;
            for (size_t i = s.first; i < s.first + s.count; ++i) bytes += block_stage_bytes(k, m, l[i], want != 0);
            if (s.alone) {
                CHECK(s.count == 1 && bytes + 256 > stage);
            } else {
                CHECK(bytes + 256 <= stage);
                // what the plan lays out fits what the split allowed
                BatchPlan p;
                plan_batch(k, m, s.count, l.data() + s.first, want != 0, nullptr, nullptr, 0x7000000000ull, p);
                CHECK(p.stage_bytes <= stage);
                CHECK(table_layout(p).bytes <= table_bytes_max(k, m));
            }
        }
        CHECK(next == l.size());
        CHECK(subs.size() == 4);  // MiB staged: 3+3+15+3 | 36 alone | 3+27 | 27 + a few bytes
        CHECK(subs[1].alone && subs[1].first == 4 && !subs[0].alone && subs[0].count == 4);
    }
    {  // the block-count cap
        std::vector<Blk> w;
        for (size_t i = 0; i < kMaxBatchBlocks + 3; ++i) w.push_back(packed(t, 0x10000000 + 64 * i, 5));
        auto lw = list(w);
        std::vector<SubBatch> subs;
        split(k, m, lw.size(), lw.data(), false, stage, subs);
        CHECK(subs.size() == 2 && subs[0].count == kMaxBatchBlocks && subs[1].first == kMaxBatchBlocks && subs[1].count == 3);
    }
}

// The copies and launches per sub-batch, as DESIGN.md states them:
//   H2D     1 (the tables) + one per run of pageable data shards contiguous in host memory
//   D2H     one per run of pageable parity shards + 1 if any digest buffer is pageable
//   launch  1 encode + 1 hash if any block has digests
void test_counts() {
    const int k = 4, m = 2, t = 6;
    const uint64_t len = 1000, stage = 0x7000000000ull, pin = 0x6000000000ull;
    for (int dig = 0; dig < 2; ++dig) {
        // three blocks: packed, packed, and one with every shard on its own
        std::vector<Blk> v{packed(t, 0x100000, len, dig ? 0x180000 : 0), packed(t, 0x200000, len, dig ? 0x280000 : 0),
                           spread(t, 0x300000, len, 24, dig ? 0x380000 : 0)};
        auto l = list(v);
        CHECK(validate(k, m, 3, l.data(), dig != 0) == kOk);
        std::vector<uint64_t> view(3 * t, 0), dview(3, 0);
        BatchPlan p;
        // all pageable
        plan_batch(k, m, 3, l.data(), dig != 0, view.data(), dview.data(), stage, p);
        CHECK(p.h2d == 1 + 1 + 1 + 4 && p.d2h == 1u + 1 + 2 + (dig ? 1 : 0) && p.launches == 1u + (dig ? 1 : 0));
        uint64_t up = 0, down = 0;
        for (const Copy& c : p.up) up += c.bytes;
        for (const Copy& c : p.down) down += c.bytes;
        CHECK(up == 3 * k * len && down == 3 * m * len);  // every byte once
        // all page-locked (shards and digests)
        for (size_t i = 0; i < 3; ++i) {
            for (int s = 0; s < t; ++s) view[i * t + s] = pin + (uint64_t)(uintptr_t)l[i].shards[s];
            dview[i] = dig ? pin + (uint64_t)(uintptr_t)l[i].digests : 0;
        }
        plan_batch(k, m, 3, l.data(), dig != 0, view.data(), dview.data(), stage, p);
        CHECK(p.h2d == 1 && p.d2h == 0 && p.launches == 1u + (dig ? 1 : 0) && p.up.empty() && p.down.empty());
        CHECK(p.digest_bytes == 0 && p.moves.empty());
        for (size_t i = 0; i < 3; ++i) {
            for (int c = 0; c < k; ++c) {
                CHECK(p.desc[i].in[c] == view[i * t + c]);                        // read in place
                CHECK(dig ? p.desc[i].copy[c] >= stage : p.desc[i].copy[c] == 0);  // copied through for the hash
            }
            for (int r = 0; r < m; ++r) {
                if (dig) CHECK(p.desc[i].out[r] >= stage && p.desc[i].out2[r] == view[i * t + k + r]);
                else CHECK(p.desc[i].out[r] == view[i * t + k + r] && p.desc[i].out2[r] == 0);
            }
        }
        CHECK(dig ? p.stage_bytes >= 3 * t * len : p.stage_bytes == 0);
        // page-locked shards, pageable digests: the digest area comes back in one copy
        if (dig) {
            std::vector<uint64_t> none(3, 0);
            plan_batch(k, m, 3, l.data(), true, view.data(), none.data(), stage, p);
            CHECK(p.h2d == 1 && p.d2h == 1 && p.launches == 2 && p.moves.size() == 3);
        }
        // mixed: block 0 page-locked, block 1 pageable, block 2 data page-locked and parity pageable
        for (int s = 0; s < t; ++s) view[1 * t + s] = 0;
        for (int s = k; s < t; ++s) view[2 * t + s] = 0;
        dview[1] = 0;
        plan_batch(k, m, 3, l.data(), dig != 0, view.data(), dview.data(), stage, p);
        CHECK(p.h2d == 1 + 1 && p.d2h == 1u + 2 + (dig ? 1 : 0) && p.launches == 1u + (dig ? 1 : 0));
    }
}

}  // namespace

int main() {
    test_validation();
    test_tiles();
    test_units();
    test_split();
    test_counts();
    printf("blocks plan ok\n");
    return 0;
}
