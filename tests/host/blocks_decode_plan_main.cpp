// blocks_decode_plan_main.cpp — the gathered block reconstruct's host planner
// (rustfs_amd/csrc/rs_blocks_decode_plan.h) on a CPU: validation, survivors,
// targets, patterns, descriptor and tile tables, the hash-unit table,
// sub-batch splits, and the copy / launch / wait counts DESIGN.md states.
// Stand-alone (its own main); tests/test_blocks_decode_plan.py builds it with
// the host compiler under AddressSanitizer + UBSan and runs it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "../../rustfs_amd/csrc/rs_blocks_decode_plan.h"

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
uint64_t addr(const void* p) { return (uint64_t)(uintptr_t)p; }

// One block's pointer list and present bytes, kept alive next to the RBlock
// that points at them.  The shard, digest and bad addresses are never
// dereferenced by the planner; the present bytes are.
struct Blk {
    std::vector<uint8_t*> ptr;
    std::vector<uint8_t> present;
    RBlock b;
};

// shards `gap` bytes apart at `base` (gap 0: back to back), all present
Blk make(int t, uint64_t base, uint64_t len, uint64_t gap = 0, uint64_t digests = 0, uint64_t bad = 0) {
    Blk x;
    for (int s = 0; s < t; ++s) x.ptr.push_back(at(base + (uint64_t)s * (len + gap)));
    x.present.assign((size_t)t, 1);
    x.b = RBlock{nullptr, len, nullptr, digests ? at(digests) : nullptr, bad ? at(bad) : nullptr};
    return x;
}
void set_mask(Blk& x, uint32_t mask) {
    for (size_t s = 0; s < x.present.size(); ++s) x.present[s] = (mask >> s & 1u) ? 7 : 0;  // any non-zero byte is "present"
}
std::vector<RBlock> list(std::vector<Blk>& v) {
    std::vector<RBlock> out;
    for (Blk& x : v) {
        x.b.shards = x.ptr.data();
        x.b.present = x.present.data();
        out.push_back(x.b);
    }
    return out;
}
int popcount(uint32_t x) {
    int c = 0;
    for (; x; x &= x - 1) ++c;
    return c;
}

void test_validation() {
    const int k = 4, m = 2, t = 6;
    {
        std::vector<Blk> v{make(t, 0x100000, 100), make(t, 0x200000, 33, 7, 0x300000, 0x310000)};
        auto l = list(v);
        CHECK(validate_r(k, m, l.size(), l.data(), kModeData, 1, true) == kROk);
        CHECK(validate_r(k, m, 0, nullptr, kModeData, 1, true) == kROk);
        CHECK(validate_r(k, m, 2, nullptr, kModeData, 1, true) == kRInvalid);
        for (int mode : {-1, 3}) CHECK(validate_r(k, m, l.size(), l.data(), mode, 1, true) == kRInvalid);
        for (int algo : {-1, 3}) CHECK(validate_r(k, m, l.size(), l.data(), kModeData, algo, true) == kRInvalid);
        for (int mode : {kModeData, kModeMissing, kModeReencode})
            for (int algo : {0, 1, 2}) CHECK(validate_r(k, m, l.size(), l.data(), mode, algo, true) == kROk);
        // no status array: fine only while no block is verified
        CHECK(validate_r(k, m, l.size(), l.data(), kModeData, 1, false) == kRInvalid);
        CHECK(validate_r(k, m, l.size(), l.data(), kModeData, 0, false) == kROk);
        CHECK(validate_r(k, m, 1, l.data(), kModeData, 1, false) == kROk);  // block 0 has no digests
        auto l2 = l;
        l2[1].shards = nullptr;
        CHECK(validate_r(k, m, l2.size(), l2.data(), kModeData, 0, true) == kRInvalid);
        l2 = l;
        l2[1].present = nullptr;
        CHECK(validate_r(k, m, l2.size(), l2.data(), kModeData, 0, true) == kRInvalid);
    }
    for (int s = 0; s < t; ++s) {  // a null shard pointer, present or not
        std::vector<Blk> v{make(t, 0x100000, 100), make(t, 0x200000, 100)};
        v[1].ptr[(size_t)s] = nullptr;
        v[1].present[(size_t)s] = 0;
        auto l = list(v);
        CHECK(validate_r(k, m, l.size(), l.data(), kModeData, 0, true) == kRInvalid);
    }
    {
        std::vector<Blk> v{make(t, 0x100000, 100), make(t, 0x200000, 0)};
        auto l = list(v);
        CHECK(validate_r(k, m, l.size(), l.data(), kModeData, 0, true) == kREmpty);
        l[1].shard_len = kMaxLen + 1;
        CHECK(validate_r(k, m, l.size(), l.data(), kModeData, 0, true) == kRInvalid);
        std::vector<Blk> w{make(t, 0x100000, 100), make(t, 0x200000, kMaxLen)};  // the largest length
        auto lw = list(w);
        CHECK(validate_r(k, m, lw.size(), lw.data(), kModeData, 0, true) == kROk);
    }
    {  // a range that wraps the address space
        std::vector<Blk> v{make(t, 0x100000, 100)};
        v[0].ptr[5] = at(UINT64_MAX - 50);
        auto l = list(v);
        CHECK(validate_r(k, m, l.size(), l.data(), kModeData, 0, true) == kRInvalid);
    }
    {  // fewer than k present in any block fails the call; exactly k is fine
        std::vector<Blk> v{make(t, 0x100000, 100), make(t, 0x200000, 100)};
        set_mask(v[1], 0x0f);
        auto l = list(v);
        CHECK(validate_r(k, m, l.size(), l.data(), kModeData, 0, true) == kROk);
        set_mask(v[1], 0x0e);
        CHECK(validate_r(k, m, l.size(), l.data(), kModeData, 0, true) == kRTooFew);
    }
    // a shard or bad range that meets any other range, in either list order
    for (int order = 0; order < 2; ++order) {
        for (int what = 0; what < 8; ++what) {
            Blk a = make(t, 0x100000, 100, 0, 0x110000, 0x120000), c = make(t, 0x200000, 100, 0, 0x210000, 0x220000);
            bool needs_verify = false, ok = false;
            switch (what) {
                case 0: c.ptr[4] = a.ptr[0] + 99; break;                                  // shard over another block's shard (1 byte)
                case 1: c.ptr[1] = c.ptr[2]; break;                                       // two shards of one block
                case 2: c.b.bad = a.ptr[3] + 99; break;                                   // bad over a shard
                case 3: c.b.bad = a.b.bad + 5; break;                                     // bad over bad (1 byte)
                case 4: c.ptr[0] = at(addr(a.b.digests) + 191); needs_verify = true; break;  // shard over digests (1 byte)
                case 5: c.b.bad = at(addr(c.b.digests) + 40); needs_verify = true; break;    // bad over its own digests
                case 6: c.b.digests = a.b.digests + 32; ok = true; break;                 // digests over digests: only read
                case 7: c.b.digests = a.b.digests; ok = true; break;                      // the same digests twice
            }
            std::vector<Blk> v;
            if (order) { v.push_back(c); v.push_back(a); } else { v.push_back(a); v.push_back(c); }
            auto l = list(v);
            CHECK((validate_r(k, m, l.size(), l.data(), kModeData, 1, true) == kROk) == ok);
            // without an algo the digest pointers do not count
            CHECK((validate_r(k, m, l.size(), l.data(), kModeData, 0, true) == kROk) == (ok || needs_verify));
        }
    }
    {  // ranges that only touch are fine
        Blk a = make(t, 0x100000, 100, 0, 0x100000 + 600, 0x100000 + 600 + 192);
        std::vector<Blk> v{a, make(t, 0x100000 + 600 + 192 + 6, 64)};
        auto l = list(v);
        CHECK(validate_r(k, m, l.size(), l.data(), kModeData, 1, true) == kROk);
    }
}

// Survivors and targets restated by hand for every mask, and the plan's
// entries against them.
void brute(int k, int t, uint32_t mask, int mode, std::vector<int>& surv, std::vector<int>& tg) {
    surv.clear();
    tg.clear();
    for (int s = 0; s < t; ++s)
        if ((mask >> s & 1u) && (int)surv.size() < k) surv.push_back(s);
    std::set<int> in_surv(surv.begin(), surv.end());
    for (int s = 0; s < t; ++s) {
        const bool have = mask >> s & 1u;
        if (s < k) {
            if (!have) tg.push_back(s);
        } else if (mode == kModeMissing) {
            if (!have) tg.push_back(s);
        } else if (mode == kModeReencode) {
            if (!in_surv.count(s)) tg.push_back(s);
        }
    }
}

void test_patterns(int k, int m) {
    const int t = k + m;
    const uint64_t len = 33, pin = 0x6000000000ull, stage = 0x7000000000ull;
    std::vector<uint32_t> masks;
    for (uint32_t mk = 0; mk < (1u << t); ++mk)
        if (popcount(mk) >= k) masks.push_back(mk);
    CHECK(masks.size() == (k == 8 ? 794u : 22u));
    // every mask twice, the second time in reverse order: equal masks far apart
    std::vector<uint32_t> all(masks);
    all.insert(all.end(), masks.rbegin(), masks.rend());
    std::vector<Blk> v;
    for (size_t i = 0; i < all.size(); ++i) {
        v.push_back(make(t, 0x1000000 + 0x1000 * i, len));
        set_mask(v.back(), all[i]);
    }
    auto l = list(v);
    const size_t n = l.size();
    std::vector<uint64_t> view(n * t);
    for (size_t i = 0; i < n; ++i)
        for (int s = 0; s < t; ++s) view[i * t + s] = pin + addr(l[i].shards[s]);
    for (int mode : {kModeData, kModeMissing, kModeReencode}) {
        CHECK(validate_r(k, m, n, l.data(), mode, 0, false) == kROk);
        RLayout L;
        layout_r(k, m, n, l.data(), false, mode, view.data(), stage, L);
        CHECK(L.up.empty() && L.unit.empty() && L.stage_bytes == 0);  // everything addressable: nothing staged
        RPlan p;
        plan_r(k, m, n, l.data(), mode, all.data(), view.data(), L, p);
        CHECK(p.down.empty() && p.pat_mask.size() == masks.size());
        for (size_t i = 0; i < n; ++i)
            for (size_t j = 0; j < n; ++j) CHECK((p.pattern[i] == p.pattern[j]) == (all[i] == all[j]));
        size_t e = 0;
        std::vector<int> surv, tg;
        for (size_t i = 0; i < n; ++i) {
            brute(k, t, all[i], mode, surv, tg);
            CHECK(!p.too_few[i] && p.pattern[i] >= 0 && p.pat_mask[(size_t)p.pattern[i]] == all[i]);
            int s2[kMaxC], t2[kMaxC + kMaxR];
            CHECK(survivors_of(k, t, all[i], s2) == k && targets_of(k, t, all[i], mode, t2) == (int)tg.size());
            for (int c = 0; c < k; ++c) CHECK(s2[c] == surv[(size_t)c]);
            for (size_t r = 0; r < tg.size(); ++r) CHECK(t2[r] == tg[r]);
            CHECK((int)tg.size() <= m);  // a parity shard among the survivors is no target: one entry holds them all
            if (tg.empty()) continue;    // no entry
            CHECK(e < p.desc.size());
            const RDesc& d = p.desc[e++];
            CHECK(d.len == len && d.rows == tg.size() && d.tab == (uint32_t)p.pattern[i] && d.pad == 0);
            for (int c = 0; c < k; ++c) CHECK(d.in[c] == view[i * t + surv[(size_t)c]]);
            for (int c = k; c < kMaxC; ++c) CHECK(d.in[c] == 0);
            for (uint32_t r = 0; r < kMaxR; ++r) CHECK(d.out[r] == (r < d.rows ? view[i * t + tg[r]] : 0));
        }
        CHECK(e == p.desc.size() && p.tile0.size() == e + 1 && p.tile0.back() == e);  // one tile an entry at this length
    }
}

// the kernel's workgroup -> (entry, tile) search and its thread -> unit map
// over every target byte
void test_tiles() {
    const int k = 8, m = 4, t = 12;
    const uint64_t lens[] = {1, kTile - 1, kTile, kTile + 1, 3ull * kTile + 5};
    const uint32_t lost[] = {0xffe, 0x0ff, 0xff6, 0x3fc, 0xfff};  // 1 data; 4 parity; 2 data; 2 data + 2 parity; none
    std::vector<Blk> v;
    uint64_t base = 0x1000000;
    for (size_t i = 0; i < 5; ++i) {
        v.push_back(make(t, base, lens[i]));
        set_mask(v.back(), lost[i]);
        base += 0x100000;
    }
    auto l = list(v);
    const size_t n = l.size();
    const uint64_t stage = 0x7000000000ull;
    for (int mode : {kModeData, kModeMissing, kModeReencode}) {
        RLayout L;
        layout_r(k, m, n, l.data(), false, mode, nullptr, stage, L);
        RPlan p;
        plan_r(k, m, n, l.data(), mode, lost, nullptr, L, p);
        const uint32_t ne = (uint32_t)p.desc.size();
        // coverage per (output address) byte
        std::vector<std::vector<uint8_t>> cover(ne * kMaxR);
        for (uint32_t wg = 0; wg < p.tile0[ne]; ++wg) {
            uint32_t lo = 0, hi = ne;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (p.tile0[mid] <= wg) lo = mid;
                else hi = mid;
            }
            CHECK(p.tile0[lo] <= wg && wg < p.tile0[lo + 1]);
            const uint64_t len = p.desc[lo].len;
            for (uint32_t r = 0; r < p.desc[lo].rows; ++r) cover[lo * kMaxR + r].resize((size_t)len, 0);
            for (uint32_t th = 0; th < 256; ++th) {
                const uint64_t off = (uint64_t)(wg - p.tile0[lo]) * kTile + th * 16u;
                if (off >= len) continue;
                for (uint64_t x = off; x < off + 16 && x < len; ++x)
                    for (uint32_t r = 0; r < p.desc[lo].rows; ++r) ++cover[lo * kMaxR + r][(size_t)x];
            }
        }
        // every target of every block is the output of exactly one (entry, row), covered once
        std::set<uint64_t> outs;
        for (uint32_t e = 0; e < ne; ++e)
            for (uint32_t r = 0; r < p.desc[e].rows; ++r) {
                CHECK(outs.insert(p.desc[e].out[r]).second);
                CHECK(cover[e * kMaxR + r].size() == p.desc[e].len);
                for (uint8_t c : cover[e * kMaxR + r]) CHECK(c == 1);
            }
        size_t want = 0;
        std::vector<int> surv, tg;
        for (size_t i = 0; i < n; ++i) {
            brute(k, t, lost[i], mode, surv, tg);
            want += tg.size();
            for (int s : tg) CHECK(outs.count(L.slot[i * t + (size_t)s]) == 1);  // pageable: rebuilt into its slot
            // a block with no target has no entry, no slot and no copy
            if (tg.empty())
                for (int s = 0; s < t; ++s) CHECK(L.slot[i * t + (size_t)s] == 0);
        }
        CHECK(outs.size() == want);
        uint64_t down = 0;
        for (const Copy& c : p.down) down += c.bytes;
        uint64_t bytes = 0;
        for (uint32_t e = 0; e < ne; ++e) bytes += (uint64_t)p.desc[e].rows * p.desc[e].len;
        CHECK(down == bytes);  // pageable targets: every rebuilt byte comes down once
    }
}

// too few usable shards: status, no entry, no copy down; neighbours unaffected
void test_effective_masks() {
    const int k = 4, m = 2, t = 6;
    const uint64_t stage = 0x7000000000ull;
    std::vector<Blk> v{make(t, 0x100000, 100, 0, 0x180000, 0x190000), make(t, 0x200000, 100, 0, 0x280000, 0x290000),
                       make(t, 0x300000, 100, 0, 0x380000, 0x390000)};
    set_mask(v[1], 0x2f);  // shard 4 absent
    auto l = list(v);
    const uint8_t none[6] = {0, 0, 0, 0, 0, 0}, one[6] = {0, 1, 0, 0, 0, 0}, two[6] = {1, 0, 0, 0, 0, 9};
    CHECK(mask_of(t, l[0].present, nullptr) == 0x3f && mask_of(t, l[0].present, none) == 0x3f);
    CHECK(mask_of(t, l[0].present, one) == 0x3d && mask_of(t, l[1].present, two) == 0x0e);
    const uint8_t bad_absent[6] = {0, 0, 0, 0, 1, 0};  // a bad byte on an absent shard changes nothing
    CHECK(mask_of(t, l[1].present, bad_absent) == 0x2f);
    RLayout L;
    layout_r(k, m, 3, l.data(), true, kModeData, nullptr, stage, L);
    // block 0 loses shard 1 to rot, block 1 shards 0 and 5 (3 usable), block 2 nothing
    const uint32_t mask[3] = {0x3d, 0x0e, 0x3f};
    RPlan p;
    plan_r(k, m, 3, l.data(), kModeData, mask, nullptr, L, p);
    CHECK(!p.too_few[0] && p.too_few[1] && !p.too_few[2] && p.pattern[1] == -1 && p.pattern[0] != p.pattern[2]);
    CHECK(p.desc.size() == 1 && p.desc[0].rows == 1 && p.desc[0].out[0] == L.slot[1]);  // the rotten shard's own slot
    CHECK(p.desc[0].in[0] == L.slot[0] && p.desc[0].in[1] == L.slot[2] && p.desc[0].in[2] == L.slot[3] && p.desc[0].in[3] == L.slot[4]);
    CHECK(p.down.size() == 1 && p.down[0].host == l[0].shards[1] && p.down[0].bytes == 100);
    // MISSING also rebuilds block 0's nothing-else and block 2's nothing: still one entry; a rotten parity
    // shard under DATA is no target
    const uint32_t rotp[3] = {0x1f, 0x2f, 0x3f};
    plan_r(k, m, 3, l.data(), kModeData, rotp, nullptr, L, p);
    CHECK(p.desc.empty() && p.down.empty() && p.launches == 1 && p.waits == 2);
    plan_r(k, m, 3, l.data(), kModeMissing, rotp, nullptr, L, p);
    CHECK(p.desc.size() == 2 && p.desc[0].out[0] == L.slot[5] && p.desc[1].out[0] == L.slot[t + 4]);
}

void test_units() {
    const int k = 3, m = 2, t = 5;
    const uint64_t lens[] = {300, 7, 70000, 300, 1, 4096};
    const uint32_t masks[] = {0x1f, 0x1f, 0x17, 0x0f, 0x1e, 0x1f};
    std::vector<Blk> v;
    uint64_t base = 0x1000000;
    for (size_t i = 0; i < 6; ++i) {
        v.push_back(make(t, base, lens[i], 0, i == 1 ? 0 : base + 0x80000, base + 0x90000));  // block 1: not verified
        set_mask(v.back(), masks[i]);
        base += 0x100000;
    }
    auto l = list(v);
    CHECK(validate_r(k, m, l.size(), l.data(), kModeData, 1, true) == kROk);
    const uint64_t stage = 0x7000000000ull;
    RLayout L;
    layout_r(k, m, l.size(), l.data(), true, kModeData, nullptr, stage, L);
    size_t want = 0;
    for (size_t i = 0; i < 6; ++i)
        if (i != 1) want += (size_t)popcount(masks[i]);
    CHECK(L.unit.size() == want && L.digest_bytes == 32 * want);
    for (size_t j = 1; j < L.unit.size(); ++j) CHECK(L.unit[j - 1].len >= L.unit[j].len);
    // a permutation: every present shard of every verified block once, with its own digest slot
    std::vector<int> seen(want, 0);
    for (const HashUnit& u : L.unit) {
        CHECK(u.pad == 0 && u.out >= L.digest_dev && (u.out - L.digest_dev) % 32 == 0);
        const size_t d = (size_t)((u.out - L.digest_dev) / 32);
        CHECK(d < want);
        ++seen[d];
        CHECK(u.addr >= stage && u.addr + u.len <= L.digest_dev);
        size_t x = 0;
        while (x < L.digest_at.size() && L.digest_at[x] != 32 * d) ++x;
        CHECK(x < L.digest_at.size());
        const size_t i = x / t, s = x % t;
        CHECK(i != 1 && (masks[i] >> s & 1u) && u.addr == L.slot[x] && u.len == lens[i]);
    }
    for (int c : seen) CHECK(c == 1);
    for (size_t x = 0; x < L.digest_at.size(); ++x)
        CHECK((L.digest_at[x] != UINT32_MAX) == (x / t != 1 && (masks[x / t] >> (x % t) & 1u)));
    // slots never overlap and lie inside the stage
    std::vector<std::pair<uint64_t, uint64_t>> r;
    for (size_t x = 0; x < L.slot.size(); ++x)
        if (L.slot[x]) r.push_back({L.slot[x], L.slot[x] + lens[x / t]});
    std::sort(r.begin(), r.end());
    for (size_t j = 1; j < r.size(); ++j) CHECK(r[j - 1].second <= r[j].first);
    CHECK(r.front().first >= stage && r.back().second <= L.digest_dev);
    CHECK(L.stage_bytes == L.digest_dev - stage + stage_round(L.digest_bytes));
}

void test_split() {
    const int k = 2, m = 1, t = 3;
    const uint64_t stage = 32u << 20;
    std::vector<Blk> v;
    uint64_t base = 0x10000000;
    const uint64_t lens[] = {1 << 20, 1 << 20, 5 << 20, 1 << 20, 12 << 20, 1 << 20, 9 << 20, 9 << 20, 1};
    for (uint64_t len : lens) {
        v.push_back(make(t, base, len, 0, base + 0x3000000, base + 0x3100000));
        set_mask(v.back(), 0x6);
        base += 0x4000000;
    }
    auto l = list(v);
    for (int verify = 0; verify < 2; ++verify) {
        std::vector<SubBatch> subs;
        split_r(k, m, l.size(), l.data(), verify != 0, stage, subs);
        size_t next = 0;
        for (const SubBatch& s : subs) {
            CHECK(s.first == next && s.count >= 1);
            next += s.count;
            uint64_t bytes = 0;
            for (size_t i = s.first; i < s.first + s.count; ++i) bytes += rblock_stage_bytes(k, m, l[i], verify != 0);
            if (s.alone) {
                CHECK(s.count == 1 && bytes + 256 > stage);
            } else {
                CHECK(bytes + 256 <= stage);
                // what the plan lays out fits what the split allowed
                for (int mode : {kModeData, kModeReencode}) {
                    RLayout L;
                    layout_r(k, m, s.count, l.data() + s.first, verify != 0, mode, nullptr, 0x7000000000ull, L);
                    CHECK(L.stage_bytes <= stage);
                    std::vector<uint32_t> mask(s.count, 0x6);
                    RPlan p;
                    plan_r(k, m, s.count, l.data() + s.first, mode, mask.data(), nullptr, L, p);
                    CHECK(rtable_layout(k, L, p).bytes <= rtable_bytes_max() && p.tile0.back() <= kMaxBatchTiles);
                }
            }
        }
        CHECK(next == l.size());
        CHECK(subs.size() == 4);  // MiB staged: 3+3+15+3 | 36 alone | 3+27 | 27 + a few bytes
        CHECK(subs[1].alone && subs[1].first == 4 && !subs[0].alone && subs[0].count == 4);
    }
    {  // the block-count cap
        std::vector<Blk> w;
        for (size_t i = 0; i < kMaxBatchBlocks + 3; ++i) w.push_back(make(t, 0x10000000 + 64 * i, 5));
        auto lw = list(w);
        std::vector<SubBatch> subs;
        split_r(k, m, lw.size(), lw.data(), false, stage, subs);
        CHECK(subs.size() == 2 && subs[0].count == kMaxBatchBlocks && subs[1].first == kMaxBatchBlocks && subs[1].count == 3);
    }
}

// The copies, launches and waits per sub-batch, as DESIGN.md states them.
//   unverified  H2D  one per run of pageable survivors + 1 (the tables)
//               D2H  one per run of pageable targets
//               1 launch, 1 wait
//   verified    H2D  1 (the hash units) + one per run of present shards + 1 (the tables)
//               D2H  1 (the digests) + one per run of pageable targets
//               2 launches, 2 waits
void test_counts() {
    const int k = 4, m = 2, t = 6;
    const uint64_t len = 1000, stage = 0x7000000000ull, pin = 0x6000000000ull;
    const uint32_t masks[3] = {0x3c, 0x3c, 0x3c};  // data shards 0 and 1 lost: survivors 2..5
    for (int ver = 0; ver < 2; ++ver) {
        // three blocks: packed, packed, and one with every shard on its own
        std::vector<Blk> v{make(t, 0x100000, len, 0, ver ? 0x180000 : 0), make(t, 0x200000, len, 0, ver ? 0x280000 : 0),
                           make(t, 0x300000, len, 24, ver ? 0x380000 : 0)};
        for (Blk& x : v) set_mask(x, 0x3c);
        auto l = list(v);
        CHECK(validate_r(k, m, 3, l.data(), kModeData, ver, true) == kROk);
        std::vector<uint64_t> view(3 * t, 0);
        RLayout L;
        RPlan p;
        // all pageable: the four survivors of a packed block go up in one copy, its two targets come down in one
        layout_r(k, m, 3, l.data(), ver != 0, kModeData, view.data(), stage, L);
        plan_r(k, m, 3, l.data(), kModeData, masks, view.data(), L, p);
        CHECK(L.up.size() == 1 + 1 + 4 && p.down.size() == 1 + 1 + 2);
        CHECK(p.h2d == 6u + 1 + ver && p.d2h == 4u + ver && p.launches == 1u + ver && p.waits == 1u + ver);
        uint64_t up = 0, down = 0;
        for (const Copy& c : L.up) up += c.bytes;
        for (const Copy& c : p.down) down += c.bytes;
        CHECK(up == 3 * k * len && down == 3 * 2 * len);  // the k survivors only (nothing else is present), every byte once
        // a surplus present shard moves only when the block is verified
        {
            const uint32_t mk5[3] = {0x3e, 0x3e, 0x3e};
            for (Blk& x : v) set_mask(x, 0x3e);
            layout_r(k, m, 3, l.data(), ver != 0, kModeData, view.data(), stage, L);
            plan_r(k, m, 3, l.data(), kModeData, mk5, view.data(), L, p);
            up = 0;
            for (const Copy& c : L.up) up += c.bytes;
            CHECK(up == 3 * (uint64_t)(ver ? 5 : 4) * len);
            for (Blk& x : v) set_mask(x, 0x3c);
        }
        // all page-locked
        for (size_t i = 0; i < 3; ++i)
            for (int s = 0; s < t; ++s) view[i * t + s] = pin + addr(l[i].shards[s]);
        layout_r(k, m, 3, l.data(), ver != 0, kModeData, view.data(), stage, L);
        plan_r(k, m, 3, l.data(), kModeData, masks, view.data(), L, p);
        if (ver) {  // hashed from the stage: present shards go up, targets are written in place
            CHECK(L.up.size() == 6 && p.down.empty() && p.h2d == 8 && p.d2h == 1 && p.launches == 2 && p.waits == 2);
            for (size_t i = 0; i < 3; ++i) {
                for (int c = 0; c < k; ++c) CHECK(p.desc[i].in[c] == L.slot[i * t + 2 + (size_t)c]);
                for (int r = 0; r < 2; ++r) CHECK(p.desc[i].out[r] == view[i * t + (size_t)r]);
            }
        } else {  // read and written in place: the tables are the only copy
            CHECK(L.up.empty() && p.down.empty() && L.stage_bytes == 0 && p.h2d == 1 && p.d2h == 0 && p.launches == 1 && p.waits == 1);
            for (size_t i = 0; i < 3; ++i) {
                for (int c = 0; c < k; ++c) CHECK(p.desc[i].in[c] == view[i * t + 2 + (size_t)c]);
                for (int r = 0; r < 2; ++r) CHECK(p.desc[i].out[r] == view[i * t + (size_t)r]);
            }
        }
        // mixed: block 0 page-locked, block 1 pageable, block 2 survivors page-locked and targets pageable
        for (int s = 0; s < t; ++s) view[1 * t + s] = 0;
        view[2 * t + 0] = view[2 * t + 1] = 0;
        layout_r(k, m, 3, l.data(), ver != 0, kModeData, view.data(), stage, L);
        plan_r(k, m, 3, l.data(), kModeData, masks, view.data(), L, p);
        if (ver) CHECK(L.up.size() == 6 && p.down.size() == 1 + 2 && p.h2d == 8 && p.d2h == 4);
        else CHECK(L.up.size() == 1 && p.down.size() == 1 + 2 && p.h2d == 2 && p.d2h == 3);
        CHECK(p.launches == 1u + ver && p.waits == 1u + ver);
        // nothing to rebuild: no tables, no launch, nothing moves
        if (!ver) {
            const uint32_t full[3] = {0x3f, 0x3f, 0x3f};
            for (Blk& x : v) set_mask(x, 0x3f);
            layout_r(k, m, 3, l.data(), false, kModeMissing, nullptr, stage, L);
            plan_r(k, m, 3, l.data(), kModeMissing, full, nullptr, L, p);
            CHECK(L.up.empty() && p.desc.empty() && p.h2d == 0 && p.d2h == 0 && p.launches == 0 && p.waits == 1);
        }
    }
}

}  // namespace

int main() {
    test_validation();
    test_patterns(4, 2);
    test_patterns(8, 4);
    test_tiles();
    test_effective_masks();
    test_units();
    test_split();
    test_counts();
    printf("blocks decode plan ok\n");
    return 0;
}
