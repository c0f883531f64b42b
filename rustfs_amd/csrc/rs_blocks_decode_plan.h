// rs_blocks_decode_plan.h — host planner of the gathered block reconstruct
// (rsg_reconstruct_blocks, k_reconstruct_blocks in rs_blocks_decode.hip): n
// unrelated degraded blocks, each the k+m host pointers rsg_reconstruct takes
// with its own present set, length and alignment, optionally checked against
// their expected digests first (BitrotReader::read, bitrot.rs:139-244) and
// rebuilt (ReedSolomonEncoder::reconstruct_data / reconstruct,
// erasure.rs:411-428) by one launch whatever the mix of loss patterns.  Plain
// C++17, no HIP headers: it compiles and runs on a CPU
// (tests/host/blocks_decode_plan_main.cpp).
//
// A sub-batch is planned in two steps, because with verification the loss
// patterns are known only after the hash pass:
//   layout_r  where every shard the passes touch lives on the device, the
//             copies up and the hash-unit table;
//   plan_r    from the effective present sets (present and not found rotten):
//             per-block status, pattern ids, the descriptor and tile tables
//             of the one reconstruct launch, and the copies down.
// The descriptor entry has no second destination per output (k_encode_blocks'
// out2): the hash pass runs before the rebuild and reads only shards that
// were read, so no rebuilt shard is needed in two places.
#pragma once

#include <map>

#include "rs_blocks_plan.h"

namespace rsg {
namespace blocks {

// The caller's block (rsg_rblock, include/rsgpu.h).
struct RBlock {
    uint8_t* const* shards;  // k+m host pointers, every one a shard_len buffer
    uint64_t shard_len;
    const uint8_t* present;  // k+m bytes
    const uint8_t* digests;  // expected (k+m)*32 bytes, or null
    uint8_t* bad;            // k+m bytes out, or null
};

// rsg_reconstruct_mode
constexpr int kModeData = 0, kModeMissing = 1, kModeReencode = 2;

enum RVerdict { kROk = 0, kRInvalid, kREmpty, kRTooFew };

// The block is hashed before it is rebuilt.
inline bool verified(const RBlock& b, bool verify) { return verify && b.digests; }

// Validation, all or nothing, in this order: null pointers, mode and algo
// (0..2) out of range and a missing status array (kRInvalid); shard_len 0
// (kREmpty) or above kMaxLen, or a range that wraps (kRInvalid); fewer than k
// present (kRTooFew); then overlaps (kRInvalid): every shard and `bad` range
// is written or may be, so it must meet no other range; digest ranges (which
// count only where the block is verified) are only read and may meet each
// other.
inline RVerdict validate_r(int k, int m, size_t n, const RBlock* b, int mode, int algo, bool have_status) {
    const int t = k + m;
    if (n && !b) return kRInvalid;
    if (mode < kModeData || mode > kModeReencode || algo < 0 || algo > 2) return kRInvalid;
    for (size_t i = 0; i < n; ++i) {
        if (!b[i].shards || !b[i].present) return kRInvalid;
        for (int s = 0; s < t; ++s)
            if (!b[i].shards[s]) return kRInvalid;
        if (verified(b[i], algo != 0) && !have_status) return kRInvalid;
    }
    struct Range {
        uint64_t lo, hi;
        bool written;
    };
    std::vector<Range> r;
    r.reserve(n * (size_t)(t + 2));
    auto add = [&r](const void* p, uint64_t len, bool written) {
        const uint64_t a = (uint64_t)(uintptr_t)p;
        if (a > UINT64_MAX - len) return false;
        r.push_back(Range{a, a + len, written});
        return true;
    };
    for (size_t i = 0; i < n; ++i) {
        const uint64_t len = b[i].shard_len;
        if (len == 0) return kREmpty;
        if (len > kMaxLen) return kRInvalid;
        for (int s = 0; s < t; ++s)
            if (!add(b[i].shards[s], len, true)) return kRInvalid;
        if (b[i].bad && !add(b[i].bad, (uint64_t)t, true)) return kRInvalid;
        if (verified(b[i], algo != 0) && !add(b[i].digests, (uint64_t)t * 32u, false)) return kRInvalid;
    }
    for (size_t i = 0; i < n; ++i) {
        int np = 0;
        for (int s = 0; s < t; ++s) np += b[i].present[s] ? 1 : 0;
        if (np < k) return kRTooFew;
    }
    std::sort(r.begin(), r.end(), [](const Range& x, const Range& y) { return x.lo < y.lo; });
    uint64_t end_any = 0, end_written = 0;
    for (const Range& x : r) {
        if (x.lo < end_written || (x.written && x.lo < end_any)) return kRInvalid;
        end_any = std::max(end_any, x.hi);
        if (x.written) end_written = std::max(end_written, x.hi);
    }
    return kROk;
}

// Staging bytes of one block when every shard is staged (the split's bound),
// as block_stage_bytes: a verified block's digests come back through the stage.
inline uint64_t rblock_stage_bytes(int k, int m, const RBlock& b, bool verify) {
    return stage_round((uint64_t)(k + m) * ((b.shard_len + 15u) & ~(uint64_t)15u)) +
           (verified(b, verify) ? (uint64_t)(k + m) * 32u : 0);
}

// split()'s rule over degraded blocks: sub-batches of at most `stage` staging
// bytes, kMaxBatchBlocks blocks and kMaxBatchTiles tiles; a block larger than
// the stage goes alone.
inline void split_r(int k, int m, size_t n, const RBlock* b, bool verify, uint64_t stage, std::vector<SubBatch>& out) {
    out.clear();
    size_t i = 0;
    while (i < n) {
        if (rblock_stage_bytes(k, m, b[i], verify) + 256u > stage) {
            out.push_back(SubBatch{i++, 1, true});
            continue;
        }
        SubBatch s{i, 0, false};
        uint64_t bytes = 256, tiles = 0;
        while (i < n && s.count < kMaxBatchBlocks) {
            const uint64_t add = rblock_stage_bytes(k, m, b[i], verify), tl = tiles_of(b[i].shard_len);
            if (bytes + add > stage || tiles + tl > kMaxBatchTiles) break;
            bytes += add;
            tiles += tl;
            ++s.count;
            ++i;
        }
        out.push_back(s);
    }
}

// A block's usable shards as a bit mask (k+m <= 20): present and not rotten.
inline uint32_t mask_of(int t, const uint8_t* present, const uint8_t* bad) {
    uint32_t mk = 0;
    for (int s = 0; s < t; ++s)
        if (present[s] && !(bad && bad[s])) mk |= 1u << s;
    return mk;
}

// The first k usable shards in ascending order (DecodePlan::survivors);
// returns how many there are (k, or fewer: the block cannot be rebuilt).
inline int survivors_of(int k, int t, uint32_t mask, int* out) {
    int c = 0;
    for (int s = 0; s < t && c < k; ++s)
        if (mask >> s & 1u) out[c++] = s;
    return c;
}

// The shards a reconstruct in `mode` writes, ascending (reconstruct_targets):
// every unusable data shard; unusable parity under MISSING; under
// REENCODE_PARITY every parity shard that is no survivor.  `mask` has at
// least k bits.  Never more than m shards: each lost data shard makes one
// more parity shard a survivor, which re-encodes to itself and is no target.
// So for m <= kMaxR one descriptor entry holds all of a block's targets.
inline int targets_of(int k, int t, uint32_t mask, int mode, int* out) {
    int surv[kMaxC], c = 0;
    const int ns = survivors_of(k, t, mask, surv);
    uint32_t smask = 0;
    for (int i = 0; i < ns; ++i) smask |= 1u << surv[i];
    for (int s = 0; s < t; ++s) {
        const bool usable = mask >> s & 1u;
        if (s < k ? !usable : (mode == kModeMissing ? !usable : mode == kModeReencode && !(smask >> s & 1u))) out[c++] = s;
    }
    return c;
}

// What k_reconstruct_blocks reads per entry, one block with something to
// rebuild (device addresses): the k survivors, its 1..m outputs, and which
// coefficient table they use.
struct RDesc {
    uint64_t in[kMaxC], out[kMaxR];
    uint32_t len, rows;  // rows: 1..kMaxR
    uint32_t tab, pad;   // tab: the block's pattern, table [kMaxR][k][5] number `tab` of the launch's table area
};

// Step 1: the stage.
struct RLayout {
    std::vector<uint64_t> slot;       // [i*(k+m)+s]: the shard's stage slot (device address), 0: none
    std::vector<uint32_t> digest_at;  // [i*(k+m)+s]: where the computed digest lands in the digest area, UINT32_MAX: not hashed
    std::vector<Copy> up;
    std::vector<HashUnit> unit;       // kernel order: non-increasing length
    uint64_t digest_dev = 0, digest_bytes = 0, stage_bytes = 0;
};

// a copy that continues the previous one in host and device memory extends it
inline void push_copy(std::vector<Copy>& v, uint8_t* host, uint64_t dev, uint64_t bytes) {
    if (!v.empty() && v.back().host + v.back().bytes == host && v.back().dev + v.back().bytes == dev) v.back().bytes += bytes;
    else v.push_back(Copy{host, dev, bytes});
}

// Lay blocks b[0..n) out in the staging buffer at device address `stage`.
// view[i*(k+m)+s]: the device's view of the shard, 0 when it cannot address it;
// may be null (everything pageable).
//
// A verified block gets a slot for every shard, and every present shard is
// copied into its slot whether the device could address it or not: the hash
// pass reads device memory, and both passes then read the slots, so each byte
// crosses the link once.  An unverified block gets slots only for what must
// move: the k survivors and the targets the device cannot address (none at
// all when it has nothing to rebuild); only survivors are copied up.  A shard
// that follows its neighbour in host memory follows it in the stage too, so
// that runs move with one copy; other slots start 16-byte aligned, a block's
// slots 256-byte aligned.
inline void layout_r(int k, int m, size_t n, const RBlock* b, bool verify, int mode, const uint64_t* view, uint64_t stage,
                     RLayout& L) {
    L = RLayout{};
    const int t = k + m;
    L.slot.assign(n * (size_t)t, 0);
    L.digest_at.assign(n * (size_t)t, UINT32_MAX);
    uint64_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t len = b[i].shard_len;
        const bool ver = verified(b[i], verify);
        uint32_t moves = 0, ups = 0;  // shards that need a slot, shards copied up
        if (ver) {
            moves = (1u << t) - 1u;
            ups = mask_of(t, b[i].present, nullptr);
        } else {
            const uint32_t mk = mask_of(t, b[i].present, nullptr);
            int surv[kMaxC], tg[kMaxC + kMaxR];
            const int ns = survivors_of(k, t, mk, surv), nt = targets_of(k, t, mk, mode, tg);
            for (int j = 0; j < ns && nt; ++j) ups |= 1u << surv[j];
            moves = ups;
            for (int j = 0; j < nt; ++j) moves |= 1u << tg[j];
            for (int s = 0; s < t; ++s)
                if (view && view[i * (size_t)t + s]) {
                    moves &= ~(1u << s);
                    ups &= ~(1u << s);
                }
        }
        for (int s = 0; s < t; ++s) {
            if (!(moves >> s & 1u)) continue;
            const size_t x = i * (size_t)t + s;
            const bool joins = s > 0 && L.slot[x - 1] && L.slot[x - 1] + len == stage + at && b[i].shards[s] == b[i].shards[s - 1] + len;
            if (!joins) at = (at + 15u) & ~(uint64_t)15u;
            L.slot[x] = stage + at;
            at += len;
            if (ups >> s & 1u) push_copy(L.up, b[i].shards[s], L.slot[x], len);
            if (ver && (ups >> s & 1u)) {  // pad = 1: out is an offset into the digest area (fixed below)
                L.digest_at[x] = (uint32_t)L.digest_bytes;
                L.unit.push_back(HashUnit{L.slot[x], L.digest_bytes, (uint32_t)len, 1u});
                L.digest_bytes += 32;
            }
        }
        at = stage_round(at);
    }
    L.digest_dev = stage + at;
    L.stage_bytes = at + stage_round(L.digest_bytes);
    for (HashUnit& u : L.unit) {
        u.out += L.digest_dev;
        u.pad = 0;
    }
    std::stable_sort(L.unit.begin(), L.unit.end(), [](const HashUnit& x, const HashUnit& y) { return x.len > y.len; });
}

// Step 2: the reconstruct launch.
struct RPlan {
    std::vector<int> too_few;        // per block: 1 when fewer than k shards are usable
    std::vector<int32_t> pattern;    // per block: its pattern id, -1 when too_few
    std::vector<uint32_t> pat_mask;  // per pattern: the effective mask
    std::vector<RDesc> desc;         // one entry per block with something to rebuild
    std::vector<uint32_t> tile0;     // desc.size() + 1 prefix sums of the entries' tile counts
    std::vector<Copy> down;
    // per sub-batch, table uploads included
    uint32_t h2d = 0, d2h = 0, launches = 0, waits = 0;
};

// mask[i]: block i's effective present set.  Blocks with equal masks share a
// pattern and its coefficient table (the runner fills table p with the rows
// of pattern p's targets over its survivors).  A block with nothing to
// rebuild or with too few usable shards gets no entry and moves nothing down.
inline void plan_r(int k, int m, size_t n, const RBlock* b, int mode, const uint32_t* mask, const uint64_t* view,
                   const RLayout& L, RPlan& p) {
    p = RPlan{};
    const int t = k + m;
    p.too_few.assign(n, 0);
    p.pattern.assign(n, -1);
    p.tile0.push_back(0);
    std::map<uint32_t, int32_t> ids;
    uint32_t tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        int surv[kMaxC], tg[kMaxC + kMaxR];
        if (survivors_of(k, t, mask[i], surv) < k) {
            p.too_few[i] = 1;
            continue;
        }
        auto it = ids.find(mask[i]);
        if (it == ids.end()) {
            it = ids.emplace(mask[i], (int32_t)p.pat_mask.size()).first;
            p.pat_mask.push_back(mask[i]);
        }
        p.pattern[i] = it->second;
        const int nt = targets_of(k, t, mask[i], mode, tg);  // <= m <= kMaxR
        if (!nt) continue;
        const uint64_t len = b[i].shard_len;
        RDesc d{};
        d.len = (uint32_t)len;
        d.rows = (uint32_t)nt;
        d.tab = (uint32_t)it->second;
        for (int c = 0; c < k; ++c) {
            const size_t x = i * (size_t)t + surv[c];
            d.in[c] = L.slot[x] ? L.slot[x] : view ? view[x] : 0;  // a slot holds what the hash pass saw
        }
        for (int r = 0; r < nt; ++r) {
            const size_t x = i * (size_t)t + tg[r];
            const uint64_t v = view ? view[x] : 0;
            d.out[r] = v ? v : L.slot[x];
            if (!v) push_copy(p.down, b[i].shards[tg[r]], L.slot[x], len);
        }
        p.desc.push_back(d);
        tiles += tiles_of(len);
        p.tile0.push_back(tiles);
    }
    const bool hashed = !L.unit.empty(), any = !p.desc.empty();
    p.h2d = (hashed ? 1u : 0u) + (uint32_t)L.up.size() + (any ? 1u : 0u);  // unit table, shards, launch tables
    p.d2h = (hashed ? 1u : 0u) + (uint32_t)p.down.size();                  // digests, rebuilt shards
    p.launches = (hashed ? 1u : 0u) + (any ? 1u : 0u);
    p.waits = (hashed ? 1u : 0u) + 1u;
}

// The tables as the runner uploads them, one area: [unit] goes up before the
// hash launch; [desc][tile0][tab] before the reconstruct launch.  Each region
// is 256-byte aligned.
struct RTableLayout {
    uint64_t unit_off, desc_off, tile_off, tab_off, bytes;
};
constexpr uint64_t rtab_bytes(int k) { return (uint64_t)kMaxR * (uint64_t)k * 5u * sizeof(uint32_t); }
inline RTableLayout rtable_layout(int k, const RLayout& L, const RPlan& p) {
    RTableLayout l;
    l.unit_off = 0;
    l.desc_off = stage_round(L.unit.size() * sizeof(HashUnit));
    l.tile_off = l.desc_off + stage_round(p.desc.size() * sizeof(RDesc));
    l.tab_off = l.tile_off + stage_round(p.tile0.size() * sizeof(uint32_t));
    l.bytes = l.tab_off + stage_round(p.pat_mask.size() * rtab_bytes(k));
    return l;
}
// The most table bytes a sub-batch needs: every block verified, with an
// entry and a pattern of its own.
constexpr uint64_t rtable_bytes_max() {
    return stage_round(kMaxBatchBlocks * (uint64_t)(kMaxC + kMaxR) * sizeof(HashUnit)) +
           stage_round(kMaxBatchBlocks * sizeof(RDesc)) + stage_round((kMaxBatchBlocks + 1) * sizeof(uint32_t)) +
           stage_round(kMaxBatchBlocks * rtab_bytes(kMaxC));
}

}  // namespace blocks
}  // namespace rsg
