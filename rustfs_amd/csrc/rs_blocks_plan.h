// rs_blocks_plan.h — host planner of the gathered block encode
// (rsg_encode_blocks / rsg_encode_hashed,
// k_encode_blocks and k_hash_blocks in rs_blocks.hip): n unrelated blocks,
// each a list of k+m host pointers as rsg_encode takes them
// (ReedSolomonEncoder::encode once per block, erasure.rs:396-408), encoded and
// optionally hashed (BitrotWriter::write, bitrot.rs:496-502) by one launch
// pair.  Plain C++17, no HIP headers: it compiles and runs on a CPU
// (tests/host/blocks_plan_main.cpp).
//
// The planner validates the caller's blocks, splits a call into sub-batches
// that fit the staging buffer, and lays one sub-batch out: where every shard
// lives on the device, the descriptor, tile and hash-unit tables the kernels
// read, and the list of copies the runner issues.  The counts of copies and
// launches of a sub-batch are the plan's (BatchPlan::h2d / d2h / launches).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace rsg {
namespace blocks {

// Bytes of one shard that one workgroup of k_encode_blocks handles: 256
// threads, one 16-byte unit each.
constexpr uint32_t kTile = 4096;
constexpr int kMaxC = 16, kMaxR = 4;           // the kernels' geometries: k = 1..16, m = 1..4
constexpr uint64_t kMaxLen = 0xffffffffull;    // shard_len the descriptors hold
constexpr size_t kMaxBatchBlocks = 4096;       // blocks per sub-batch (bounds the tables)
constexpr uint64_t kMaxBatchTiles = 1u << 22;  // workgroups per launch

constexpr bool kernel_geometry(int k, int m) { return k >= 1 && k <= kMaxC && m >= 1 && m <= kMaxR; }

// The caller's block (rsg_block, include/rsgpu.h).
struct Block {
    uint8_t* const* shards;  // k+m host pointers, k data then m parity
    uint64_t shard_len;
    uint8_t* digests;  // (k+m)*32 bytes in shard order, or null
};

// What k_encode_blocks reads per block (device addresses).  in[c]: data shard
// c; copy[c]: where the pass also stores it verbatim (0: nowhere); out[r]:
// parity shard r; out2[r]: its second destination (0: none).
struct BlockDesc {
    uint64_t in[kMaxC], copy[kMaxC], out[kMaxR], out2[kMaxR];
    uint32_t len, pad;
};

// What k_hash_blocks reads per quad: the message and where its 32 digest
// bytes go (device addresses).
struct HashUnit {
    uint64_t addr, out;
    uint32_t len, pad;
};

enum Verdict { kOk = 0, kInvalid, kEmpty };

constexpr uint64_t stage_round(uint64_t b) { return (b + 255u) & ~(uint64_t)255u; }
inline uint32_t tiles_of(uint64_t len) { return (uint32_t)((len + kTile - 1) / kTile); }

// Validation, all or nothing.  Rejects a null block list, shard list or shard
// pointer (kInvalid), shard_len == 0 (kEmpty, rsg_encode's EmptyShard),
// shard_len above kMaxLen or a range that wraps the address space (kInvalid),
// and a parity or digest range that meets any other shard or digest range of
// the call (kInvalid).  Data ranges may overlap each other: they are only
// read.  want_digests: the digests pointers count (an algo other than NONE).
inline Verdict validate(int k, int m, size_t n, const Block* b, bool want_digests) {
    if (n && !b) return kInvalid;
    for (size_t i = 0; i < n; ++i) {
        if (!b[i].shards) return kInvalid;
        for (int s = 0; s < k + m; ++s)
            if (!b[i].shards[s]) return kInvalid;
    }
    struct Range {
        uint64_t lo, hi;
        bool written;
    };
    std::vector<Range> r;
    r.reserve(n * (size_t)(k + m + 1));
    for (size_t i = 0; i < n; ++i) {
        const uint64_t len = b[i].shard_len;
        if (len == 0) return kEmpty;
        if (len > kMaxLen) return kInvalid;
        for (int s = 0; s < k + m; ++s) {
            const uint64_t a = (uint64_t)(uintptr_t)b[i].shards[s];
            if (a > UINT64_MAX - len) return kInvalid;
            r.push_back(Range{a, a + len, s >= k});
        }
        if (want_digests && b[i].digests) {
            const uint64_t a = (uint64_t)(uintptr_t)b[i].digests, dl = (uint64_t)(k + m) * 32u;
            if (a > UINT64_MAX - dl) return kInvalid;
            r.push_back(Range{a, a + dl, true});
        }
    }
    // by start: a range collides if it starts below the furthest end of the
    // written ranges before it, or is written and starts below any end before it
    std::sort(r.begin(), r.end(), [](const Range& x, const Range& y) { return x.lo < y.lo; });
    uint64_t end_any = 0, end_written = 0;
    for (const Range& x : r) {
        if (x.lo < end_written || (x.written && x.lo < end_any)) return kInvalid;
        end_any = std::max(end_any, x.hi);
        if (x.written) end_written = std::max(end_written, x.hi);
    }
    return kOk;
}

// Staging bytes of one block when every shard is staged: the split's bound
// (which shards the device can address is known only to the runner; a block
// with digests is staged whole anyway).  Slots start 16-byte aligned, a
// block's slots 256-byte aligned.
inline uint64_t block_stage_bytes(int k, int m, const Block& b, bool want_digests) {
    return stage_round((uint64_t)(k + m) * ((b.shard_len + 15u) & ~(uint64_t)15u)) +
           (want_digests && b.digests ? (uint64_t)(k + m) * 32u : 0);
}

// A run of consecutive blocks run as one launch pair; alone: one block larger
// than the stage, which goes through the per-block path.
struct SubBatch {
    size_t first, count;
    bool alone;
};

// Split a validated list into sub-batches of at most `stage` staging bytes
// (digest area rounded as a whole), kMaxBatchBlocks blocks and kMaxBatchTiles
// tiles.  Covers every block once, in order.
inline void split(int k, int m, size_t n, const Block* b, bool want_digests, uint64_t stage, std::vector<SubBatch>& out) {
    out.clear();
    size_t i = 0;
    while (i < n) {
        if (block_stage_bytes(k, m, b[i], want_digests) + 256u > stage) {
            out.push_back(SubBatch{i++, 1, true});
            continue;
        }
        SubBatch s{i, 0, false};
        uint64_t bytes = 256, tiles = 0;  // 256: the digest area's rounding
        while (i < n && s.count < kMaxBatchBlocks) {
            const uint64_t add = block_stage_bytes(k, m, b[i], want_digests);
            if (bytes + add > stage || tiles + tiles_of(b[i].shard_len) > kMaxBatchTiles) break;
            bytes += add;
            tiles += tiles_of(b[i].shard_len);
            ++s.count;
            ++i;
        }
        out.push_back(s);
    }
}

// One host <-> device copy of the runner.
struct Copy {
    uint8_t* host;
    uint64_t dev;  // device address, inside the staging buffer
    uint64_t bytes;
};

// A digest the runner moves from the page-locked mirror of the staged digest
// area to the caller's buffer after the one copy back.
struct DigestMove {
    uint8_t* host;
    uint64_t off;  // in the digest area
};

// The layout of one sub-batch.
struct BatchPlan {
    std::vector<BlockDesc> desc;
    std::vector<uint32_t> tile0;  // tile0[i]: first workgroup of block i; tile0[n]: the grid
    std::vector<HashUnit> unit;   // kernel order: non-increasing length
    std::vector<Copy> up, down;   // H2D before the launches, D2H after them
    std::vector<DigestMove> moves;
    uint64_t digest_dev = 0, digest_bytes = 0;  // the staged digest area (0 bytes: none)
    uint64_t stage_bytes = 0;                   // shards + digest area
    // copies per direction (the one table upload included) and launches
    uint32_t h2d = 0, d2h = 0, launches = 0;
};

// Lay blocks b[0..n) out in the staging buffer at device address `stage`.
// view[i*(k+m) + s]: the device's view of shard s of block i, 0 when the
// device cannot address it (pageable memory); dview[i]: likewise for block i's
// digest buffer.  Both may be null (everything pageable).
//
// Without digests a shard the device can address is used in place and only
// the others get a stage slot.  With digests every shard of the block gets a
// slot, because the hash pass reads device memory: a pageable data shard is
// copied up, an addressable one is read in place by the encode pass, which
// also stores it into its slot (copy); parity is computed into its slot and,
// where the device can address the caller's buffer, stored there by the same
// pass (out2), else copied down.  So every data byte and every parity byte
// crosses the link once.  Consecutive pageable shards of one block that are
// contiguous in host memory share one copy (never data with parity: they move
// in opposite directions).  A digest goes straight into an addressable digest
// buffer, the others into the staged digest area, which comes back in one
// copy.
inline void plan_batch(int k, int m, size_t n, const Block* b, bool want_digests, const uint64_t* view,
                       const uint64_t* dview, uint64_t stage, BatchPlan& p) {
    p = BatchPlan{};
    p.desc.resize(n);
    p.tile0.resize(n + 1);
    const int t = k + m;
    uint64_t at = 0;  // stage offset
    uint32_t tiles = 0;
    bool any_hash = false;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t len = b[i].shard_len;
        const bool hashed = want_digests && b[i].digests;
        BlockDesc& d = p.desc[i];
        d = BlockDesc{};
        d.len = (uint32_t)len;
        p.tile0[i] = tiles;
        tiles += tiles_of(len);
        Copy* run = nullptr;  // the copy the previous shard ended, if a pageable neighbour may extend it
        uint64_t slot_of[kMaxC + kMaxR] = {};
        for (int s = 0; s < t; ++s) {
            const uint64_t v = view ? view[i * (size_t)t + s] : 0;
            const bool parity = s >= k;
            if (s == k) run = nullptr;
            uint64_t slot = 0;
            if (hashed || !v) {
                const bool joins = !v && run && run->host + run->bytes == b[i].shards[s];
                if (!joins) at = (at + 15u) & ~(uint64_t)15u;
                slot = stage + at;
                at += len;
                if (!v) {
                    if (joins) {
                        run->bytes += len;
                    } else {
                        std::vector<Copy>& cp = parity ? p.down : p.up;
                        cp.push_back(Copy{b[i].shards[s], slot, len});
                        run = &cp.back();
                    }
                } else {
                    run = nullptr;
                }
            } else {
                run = nullptr;
            }
            slot_of[s] = slot;
            if (!parity) {
                d.in[s] = v ? v : slot;
                d.copy[s] = v ? slot : 0;  // 0 when not hashed
            } else {
                d.out[s - k] = slot ? slot : v;
                d.out2[s - k] = slot ? v : 0;
            }
        }
        at = stage_round(at);
        if (hashed) {
            any_hash = true;
            const uint64_t dv = dview ? dview[i] : 0;
            for (int s = 0; s < t; ++s)  // pad = 1: out is an offset into the digest area (fixed below)
                p.unit.push_back(HashUnit{slot_of[s], (dv ? dv : p.digest_bytes) + 32u * (uint64_t)s, (uint32_t)len, dv ? 0u : 1u});
            if (!dv) {
                p.moves.push_back(DigestMove{b[i].digests, p.digest_bytes});
                p.digest_bytes += 32u * (uint64_t)t;
            }
        }
    }
    p.tile0[n] = tiles;
    p.digest_dev = stage + at;
    p.stage_bytes = at + stage_round(p.digest_bytes);
    for (HashUnit& u : p.unit)
        if (u.pad) {
            u.out += p.digest_dev;
            u.pad = 0;
        }
    std::stable_sort(p.unit.begin(), p.unit.end(), [](const HashUnit& x, const HashUnit& y) { return x.len > y.len; });
    p.h2d = 1u + (uint32_t)p.up.size();  // the tables, then the pageable data runs
    p.d2h = (uint32_t)p.down.size() + (p.digest_bytes ? 1u : 0u);
    p.launches = 1u + (any_hash ? 1u : 0u);
}

// The tables as the runner uploads them, one blob: [desc][tile0][unit], each
// region 256-byte aligned.
struct TableLayout {
    uint64_t desc_off, tile_off, unit_off, bytes;
};
inline TableLayout table_layout(const BatchPlan& p) {
    TableLayout l;
    l.desc_off = 0;
    l.tile_off = stage_round(p.desc.size() * sizeof(BlockDesc));
    l.unit_off = l.tile_off + stage_round(p.tile0.size() * sizeof(uint32_t));
    l.bytes = l.unit_off + stage_round(p.unit.size() * sizeof(HashUnit));
    return l;
}
// The most table bytes a sub-batch of geometry (k, m) needs.
constexpr uint64_t table_bytes_max(int k, int m) {
    return stage_round(kMaxBatchBlocks * sizeof(BlockDesc)) + stage_round((kMaxBatchBlocks + 1) * sizeof(uint32_t)) +
           stage_round(kMaxBatchBlocks * (uint64_t)(k + m) * sizeof(HashUnit));
}

}  // namespace blocks
}  // namespace rsg
