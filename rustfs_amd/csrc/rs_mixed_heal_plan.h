// rs_mixed_heal_plan.h — host planner of the mixed-length batch heal
// (rsg_heal_mixed_dev / _host, k_heal_mixed in rs_mixed_heal.hip): a batch of
// [digest][shard] record stripes, each with its own shard length and its own
// set of present shards, healed into the record arenas of the target shards.
// Plain C++17, no HIP headers: it compiles and runs on a CPU
// (tests/host/mixed_heal_plan_main.cpp).
//
// Shared with the mixed-length GET (rs_mixed_decode_plan.h): the descriptors
// (RecordDesc, whose out_off here is the offset of the stripe's record in every
// target arena; DecDesc), grouping by mask, the kernel order by descending
// chunk count with `job` mapping back, and the redo rule.  Heal-specific: the
// validation of target ranges, the plan of a mask (targets are computed and
// never read) and the sub-batches of the host form.
#pragma once

#include "rs_mixed_decode_plan.h"

namespace rsg {
namespace mixed {

// Shapes k_heal_mixed is instantiated for: C sources, R = targets + surplus
// computed rows.  R = 0 does not exist: a heal has a target.
constexpr bool heal_kernel_shape(int C, int R) { return C >= 1 && C <= kDecMaxC && R >= 1 && R <= kDecMaxR; }

// Geometries that run the kernel; others go through rsg_heal_records_dev,
// stripe by stripe.
constexpr bool heal_kernel_geometry(int k, int m) { return heal_kernel_shape(k, m); }

// Validation (k + m <= 32).  file_base[i] / target_base[i]: the address of
// shard i's source / target arena, 0 for NULL.  A target shard is never read:
// its file arena and its `present` bit are ignored.  True when
//   - there is at least one target,
//   - no `present` has a bit at or above k+m,
//   - record ranges [rec_off, +32+len) are strictly ascending and disjoint in
//     list order, and so are the target ranges [out_off, +32+len), those of
//     zero-length stripes (32 bytes) included,
//   - no range wraps the address space (relative to any arena that is there),
//   - no target's span (first range's start to last range's end) meets the
//     record span of an arena that some stripe may read, or another target's
//     span.
inline bool validate_heal(int k, int m, size_t n, const RecordDesc* d, const uint64_t* file_base,
                          const uint64_t* target_base) {
    if (k <= 0 || m < 0 || k + m > 32) return false;
    if (!file_base || !target_base || (n && !d)) return false;
    const int t = k + m;
    const uint32_t all = t == 32 ? 0xffffffffu : (1u << t) - 1u;
    const uint32_t targets = arena_mask(t, target_base);
    if (!targets) return false;
    const uint32_t arenas = arena_mask(t, file_base) & ~targets;
    uint64_t max_file = 0, max_target = 0;
    for (int i = 0; i < t; ++i) {
        if (arenas >> i & 1u) max_file = std::max(max_file, file_base[i]);
        max_target = std::max(max_target, target_base[i]);
    }
    uint64_t rend = 0, oend = 0, out_lo = 0, rec_lo = 0;
    uint32_t used = 0;
    for (size_t i = 0; i < n; ++i) {
        if (d[i].present & ~all) return false;
        used |= d[i].present & arenas;
        const uint64_t rl = kRecHeader + d[i].shard_len;  // < 2^33
        if (d[i].rec_off > UINT64_MAX - rl || max_file > UINT64_MAX - rl - d[i].rec_off) return false;
        if (d[i].out_off > UINT64_MAX - rl || max_target > UINT64_MAX - rl - d[i].out_off) return false;
        if (i && (d[i].rec_off < rend || d[i].out_off < oend)) return false;
        if (i == 0) {
            rec_lo = d[i].rec_off;
            out_lo = d[i].out_off;
        }
        rend = d[i].rec_off + rl;
        oend = d[i].out_off + rl;
    }
    if (n == 0) return true;
    for (int i = 0; i < t; ++i) {
        if (!(targets >> i & 1u)) continue;
        const uint64_t o0 = target_base[i] + out_lo, o1 = target_base[i] + oend;
        for (int j = 0; j < t; ++j) {
            if (used >> j & 1u) {
                const uint64_t f0 = file_base[j] + rec_lo, f1 = file_base[j] + rend;
                if (o0 < f1 && f0 < o1) return false;
            }
            if (j != i && (targets >> j & 1u)) {
                const uint64_t p0 = target_base[j] + out_lo, p1 = target_base[j] + oend;
                if (o0 < p1 && p0 < o1) return false;
            }
        }
    }
    return true;
}

// The heal plan of one mask of readable non-target shards: the first k of them
// in ascending index are the sources (the oracle's rule); the computed rows
// are all targets, then every readable shard past the sources, which is
// re-derived and compared (heal.rs:180-196).  The surplus shards are parity
// shards: the sources take the first k readable ones and there are k data
// shards.  R = targets + surplus <= m whenever the plan exists.  False: fewer
// than k readable shards (more than m targets always ends here).
struct HealPlan {
    std::vector<int> src, tgt, surplus;
    uint32_t read_mask() const {
        uint32_t r = 0;
        for (int i : src) r |= 1u << i;
        for (int i : surplus) r |= 1u << i;
        return r;
    }
    int rows() const { return (int)(tgt.size() + surplus.size()); }
};

inline bool plan_heal_mask(int k, int m, uint32_t mask, uint32_t targets, HealPlan& p) {
    p.src.clear();
    p.tgt.clear();
    p.surplus.clear();
    mask &= ~targets;
    if (popcount32(mask) < k) return false;
    for (int i = 0; i < k + m; ++i) {
        if (targets >> i & 1u) p.tgt.push_back(i);
        if (!(mask >> i & 1u)) continue;
        if ((int)p.src.size() < k) p.src.push_back(i);
        else p.surplus.push_back(i);
    }
    return true;
}

// The kernel's table for one group: order_group_for_kernel's order and `job`,
// with out_off the record's offset in the target arenas relative to out_lo,
// for zero-length stripes too (their record is the bare digest).
inline void order_heal_group_for_kernel(const RecordDesc* d, const std::vector<uint32_t>& stripes, size_t first,
                                        uint64_t rec_lo, uint64_t out_lo, std::vector<DecDesc>& out) {
    order_group_for_kernel(d, stripes, first, rec_lo, out_lo, out);
    for (DecDesc& o : out) o.out_off = d[first + o.job].out_off - out_lo;
}

// A run of consecutive caller-order stripes handled as one unit by the host
// form: the record span [rec_lo, rec_hi) of every arena that may be read goes
// up, the target span [out_lo, out_hi) is staged once per target and comes
// back whole.
struct HealSubBatch {
    size_t first, count;
    uint64_t rec_lo, rec_hi, out_lo, out_hi;
};

// Staging bytes of a sub-batch: the record span once per arena copied up, the
// target span once per target (each region 256-byte aligned).
inline uint64_t heal_stage_bytes(const HealSubBatch& b, int files, int targets) {
    return (uint64_t)files * stage_round(b.rec_hi - b.rec_lo) + (uint64_t)targets * stage_round(b.out_hi - b.out_lo);
}

// Split a validated list into sub-batches of at most `stage` staging bytes
// (and `max_count` stripes) with `files` arenas copied up and `targets`
// targets staged.  A single stripe larger than `stage` gets a sub-batch of its
// own.  Covers every stripe once, in order.
inline void split_heal(int files, int targets, size_t n, const RecordDesc* d, uint64_t stage, size_t max_count,
                       std::vector<HealSubBatch>& out) {
    out.clear();
    size_t i = 0;
    while (i < n) {
        HealSubBatch b{i, 0, 0, 0, 0, 0};
        while (i < n && b.count < max_count) {
            HealSubBatch t = b;
            t.count = b.count + 1;
            const uint64_t rl = kRecHeader + d[i].shard_len;
            if (b.count == 0) {
                t.rec_lo = d[i].rec_off;
                t.out_lo = d[i].out_off;
            }
            t.rec_hi = d[i].rec_off + rl;
            t.out_hi = d[i].out_off + rl;
            if (b.count && heal_stage_bytes(t, files, targets) > stage) break;
            b = t;
            ++i;
        }
        out.push_back(b);
    }
}

// redo_from_flags for heal plans: every stripe of `groups` in which a record
// its plan read did not verify loses those bits in masks[s] and goes into
// `redo` (ascending).  Each redone stripe loses at least one bit, so a stripe
// is redone at most k+m times.
inline void redo_heal_from_flags(int k, int m, uint32_t targets, const std::vector<MaskGroup>& groups, size_t first,
                                 const uint8_t* flags, size_t fstride, uint32_t* masks, std::vector<uint32_t>& redo) {
    redo.clear();
    HealPlan p;
    for (const MaskGroup& g : groups) {
        if (!plan_heal_mask(k, m, g.mask, targets, p)) continue;  // no launch: nothing was read
        const uint32_t read = p.read_mask();
        for (uint32_t s : g.stripes) {
            uint32_t bad = 0;
            for (int i = 0; i < k + m; ++i)
                if ((read >> i & 1u) && !flags[(s - first) * fstride + (size_t)i]) bad |= 1u << i;
            if (bad) {
                masks[s] &= ~bad;
                redo.push_back(s);
            }
        }
    }
    std::sort(redo.begin(), redo.end());
}

}  // namespace mixed
}  // namespace rsg
