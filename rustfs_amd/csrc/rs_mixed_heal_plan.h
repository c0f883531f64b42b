// rs_mixed_heal_plan.h — host planner of the mixed-length batch heal
// (rsg_heal_mixed_dev / _host, k_heal_mixed in rs_mixed_heal.hip): a batch of
// [digest][shard] record stripes, each with its own shard length and its own
// set of present shards, healed into the record arenas of the target shards.
// Plain C++17, no HIP headers: it compiles and runs on a CPU
// (tests/host/mixed_heal_plan_main.cpp).
//
// Shared with the mixed-length GET (rs_mixed_decode_plan.h): the descriptors
// (RecordDesc, whose out_off here is the offset of the stripe's record in every
// target arena; DecDesc), the plan struct (MaskPlan: the targets are its
// written rows), the sub-batches of the host form (split_records,
// record_stage_bytes), and the whole of a round: grouping by mask, the kernel
// order by descending chunk count with `job` mapping back, the concatenated
// table and row_shard[] of every launch (plan_round), the kernel's row flags
// to shard flags (shard_flags_from_rows) and the redo rule (redo_from_flags).
// Heal-specific, all of it here: the kernel's shapes, the validation of target
// ranges, the plan of a mask (plan_heal_mask: targets are computed and never
// read) and the out-range rule (heal_out_rule: the record, empty stripes too).
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
// are all targets (written), then every readable shard past the sources, which
// is re-derived and compared (heal.rs:180-196).  The surplus shards are parity
// shards: the sources take the first k readable ones and there are k data
// shards.  rows() <= m whenever the plan exists.  False: fewer than k readable
// shards (more than m targets always ends here).
inline bool plan_heal_mask(int k, int m, uint32_t mask, uint32_t targets, MaskPlan& p) {
    p.src.clear();
    p.written.clear();
    p.surplus.clear();
    mask &= ~targets;
    if (popcount32(mask) < k) return false;
    for (int i = 0; i < k + m; ++i) {
        if (targets >> i & 1u) p.written.push_back(i);
        if (!(mask >> i & 1u)) continue;
        if ((int)p.src.size() < k) p.src.push_back(i);
        else p.surplus.push_back(i);
    }
    return true;
}

// Heal: the stripe's record [digest][shard] in every one of the `targets`
// target arenas; an empty stripe's record is the bare digest.
constexpr OutRule heal_out_rule(int targets) { return OutRule{kRecHeader, 1, targets}; }

}  // namespace mixed
}  // namespace rsg
