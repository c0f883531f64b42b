// rs_mixed_decode_plan.h — host planner of the mixed-length batch GET
// (rsg_decode_mixed_dev / _host, k_decode_mixed in rs_mixed_decode.hip): a
// batch of [digest][shard] record stripes, each with its own shard length and
// its own set of present shards.  Plain C++17, no HIP headers: it compiles and
// runs on a CPU (tests/host/mixed_decode_plan_main.cpp).
//
// The planner validates the caller's descriptors, splits a host batch into
// sub-batches that fit the staging buffers, and plans the rounds of a launch
// sequence: a round groups the stripes still to do by their mask of readable
// shards (one plan and one launch per distinct mask), orders each group for
// the kernel into one concatenated table, and, from the verify flags the
// launches leave, finds the stripes to run again under a smaller mask.
//
// Everything from OutRule down is the record-stripe machinery the mixed-length
// heal (rs_mixed_heal_plan.h) runs through as well: the two operations differ
// in their validation, in the plan of a mask (plan_mask here, plan_heal_mask
// there) and in the out range of a stripe (get_out_rule, heal_out_rule).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <vector>

#include "rs_mixed_plan.h"

namespace rsg {
namespace mixed {

// The caller's descriptor (rsg_record_desc, include/rsgpu.h): shard i's record
// [32-byte digest][shard_len bytes] at files[i] + rec_off, a rebuilt data
// shard c at out + out_off + c*shard_len.
struct RecordDesc {
    uint64_t rec_off, out_off;
    uint32_t shard_len, present;
};

// The kernel's descriptor: offsets relative to the launch's bases, `job` the
// stripe's index in the launch's flag / mismatch arrays (caller order).
struct DecDesc {
    uint64_t rec_off, out_off;
    uint32_t len, job;
};

constexpr uint64_t kRecHeader = 32;  // digest bytes in front of every shard
constexpr int kDecMaxC = 16, kDecMaxR = 4;

// Geometries k_decode_mixed is instantiated for (m = 0 only verifies); others
// run the per-length engines stripe by stripe.
constexpr bool decode_kernel_geometry(int k, int m) { return k >= 1 && k <= kDecMaxC && m >= 0 && m <= kDecMaxR; }

// Stripes per workgroup of k_decode_mixed for T = C + R rows: the encode
// kernel's rule, but two at T = 20 (RS(16,4) with four computed rows), whose
// four-stripe workgroup of nine waves would hold the GF wave to 168 VGPRs.
constexpr int decode_spw_for(int T) { return T >= 20 ? 2 : spw_for(T); }

// Bit i set: arena i is there (non-NULL).
inline uint32_t arena_mask(int t, const uint64_t* file_base) {
    uint32_t a = 0;
    for (int i = 0; i < t && i < 32; ++i)
        if (file_base[i]) a |= 1u << i;
    return a;
}

inline int popcount32(uint32_t v) {
    int c = 0;
    for (; v; v &= v - 1) ++c;
    return c;
}

// Validation (k + m <= 32).  file_base[i]: arena i's address, 0 for a NULL
// arena; out_base: the out arena's address.  True when
//   - no `present` has a bit at or above k+m,
//   - record ranges [rec_off, +32+len) are strictly ascending and disjoint in
//     list order, and so are the non-empty out ranges [out_off, +k*len),
//   - no range wraps the address space (relative to any arena that is there),
//   - the out span (first non-empty out range's start to the last one's end)
//     does not meet the record span of an arena that some stripe may read.
inline bool validate_decode(int k, int m, size_t n, const RecordDesc* d, const uint64_t* file_base, uint64_t out_base) {
    if (k <= 0 || m < 0 || k + m > 32) return false;
    if (n && (!d || !file_base)) return false;
    const int t = k + m;
    const uint32_t all = t == 32 ? 0xffffffffu : (1u << t) - 1u;
    const uint32_t arenas = arena_mask(t, file_base);
    uint64_t max_base = 0;
    for (int i = 0; i < t; ++i) max_base = std::max(max_base, file_base[i]);
    bool have_out = false;
    uint64_t rend = 0, oend = 0, out_lo = 0, out_hi = 0, rec_lo = 0, rec_hi = 0;
    uint32_t used = 0;
    for (size_t i = 0; i < n; ++i) {
        if (d[i].present & ~all) return false;
        used |= d[i].present & arenas;
        const uint64_t len = d[i].shard_len, rl = kRecHeader + len, ol = (uint64_t)k * len;  // < 2^37
        if (d[i].rec_off > UINT64_MAX - rl || max_base > UINT64_MAX - rl - d[i].rec_off) return false;
        if (i && d[i].rec_off < rend) return false;
        if (i == 0) rec_lo = d[i].rec_off;
        rend = rec_hi = d[i].rec_off + rl;
        if (len == 0) continue;  // an empty out range occupies nothing
        if (d[i].out_off > UINT64_MAX - ol || out_base > UINT64_MAX - ol - d[i].out_off) return false;
        if (have_out && d[i].out_off < oend) return false;
        if (!have_out) out_lo = d[i].out_off;
        oend = out_hi = d[i].out_off + ol;
        have_out = true;
    }
    if (!have_out) return true;
    const uint64_t o0 = out_base + out_lo, o1 = out_base + out_hi;
    for (int i = 0; i < t; ++i) {
        if (!(used >> i & 1u)) continue;
        const uint64_t f0 = file_base[i] + rec_lo, f1 = file_base[i] + rec_hi;
        if (o0 < f1 && f0 < o1) return false;
    }
    return true;
}

// The plan of one mask, for GET and heal alike: the sources, the computed rows
// that are written (GET: the lost data shards; heal: the targets; never read),
// and the surplus shards, which are read, re-derived and compared.
struct MaskPlan {
    std::vector<int> src, written, surplus;
    uint32_t read_mask() const {
        uint32_t r = 0;
        for (int i : src) r |= 1u << i;
        for (int i : surplus) r |= 1u << i;
        return r;
    }
    int rows() const { return (int)(written.size() + surplus.size()); }  // computed rows
};

// The decode plan of one mask: the first k readable shards in ascending index
// are the sources (the oracle's rule), the data shards outside the mask are
// rebuilt, and, when something is rebuilt and `verify_surplus`, every readable
// shard past the sources is re-derived and compared.  When every data shard
// is readable nothing is rebuilt and no parity record is read.  False: fewer
// than k readable shards.
inline bool plan_mask(int k, int m, uint32_t mask, bool verify_surplus, MaskPlan& p) {
    p.src.clear();
    p.written.clear();
    p.surplus.clear();
    if (popcount32(mask) < k) return false;
    for (int i = 0; i < k; ++i)
        if (!(mask >> i & 1u)) p.written.push_back(i);
    for (int i = 0; i < k + m; ++i) {
        if (!(mask >> i & 1u)) continue;
        if ((int)p.src.size() < k) p.src.push_back(i);
        else if (verify_surplus && !p.written.empty()) p.surplus.push_back(i);
    }
    return true;
}

// The out-range rule of an operation: a stripe of shard length len occupies
// [out_off, +bytes(len)) of every one of the `copies` out arenas, and nothing,
// its out_off not looked at, where bytes(len) is 0.
struct OutRule {
    uint64_t fixed, per_byte;
    int copies;
    constexpr uint64_t bytes(uint32_t len) const { return fixed + per_byte * len; }
};

// GET: the k rebuilt data shards side by side in the one out arena; an empty
// stripe occupies nothing.
constexpr OutRule get_out_rule(int k) { return OutRule{0, (uint64_t)k, 1}; }

// Stripes that share a mask, in the order given (stable: caller order holds
// inside a group); groups in order of first appearance.
struct MaskGroup {
    uint32_t mask;
    std::vector<uint32_t> stripes;
};

inline void group_by_mask(const uint32_t* masks, const std::vector<uint32_t>& todo, std::vector<MaskGroup>& out) {
    out.clear();
    std::map<uint32_t, size_t> at;
    for (uint32_t s : todo) {
        auto it = at.find(masks[s]);
        if (it == at.end()) {
            it = at.emplace(masks[s], out.size()).first;
            out.push_back(MaskGroup{masks[s], {}});
        }
        out[it->second].stripes.push_back(s);
    }
}

// The kernel's table for one group, appended to `out`: sorted by chunk count,
// descending (stable: equal counts keep the group's order), offsets relative
// to (rec_lo, out_lo), job = stripe index - first (the launch's flag arrays
// are in caller order whatever the table's order).  A stripe without an out
// range gets out_off 0.
inline void order_group_for_kernel(const OutRule& rule, const RecordDesc* d, const std::vector<uint32_t>& stripes,
                                   size_t first, uint64_t rec_lo, uint64_t out_lo, std::vector<DecDesc>& out) {
    const size_t at = out.size();
    out.reserve(at + stripes.size());
    for (uint32_t j : stripes) {
        const RecordDesc& s = d[j];
        out.push_back(DecDesc{s.rec_off - rec_lo, rule.bytes(s.shard_len) ? s.out_off - out_lo : 0, s.shard_len,
                              (uint32_t)(j - first)});
    }
    std::stable_sort(out.begin() + (ptrdiff_t)at, out.end(),
                     [](const DecDesc& a, const DecDesc& b) { return chunks_of(a.len) > chunks_of(b.len); });
}

// A run of consecutive caller-order stripes handled as one unit by a host
// form: the record span [rec_lo, rec_hi) of every arena that may be read goes
// up, the out span [out_lo, out_hi) is staged beside it once per out arena
// (out_lo = out_hi = 0 without a stripe that has an out range).
struct RecSubBatch {
    size_t first, count;
    uint64_t rec_lo, rec_hi, out_lo, out_hi;
};

// Staging bytes of a sub-batch: the record span once per arena copied up, the
// out span once per out arena (each region 256-byte aligned).
inline uint64_t record_stage_bytes(const OutRule& rule, const RecSubBatch& b, int files) {
    return (uint64_t)files * stage_round(b.rec_hi - b.rec_lo) + (uint64_t)rule.copies * stage_round(b.out_hi - b.out_lo);
}

// Split a validated list into sub-batches of at most `stage` staging bytes
// (and `max_count` stripes) with `files` arenas copied up.  A single stripe
// larger than `stage` gets a sub-batch of its own.  Covers every stripe once,
// in order.
inline void split_records(const OutRule& rule, int files, size_t n, const RecordDesc* d, uint64_t stage,
                          size_t max_count, std::vector<RecSubBatch>& out) {
    out.clear();
    size_t i = 0;
    while (i < n) {
        RecSubBatch b{i, 0, 0, 0, 0, 0};
        bool have_out = false;
        while (i < n && b.count < max_count) {
            RecSubBatch t = b;
            t.count = b.count + 1;
            const uint64_t ol = rule.bytes(d[i].shard_len);
            if (b.count == 0) t.rec_lo = d[i].rec_off;
            t.rec_hi = d[i].rec_off + kRecHeader + d[i].shard_len;
            if (ol) {
                if (!have_out) t.out_lo = d[i].out_off;
                t.out_hi = d[i].out_off + ol;
            }
            if (b.count && record_stage_bytes(rule, t, files) > stage) break;
            b = t;
            have_out = have_out || ol != 0;
            ++i;
        }
        out.push_back(b);
    }
}

// One round over the stripes of `todo`: their groups by mask; for every group
// whose mask has a plan, a launch; the launches' tables, concatenated in launch
// order.  A group without a plan (too few readable shards) has no launch and
// read[] 0: nothing of it is read.
struct RoundLaunch {
    size_t group;                // index into groups
    size_t at, n;                // its slice of the table
    MaskPlan plan;
    std::vector<int> row_shard;  // kernel row -> shard read for it; -1: a written row, not read
};

struct Round {
    std::vector<MaskGroup> groups;
    std::vector<uint32_t> read;  // per group: the shards its launch reads, 0 without a launch
    std::vector<RoundLaunch> launches;
    std::vector<DecDesc> table;
};

// plan(mask, MaskPlan&) is the operation's plan of a mask (plan_mask,
// plan_heal_mask); rows are the sources, then the written, then the surplus.
template <class PlanFn>
inline void plan_round(const OutRule& rule, const RecordDesc* d, size_t first, uint64_t rec_lo, uint64_t out_lo,
                       const uint32_t* masks, const std::vector<uint32_t>& todo, PlanFn plan, Round& r) {
    group_by_mask(masks, todo, r.groups);
    r.read.assign(r.groups.size(), 0);
    r.launches.clear();
    r.table.clear();
    MaskPlan p;
    for (size_t g = 0; g < r.groups.size(); ++g) {
        if (!plan(r.groups[g].mask, p)) continue;
        r.read[g] = p.read_mask();
        const size_t at = r.table.size();
        order_group_for_kernel(rule, d, r.groups[g].stripes, first, rec_lo, out_lo, r.table);
        r.launches.push_back(RoundLaunch{g, at, r.table.size() - at, p, p.src});
        std::vector<int>& rs = r.launches.back().row_shard;
        rs.insert(rs.end(), p.written.size(), -1);
        rs.insert(rs.end(), p.surplus.begin(), p.surplus.end());
    }
}

// After the launches of a round: the kernels' flags, rows[job*fstride + row]
// (job = stripe - first), to flags by shard, flags[(s - first)*fstride + shard],
// for every stripe of every launch and every row read.  Other entries of
// `flags` stay as they are.
inline void shard_flags_from_rows(const Round& r, size_t first, const uint8_t* rows, size_t fstride, uint8_t* flags) {
    for (const RoundLaunch& l : r.launches) {
        const int* row_shard = l.row_shard.data();
        const size_t nrows = l.row_shard.size();
        for (uint32_t s : r.groups[l.group].stripes) {  // the stripes of the launch's slice, in caller order
            const uint8_t* in = rows + (s - first) * fstride;
            uint8_t* out = flags + (s - first) * fstride;
            for (size_t row = 0; row < nrows; ++row)
                if (row_shard[row] >= 0) out[row_shard[row]] = in[row];
        }
    }
}

// After a round: flags[(s - first)*fstride + i] is 1 where shard i's record of
// stripe s verified, 0 where it did not, and is looked at only for the shards
// of read[g], the shards the launch of the stripe's group read (0: no launch).
// Every stripe whose verified set is smaller than its mask gets the unverified
// bits cleared in masks[s] and goes into `redo` (ascending).  Each redone
// stripe loses at least one bit, so a stripe is redone at most t = k+m times.
inline void redo_from_flags(int t, const std::vector<MaskGroup>& groups, const uint32_t* read, size_t first,
                            const uint8_t* flags, size_t fstride, uint32_t* masks, std::vector<uint32_t>& redo) {
    redo.clear();
    for (size_t g = 0; g < groups.size(); ++g) {
        if (!read[g]) continue;
        for (uint32_t s : groups[g].stripes) {
            uint32_t bad = 0;
            for (int i = 0; i < t; ++i)
                if ((read[g] >> i & 1u) && !flags[(s - first) * fstride + (size_t)i]) bad |= 1u << i;
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
