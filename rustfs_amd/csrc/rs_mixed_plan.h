// rs_mixed_plan.h — host planner of the mixed-length batch encode
// (rsg_encode_mixed_dev / _host, k_encode_hash_mixed in rs_mixed.hip): a batch
// whose stripes each have their own shard length.  Plain C++17, no HIP
// headers: it compiles and runs on a CPU (tests/host/mixed_plan_main.cpp).
//
// The planner validates the caller's descriptors, orders them for the kernel
// (stripes of near-equal chunk count share a workgroup) and splits a host
// batch into sub-batches that fit the staging buffers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "rs_fused.h"

namespace rsg {
namespace mixed {

constexpr uint32_t kChunk = kFusedChunk;  // bytes per shard per kernel step

// The caller's descriptor (rsg_stripe_desc, include/rsgpu.h): data shard c at
// data + data_off + c*shard_len, parity shard r at parity + parity_off + r*shard_len.
struct StripeDesc {
    uint64_t data_off, parity_off, shard_len;
};

// The kernel's descriptor: `job` is the caller's index (digests are written in
// caller order whatever the table's order).
struct MixedDesc {
    uint64_t data_off, parity_off;
    uint32_t len, job;
};

// Stripes per workgroup: the fused kernels' rule (rs_fused.h).
constexpr int spw_for(int T) { return fused_spw_for(T); }

// Geometries the one-launch kernel is instantiated for (the packed kernel's
// range); others run the per-length paths.
constexpr bool kernel_geometry(int k, int m) { return k >= 1 && k <= 16 && m >= 1 && m <= 4; }

// a shard's chunk count (rs_fused.h): no overflow at len = 0xffffffff, 0 for an empty shard
constexpr uint32_t chunks_of(uint64_t len) { return fused_chunks(len); }

// Validation.  data_base / parity_base: the arenas' addresses (equal for an
// aliased layout such as a3: parity_off = data_off + k*shard_len).  True when
//   - every shard_len <= 0xffffffff and no range wraps the address space,
//   - data ranges [data_off, +k*len) are strictly ascending and disjoint,
//   - parity ranges [parity_off, +m*len) are strictly ascending and disjoint,
//   - no parity range meets a data range (absolute addresses; an O(n) merge
//     of the two sorted lists).
// A zero-length stripe occupies no range: its offsets are not looked at.
inline bool validate(int k, int m, size_t n, const StripeDesc* d, uint64_t data_base, uint64_t parity_base) {
    if (k <= 0 || m < 0) return false;
    if (n && !d) return false;
    const uint64_t K = (uint64_t)k, M = (uint64_t)m;
    bool have = false;
    uint64_t dend = 0, pend = 0;  // ends of the previous non-empty stripe's ranges
    for (size_t i = 0; i < n; ++i) {
        const uint64_t len = d[i].shard_len;
        if (len > 0xffffffffull) return false;
        if (len == 0) continue;
        const uint64_t dl = K * len, pl = M * len;  // < 2^40
        if (d[i].data_off > UINT64_MAX - dl || data_base > UINT64_MAX - dl - d[i].data_off) return false;
        if (d[i].parity_off > UINT64_MAX - pl || parity_base > UINT64_MAX - pl - d[i].parity_off) return false;
        if (have) {
            if (d[i].data_off < dend) return false;
            if (m > 0 && d[i].parity_off < pend) return false;
        }
        dend = d[i].data_off + dl;
        pend = d[i].parity_off + pl;
        have = true;
    }
    if (m == 0) return true;
    // parity against data, absolute addresses: both lists are sorted and
    // disjoint in themselves, so one forward merge finds any intersection
    size_t a = 0, b = 0;
    while (a < n && b < n) {
        if (d[a].shard_len == 0) { ++a; continue; }
        if (d[b].shard_len == 0) { ++b; continue; }
        const uint64_t d0 = data_base + d[a].data_off, d1 = d0 + K * d[a].shard_len;
        const uint64_t p0 = parity_base + d[b].parity_off, p1 = p0 + M * d[b].shard_len;
        if (d0 < p1 && p0 < d1) return false;
        if (d1 <= p1) ++a;
        else ++b;
    }
    return true;
}

// The kernel's table for stripes [first, first + count) of the caller's list:
// sorted by chunk count, descending (stable: equal counts keep caller order),
// offsets relative to (data_lo, parity_lo), job = caller index - first.  A
// zero-length stripe gets offsets 0 (it touches no memory).
inline void order_for_kernel(const StripeDesc* d, size_t first, size_t count, uint64_t data_lo, uint64_t parity_lo,
                             std::vector<MixedDesc>& out) {
    out.resize(count);
    for (size_t i = 0; i < count; ++i) {
        const StripeDesc& s = d[first + i];
        MixedDesc& o = out[i];
        o.len = (uint32_t)s.shard_len;
        o.job = (uint32_t)i;
        o.data_off = s.shard_len ? s.data_off - data_lo : 0;
        o.parity_off = s.shard_len ? s.parity_off - parity_lo : 0;
    }
    std::stable_sort(out.begin(), out.end(),
                     [](const MixedDesc& a, const MixedDesc& b) { return chunks_of(a.len) > chunks_of(b.len); });
}

// A run of consecutive caller-order stripes handled by one launch of the host
// form.  Spans are min start to max end over the run's non-empty stripes
// (lo = hi = 0 when it has none).
struct SubBatch {
    size_t first, count;
    uint64_t data_lo, data_hi, parity_lo, parity_hi;
};

constexpr uint64_t kStageAlign = 256;
constexpr uint64_t stage_round(uint64_t x) { return (x + kStageAlign - 1) / kStageAlign * kStageAlign; }

// Staging bytes of a sub-batch: data span, parity span, digests (each region
// 256-byte aligned).
inline uint64_t stage_bytes(const SubBatch& b, int k, int m, bool digests) {
    return stage_round(b.data_hi - b.data_lo) + stage_round(b.parity_hi - b.parity_lo) +
           (digests ? stage_round((uint64_t)b.count * (uint64_t)(k + m) * 32u) : 0);
}

// Split a validated list into sub-batches of at most `stage` staging bytes
// (and `max_count` stripes).  A single stripe larger than `stage` gets a
// sub-batch of its own.  Covers every stripe once, in order.
inline void split(int k, int m, size_t n, const StripeDesc* d, bool digests, uint64_t stage, size_t max_count,
                  std::vector<SubBatch>& out) {
    out.clear();
    size_t i = 0;
    while (i < n) {
        SubBatch b{i, 0, 0, 0, 0, 0};
        bool have = false;
        while (i < n && b.count < max_count) {
            SubBatch t = b;
            t.count = b.count + 1;
            const uint64_t len = d[i].shard_len;
            if (len) {
                const uint64_t d0 = d[i].data_off, d1 = d0 + (uint64_t)k * len;
                const uint64_t p0 = d[i].parity_off, p1 = p0 + (uint64_t)m * len;
                // validated lists ascend: lo is the first non-empty stripe's
                // start, hi the last one's end
                if (!have) {
                    t.data_lo = d0;
                    t.parity_lo = m ? p0 : 0;
                }
                t.data_hi = d1;
                t.parity_hi = m ? p1 : 0;
            }
            if (b.count && stage_bytes(t, k, m, digests) > stage) break;
            b = t;
            have = have || len != 0;
            ++i;
        }
        out.push_back(b);
    }
}

}  // namespace mixed
}  // namespace rsg
