// rs_mixed_verify_plan.h — host planner of the mixed-length batch deep scan
// (rsg_bitrot_verify_mixed_dev / _host, k_verify_mixed in rs_mixed_verify.hip):
// whole-shard-file verification (bitrot_verify, bitrot.rs:616-655) of n
// unrelated [digest][shard] record files, each with its own part size, shard
// size and length, spread over up to 32 arenas (one per disk).  Plain C++17, no
// HIP headers: it compiles and runs on a CPU
// (tests/host/mixed_verify_plan_main.cpp).
//
// The planner validates the caller's descriptors, expands every file into
// units (one complete record each), orders the units for the kernel, splits a
// host batch into sub-batches that fit the staging buffers, and reduces the
// kernel's per-unit flags to per-file verdicts in rsg_bitrot_verify_dev's
// decision order.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <map>
#include <vector>

#include "rs_mixed_decode_plan.h"

namespace rsg {
namespace mixed {

constexpr int kVerifyMaxArenas = 32;

// The caller's descriptor (rsg_file_desc, include/rsgpu.h).
struct FileDesc {
    uint64_t off;         // the file's bytes at arenas[arena] + off
    uint64_t file_len;    // bytes that are there
    uint64_t want_size;   // the size the caller expects
    uint64_t part_size;   // body bytes of the file
    uint32_t shard_size;  // body bytes of a full record
    uint32_t arena;       // < n_arenas
};

// The kernel's descriptor: one complete record.  The body's `len` (> 0) bytes
// are at `addr` (an address once the arena bases are added, an offset with
// bases of 0), its 32-byte digest in front of them; the quad's verdict goes to
// flags[flag].
struct VerifyUnit {
    uint64_t addr;
    uint32_t len, flag;
};

// A file's verdict, in decision order (the C ABI maps them to RSG_ERR_*).
enum VerifyVerdict {
    kVerifyOk = 0,
    kVerifySizeMismatch,  // want_size is not the size of such a part: nothing read
    kVerifyBitrot,        // the first bad digest among the complete records
    kVerifyEof,           // file_len < want_size
    kVerifyTrailing,      // file_len > want_size
};

// bitrot_shard_file_size (bitrot.rs:593-601); hs: digest bytes per record (32
// for the streaming algorithms, 0 for NONE).  False: the size does not fit 64
// bits (no want_size equals it).
inline bool verify_expect_size(uint64_t part, uint64_t shard, uint64_t hs, uint64_t& out) {
    out = part;
    if (!hs || !part) return true;
    const uint64_t recs = part / shard + (part % shard ? 1 : 0);  // shard > 0 (validated)
    if (recs > (UINT64_MAX - part) / hs) return false;
    out = recs * hs + part;
    return true;
}

inline bool verify_size_ok(const FileDesc& f, uint64_t hs) {
    uint64_t e;
    return verify_expect_size(f.part_size, f.shard_size, hs, e) && e == f.want_size;
}

// The complete records of a file (rsg_bitrot_verify_dev's avail / full / tail):
// those that lie wholly inside min(file_len, want_size); the short last record
// is one of them when all of it is there.  0 for a size mismatch, an empty
// part, or hs == 0.
inline uint64_t verify_records(const FileDesc& f, uint64_t hs) {
    if (!hs || !f.part_size || !verify_size_ok(f, hs)) return 0;
    const uint64_t full = f.part_size / f.shard_size, tail = f.part_size - full * f.shard_size;
    const uint64_t rec = hs + f.shard_size;
    const uint64_t len = std::min(f.file_len, f.want_size);
    uint64_t a = std::min(len / rec, full);
    if (a == full && tail && len - full * rec >= hs + tail) a = full + 1;
    return a;
}

// Validation.  arena_base[a]: arena a's address, 0 for a NULL arena.  True when
//   - 1 <= n_arenas <= 32 and every file's arena is below n_arenas,
//   - no file has shard_size == 0 with part_size > 0,
//   - a NULL arena holds only files with file_len == 0,
//   - no range [off, +file_len) wraps the address space (relative to its arena),
//   - the non-empty ranges of one arena are ascending and disjoint in list
//     order (files of different arenas interleave freely).
inline bool validate_verify(int n_arenas, size_t n, const FileDesc* d, const uint64_t* arena_base) {
    if (n_arenas < 1 || n_arenas > kVerifyMaxArenas || !arena_base || (n && !d)) return false;
    uint64_t end[kVerifyMaxArenas] = {};
    for (size_t i = 0; i < n; ++i) {
        const FileDesc& f = d[i];
        if (f.arena >= (uint32_t)n_arenas) return false;
        if (f.shard_size == 0 && f.part_size > 0) return false;
        if (f.file_len == 0) continue;  // occupies nothing
        const uint64_t base = arena_base[f.arena];
        if (!base) return false;
        if (f.off > UINT64_MAX - f.file_len || base > UINT64_MAX - f.file_len - f.off) return false;
        if (f.off < end[f.arena]) return false;
        end[f.arena] = f.off + f.file_len;
    }
    return true;
}

// Units of files d[first .. first+count), appended in caller order
// [file][record]; flag0[j] is the flag index of file first+j's record 0 and
// flag0[count] the unit count (flag indices count from 0 at `first`).
// base[a]: what is added to a file's `off` (the arena's address, or that of
// its staged span less the span's start; 0: offsets).  False: more than 2^32-1
// units.
inline bool expand_units(const FileDesc* d, size_t first, size_t count, uint64_t hs, const uint64_t* base,
                         std::vector<VerifyUnit>& units, std::vector<uint64_t>& flag0) {
    units.clear();
    flag0.assign(count + 1, 0);
    uint64_t total = 0;
    for (size_t j = 0; j < count; ++j) {
        flag0[j] = total;
        total += verify_records(d[first + j], hs);
    }
    flag0[count] = total;
    if (total > 0xffffffffull) return false;
    units.reserve((size_t)total);
    for (size_t j = 0; j < count; ++j) {
        const FileDesc& f = d[first + j];
        const uint64_t a = flag0[j + 1] - flag0[j];
        if (!a) continue;
        const uint64_t full = f.part_size / f.shard_size, rec = hs + f.shard_size;
        const uint64_t at = base[f.arena] + f.off + hs;
        for (uint64_t r = 0; r < a; ++r) {
            const uint32_t len = r < full ? f.shard_size : (uint32_t)(f.part_size - full * f.shard_size);
            units.push_back(VerifyUnit{at + r * rec, len, (uint32_t)(flag0[j] + r)});
        }
    }
    return true;
}

// 256-byte batches of a unit: what the kernel's quads loop over.
inline uint32_t verify_unit_batches(const VerifyUnit& u) { return u.len >> 8; }

// Kernel order: stable by batch count, descending, so the 16 quads of a wave
// run near-equal trip counts and the longest chains start first.  A counting
// sort (a file's records share one or two counts).
inline void order_units_for_kernel(const std::vector<VerifyUnit>& in, std::vector<VerifyUnit>& out) {
    std::map<uint32_t, uint64_t, std::greater<uint32_t>> at;  // batch count -> units, then first slot
    uint32_t last = 0;
    uint64_t* slot = nullptr;
    for (const VerifyUnit& u : in) {
        const uint32_t b = verify_unit_batches(u);
        if (!slot || b != last) {
            slot = &at[b];
            last = b;
        }
        ++*slot;
    }
    uint64_t sum = 0;
    for (auto& kv : at) {
        const uint64_t c = kv.second;
        kv.second = sum;
        sum += c;
    }
    out.resize(in.size());
    slot = nullptr;
    for (const VerifyUnit& u : in) {
        const uint32_t b = verify_unit_batches(u);
        if (!slot || b != last) {
            slot = &at[b];
            last = b;
        }
        out[(size_t)(*slot)++] = u;
    }
}

// A run of consecutive caller-order files handled as one unit by the host form:
// of every arena it touches (a file with a complete record), the span [lo, hi)
// from its first such file's start to the end of what is read of its last one,
// off + min(file_len, want_size), goes up in one copy.  Bytes past want_size
// and files without a complete record are never read, so they are not staged.
struct VerifySubBatch {
    size_t first, count;
    uint32_t touched;  // bit a: arena a has a file with a complete record here
    uint64_t units;
    uint64_t lo[kVerifyMaxArenas], hi[kVerifyMaxArenas];
};

// Staging bytes of a sub-batch: the span of every touched arena, the unit
// table, the flags (each region 256-byte aligned).
inline uint64_t verify_stage_bytes(const VerifySubBatch& b) {
    uint64_t s = stage_round(b.units * sizeof(VerifyUnit)) + stage_round(b.units);
    for (int a = 0; a < kVerifyMaxArenas; ++a)
        if (b.touched >> a & 1u) s += stage_round(b.hi[a] - b.lo[a]);
    return s;
}

// Split a validated list into sub-batches of at most `stage` staging bytes.  A
// file that alone needs more gets a sub-batch of its own.  Covers every file
// once, in order.  A file without a complete record (a size mismatch, an
// empty part, a file cut inside its first record) is never read: it joins the
// sub-batch at hand and adds nothing to it.
inline void split_verify(size_t n, const FileDesc* d, uint64_t hs, uint64_t stage, std::vector<VerifySubBatch>& out) {
    out.clear();
    size_t i = 0;
    while (i < n) {
        VerifySubBatch b{};
        b.first = i;
        while (i < n) {
            VerifySubBatch t = b;
            t.count = b.count + 1;
            const FileDesc& f = d[i];
            if (const uint64_t recs = verify_records(f, hs)) {
                if (!(t.touched >> f.arena & 1u)) {
                    t.touched |= 1u << f.arena;
                    t.lo[f.arena] = f.off;
                }
                t.hi[f.arena] = f.off + std::min(f.file_len, f.want_size);
                t.units += recs;
            }
            if (b.count && verify_stage_bytes(t) > stage) break;
            b = t;
            ++i;
        }
        out.push_back(b);
    }
}

// Verdicts of files d[first .. first+count) from the unit flags (indexed as
// expand_units numbered them): the first zero flag of a file decides; EOF and
// trailing data come after that.  flags may be null when there is no unit.
inline void reduce_verdicts(const FileDesc* d, size_t first, size_t count, uint64_t hs, const std::vector<uint64_t>& flag0,
                            const uint8_t* flags, VerifyVerdict* out) {
    for (size_t j = 0; j < count; ++j) {
        const FileDesc& f = d[first + j];
        VerifyVerdict v = kVerifyOk;
        if (!verify_size_ok(f, hs)) {
            v = kVerifySizeMismatch;
        } else {
            for (uint64_t r = flag0[j]; r < flag0[j + 1]; ++r)
                if (!flags[r]) {
                    v = kVerifyBitrot;
                    break;
                }
            if (v == kVerifyOk && f.file_len < f.want_size) v = kVerifyEof;
            if (v == kVerifyOk && f.file_len > f.want_size) v = kVerifyTrailing;
        }
        out[j] = v;
    }
}

}  // namespace mixed
}  // namespace rsg
