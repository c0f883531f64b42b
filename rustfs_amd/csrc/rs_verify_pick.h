// rs_verify_pick.h — which kernel a HighwayHash launch runs: the decision of
// launch_hh256 (rs_kernels.hip) and launch_verify_records_dma (rs_verify.hip)
// as one pure function of the launch's shape.  Plain C++17, no HIP headers: it
// compiles and runs on a CPU (tests/host/verify_pick_main.cpp), and
// tests/verify_shapes.py restates it for the GPU tests' shape sweeps.
//
// The verify-only record walks (the all-present GET, the parity check after a
// rotten data record, whole-file bitrot_verify, the two-pass engines' verify
// step) all end here, in one of two kernel families:
//  - the LDS-DMA ring k_verify_records_dma<NF> (rs_verify.hip), NF = 1..15
//    files, records off 16-byte alignment; it writes each record's flag whole
//    (1 verified, 0 not);
//  - k_hh256_quad<COPY, DEPTH, UNAL> (rs_kernels.hip); in verify mode it only
//    clears a flag, which the caller has set to 1.
#pragma once

#include <stdint.h>

#ifndef RSG_VERIFY_DMA
#define RSG_VERIFY_DMA 1  // 0: never the ring (A/B builds)
#endif

namespace rsg {

constexpr int kPickMaxBases = 32;      // kMaxHashBases (rs_kernels.h)
constexpr uint32_t kPickStep = 512;    // dma::CH (rs_device.h): bytes per record per ring step
constexpr int kPickRingRecords = 4;    // records per file per ring workgroup (rs_verify.hip kVG)
constexpr int kPickMaxRingFiles = 15;  // the ring's instantiations: NF = 1..15

// The shape of one launch (HashParams, rs_kernels.h, without its payload) and
// the tuning snapshot's values the choice reads.
struct HashPickIn {
    uint64_t n;              // messages
    uint32_t nbases;         // multi-file mode: files (0: the plain / per-shard batch form)
    uint64_t per_base;       // records per file
    uint64_t len;            // message length
    uint64_t stripe_stride;  // bytes between a file's records (plain form: between stripes)
    int64_t digest_off;
    bool flags;              // HashParams::flags set (one flag array for the whole launch)
    uint64_t data;           // plain form: address of message 0
    uint64_t shard_pitch;    // plain form: bytes between messages of one stripe
    uint64_t base[kPickMaxBases];  // address of record 0's body, per file
    bool has_copy[kPickMaxBases];  // copy_base[b] set
    bool has_flag[kPickMaxBases];  // flag_base[b] set
    int depth;               // Tuning::hash_depth
    bool unal;               // Tuning::hash_unal
    bool direct_copy;        // Tuning::hash_direct_copy
};

enum HashPickKind {
    kPickNone = 0,  // n = 0: nothing to launch
    kPickInvalid,   // more workgroups than a grid takes: hipErrorInvalidValue
    kPickRing,      // k_verify_records_dma<nf>
    kPickQuad,      // k_hh256_quad<copy, depth, unal>
};

struct HashPick {
    HashPickKind kind;
    uint64_t blocks;  // workgroups of the launch
    // ring: files, ring slots, 512-byte steps of a record walk
    int nf, rd;
    uint32_t steps;
    // quad: COPY (0 none, 1 direct 8-byte stores, 2 staged), DEPTH, UNAL
    int copy, depth;
    bool unal;
};

// A multi-file verify launch (nbases files of per_base records at pitch
// stripe_stride, digest 32 bytes before each body, flags per file and record,
// no copies) runs on the DMA ring when the records sit off 16-byte alignment.
// Up to 12 files: a 3-slot ring (two steps of DMA in flight), two workgroups
// a CU; 13-15 files: a 2-slot ring (RS(10,4)'s 14 files 10 % faster than the
// quad kernel; RS(12,4)'s 16, 1 % slower, stay on it).  Launches of 13-15
// files at odd record pitches stay on the quad kernel's funnel (RS(14,2)'s 16:
// 12 % slower on the ring), more files too; split launches of 8 + 8 files
// measured 12-24 % slower than either, and 2-record workgroups on a 3-slot
// ring past 12 files 12-30 % slower (profiles/r05/ab_verify/, g2/).
// false: not taken (the launch runs k_hh256_quad).
inline bool pick_verify_ring(const HashPickIn& h, HashPick& out) {
    if (!RSG_VERIFY_DMA || h.nbases < 1 || h.nbases > (uint32_t)kPickMaxRingFiles || h.digest_off != -32 ||
        h.len == 0 || h.per_base == 0 || h.flags)
        return false;
    bool aligned = h.stripe_stride % 16 == 0;
    for (uint32_t b = 0; b < h.nbases; ++b) {
        if (h.has_copy[b] || !h.has_flag[b]) return false;
        aligned = aligned && h.base[b] % 16 == 0;
    }
    if (aligned) return false;  // the quad kernel's loads are aligned: nothing to gain
    bool odd = h.stripe_stride % 2 != 0;
    for (uint32_t b = 0; b < h.nbases; ++b) odd = odd || h.base[b] % 2 != 0;
    if (h.nbases > 12 && odd) return false;
    const uint64_t steps = (h.len + kPickStep - 1) / kPickStep;
    const uint64_t blocks = (h.per_base + kPickRingRecords - 1) / kPickRingRecords;
    // per-lane DMA offsets are 32-bit: HS records and a body
    if (steps > 0xffffffffull || blocks > 0x7fffffffull || 3 * h.stripe_stride >= (1ull << 32)) return false;
    out.kind = kPickRing;
    out.blocks = blocks;
    out.nf = (int)h.nbases;
    out.rd = h.nbases <= 12 ? 3 : 2;
    out.steps = (uint32_t)steps;
    return true;
}

inline HashPick pick_hash_launch(const HashPickIn& h) {
    HashPick out = {};
    out.kind = kPickNone;
    if (h.n == 0) return out;
    const uint64_t blocks = (h.n * 4u + 255u) / 256u;  // one quad per message
    if (blocks > 0x7fffffffull) {
        out.kind = kPickInvalid;
        return out;
    }
    bool copy = false;  // copy mode when any file of the launch has a copy target
    for (uint32_t b = 0; b < h.nbases; ++b) copy = copy || h.has_copy[b];
    if (!copy && pick_verify_ring(h, out)) return out;
    // messages at odd offsets (record pitch 174795 of RS(6,4) at 1 MiB
    // blocks): aligned loads and a funnel shift, 1.005 -> 0.899 ms for the
    // all-present GET; at even offsets (RS(10,4), RS(12,4): 2 mod 8) the
    // hardware's unaligned loads are 4-5 % faster than the funnel
    // (profiles/r04/o/).  Tuning::hash_unal, RSG_HASH_UNAL=0: always the loads.
    bool even = true;
    if (h.nbases) {
        even = h.stripe_stride % 2 == 0;
        for (uint32_t b = 0; b < h.nbases; ++b) even = even && h.base[b] % 2 == 0;
    } else {
        even = h.data % 2 == 0 && h.stripe_stride % 2 == 0 && h.shard_pitch % 2 == 0;
    }
    out.kind = kPickQuad;
    out.blocks = blocks;
    // copy mode: staged 16-byte stores (COPY = 2) by default (Tuning:
    // direct 8-byte stores for A/B runs); 8-packet batches in flight per
    // lane: 2 by default
    out.copy = !copy ? 0 : h.direct_copy ? 1 : 2;
    out.unal = !copy && h.depth == 2 && !even && h.unal;
    out.depth = out.unal ? 2 : h.depth == 1 ? 1 : h.depth == 2 ? 2 : 3;
    return out;
}

}  // namespace rsg
