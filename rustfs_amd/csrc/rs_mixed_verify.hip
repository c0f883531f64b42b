// rs_mixed_verify.hip — mixed-length batch deep scan (bitrot_verify,
// bitrot.rs:616-655, once per part per disk from LocalDisk::verify_file):
// every complete [digest][shard] record of n unrelated shard files hashed and
// compared with its header in one launch, each record with its own length and
// its own alignment.
//
// k_verify_mixed<DEPTH> is k_hh256_quad<0, DEPTH, true> (rs_kernels.hip) with
// the message taken from a unit table instead of base[b] + r*stride and one
// `len` per launch: 256 threads, one 4-lane quad per unit (mixed::VerifyUnit,
// rs_mixed_verify_plan.h), quad j takes unit[j] of the planner's sorted table
// (descending 256-byte batch count, so the 16 quads of a wave run near-equal
// trip counts).  Same aligned-word loads, DPP quad_perm [1,2,3,0] rotate and
// v_alignbyte_b32 funnel, same register pipeline of DEPTH 8-packet batches
// with loads clamped inside the message.  No LDS.
//
// Per-quad bounds.  The batch loop, the single-packet loop and the remainder
// take their bounds from the unit, which all four lanes of a quad load from
// the same address, so every bound is uniform within a quad: the four lanes
// enter and leave each loop together.  That is what the hash needs, because
// its DPP moves (quad_perm within the quad) read the partner lanes' registers
// and a partner that had left the loop would hand over a stale one.  The
// quads of a wave may leave a loop at different trips; lanes of other quads
// are never read.  A quad past the table exits whole (j is the same in its
// four lanes).
//
// Per-quad misalignment.  mis = address & 7 differs between the quads of a
// wave: it is a VGPR operand of v_alignbyte_b32, and the `mis < 4` word select
// is per lane.
//
// What the aligned-word loads touch.  The word of a batch's first packet
// begins up to 7 bytes below the body: those bytes are the record's own
// 32-byte header, which is in front of every body, so no load reaches below
// the file.  Lane 3's last word of a batch needs the aligned word that starts
// the next packet (w[8]): when mis != 0 that word begins mis bytes below byte
// (t0 + 8) * 32 of the body, which is at most its length, so the word holds a
// body byte: an aligned 8-byte word that holds a byte of the file lies in the
// file's own 8-byte granule and the load stays inside the caller's buffer
// (k_hh256_quad's argument).  When mis == 0 the word would begin AT byte
// (t0 + 8) * 32, which may be the first byte past the file, and it is not
// needed (the funnel shifts by 0): the quad loads the batch's last word again
// instead.  The address is selected, not the load: a load under a per-lane
// branch would wait for every load in flight.  Batches past the unit's last
// one are clamped to it, as in k_hh256_quad.  The single-packet loop and the
// remainder read body bytes only, the digest compare the 32 header bytes.
//
// Every unit's flag byte is written whole, 1 or 0 (a vector byte store by the
// quad's lane 0): nothing presets the flags.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rs_device.h"
#include "rs_mixed.h"

namespace rsg {

using mixed::VerifyUnit;

template <int DEPTH>
__global__ __launch_bounds__(256) void k_verify_mixed(const VerifyMixedParams p) {
    const uint64_t j = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 2;
    const uint32_t q = threadIdx.x & 3u;
    if (j >= p.n) return;  // whole quads exit together
    const VerifyUnit u = p.unit[j];  // the same 16 bytes in the quad's four lanes
    const uint8_t* const msg = (const uint8_t*)(uintptr_t)u.addr;
    const uint32_t len = u.len;  // > 0
    HHQuad s;
    hhq_init(s, p.key, q);
    const uint32_t packets = len >> 5, nb = packets >> 3;  // whole packets, whole 8-packet batches
    const uint32_t mis = (uint32_t)(u.addr & 7u);          // the body's byte offset in its word
    const uint8_t* const am = msg - mis;
    const uint32_t back8 = mis ? 0u : 8u;  // mis == 0: w[8] is the batch's last word again (unused)
    // batch x: aligned words of packets 8x .. 8x+7, w[8] = the word that starts the next packet
    auto fetch = [&](uint64_t (&w)[9], uint32_t x) {
        const uint8_t* const b = am + ((uint64_t)x << 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = *(const uint64_t*)(b + i * 32 + 8 * q);
        w[8] = *(const uint64_t*)(b + 256 - back8);
    };
    // lane q's message word = its aligned word >> 8 mis, filled from the next
    // lane's (lane 3: the next packet's first word), then hashed
    auto consume = [&](uint64_t (&w)[9]) {
        uint64_t nx[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const u32x2 v = __builtin_bit_cast(u32x2, w[i]);
            u32x2 r;
            r.x = (uint32_t)__builtin_amdgcn_mov_dpp((int)v.x, 0x39, 0xF, 0xF, false);  // quad_perm [1,2,3,0]
            r.y = (uint32_t)__builtin_amdgcn_mov_dpp((int)v.y, 0x39, 0xF, 0xF, false);
            nx[i] = __builtin_bit_cast(uint64_t, r);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint64_t hi = q == 3 ? (i < 7 ? nx[i + 1] : w[8]) : nx[i];
            const uint32_t l0 = (uint32_t)w[i], l1 = (uint32_t)(w[i] >> 32), h0 = (uint32_t)hi,
                           h1 = (uint32_t)(hi >> 32);
            const uint32_t a0 = __builtin_amdgcn_alignbyte(l1, l0, mis), a1 = __builtin_amdgcn_alignbyte(h0, l1, mis);
            const uint32_t b1 = __builtin_amdgcn_alignbyte(h1, h0, mis);
            hhq_update(s, mis < 4 ? ((uint64_t)a1 << 32 | a0) : ((uint64_t)b1 << 32 | a1));
        }
    };
    if (nb) {
        if constexpr (DEPTH >= 2) {
            // DEPTH register batches: batch x lives in w[x % DEPTH]; the loads
            // of batch x + DEPTH - 1 are issued before batch x is hashed.
            // Loads past the last batch are clamped to it (inside the body)
            // and unused.
            uint64_t w[DEPTH][9];
#pragma unroll
            for (int d = 0; d < DEPTH - 1; ++d) fetch(w[d], (uint32_t)d < nb ? (uint32_t)d : nb - 1);
            uint32_t b = 0;
            for (; b + DEPTH <= nb; b += DEPTH) {
#pragma unroll
                for (int d = 0; d < DEPTH; ++d) {
                    const uint32_t nxt = b + d + DEPTH - 1;
                    fetch(w[(d + DEPTH - 1) % DEPTH], nxt < nb ? nxt : nb - 1);
                    consume(w[d]);
                }
            }
#pragma unroll
            for (int d = 0; d < DEPTH - 1; ++d)  // fewer than DEPTH batches left, all fetched
                if (b + d < nb) consume(w[d]);
        } else {
            for (uint32_t b = 0; b < nb; ++b) {
                uint64_t w[9];
                fetch(w, b);
                consume(w);
            }
        }
    }
    for (uint32_t t = nb * 8; t < packets; ++t) hhq_update(s, ld64_any(msg + (uint64_t)t * 32 + 8 * q));
    const uint32_t rem = len & 31u;
    if (rem) hhq_remainder(s, msg + (uint64_t)packets * 32, rem, q);
    // the digest against the 32 bytes in front of the body; the quad's verdict, written whole
    const uint64_t h = hhq_digest(s, q);
    uint32_t ok = h == ld64_any(msg - mixed::kRecHeader + 8 * q) ? 1u : 0u;
    ok &= quad_swap_pairs(ok);
    ok &= quad_swap_halves(ok);
    if (q == 0) p.flags[u.flag] = (uint8_t)ok;
}

hipError_t launch_verify_mixed(const VerifyMixedParams& p, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    if (!p.unit || !p.flags || p.n > 0x1fffffffull) return hipErrorInvalidValue;
    const Tuning& t = tuning();  // one snapshot for the whole launch
    const int depth = t.hash_depth;
    using Kernel = void (*)(const VerifyMixedParams);
    const Kernel k = depth == 1 ? k_verify_mixed<1> : depth == 2 ? k_verify_mixed<2> : k_verify_mixed<3>;
    const uint64_t blocks = (p.n * 4u + 255u) / 256u;  // one quad per unit
    hipLaunchKernelGGL(k, dim3((uint32_t)blocks), dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace rsg
