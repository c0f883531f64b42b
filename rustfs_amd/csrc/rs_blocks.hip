// rs_blocks.hip — the gathered block encode: the parity (k_encode_blocks) and
// the k+m HighwayHash-256 digests (k_hash_blocks) of n unrelated blocks, each
// a list of shard addresses of any alignment, in one launch each
// (rsg_encode_blocks and rsg_encode_hashed;
// ReedSolomonEncoder::encode per 1 MiB block, erasure.rs:396-408, and
// BitrotWriter::write's hash of every shard, bitrot.rs:496-502).
//
// k_encode_blocks<C,R> (C = 1..8; k_encode_blocks_loop<R,G> for C = 9..16, the
// same work rolled over groups of inputs): one workgroup of 256 threads per
// column tile of
// blocks::kTile bytes of one block, thread t the 16-byte unit t of the tile,
// as the vector GF kernel (rs_kernels.hip) splits a stripe: the launch is
// parallel over columns, so a handful of 1 MiB blocks fills the GPU.  The
// workgroup finds its block by a binary search over the per-block prefix sums
// of tile counts (tile0, n + 1 words): every lane reads the same words, so
// the search runs on scalar registers and costs log2(n) 4-byte loads; the
// table is O(n), not O(grid).  The block's descriptor (blocks::BlockDesc) is
// read the same way.
//
// Loads.  A unit that lies wholly inside [0, len) is one 16-byte load at the
// shard's own alignment (unaligned-access mode, ld16): every byte of it is a
// byte of the input.  The last unit of a shard whose length is no multiple of
// 16 is loaded byte by byte, bytes below len only.  So the kernel never reads
// a byte outside [addr, addr + len) of an input, which is stricter than the
// aligned-word rule of the hash kernels.
// Stores.  Likewise: whole units with one 16-byte store, the ragged unit byte
// by byte, and nothing at or past len.  All stores are vector stores.
// Every data shard with a copy address is also stored there verbatim, every
// parity shard with a second address there too (the runner's digest scheme,
// rs_blocks_plan.h).
//
// k_hash_blocks<DEPTH> is k_verify_mixed (rs_mixed_verify.hip) with the digest
// written instead of compared: one quad per unit of a table sorted by
// descending length, the same walk (hhq_walk below).  The word that holds a message's first
// byte begins up to 7 bytes below it: an aligned 8-byte word that holds a byte
// of the message, which cannot leave that byte's page; every other load is
// argued in rs_mixed_verify.hip.  Lane q stores digest bytes [8q, 8q + 8),
// 32 bytes per unit and no more.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rs_blocks.h"
#include "rs_device.h"

namespace rsg {

using blocks::BlockDesc;
using blocks::HashUnit;
using blocks::kTile;

namespace {

// the first n (1..15) bytes at p, the rest zero
__device__ __forceinline__ uint4 ld_ragged(const uint8_t* p, uint32_t n) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b)
        if (b < n) w[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3u));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void st_ragged(uint8_t* p, const uint4& v, uint32_t n) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b)
        if (b < n) p[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3u)));
}

// k_verify_mixed's walk (rs_mixed_verify.hip), kept as a copy of its own:
// calling one shared function from both kernels changed k_verify_mixed's
// generated code, which this file must leave as it is.
// addr, len (> 0): the same in the quad's four lanes; q: the lane in its quad.
template <int DEPTH>
__device__ __forceinline__ void hhq_walk(HHQuad& s, uint64_t addr, uint32_t len, uint32_t q) {
    const uint8_t* const msg = (const uint8_t*)(uintptr_t)addr;
    const uint32_t packets = len >> 5, nb = packets >> 3;  // whole packets, whole 8-packet batches
    const uint32_t mis = (uint32_t)(addr & 7u);            // the body's byte offset in its word
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
}

// One unit of every shard of one block, unrolled over its C <= 8 inputs with
// their tables in scalar registers: `bytes` = 16 (FULL) or 1..15.
template <int C, int R, bool FULL>
__device__ __forceinline__ void encode_unit(const EncodeBlocksParams& p, const BlockDesc& d, uint64_t off, uint32_t bytes) {
    uint32_t acc[R][4] = {};
    constexpr int G = 4;  // inputs loaded together
#pragma unroll
    for (int c0 = 0; c0 < C; c0 += G) {
        uint4 x[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            if (c0 + i >= C) break;
            const uint8_t* src = (const uint8_t*)(uintptr_t)d.in[c0 + i] + off;
            x[i] = FULL ? ld16(src) : ld_ragged(src, bytes);
        }
#pragma unroll
        for (int i = 0; i < G; ++i) {
            if (c0 + i >= C) break;
            const int c = c0 + i;
            if (d.copy[c]) {  // wave-uniform
                uint8_t* dst = (uint8_t*)(uintptr_t)d.copy[c] + off;
                if (FULL) st16(dst, x[i]);
                else st_ragged(dst, x[i], bytes);
            }
            const uint32_t w[4] = {x[i].x, x[i].y, x[i].z, x[i].w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t s0 = w[q] & 0x07070707u;
                const uint32_t s1 = (w[q] >> 3) & 0x07070707u;
                const uint32_t s2 = (w[q] >> 6) & 0x03030303u;
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r][q] ^= gf_mul_word(p.tab[r][c], s0, s1, s2);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint4 v = make_uint4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
        uint8_t* dst = (uint8_t*)(uintptr_t)d.out[r] + off;
        if (FULL) st16(dst, v);
        else st_ragged(dst, v, bytes);
        if (d.out2[r]) {  // wave-uniform
            uint8_t* dst2 = (uint8_t*)(uintptr_t)d.out2[r] + off;
            if (FULL) st16(dst2, v);
            else st_ragged(dst2, v, bytes);
        }
    }
}

}  // namespace

template <int C, int R>
__global__ __launch_bounds__(256) void k_encode_blocks(const EncodeBlocksParams p) {
    const uint32_t wg = blockIdx.x;
    // the last block whose first tile is at or below wg (tile0[0] = 0 <= wg < tile0[n])
    uint32_t lo = 0, hi = p.n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (p.tile0[mid] <= wg) lo = mid;
        else hi = mid;
    }
    const BlockDesc& d = p.desc[lo];
    const uint32_t len = d.len;
    const uint64_t off = (uint64_t)(wg - p.tile0[lo]) * kTile + threadIdx.x * 16u;
    if (off >= len) return;
    const uint64_t left = len - off;
    if (left >= 16) encode_unit<C, R, true>(p, d, off, 16);
    else encode_unit<C, R, false>(p, d, off, (uint32_t)left);
}

// More than 8 inputs: rolled over the inputs in groups of G, the next group's
// loads issued before the current group's arithmetic and the tables indexed
// by the scalar loop counter (scalar loads, one group's worth in scalar
// registers), as k_gf_apply_loop (rs_kernels.hip) and for its reason:
// unrolled, the C * R tables no longer fit the scalar registers and are
// parked in ~250 vector registers.  G = 12 for 9..12 inputs (every load in
// flight at once), 8 beyond.  The body stays in the kernel: the tables are
// indexed at run time straight from the kernel arguments.
template <int R, int G>
__global__ __launch_bounds__(256) void k_encode_blocks_loop(const EncodeBlocksParams p) {
    const uint32_t wg = blockIdx.x;
    uint32_t lo = 0, hi = p.n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (p.tile0[mid] <= wg) lo = mid;
        else hi = mid;
    }
    const BlockDesc& d = p.desc[lo];
    const uint32_t len = d.len, C = p.C;
    const uint64_t off = (uint64_t)(wg - p.tile0[lo]) * kTile + threadIdx.x * 16u;
    if (off >= len) return;
    const uint64_t left = len - off;
    const bool full = left >= 16;
    const uint32_t bytes = full ? 16u : (uint32_t)left;
    uint32_t acc[R][4] = {};
    uint4 x[G], y[G];
#pragma unroll
    for (int g = 0; g < G; ++g)
        if ((uint32_t)g < C) {
            const uint8_t* src = (const uint8_t*)(uintptr_t)d.in[g] + off;
            x[g] = full ? ld16(src) : ld_ragged(src, bytes);
        }
#pragma unroll 1
    for (uint32_t c0 = 0; c0 < C; c0 += G) {
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (c0 + G + g < C) {
                const uint8_t* src = (const uint8_t*)(uintptr_t)d.in[c0 + G + g] + off;
                y[g] = full ? ld16(src) : ld_ragged(src, bytes);
            }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const uint32_t c = c0 + g;
            if (c >= C) break;  // wave-uniform
            if (d.copy[c]) {    // wave-uniform
                uint8_t* dst = (uint8_t*)(uintptr_t)d.copy[c] + off;
                if (full) st16(dst, x[g]);
                else st_ragged(dst, x[g], bytes);
            }
            const uint32_t w[4] = {x[g].x, x[g].y, x[g].z, x[g].w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t s0 = w[q] & 0x07070707u;
                const uint32_t s1 = (w[q] >> 3) & 0x07070707u;
                const uint32_t s2 = (w[q] >> 6) & 0x03030303u;
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r][q] ^= gf_mul_word(p.tab[r][c], s0, s1, s2);
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) x[g] = y[g];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint4 v = make_uint4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
        uint8_t* dst = (uint8_t*)(uintptr_t)d.out[r] + off;
        if (full) st16(dst, v);
        else st_ragged(dst, v, bytes);
        if (d.out2[r]) {  // wave-uniform
            uint8_t* dst2 = (uint8_t*)(uintptr_t)d.out2[r] + off;
            if (full) st16(dst2, v);
            else st_ragged(dst2, v, bytes);
        }
    }
}

template <int DEPTH>
__global__ __launch_bounds__(256) void k_hash_blocks(const HashBlocksParams p) {
    const uint64_t j = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 2;
    const uint32_t q = threadIdx.x & 3u;
    if (j >= p.n) return;  // whole quads exit together
    const HashUnit u = p.unit[j];  // the same bytes in the quad's four lanes
    HHQuad s;
    hhq_init(s, p.key, q);
    hhq_walk<DEPTH>(s, u.addr, u.len, q);  // len > 0
    st64_any((uint8_t*)(uintptr_t)u.out + 8 * q, hhq_digest(s, q));
}

namespace {
using EncKernel = void (*)(const EncodeBlocksParams);

template <int R>
EncKernel encode_kernel_c(int C) {
    switch (C) {
#define RSG_BLK_CASE(c) \
    case c: return k_encode_blocks<c, R>;
        RSG_BLK_CASE(1) RSG_BLK_CASE(2) RSG_BLK_CASE(3) RSG_BLK_CASE(4) RSG_BLK_CASE(5) RSG_BLK_CASE(6)
        RSG_BLK_CASE(7) RSG_BLK_CASE(8)
#undef RSG_BLK_CASE
    }
    return C <= 12 ? k_encode_blocks_loop<R, 12> : k_encode_blocks_loop<R, 8>;
}
}  // namespace

hipError_t launch_encode_blocks(EncodeBlocksParams p, int C, int R, uint32_t tiles, hipStream_t stream) {
    if (p.n == 0 || tiles == 0) return hipSuccess;
    p.C = (uint32_t)C;
    if (!p.desc || !p.tile0 || !blocks::kernel_geometry(C, R) || tiles > blocks::kMaxBatchTiles) return hipErrorInvalidValue;
    const EncKernel k = R == 1 ? encode_kernel_c<1>(C) : R == 2 ? encode_kernel_c<2>(C) : R == 3 ? encode_kernel_c<3>(C)
                                                                                                 : encode_kernel_c<4>(C);
    hipLaunchKernelGGL(k, dim3(tiles), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_hash_blocks(const HashBlocksParams& p, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    if (!p.unit || p.n > 0x1fffffffull) return hipErrorInvalidValue;
    const int depth = tuning().hash_depth;
    using Kernel = void (*)(const HashBlocksParams);
    const Kernel k = depth == 1 ? k_hash_blocks<1> : depth == 2 ? k_hash_blocks<2> : k_hash_blocks<3>;
    const uint64_t wgs = (p.n * 4u + 255u) / 256u;  // one quad per unit
    hipLaunchKernelGGL(k, dim3((uint32_t)wgs), dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace rsg
