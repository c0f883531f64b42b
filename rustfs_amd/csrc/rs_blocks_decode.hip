// rs_blocks_decode.hip — the gathered block reconstruct: the lost shards of n
// unrelated degraded blocks, each a list of shard addresses of any alignment
// with its own loss pattern, in one launch (rsg_reconstruct_blocks;
// ReedSolomonEncoder::reconstruct_data / reconstruct per block,
// erasure.rs:411-428).
//
// k_reconstruct_blocks<C> (C = 1..8; k_reconstruct_blocks_loop<G> for
// C = 9..16, rolled over groups of G inputs) is k_encode_blocks
// (rs_blocks.hip) with two things read per entry instead of per launch: the
// coefficient table and the row count.  One workgroup of 256 threads per
// column tile of blocks::kTile bytes of one descriptor entry (a block and up
// to four of its targets), thread t the 16-byte unit t of the tile.  The
// workgroup finds its entry by the same binary search over the prefix sums
// tile0; the search, the entry's fields and its table all depend on
// blockIdx.x alone, so they are scalar loads into scalar registers.  The row
// count R selects one of four unrolled bodies by a branch every lane of the
// workgroup takes alike: an entry with one target does one row's arithmetic.
//
// Loads and stores follow k_encode_blocks' rule: whole units with one 16-byte
// access at the shard's own alignment, the ragged last unit byte by byte, and
// no byte outside [addr, addr + len) of any input or output is touched.  All
// stores are vector stores.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rs_blocks_decode.h"
#include "rs_device.h"

namespace rsg {

using blocks::kTile;
using blocks::RDesc;

namespace {

// The descriptor, tile and coefficient tables are written before the launch
// and never during it: read through the constant address space, a load at a
// workgroup-uniform address is a scalar load whatever stores the kernel makes
// (through a generic pointer the compiler, which cannot tell the outputs from
// the tables, used vector loads with a scalar base for most of them).
#define RSG_CONST_AS __attribute__((address_space(4)))
template <class T>
__device__ __forceinline__ const RSG_CONST_AS T* const_as(const T* p) {
    return (const RSG_CONST_AS T*)p;
}
using CDesc = const RSG_CONST_AS RDesc;
using CTab = const RSG_CONST_AS uint32_t;

// gf_mul_word (rs_device.h) over a table in the constant address space
__device__ __forceinline__ uint32_t gf_mul_tab(CTab* t, uint32_t s0, uint32_t s1, uint32_t s2) {
    return __builtin_amdgcn_perm(t[1], t[0], s0) ^ __builtin_amdgcn_perm(t[3], t[2], s1) ^
           __builtin_amdgcn_perm(t[4], t[4], s2);
}

// the first n (1..15) bytes at p, the rest zero
__device__ __forceinline__ uint4 ldr_ragged(const uint8_t* p, uint32_t n) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b)
        if (b < n) w[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3u));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void str_ragged(uint8_t* p, const uint4& v, uint32_t n) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b)
        if (b < n) p[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3u)));
}

template <int R>
__device__ __forceinline__ void store_rows(CDesc& d, const uint32_t (&acc)[R][4], uint64_t off, bool full, uint32_t bytes) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint4 v = make_uint4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
        uint8_t* dst = (uint8_t*)(uintptr_t)d.out[r] + off;
        if (full) st16(dst, v);
        else str_ragged(dst, v, bytes);
    }
}

// One unit of R targets of one entry, unrolled over its C <= 8 survivors;
// tab: the entry's table [kMaxR][C][5].
template <int C, int R, bool FULL>
__device__ __forceinline__ void recon_unit(CDesc& d, CTab* tab, uint64_t off, uint32_t bytes) {
    uint32_t acc[R][4] = {};
    constexpr int G = 4;  // inputs loaded together
#pragma unroll
    for (int c0 = 0; c0 < C; c0 += G) {
        uint4 x[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            if (c0 + i >= C) break;
            const uint8_t* src = (const uint8_t*)(uintptr_t)d.in[c0 + i] + off;
            x[i] = FULL ? ld16(src) : ldr_ragged(src, bytes);
        }
#pragma unroll
        for (int i = 0; i < G; ++i) {
            if (c0 + i >= C) break;
            const int c = c0 + i;
            const uint32_t w[4] = {x[i].x, x[i].y, x[i].z, x[i].w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t s0 = w[q] & 0x07070707u;
                const uint32_t s1 = (w[q] >> 3) & 0x07070707u;
                const uint32_t s2 = (w[q] >> 6) & 0x03030303u;
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r][q] ^= gf_mul_tab(tab + (r * C + c) * 5, s0, s1, s2);
            }
        }
    }
    store_rows<R>(d, acc, off, FULL, bytes);
}

template <int C, int R>
__device__ __forceinline__ void recon_rows(CDesc& d, CTab* tab, uint64_t off, uint64_t left) {
    if (left >= 16) recon_unit<C, R, true>(d, tab, off, 16);
    else recon_unit<C, R, false>(d, tab, off, (uint32_t)left);
}

// More than 8 survivors: rolled over the inputs in groups of G, the next
// group's loads issued before the current group's arithmetic and the tables
// indexed by the scalar loop counter, as k_encode_blocks_loop and for its
// reason (unrolled, C * R tables do not fit the scalar registers).
template <int R, int G>
__device__ __forceinline__ void recon_loop(CDesc& d, CTab* tab, uint32_t C, uint64_t off,
                                           uint64_t left) {
    const bool full = left >= 16;
    const uint32_t bytes = full ? 16u : (uint32_t)left;
    uint32_t acc[R][4] = {};
    uint4 x[G], y[G];
#pragma unroll
    for (int g = 0; g < G; ++g)
        if ((uint32_t)g < C) {
            const uint8_t* src = (const uint8_t*)(uintptr_t)d.in[g] + off;
            x[g] = full ? ld16(src) : ldr_ragged(src, bytes);
        }
#pragma unroll 1
    for (uint32_t c0 = 0; c0 < C; c0 += G) {
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (c0 + G + g < C) {
                const uint8_t* src = (const uint8_t*)(uintptr_t)d.in[c0 + G + g] + off;
                y[g] = full ? ld16(src) : ldr_ragged(src, bytes);
            }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const uint32_t c = c0 + g;
            if (c >= C) break;  // wave-uniform
            const uint32_t w[4] = {x[g].x, x[g].y, x[g].z, x[g].w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t s0 = w[q] & 0x07070707u;
                const uint32_t s1 = (w[q] >> 3) & 0x07070707u;
                const uint32_t s2 = (w[q] >> 6) & 0x03030303u;
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r][q] ^= gf_mul_tab(tab + ((uint32_t)r * C + c) * 5u, s0, s1, s2);
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) x[g] = y[g];
    }
    store_rows<R>(d, acc, off, full, bytes);
}

// the last entry whose first tile is at or below wg (tile0[0] = 0 <= wg < tile0[n])
__device__ __forceinline__ uint32_t find_entry(CTab* tile0, uint32_t n, uint32_t wg) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tile0[mid] <= wg) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace

template <int C>
__global__ __launch_bounds__(256) void k_reconstruct_blocks(const ReconBlocksParams p) {
    const uint32_t wg = blockIdx.x;
    CTab* tile0 = const_as(p.tile0);
    const uint32_t e = find_entry(tile0, p.n, wg);
    CDesc& d = const_as(p.desc)[e];
    const uint32_t len = d.len;
    const uint64_t off = (uint64_t)(wg - tile0[e]) * kTile + threadIdx.x * 16u;
    if (off >= len) return;
    const uint64_t left = len - off;
    CTab* tab = const_as(p.tab) + (uint64_t)d.tab * (uint32_t)(blocks::kMaxR * C * 5);
    switch (d.rows) {  // the same in every lane of the workgroup
        case 1: recon_rows<C, 1>(d, tab, off, left); break;
        case 2: recon_rows<C, 2>(d, tab, off, left); break;
        case 3: recon_rows<C, 3>(d, tab, off, left); break;
        case 4: recon_rows<C, 4>(d, tab, off, left); break;
    }
}

template <int G>
__global__ __launch_bounds__(256) void k_reconstruct_blocks_loop(const ReconBlocksParams p) {
    const uint32_t wg = blockIdx.x;
    CTab* tile0 = const_as(p.tile0);
    const uint32_t e = find_entry(tile0, p.n, wg);
    CDesc& d = const_as(p.desc)[e];
    const uint32_t len = d.len, C = p.C;
    const uint64_t off = (uint64_t)(wg - tile0[e]) * kTile + threadIdx.x * 16u;
    if (off >= len) return;
    const uint64_t left = len - off;
    CTab* tab = const_as(p.tab) + (uint64_t)d.tab * ((uint32_t)blocks::kMaxR * C * 5u);
    switch (d.rows) {  // the same in every lane of the workgroup
        case 1: recon_loop<1, G>(d, tab, C, off, left); break;
        case 2: recon_loop<2, G>(d, tab, C, off, left); break;
        case 3: recon_loop<3, G>(d, tab, C, off, left); break;
        case 4: recon_loop<4, G>(d, tab, C, off, left); break;
    }
}

hipError_t launch_reconstruct_blocks(const ReconBlocksParams& p, uint32_t tiles, hipStream_t stream) {
    if (p.n == 0 || tiles == 0) return hipSuccess;
    const int C = (int)p.C;
    if (!p.desc || !p.tile0 || !p.tab || C < 1 || C > blocks::kMaxC || tiles > blocks::kMaxBatchTiles) return hipErrorInvalidValue;
    using Kernel = void (*)(const ReconBlocksParams);
    Kernel k = C <= 12 ? k_reconstruct_blocks_loop<12> : k_reconstruct_blocks_loop<8>;
    switch (C) {
#define RSG_RBLK_CASE(c) \
    case c: k = k_reconstruct_blocks<c>; break;
        RSG_RBLK_CASE(1) RSG_RBLK_CASE(2) RSG_RBLK_CASE(3) RSG_RBLK_CASE(4) RSG_RBLK_CASE(5) RSG_RBLK_CASE(6)
        RSG_RBLK_CASE(7) RSG_RBLK_CASE(8)
#undef RSG_RBLK_CASE
    }
    hipLaunchKernelGGL(k, dim3(tiles), dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace rsg
