// rs_fused.h — what the fused encode / verify kernels share: the packed
// k_encode_hash_fused (rs_kernels.hip), the mixed-length k_encode_hash_mixed
// (rs_mixed.hip) and k_decode_mixed (rs_mixed_decode.hip).  All three walk
// their stripes in kFusedChunk-byte steps with GF waves that stage the step's
// rows in LDS and hasher waves (one 4-lane quad per row) that hash them there.
//
// The first part is plain C++17 (the host planners rs_mixed_plan.h and
// rs_mixed_decode_plan.h use it and compile without HIP): the step geometry
// and the run-time to compile-time dispatch of the launchers.  The second
// part, device code, is the kernels' common inner parts.  The mixed kernels'
// three-form tail loaders (load_chunk) are not here: the decode kernel's form
// (scalar 64-bit base per row + 32-bit lane offset) costs the encode kernel
// registers and scratch (profiles/r08/fused_parts/README.md).  Internal.
#pragma once

#include <stdint.h>

#include <type_traits>

namespace rsg {

constexpr uint32_t kFusedChunk = 512;               // bytes per shard per step
constexpr uint32_t kFusedPitch = kFusedChunk + 32;  // LDS row pitch: conflict-free ds_read_b64

// stripes per workgroup for T rows per stripe: fill the hasher waves, cap LDS
constexpr int fused_spw_for(int T) { return (T % 16 == 0) ? 1 : (T % 8 == 0) ? 2 : (T % 4 == 0 || T <= 6) ? 4 : 2; }

// ceil(len / kFusedChunk) without overflow at len = 0xffffffff; 0 for an empty shard
constexpr uint32_t fused_chunks(uint64_t len) {
    return (uint32_t)(len / kFusedChunk) + (len % kFusedChunk ? 1u : 0u);
}

// f(std::integral_constant<int, v>()) for a run-time v in [Lo, Hi], `none`
// for any other: the launchers' step from run-time C, R to an instantiation.
template <int Lo, int Hi, class Ret, class F>
Ret dispatch_int(int v, Ret none, F&& f) {
    if constexpr (Lo > Hi) {
        return none;
    } else {
        if (v == Lo) return f(std::integral_constant<int, Lo>());
        return dispatch_int<Lo + 1, Hi>(v, none, f);
    }
}

}  // namespace rsg

#ifdef __HIPCC__

#include "rs_device.h"

namespace rsg {

// The [C][R] coefficient tables (32 B each: T0 T0' T1 T1' | T2) from the
// kernel's arguments to the front of LDS, by the whole workgroup; the caller
// runs a barrier before fused_gf_rows reads them.  Tables are read from LDS
// (broadcast) at their use: held in registers across the chunk loop they cost
// 64+ VGPRs.  R = 0: nothing.
template <int C, int R, int NR, int NC>
__device__ __forceinline__ void fused_tables_to_lds(const uint32_t (&tab)[NR][NC][5], uint8_t* lds) {
    static_assert(R <= NR && C <= NC, "table extents");
    if constexpr (R > 0) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)(C * R); i += blockDim.x) {
            const int c = i / R, r = i % R;
            uint8_t* d = lds + i * 32;
            *(uint4*)d = make_uint4(tab[r][c][0], tab[r][c][1], tab[r][c][2], tab[r][c][3]);
            *(uint32_t*)(d + 16) = tab[r][c][4];
        }
    }
}

// The R GF rows of one chunk: acc[r] = sum over c < C of tab[r][c] * x[c]
// (x: 8 bytes of every input per lane; m7, m3: vgpr_const 0x07070707 and
// 0x03030303; lds_tabs: where fused_tables_to_lds put the tables).
template <int C, int R, int NX, int NA>
__device__ __forceinline__ void fused_gf_rows(const uint8_t* lds_tabs, uint32_t m7, uint32_t m3, const uint2 (&x)[NX],
                                              uint32_t (&acc)[NA][2]) {
    static_assert(C <= NX && R <= NA, "array extents");
    if constexpr (R > 0) {
        // opaque per-iteration zero: keeps the table reads at their use
        // instead of hoisted out of the loop into (spilled) registers
        uint32_t tz;
        asm volatile("s_mov_b32 %0, 0" : "=s"(tz));
        const uint8_t* tabs = lds_tabs + tz;
        uint32_t pend[R][2];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][0] = acc[r][1] = pend[r][0] = pend[r][1] = 0u;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const uint32_t s0a = x[c].x & m7, s0b = x[c].y & m7;
            const uint32_t s1a = (x[c].x >> 3) & m7, s1b = (x[c].y >> 3) & m7;
            const uint32_t s2a = (x[c].x >> 6) & m3, s2b = (x[c].y >> 6) & m3;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint8_t* tp = tabs + (c * R + r) * 32;  // wave-uniform: broadcast read
                const uint4 t4 = *(const uint4*)tp;
                const uint32_t t2 = *(const uint32_t*)(tp + 16);
                gf_fold(c & 1, acc[r][0], pend[r][0], __builtin_amdgcn_perm(t4.y, t4.x, s0a),
                        __builtin_amdgcn_perm(t4.w, t4.z, s1a), __builtin_amdgcn_perm(t2, t2, s2a));
                gf_fold(c & 1, acc[r][1], pend[r][1], __builtin_amdgcn_perm(t4.y, t4.x, s0b),
                        __builtin_amdgcn_perm(t4.w, t4.z, s1b), __builtin_amdgcn_perm(t2, t2, s2b));
            }
        }
        if constexpr (C % 2 == 1) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                acc[r][0] ^= pend[r][0];
                acc[r][1] ^= pend[r][1];
            }
        }
    }
}

// A hasher quad's walk over its row of one workgroup: lane q of the quad,
// stream state st (hhq_init done), the row's LDS chunk at row0, my_chunks
// chunks of which the last holds `tail` bytes (1..512), nothing to do when
// !live.  finish() ends the stream (digest out, or digest compared).
//
// Barrier count: a hasher wave runs exactly 2*wg_chunks lds_barrier() calls
// here, and a GF wave of the same workgroup runs the same A/B pair in each of
// its wg_chunks steps.  wg_chunks is the maximum chunk count over the
// workgroup's stripes, which every wave computes from the same descriptor
// words and makes wave-uniform with readfirstlane; no barrier sits under a
// condition on a stripe's own length, on `live` or on a lane.  A stream with
// fewer chunks finishes (tail packets, remainder, finish) at its own last
// chunk, inside the barrier-free part of the step, and then only passes
// barriers.
template <class Finish>
__device__ __forceinline__ void fused_hash_stream(HHQuad& st, const uint8_t* row0, uint32_t q, bool live,
                                                  uint32_t my_chunks, uint32_t tail, uint32_t wg_chunks,
                                                  Finish&& finish) {
    const uint8_t* row = row0 + 8 * q;
    if (live && my_chunks == 0) finish();  // the empty message
#pragma unroll 1
    for (uint32_t ch = 0; ch < wg_chunks; ++ch) {
        lds_barrier();  // A: the GF waves write this chunk's rows after it
        lds_barrier();  // B: this chunk's rows are ready
        if (live && ch + 1 < my_chunks) {
#pragma unroll 4
            for (int t = 0; t < (int)(kFusedChunk / 32); ++t)
                hhq_update(st, __builtin_bit_cast(uint64_t, *(const u32x2*)(row + t * 32)));
        } else if (live && ch + 1 == my_chunks) {
            // this stream's last chunk: whole packets, the remainder packet,
            // the digest; afterwards the quad only passes barriers
            const uint32_t full = tail / 32;
#pragma unroll 1
            for (uint32_t t = 0; t < full; ++t)
                hhq_update(st, __builtin_bit_cast(uint64_t, *(const u32x2*)(row + t * 32)));
            if (tail % 32) hhq_remainder(st, row0 + full * 32, tail % 32, q);
            finish();
        }
    }
}

}  // namespace rsg

#endif  // __HIPCC__
