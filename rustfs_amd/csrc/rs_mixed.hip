// rs_mixed.hip — mixed-length fused RS encode + per-shard HighwayHash-256:
// one launch over n unrelated stripes, each with its own shard length (the
// small objects of encode_inline_shards_with_size_hint, encode.rs:601-628, and
// the short last blocks of encode_batched, erasure.rs:848-887).
//
// k_encode_hash_mixed<C,R,SPW> keeps the structure of the packed kernel
// k_encode_hash_fused (rs_kernels.hip): SPW encoder waves (one per stripe),
// ceil(SPW*T/16) hasher waves (one 4-lane quad per shard stream), coefficient
// tables then SPW x T rows of kFusedPitch in LDS, an A/B barrier pair per
// 512-byte chunk.  What differs is where a stripe lives and how long it is:
// a per-stripe descriptor table in device memory (mixed::MixedDesc) gives
//   data shard c    at data   + data_off   + c*len
//   parity shard r  at parity + parity_off + r*len
//   digests         at out + (job*T + shard)*32
// and a stripe's chunk count and tail come from its own len.
//
// Barrier count: every wave of a workgroup runs exactly 2*wg_chunks
// lds_barrier() calls, wg_chunks = the maximum chunk count over the
// workgroup's SPW descriptors (len = 0 past the end of the table).  Every wave
// computes wg_chunks from the same descriptor words and makes it wave-uniform
// with readfirstlane; no barrier sits under a condition on a stripe's own
// length, on `live` or on a lane.  A stripe with fewer chunks keeps its
// encoder wave in the sequence with loads, stores and LDS writes masked; its
// hasher quads finish (tail packets, remainder, digest) at their own last
// chunk, inside the barrier-free part of the step, and then only pass barriers.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rs_device.h"
#include "rs_mixed.h"

namespace rsg {

using mixed::MixedDesc;

// chunk count of descriptor idx of the table (0 past its end)
__device__ __forceinline__ uint32_t desc_chunks(const MixedDesc* desc, uint64_t idx, uint64_t n) {
    const uint32_t len = idx < n ? desc[idx].len : 0u;
    return (len >> 9) + ((len & (kFusedChunk - 1)) ? 1u : 0u);
}

// Waves per SIMD asked of the register allocator: the packed kernel's rule up
// to C = 10.  Wider geometries need more registers here than there (RS(12,4)
// 111 VGPRs against 92, RS(16,4) 144 against 109: the three-way chunk load
// keeps more per-shard addresses live) and take the next budget up, so that
// no instantiation uses scratch (profiles/r07/mixed/README.md).
constexpr int mixed_waves_per_eu(int C, int R) { return C > 14 ? 3 : R == 1 ? 4 : C <= 8 ? 7 : C <= 10 ? 5 : 4; }

template <int C, int R, int SPW>
__global__ __launch_bounds__(64 * (SPW + (SPW * (C + R) + 15) / 16))
__attribute__((amdgpu_waves_per_eu(mixed_waves_per_eu(C, R))))
void k_encode_hash_mixed(const GfApplyParams p, const HashParams h, const MixedDesc* __restrict__ desc, const uint64_t n) {
    // LDS: [C][R] coefficient tables (32 B each), then SPW x (C+R) chunk rows
    extern __shared__ uint8_t lds_all[];
    constexpr int T = C + R;
    constexpr uint32_t kTabBytes = C * R * 32;
    constexpr uint32_t kStripeRows = T * kFusedPitch;
    uint8_t* rows = lds_all + kTabBytes;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u, q = lane & 3u;
    const uint64_t first = (uint64_t)blockIdx.x * SPW;

    for (uint32_t i = threadIdx.x; i < (uint32_t)(C * R); i += blockDim.x) {
        const int c = i / R, r = i % R;
        uint8_t* d = lds_all + i * 32;
        *(uint4*)d = make_uint4(p.tab[r][c][0], p.tab[r][c][1], p.tab[r][c][2], p.tab[r][c][3]);
        *(uint32_t*)(d + 16) = p.tab[r][c][4];
    }
    __syncthreads();

    // The workgroup's step count: the same SPW descriptor words in every wave.
    uint32_t wgc = 0;
#pragma unroll
    for (int s = 0; s < SPW; ++s) {
        const uint32_t c = desc_chunks(desc, first + s, n);
        wgc = c > wgc ? c : wgc;
    }
    const uint32_t wg_chunks = uniform32(wgc);

    if (wave < (uint32_t)SPW) {
        // ------------------------------ encoder ------------------------------
        const uint64_t idx = first + wave;
        const bool live = idx < n;
        // the stripe's descriptor, wave-uniform (scalar registers)
        const uint64_t S = uniform32(live ? desc[idx].len : 0u);  // 0: no chunk, no memory access
        const uint32_t my_chunks = (uint32_t)(S >> 9) + ((S & (kFusedChunk - 1)) ? 1u : 0u);
        const uint8_t* db = p.base + uniform64(live ? desc[idx].data_off : 0);
        uint8_t* pb = p.out_base + uniform64(live ? desc[idx].parity_off : 0);
        uint8_t* my_rows = rows + wave * kStripeRows;
        const uint32_t m7 = vgpr_const(0x07070707u), m3 = vgpr_const(0x03030303u);
        // the GF rows of one chunk (x: 8 bytes of every data shard per lane)
        auto rows_of = [&](const uint2 (&x)[C], uint32_t (&acc)[R][2]) {
            // opaque per-iteration zero: keeps the table reads at their use
            // instead of hoisted out of the loop into (spilled) registers
            uint32_t tz;
            asm volatile("s_mov_b32 %0, 0" : "=s"(tz));
            const uint8_t* tabs = lds_all + tz;
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
        };
        // Chunk ch of the k data shards, fetched one step ahead (in flight
        // across the barriers): whole 8-byte loads while the chunk ends at or
        // before S.  The partial last chunk reads nothing at or past S and
        // yields zeros there, so the parity bytes past S are zero too.
        auto load_chunk = [&](uint2 (&v)[C], uint32_t ch) {
            const uint64_t off = (uint64_t)ch * kFusedChunk + lane * 8u;
            if (((uint64_t)ch + 1) * kFusedChunk <= S) {  // wave-uniform
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = __builtin_bit_cast(uint2, ld64_any(db + (uint64_t)c * S + off));
            } else if (S >= 8) {  // wave-uniform
                // The lane that straddles S loads the shard's last 8 bytes and
                // shifts out those before its offset; lanes at or past S load
                // them too and shift everything out.  (Byte-wise loads, 8 per
                // shard in flight beside the current chunk, cost 26 VGPRs more
                // at C = 8.)
                const bool in = off + 8 <= S;
                const uint64_t at = in ? off : S - 8;
                const uint64_t drop = in ? 0u : (off < S ? off + 8 - S : 8u);  // bytes before `off`
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const uint64_t w = ld64_any(db + (uint64_t)c * S + at);
                    v[c] = __builtin_bit_cast(uint2, drop < 8 ? w >> (8 * (uint32_t)drop) : 0ull);
                }
            } else {  // a shard of 1..7 bytes: lane 0 gathers it byte by byte
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = make_uint2(0u, 0u);
#pragma unroll 1
                for (uint32_t b = 0; b < (uint32_t)S; ++b) {
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const uint32_t byte = lane == 0 ? (uint32_t)db[(uint64_t)c * S + b] : 0u;
                        if (b < 4) v[c].x |= byte << (8 * b);
                        else v[c].y |= byte << (8 * (b - 4));
                    }
                }
            }
        };
        uint2 x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = make_uint2(0u, 0u);
        if (my_chunks) load_chunk(x, 0);
#pragma unroll 1
        for (uint32_t ch = 0; ch < wg_chunks; ++ch) {
            const bool act = ch < my_chunks;      // wave-uniform
            const bool nxt = ch + 1 < my_chunks;  // wave-uniform
            uint32_t acc[R][2];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r][0] = acc[r][1] = 0u;
            if (act) {
                const uint64_t off = (uint64_t)ch * kFusedChunk + lane * 8u;
                rows_of(x, acc);
                if (((uint64_t)ch + 1) * kFusedChunk <= S) {
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        st64_any(pb + (uint64_t)r * S + off, (uint64_t)acc[r][0] | ((uint64_t)acc[r][1] << 32));
                } else {  // the partial last chunk: nothing written at or past S
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        st64_part(pb + (uint64_t)r * S + off, (uint64_t)acc[r][0] | ((uint64_t)acc[r][1] << 32), off, S);
                }
            }
            uint2 y[C];
            if (nxt) load_chunk(y, ch + 1);  // in flight across the barriers
            lds_barrier();  // A: the hashers are done with the previous chunk's rows
            if (act) {
#pragma unroll
                for (int c = 0; c < C; ++c) *(uint2*)(my_rows + c * kFusedPitch + lane * 8u) = x[c];
#pragma unroll
                for (int r = 0; r < R; ++r)
                    *(uint2*)(my_rows + (C + r) * kFusedPitch + lane * 8u) = make_uint2(acc[r][0], acc[r][1]);
            }
            lds_barrier();  // B: this chunk's rows are ready
            if (nxt) {
#pragma unroll
                for (int c = 0; c < C; ++c) x[c] = y[c];
            }
        }
    } else {
        // ------------------------------ hasher -------------------------------
        const uint32_t g = (wave - SPW) * 16u + (lane >> 2);  // stream of this quad
        const uint32_t ls = g / T, shard = g - ls * T;        // local stripe, shard
        const uint64_t idx = first + ls;
        // no digest wanted (h.out null): the hasher waves only pass the barriers
        const bool live = h.out != nullptr && g < (uint32_t)(SPW * T) && idx < n;
        const uint32_t len = live ? desc[idx].len : 0u;
        const uint32_t job = live ? desc[idx].job : 0u;
        const uint32_t my_chunks = (len >> 9) + ((len & (kFusedChunk - 1)) ? 1u : 0u);  // per quad
        const uint32_t tail = my_chunks ? len - (my_chunks - 1) * kFusedChunk : 0u;     // 1..512
        const uint8_t* row0 = rows + (live ? ls * kStripeRows + shard * kFusedPitch : 0);
        const uint8_t* row = row0 + 8 * q;
        uint8_t* dig = h.out + ((uint64_t)job * T + shard) * 32u;
        HHQuad st;
        hhq_init(st, h.key, q);
        if (live && my_chunks == 0) hhq_finish(st, dig, q);  // the empty message
#pragma unroll 1
        for (uint32_t ch = 0; ch < wg_chunks; ++ch) {
            lds_barrier();  // A
            lds_barrier();  // B
            if (live && ch + 1 < my_chunks) {
#pragma unroll 4
                for (int t = 0; t < (int)(kFusedChunk / 32); ++t)
                    hhq_update(st, __builtin_bit_cast(uint64_t, *(const u32x2*)(row + t * 32)));
            } else if (live && ch + 1 == my_chunks) {
                // this stream's last chunk: whole packets, the remainder
                // packet, the digest; afterwards the quad only passes barriers
                const uint32_t full = tail / 32;
#pragma unroll 1
                for (uint32_t t = 0; t < full; ++t) hhq_update(st, __builtin_bit_cast(uint64_t, *(const u32x2*)(row + t * 32)));
                if (tail % 32) hhq_remainder(st, row0 + full * 32, tail % 32, q);
                hhq_finish(st, dig, q);
            }
        }
    }
}

using MixedKernel = void (*)(const GfApplyParams, const HashParams, const MixedDesc*, const uint64_t);

struct MixedPick {
    MixedKernel k;
    int spw, waves;
};

template <int C, int R>
static MixedPick mixed_entry() {
    constexpr int spw = mixed::spw_for(C + R);
    return {k_encode_hash_mixed<C, R, spw>, spw, spw + (spw * (C + R) + 15) / 16};
}

template <int C>
static MixedPick pick_mixed_r(int R) {
    switch (R) {
        case 1: return mixed_entry<C, 1>();
        case 2: return mixed_entry<C, 2>();
        case 3: return mixed_entry<C, 3>();
        case 4: return mixed_entry<C, 4>();
    }
    return {nullptr, 0, 0};
}

static MixedPick pick_mixed(int C, int R) {
    switch (C) {
        case 1: return pick_mixed_r<1>(R);
        case 2: return pick_mixed_r<2>(R);
        case 3: return pick_mixed_r<3>(R);
        case 4: return pick_mixed_r<4>(R);
        case 5: return pick_mixed_r<5>(R);
        case 6: return pick_mixed_r<6>(R);
        case 7: return pick_mixed_r<7>(R);
        case 8: return pick_mixed_r<8>(R);
        case 9: return pick_mixed_r<9>(R);
        case 10: return pick_mixed_r<10>(R);
        case 11: return pick_mixed_r<11>(R);
        case 12: return pick_mixed_r<12>(R);
        case 13: return pick_mixed_r<13>(R);
        case 14: return pick_mixed_r<14>(R);
        case 15: return pick_mixed_r<15>(R);
        case 16: return pick_mixed_r<16>(R);
    }
    return {nullptr, 0, 0};
}

hipError_t launch_encode_hash_mixed(GfApplyParams p, HashParams h, const mixed::MixedDesc* d_desc, uint64_t n,
                                    hipStream_t stream) {
    if (!mixed::kernel_geometry((int)p.C, (int)p.R) || !d_desc || n == 0 || n > 0x7fffffffull)
        return hipErrorInvalidValue;
    const MixedPick f = pick_mixed((int)p.C, (int)p.R);
    if (!f.k) return hipErrorInvalidValue;
    const size_t lds = (size_t)p.C * p.R * 32 + (size_t)f.spw * (p.C + p.R) * kFusedPitch;
    const uint64_t blocks = (n + f.spw - 1) / f.spw;
    hipLaunchKernelGGL(f.k, dim3((uint32_t)blocks), dim3(64 * f.waves), lds, stream, p, h, d_desc, n);
    return hipGetLastError();
}

}  // namespace rsg
