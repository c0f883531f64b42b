// rs_mixed.hip — mixed-length fused RS encode + per-shard HighwayHash-256:
// one launch over n unrelated stripes, each with its own shard length (the
// small objects of encode_inline_shards_with_size_hint, encode.rs:601-628, and
// the short last blocks of encode_batched, erasure.rs:848-887).
//
// k_encode_hash_mixed<C,R,SPW> is one of the three fused kernels built from
// the parts in rs_fused.h (table fill, GF rows, hasher walk, step geometry;
// the three-form tail loader stays per kernel): SPW encoder waves (one per stripe), ceil(SPW*T/16) hasher waves
// (one 4-lane quad per shard stream), coefficient tables then SPW x T rows of
// kFusedPitch in LDS, an A/B barrier pair per 512-byte chunk.  Against the
// packed kernel k_encode_hash_fused (rs_kernels.hip) what differs is where a
// stripe lives and how long it is: a per-stripe descriptor table in device
// memory (mixed::MixedDesc) gives
//   data shard c    at data   + data_off   + c*len
//   parity shard r  at parity + parity_off + r*len
//   digests         at out + (job*T + shard)*32
// and a stripe's chunk count and tail come from its own len.
//
// Barrier count: one __syncthreads(), then every wave of a workgroup runs
// exactly 2*wg_chunks lds_barrier() calls (the argument stands at
// fused_hash_stream, rs_fused.h), wg_chunks = the maximum chunk count over the
// workgroup's SPW descriptors (len = 0 past the end of the table).  A stripe
// with fewer chunks keeps its encoder wave in the sequence with loads, stores
// and LDS writes masked.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rs_device.h"
#include "rs_fused.h"
#include "rs_mixed.h"

namespace rsg {

using mixed::MixedDesc;

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

    fused_tables_to_lds<C, R>(p.tab, lds_all);
    __syncthreads();

    // The workgroup's step count: the same SPW descriptor words in every wave
    // (no chunk past the end of the table).
    uint32_t wgc = 0;
#pragma unroll
    for (int s = 0; s < SPW; ++s) {
        const uint32_t c = fused_chunks(first + s < n ? desc[first + s].len : 0u);
        wgc = c > wgc ? c : wgc;
    }
    const uint32_t wg_chunks = uniform32(wgc);

    if (wave < (uint32_t)SPW) {
        // ------------------------------ encoder ------------------------------
        const uint64_t idx = first + wave;
        const bool live = idx < n;
        // the stripe's descriptor, wave-uniform (scalar registers)
        const uint64_t S = uniform32(live ? desc[idx].len : 0u);  // 0: no chunk, no memory access
        const uint32_t my_chunks = fused_chunks(S);
        const uint8_t* db = p.base + uniform64(live ? desc[idx].data_off : 0);
        uint8_t* pb = p.out_base + uniform64(live ? desc[idx].parity_off : 0);
        uint8_t* my_rows = rows + wave * kStripeRows;
        const uint32_t m7 = vgpr_const(0x07070707u), m3 = vgpr_const(0x03030303u);
        // Chunk ch of the k data shards, fetched one step ahead (in flight
        // across the barriers): whole 8-byte loads while the chunk ends at or
        // before S.  The partial last chunk reads nothing at or past S and
        // yields zeros there, so the parity bytes past S are zero too.
        // (Its own loader: k_decode_mixed's address form spills here, rs_fused.h.)
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
                fused_gf_rows<C, R>(lds_all, m7, m3, x, acc);
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
        const uint32_t my_chunks = fused_chunks(len);                                // per quad
        const uint32_t tail = my_chunks ? len - (my_chunks - 1) * kFusedChunk : 0u;  // 1..512
        const uint8_t* row0 = rows + (live ? ls * kStripeRows + shard * kFusedPitch : 0);
        uint8_t* dig = h.out + ((uint64_t)job * T + shard) * 32u;
        HHQuad st;
        hhq_init(st, h.key, q);
        fused_hash_stream(st, row0, q, live, my_chunks, tail, wg_chunks, [&] { hhq_finish(st, dig, q); });
    }
}

using MixedKernel = void (*)(const GfApplyParams, const HashParams, const MixedDesc*, const uint64_t);

struct MixedPick {
    MixedKernel k;
    int spw, waves;
};

template <int C, int R>
static MixedPick mixed_entry() {
    constexpr int spw = fused_spw_for(C + R);
    return {k_encode_hash_mixed<C, R, spw>, spw, spw + (spw * (C + R) + 15) / 16};
}

static MixedPick pick_mixed(int C, int R) {
    return dispatch_int<1, 16>(C, MixedPick{}, [R](auto c) {
        return dispatch_int<1, 4>(R, MixedPick{},
                                  [](auto r) { return mixed_entry<decltype(c)::value, decltype(r)::value>(); });
    });
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
