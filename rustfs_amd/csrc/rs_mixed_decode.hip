// rs_mixed_decode.hip — mixed-length batch GET: verify-before-use of
// [digest][shard] records (bitrot.rs:139-247) and the rebuild of the data
// shards no verified record serves (erasure.rs:935-973), over n unrelated
// stripes in one launch, each with its own shard length.
//
// k_decode_mixed<C,R,SPW> keeps the structure of k_encode_hash_mixed
// (rs_mixed.hip): SPW GF waves (one per stripe), ceil(SPW*T/16) hasher waves
// (one 4-lane quad per row, T = C + R), coefficient tables, then the records'
// 32-byte headers, then SPW x T rows of kFusedPitch in LDS, an A/B barrier
// pair per 512-byte chunk, a per-stripe descriptor table in device memory
// (mixed::DecDesc).  One launch serves one mask group, so every stripe of a
// workgroup shares the decode plan (DecodeMixedParams, rs_mixed.h):
//   row c < C      source c: read from file[c], hashed, input of the GF rows
//   row C + r, r < e   rebuilt data shard lost[r]: computed, stored to out
//   row C + r, r >= e  surplus shard: read from file[C + r], hashed, and
//                      compared with computed row r
// The GF wave loads every row that is read straight from the record files
// (any byte alignment, one step ahead), and the hashers hash the same bytes
// out of LDS, so what is used is what was verified.  R = 0 only verifies.
//
// Barrier count: every wave of a workgroup runs one __syncthreads() and then
// exactly 2*wg_chunks lds_barrier() calls, wg_chunks = the maximum chunk count
// over the workgroup's SPW descriptors (len = 0 past the end of the table),
// made wave-uniform with readfirstlane from the same descriptor words in
// every wave.  No barrier sits under a condition on a stripe's own length, on
// `live`, on the plan or on a lane.
//
// Built in kMdecParts (4) translation units: part i (RSG_MDEC_PART=i)
// instantiates C = i+1, i+1+PARTS, ...; without RSG_MDEC_PART: the launcher.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rs_device.h"
#include "rs_mixed.h"

namespace rsg {

using mixed::DecDesc;

constexpr int kMdecParts = 4;

using DecodeMixedKernel = void (*)(const DecodeMixedParams, const DecDesc*, const uint64_t);

struct DecodeMixedPick {
    DecodeMixedKernel k;
    int spw, waves;
};

#define RSG_MDEC_PART_DECL(i) DecodeMixedPick pick_decode_mixed_part##i(int C, int R);
RSG_MDEC_PART_DECL(0)
RSG_MDEC_PART_DECL(1)
RSG_MDEC_PART_DECL(2)
RSG_MDEC_PART_DECL(3)
#undef RSG_MDEC_PART_DECL

#ifdef RSG_MDEC_PART

// chunk count of descriptor idx of the table (0 past its end)
__device__ __forceinline__ uint32_t dec_chunks(const DecDesc* desc, uint64_t idx, uint64_t n) {
    const uint32_t len = idx < n ? desc[idx].len : 0u;
    return (len >> 9) + ((len & (kFusedChunk - 1)) ? 1u : 0u);
}

// Waves per SIMD asked of the register allocator: per geometry, the highest
// request at which the resource-usage report shows no scratch
// (profiles/r07/mixed_get/resource_usage.txt).  The GF wave holds two chunks
// of every row it reads (the current one and the one in flight) and a 64-bit
// address per row, about 10 VGPRs per source, so wide geometries take lower
// requests than the encode kernel's.
constexpr int decode_mixed_waves_per_eu(int C, int R) {
#ifdef RSG_MDEC_WPE  // the sweep behind the table
    return RSG_MDEC_WPE + 0 * (C + R);
#else
    constexpr int8_t w[mixed::kDecMaxR + 1][mixed::kDecMaxC] = {
        {8, 8, 8, 8, 8, 8, 8, 7, 5, 4, 4, 4, 3, 3, 3, 3},
        {8, 8, 8, 7, 6, 5, 5, 4, 4, 3, 3, 3, 3, 2, 2, 2},
        {8, 7, 6, 5, 5, 5, 4, 4, 3, 3, 3, 3, 2, 2, 2, 2},
        {7, 5, 5, 5, 4, 4, 4, 3, 3, 3, 3, 2, 2, 2, 2, 2},
        {5, 4, 4, 4, 4, 4, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2},
    };
    return w[R][C - 1];
#endif
}

template <int C, int R, int SPW>
__global__ __launch_bounds__(64 * (SPW + (SPW * (C + R) + 15) / 16))
__attribute__((amdgpu_waves_per_eu(decode_mixed_waves_per_eu(C, R))))
void k_decode_mixed(const DecodeMixedParams p, const DecDesc* __restrict__ desc, const uint64_t n) {
    // LDS: [C][R] coefficient tables (32 B each), SPW x T record headers
    // (32 B each), then SPW x T chunk rows
    extern __shared__ uint8_t lds_all[];
    constexpr int T = C + R;
    constexpr int RR = R ? R : 1;  // array extents
    constexpr uint32_t kTabBytes = C * R * 32;
    constexpr uint32_t kHdrBytes = SPW * T * 32;
    constexpr uint32_t kStripeRows = T * kFusedPitch;
    uint8_t* hdrs = lds_all + kTabBytes;
    uint8_t* rows = hdrs + kHdrBytes;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u, q = lane & 3u;
    const uint64_t first = (uint64_t)blockIdx.x * SPW;
    const uint32_t e = p.e;  // rows r < e are stored, rows r >= e compared
    // row `row` is read from its file (wave-uniform; `row` a constant after unrolling)
    auto is_read = [&](int row) { return row < C || (uint32_t)(row - C) >= e; };

    if constexpr (R > 0) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)(C * R); i += blockDim.x) {
            const int c = i / R, r = i % R;
            uint8_t* d = lds_all + i * 32;
            *(uint4*)d = make_uint4(p.tab[r][c][0], p.tab[r][c][1], p.tab[r][c][2], p.tab[r][c][3]);
            *(uint32_t*)(d + 16) = p.tab[r][c][4];
        }
    }

    // The workgroup's step count: the same SPW descriptor words in every wave.
    uint32_t wgc = 0;
#pragma unroll
    for (int s = 0; s < SPW; ++s) {
        const uint32_t c = dec_chunks(desc, first + s, n);
        wgc = c > wgc ? c : wgc;
    }
    const uint32_t wg_chunks = uniform32(wgc);

    // The GF wave's stripe (wave-uniform, scalar registers); zeros in a hasher wave.
    const bool gf = wave < (uint32_t)SPW;
    const uint64_t gidx = first + wave;
    const bool glive = gf && gidx < n;
    const uint64_t S = uniform32(glive ? desc[gidx].len : 0u);  // 0: no chunk
    const uint64_t rec = uniform64(glive ? desc[gidx].rec_off : 0);
    const uint64_t oo = uniform64(glive ? desc[gidx].out_off : 0);
    const uint32_t gjob = uniform32(glive ? desc[gidx].job : 0u);
    if (glive && lane < 4) {
        // the records' headers, for the hashers to compare their digests with
#pragma unroll
        for (int row = 0; row < T; ++row)
            if (is_read(row))
                *(uint64_t*)(hdrs + (wave * T + row) * 32 + lane * 8) = ld64_any(p.file[row] + rec + lane * 8u);
    }
    __syncthreads();

    if (gf) {
        // ------------------------------ GF wave ------------------------------
        const uint32_t my_chunks = (uint32_t)(S >> 9) + ((S & (kFusedChunk - 1)) ? 1u : 0u);
        uint8_t* ob = p.out + oo;
        uint8_t* my_rows = rows + wave * kStripeRows;
        const uint32_t m7 = vgpr_const(0x07070707u), m3 = vgpr_const(0x03030303u);
        // the R computed rows of one chunk (x: 8 bytes of every source per lane)
        auto rows_of = [&](const uint2 (&x)[T], uint32_t (&acc)[RR][2]) {
            if constexpr (R > 0) {
                // opaque per-iteration zero: keeps the table reads at their use
                // instead of hoisted out of the loop into (spilled) registers
                uint32_t tz;
                asm volatile("s_mov_b32 %0, 0" : "=s"(tz));
                const uint8_t* tabs = lds_all + tz;
                uint32_t pend[RR][2];
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
                // The rows are complete here: without this the compiler sinks
                // each row's lookups into the store / compare branch that uses
                // it (`r < e` is a run-time test) and keeps all C x R tables
                // in registers across the branches (RS(8,4): over 256 VGPRs).
#pragma unroll
                for (int r = 0; r < R; ++r) asm volatile("" : "+v"(acc[r][0]), "+v"(acc[r][1]));
            }
        };
        // Chunk ch of every row that is read, fetched one step ahead (in
        // flight across the barriers), the encode kernel's three forms: whole
        // 8-byte loads while the chunk ends at or before S; the shard's last 8
        // bytes, shifted, for the lane that straddles S; byte by byte for a
        // shard of 1..7 bytes.  Nothing at or past S is read; those bytes are
        // zeros, so computed bytes past S are zero too.
        auto load_chunk = [&](uint2 (&v)[T], uint32_t ch) {
            // addresses: a wave-uniform 64-bit base per row (scalar registers)
            // plus a 32-bit lane offset
            const uint64_t cb = rec + mixed::kRecHeader + (uint64_t)ch * kFusedChunk;  // the chunk in its record
            const uint32_t l8 = lane * 8u;
            if (((uint64_t)ch + 1) * kFusedChunk <= S) {  // wave-uniform
#pragma unroll
                for (int row = 0; row < T; ++row)
                    if (is_read(row)) v[row] = __builtin_bit_cast(uint2, ld64_any(p.file[row] + cb + l8));
            } else if (S >= 8) {  // wave-uniform
                const uint32_t tail = (uint32_t)(S - (uint64_t)ch * kFusedChunk);  // 1..511 bytes of this chunk
                // lanes whose 8 bytes end at or before S load them; the others
                // load the shard's last 8 bytes (which may begin before the
                // chunk) and shift out those before their own offset
                const bool in = l8 + 8u <= tail;
                const uint32_t back = tail < 8u ? 8u - tail : 0u;  // wave-uniform: the last 8 bytes begin `back` before the chunk
                const uint32_t at = in ? l8 + back : tail + back - 8u;
                const uint32_t drop = in ? 0u : (l8 < tail ? l8 + 8u - tail : 8u);  // bytes before the lane's offset
#pragma unroll
                for (int row = 0; row < T; ++row)
                    if (is_read(row)) {
                        const uint64_t w = ld64_any(p.file[row] + (cb - back) + at);
                        v[row] = __builtin_bit_cast(uint2, drop < 8u ? w >> (8u * drop) : 0ull);
                    }
            } else {  // a shard of 1..7 bytes: lane 0 gathers it byte by byte
#pragma unroll
                for (int row = 0; row < T; ++row) v[row] = make_uint2(0u, 0u);
#pragma unroll 1
                for (uint32_t b = 0; b < (uint32_t)S; ++b) {
#pragma unroll
                    for (int row = 0; row < T; ++row)
                        if (is_read(row)) {
                            const uint32_t byte = lane == 0 ? (uint32_t)p.file[row][cb + b] : 0u;
                            if (b < 4) v[row].x |= byte << (8 * b);
                            else v[row].y |= byte << (8 * (b - 4));
                        }
                }
            }
        };
        uint2 x[T];
#pragma unroll
        for (int row = 0; row < T; ++row) x[row] = make_uint2(0u, 0u);
        if (my_chunks) load_chunk(x, 0);
        uint32_t diff = 0;  // OR of (computed ^ read) over the surplus rows
#pragma unroll 1
        for (uint32_t ch = 0; ch < wg_chunks; ++ch) {
            const bool act = ch < my_chunks;      // wave-uniform
            const bool nxt = ch + 1 < my_chunks;  // wave-uniform
            if (act) {
                if constexpr (R > 0) {
                    const uint64_t cb = (uint64_t)ch * kFusedChunk;  // wave-uniform
                    const uint32_t l8 = lane * 8u;
                    const bool whole = cb + kFusedChunk <= S;
                    const uint32_t tail = whole ? kFusedChunk : (uint32_t)(S - cb);
                    uint32_t acc[RR][2];
                    rows_of(x, acc);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if ((uint32_t)r < e) {  // a lost data row: nothing written at or past S
                            uint8_t* dst = ob + ((uint64_t)p.lost[r] * S + cb) + l8;
                            const uint64_t v = (uint64_t)acc[r][0] | ((uint64_t)acc[r][1] << 32);
                            if (whole) st64_any(dst, v);
                            else st64_part(dst, v, l8, tail);
                        } else {  // a surplus row against its record
                            diff = or_diff(diff, acc[r][0], x[C + r].x);
                            diff = or_diff(diff, acc[r][1], x[C + r].y);
                        }
                    }
                }
            }
            uint2 y[T];
            if (nxt) load_chunk(y, ch + 1);  // in flight across the barriers
            lds_barrier();  // A: the hashers are done with the previous chunk's rows
            if (act) {
#pragma unroll
                for (int row = 0; row < T; ++row)
                    if (is_read(row)) *(uint2*)(my_rows + row * kFusedPitch + lane * 8u) = x[row];
            }
            lds_barrier();  // B: this chunk's rows are ready
            if (nxt) {
#pragma unroll
                for (int row = 0; row < T; ++row) x[row] = y[row];
            }
        }
        if constexpr (R > 0) {
            // the stripe's mismatch word, written whole
            const bool bad = __builtin_amdgcn_ballot_w64(diff != 0u) != 0ull;
            if (glive && lane == 0) p.mismatch[gjob] = bad ? 1u : 0u;
        }
    } else {
        // ------------------------------ hasher -------------------------------
        const uint32_t g = (wave - SPW) * 16u + (lane >> 2);  // stream of this quad
        const uint32_t ls = g / T, row = g - ls * T;          // local stripe, row
        const uint64_t idx = first + ls;
        const bool live = g < (uint32_t)(SPW * T) && idx < n && (row < (uint32_t)C || row - (uint32_t)C >= e);
        const uint32_t len = live ? desc[idx].len : 0u;
        const uint32_t job = live ? desc[idx].job : 0u;
        const uint32_t my_chunks = (len >> 9) + ((len & (kFusedChunk - 1)) ? 1u : 0u);  // per quad
        const uint32_t tail = my_chunks ? len - (my_chunks - 1) * kFusedChunk : 0u;     // 1..512
        const uint8_t* row0 = rows + (live ? ls * kStripeRows + row * kFusedPitch : 0);
        const uint8_t* rp = row0 + 8 * q;
        const uint8_t* hdr = hdrs + (live ? (ls * T + row) * 32 : 0);
        uint8_t* flag = p.flags + (uint64_t)job * p.fstride + row;
        HHQuad st;
        hhq_init(st, p.key, q);
        // digest against the record's header; the quad's verdict, written whole
        auto finish = [&]() {
            const uint64_t h = hhq_digest(st, q);
            uint32_t ok = h == *(const uint64_t*)(hdr + 8 * q) ? 1u : 0u;
            ok &= quad_swap_pairs(ok);
            ok &= quad_swap_halves(ok);
            if (q == 0) *flag = (uint8_t)ok;
        };
        if (live && my_chunks == 0) finish();  // the empty message
#pragma unroll 1
        for (uint32_t ch = 0; ch < wg_chunks; ++ch) {
            lds_barrier();  // A
            lds_barrier();  // B
            if (live && ch + 1 < my_chunks) {
#pragma unroll 4
                for (int t = 0; t < (int)(kFusedChunk / 32); ++t)
                    hhq_update(st, __builtin_bit_cast(uint64_t, *(const u32x2*)(rp + t * 32)));
            } else if (live && ch + 1 == my_chunks) {
                // this stream's last chunk: whole packets, the remainder
                // packet, the digest; afterwards the quad only passes barriers
                const uint32_t full = tail / 32;
#pragma unroll 1
                for (uint32_t t = 0; t < full; ++t) hhq_update(st, __builtin_bit_cast(uint64_t, *(const u32x2*)(rp + t * 32)));
                if (tail % 32) hhq_remainder(st, row0 + full * 32, tail % 32, q);
                finish();
            }
        }
    }
}

template <int C, int R>
static DecodeMixedPick decode_mixed_entry() {
    constexpr int spw = mixed::decode_spw_for(C + R);
    return {k_decode_mixed<C, R, spw>, spw, spw + (spw * (C + R) + 15) / 16};
}

template <int C>
static DecodeMixedPick pick_decode_mixed_r(int R) {
    switch (R) {
        case 0: return decode_mixed_entry<C, 0>();
        case 1: return decode_mixed_entry<C, 1>();
        case 2: return decode_mixed_entry<C, 2>();
        case 3: return decode_mixed_entry<C, 3>();
        case 4: return decode_mixed_entry<C, 4>();
    }
    return {nullptr, 0, 0};
}

#define RSG_MDEC_CAT2(a, b) a##b
#define RSG_MDEC_CAT(a, b) RSG_MDEC_CAT2(a, b)

DecodeMixedPick RSG_MDEC_CAT(pick_decode_mixed_part, RSG_MDEC_PART)(int C, int R) {
    constexpr int P = RSG_MDEC_PART;
    static_assert(P >= 0 && P < kMdecParts, "RSG_MDEC_PART");
    switch ((C - 1 - P) / kMdecParts) {
        case 0: return pick_decode_mixed_r<P + 1>(R);
        case 1: return pick_decode_mixed_r<P + 1 + kMdecParts>(R);
        case 2: return pick_decode_mixed_r<P + 1 + 2 * kMdecParts>(R);
        case 3: return pick_decode_mixed_r<P + 1 + 3 * kMdecParts>(R);
    }
    return {nullptr, 0, 0};
}

#else  // the launcher

hipError_t launch_decode_mixed(const DecodeMixedParams& p, const mixed::DecDesc* d_desc, uint64_t n,
                               hipStream_t stream) {
    const int C = (int)p.C, R = (int)p.R;
    if (C < 1 || C > mixed::kDecMaxC || R < 0 || R > mixed::kDecMaxR || p.e > p.R || !d_desc || !p.flags ||
        (R > 0 && !p.mismatch) || n == 0 || n > 0x7fffffffull)
        return hipErrorInvalidValue;
    DecodeMixedPick f{nullptr, 0, 0};
    switch ((C - 1) % kMdecParts) {
        case 0: f = pick_decode_mixed_part0(C, R); break;
        case 1: f = pick_decode_mixed_part1(C, R); break;
        case 2: f = pick_decode_mixed_part2(C, R); break;
        case 3: f = pick_decode_mixed_part3(C, R); break;
    }
    if (!f.k) return hipErrorInvalidValue;
    const size_t lds = (size_t)C * R * 32 + (size_t)f.spw * (C + R) * (32 + kFusedPitch);
    const uint64_t blocks = (n + f.spw - 1) / f.spw;
    hipLaunchKernelGGL(f.k, dim3((uint32_t)blocks), dim3(64 * f.waves), lds, stream, p, d_desc, n);
    return hipGetLastError();
}

#endif

}  // namespace rsg
