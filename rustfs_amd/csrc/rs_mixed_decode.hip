// rs_mixed_decode.hip — mixed-length batch GET: verify-before-use of
// [digest][shard] records (bitrot.rs:139-247) and the rebuild of the data
// shards no verified record serves (erasure.rs:935-973), over n unrelated
// stripes in one launch, each with its own shard length.
//
// k_decode_mixed<C,R,SPW> is one of the three fused kernels built from the
// parts in rs_fused.h (table fill, GF rows, hasher walk, step geometry; the
// three-form tail loader stays per kernel), beside k_encode_hash_mixed (rs_mixed.hip): SPW GF waves (one per
// stripe), ceil(SPW*T/16) hasher waves (one 4-lane quad per row, T = C + R),
// coefficient tables, then the records' 32-byte headers, then SPW x T rows of
// kFusedPitch in LDS, an A/B barrier pair per 512-byte chunk, a per-stripe
// descriptor table in device memory (mixed::DecDesc).  Its hashers compare
// each digest with the record's header instead of writing it out.  One launch
// serves one mask group, so every stripe of a workgroup shares the decode
// plan (DecodeMixedParams, rs_mixed.h):
//   row c < C      source c: read from file[c], hashed, input of the GF rows
//   row C + r, r < e   rebuilt data shard lost[r]: computed, stored to out
//   row C + r, r >= e  surplus shard: read from file[C + r], hashed, and
//                      compared with computed row r
// The GF wave loads every row that is read straight from the record files
// (any byte alignment, one step ahead), and the hashers hash the same bytes
// out of LDS, so what is used is what was verified.  R = 0 only verifies.
//
// Barrier count: every wave of a workgroup runs one __syncthreads() and then
// exactly 2*wg_chunks lds_barrier() calls (the argument stands at
// fused_hash_stream, rs_fused.h), wg_chunks = the maximum chunk count over the
// workgroup's SPW descriptors (len = 0 past the end of the table); nor does a
// barrier sit under a condition on the plan.
//
// Built in kMdecParts (4) translation units: part i (RSG_MDEC_PART=i)
// instantiates C = i+1, i+1+PARTS, ...; without RSG_MDEC_PART: the launcher.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rs_device.h"
#include "rs_fused.h"
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

    fused_tables_to_lds<C, R>(p.tab, lds_all);

    // The workgroup's step count: the same SPW descriptor words in every wave
    // (no chunk past the end of the table).
    uint32_t wgc = 0;
#pragma unroll
    for (int s = 0; s < SPW; ++s) {
        const uint32_t c = fused_chunks(first + s < n ? desc[first + s].len : 0u);
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
        const uint32_t my_chunks = fused_chunks(S);
        uint8_t* ob = p.out + oo;
        uint8_t* my_rows = rows + wave * kStripeRows;
        const uint32_t m7 = vgpr_const(0x07070707u), m3 = vgpr_const(0x03030303u);
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
                    // the R computed rows of this chunk (x: 8 bytes of every source per lane)
                    fused_gf_rows<C, R>(lds_all, m7, m3, x, acc);
                    // The rows are complete here: without this the compiler sinks
                    // each row's lookups into the store / compare branch that uses
                    // it (`r < e` is a run-time test) and keeps all C x R tables
                    // in registers across the branches (RS(8,4): over 256 VGPRs).
#pragma unroll
                    for (int r = 0; r < R; ++r) asm volatile("" : "+v"(acc[r][0]), "+v"(acc[r][1]));
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
        const uint32_t my_chunks = fused_chunks(len);                                // per quad
        const uint32_t tail = my_chunks ? len - (my_chunks - 1) * kFusedChunk : 0u;  // 1..512
        const uint8_t* row0 = rows + (live ? ls * kStripeRows + row * kFusedPitch : 0);
        const uint8_t* hdr = hdrs + (live ? (ls * T + row) * 32 : 0);
        uint8_t* flag = p.flags + (uint64_t)job * p.fstride + row;
        HHQuad st;
        hhq_init(st, p.key, q);
        // digest against the record's header; the quad's verdict, written whole
        fused_hash_stream(st, row0, q, live, my_chunks, tail, wg_chunks, [&] {
            const uint64_t h = hhq_digest(st, q);
            uint32_t ok = h == *(const uint64_t*)(hdr + 8 * q) ? 1u : 0u;
            ok &= quad_swap_pairs(ok);
            ok &= quad_swap_halves(ok);
            if (q == 0) *flag = (uint8_t)ok;
        });
    }
}

template <int C, int R>
static DecodeMixedPick decode_mixed_entry() {
    constexpr int spw = mixed::decode_spw_for(C + R);
    return {k_decode_mixed<C, R, spw>, spw, spw + (spw * (C + R) + 15) / 16};
}

#define RSG_MDEC_CAT2(a, b) a##b
#define RSG_MDEC_CAT(a, b) RSG_MDEC_CAT2(a, b)

// this part's source counts: C = P + 1 + j*kMdecParts, j = 0..3
DecodeMixedPick RSG_MDEC_CAT(pick_decode_mixed_part, RSG_MDEC_PART)(int C, int R) {
    constexpr int P = RSG_MDEC_PART;
    static_assert(P >= 0 && P < kMdecParts, "RSG_MDEC_PART");
    return dispatch_int<0, 3>((C - 1 - P) / kMdecParts, DecodeMixedPick{}, [R](auto j) {
        return dispatch_int<0, mixed::kDecMaxR>(R, DecodeMixedPick{}, [](auto r) {
            return decode_mixed_entry<P + 1 + decltype(j)::value * kMdecParts, decltype(r)::value>();
        });
    });
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
