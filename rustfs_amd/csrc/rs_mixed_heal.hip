// rs_mixed_heal.hip — mixed-length batch heal (Erasure::heal, heal.rs:112-206,
// decode_data_and_parity, erasure.rs:917): verify-before-use of the source
// [digest][shard] records (bitrot.rs:139-247), the rebuild of the heal
// targets' shards, data or parity, and their BitrotWriter records, over n
// unrelated stripes in one launch, each with its own shard length.
//
// k_heal_mixed<C,R,SPW> is the fourth fused kernel built from the parts in
// rs_fused.h (table fill, GF rows, hasher walk, step geometry), and it is
// k_decode_mixed's read half (rs_mixed_decode.hip) joined with
// k_encode_hash_mixed's write half (rs_mixed.hip): SPW GF waves (one per
// stripe), ceil(SPW*T/16) hasher waves (one 4-lane quad per row, T = C + R),
// coefficient tables, then the records' 32-byte headers, then SPW x T rows of
// kFusedPitch in LDS, an A/B barrier pair per 512-byte chunk, a per-stripe
// descriptor table in device memory (mixed::DecDesc; out_off is the offset of
// the stripe's record in every target arena).  One launch serves one mask
// group, so every stripe of a workgroup shares the heal plan (HealMixedParams,
// rs_mixed.h):
//   row c < C          source c: read from file[c], hashed against its header,
//                      input of the GF rows
//   row C + r, r < e   heal target r: computed; the GF wave stores the body at
//                      target[r] + out_off + 32 (exact byte ranges: nothing at
//                      or past the shard's end, where another workgroup writes
//                      the next record's header) and stages the chunk in LDS;
//                      the row's hasher quad hashes the staged bytes, which
//                      are the stored bytes, and writes the digest to
//                      target[r] + out_off.  Nothing is read for it.
//   row C + r, r >= e  surplus shard: read from file[C + r], hashed against
//                      its header, re-derived and compared (mismatch word)
// R = e + surplus <= m (a target is never read), e >= 1: a heal has a target.
//
// Barrier count: every wave of a workgroup runs one __syncthreads() and then
// exactly 2*wg_chunks lds_barrier() calls (the argument stands at
// fused_hash_stream, rs_fused.h).  wg_chunks is the maximum chunk count over
// the workgroup's SPW descriptors (len = 0 past the end of the table), which
// every wave computes from the same descriptor words and makes wave-uniform
// with readfirstlane.  A GF wave runs the A/B pair once in each of its
// wg_chunks steps, outside every `if`; a hasher wave runs them inside
// fused_hash_stream's loop of wg_chunks steps.  No barrier sits under a
// condition on the plan, on e, on `live` or on a lane: what a row is (source,
// target, surplus) only selects what is done between the barriers.
//
// The three-form tail loader is a copy of k_decode_mixed's: moving it into a
// header would recompile all 80 k_decode_mixed instantiations, whose registers
// and occupancy then have to be shown unchanged one by one; a shared loader
// has already cost the encode kernel scratch once (rs_fused.h).  The copy
// leaves the existing kernels' code as it was.
//
// Built in kMhealParts (4) translation units: part i (RSG_MHEAL_PART=i)
// instantiates C = i+1, i+1+PARTS, ...; without RSG_MHEAL_PART: the launchers.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rs_device.h"
#include "rs_fused.h"
#include "rs_mixed.h"

namespace rsg {

using mixed::DecDesc;

constexpr int kMhealParts = 4;

using HealMixedKernel = void (*)(const HealMixedParams, const DecDesc*, const uint64_t);

struct HealMixedPick {
    HealMixedKernel k;
    int spw, waves;
};

#define RSG_MHEAL_PART_DECL(i) HealMixedPick pick_heal_mixed_part##i(int C, int R);
RSG_MHEAL_PART_DECL(0)
RSG_MHEAL_PART_DECL(1)
RSG_MHEAL_PART_DECL(2)
RSG_MHEAL_PART_DECL(3)
#undef RSG_MHEAL_PART_DECL

#ifdef RSG_MHEAL_PART

// Waves per SIMD asked of the register allocator: per geometry, the highest
// request at which the resource-usage report shows no scratch
// (profiles/r09/mixed_heal/resource_usage.txt; derived like
// decode_mixed_waves_per_eu, by a sweep of requests 2..8 with RSG_MHEAL_WPE).
constexpr int heal_mixed_waves_per_eu(int C, int R) {
#ifdef RSG_MHEAL_WPE  // the sweep behind the table
    return RSG_MHEAL_WPE + 0 * (C + R);
#else
    constexpr int8_t w[mixed::kDecMaxR][mixed::kDecMaxC] = {
        {8, 8, 8, 7, 6, 5, 5, 4, 4, 3, 3, 3, 3, 2, 2, 2},
        {8, 7, 6, 5, 5, 4, 4, 4, 3, 3, 3, 2, 2, 2, 2, 2},
        {6, 5, 5, 4, 4, 4, 4, 3, 3, 3, 2, 2, 2, 2, 2, 2},
        {5, 4, 4, 4, 4, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2},
    };
    return w[R - 1][C - 1];
#endif
}

template <int C, int R, int SPW>
__global__ __launch_bounds__(64 * (SPW + (SPW * (C + R) + 15) / 16))
__attribute__((amdgpu_waves_per_eu(heal_mixed_waves_per_eu(C, R))))
void k_heal_mixed(const HealMixedParams p, const DecDesc* __restrict__ desc, const uint64_t n) {
    // LDS: [C][R] coefficient tables (32 B each), SPW x T record headers
    // (32 B each), then SPW x T chunk rows
    extern __shared__ uint8_t lds_all[];
    static_assert(R >= 1, "a heal has a target");
    constexpr int T = C + R;
    constexpr uint32_t kTabBytes = C * R * 32;
    constexpr uint32_t kHdrBytes = SPW * T * 32;
    constexpr uint32_t kStripeRows = T * kFusedPitch;
    uint8_t* hdrs = lds_all + kTabBytes;
    uint8_t* rows = hdrs + kHdrBytes;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u, q = lane & 3u;
    const uint64_t first = (uint64_t)blockIdx.x * SPW;
    const uint32_t e = p.e;  // rows r < e are targets, rows r >= e compared
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
        // the source records' headers, for the hashers to compare their digests with
#pragma unroll
        for (int row = 0; row < T; ++row)
            if (is_read(row))
                *(uint64_t*)(hdrs + (wave * T + row) * 32 + lane * 8) = ld64_any(p.file[row] + rec + lane * 8u);
    }
    __syncthreads();

    if (gf) {
        // ------------------------------ GF wave ------------------------------
        const uint32_t my_chunks = fused_chunks(S);
        uint8_t* my_rows = rows + wave * kStripeRows;
        const uint32_t m7 = vgpr_const(0x07070707u), m3 = vgpr_const(0x03030303u);
        // Chunk ch of every row that is read, fetched one step ahead (in
        // flight across the barriers), k_decode_mixed's three forms (a copy:
        // see the head comment): whole 8-byte loads while the chunk ends at or
        // before S; the shard's last 8 bytes, shifted, for the lane that
        // straddles S; byte by byte for a shard of 1..7 bytes.  Nothing at or
        // past S is read; those bytes are zeros, so computed bytes past S are
        // zero too.
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
        // x[row]: this chunk of row `row`; a target's slot (never loaded)
        // takes the computed row, so one loop stages all T rows in LDS
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
                const uint64_t cb = (uint64_t)ch * kFusedChunk;  // wave-uniform
                const uint32_t l8 = lane * 8u;
                const bool whole = cb + kFusedChunk <= S;
                const uint32_t tail = whole ? kFusedChunk : (uint32_t)(S - cb);
                uint32_t acc[R][2];
                // the R computed rows of this chunk (x: 8 bytes of every source per lane)
                fused_gf_rows<C, R>(lds_all, m7, m3, x, acc);
                // The rows are complete here: without this the compiler sinks
                // each row's lookups into the store / compare branch that uses
                // it (`r < e` is a run-time test) and keeps all C x R tables
                // in registers across the branches (k_decode_mixed).
#pragma unroll
                for (int r = 0; r < R; ++r) asm volatile("" : "+v"(acc[r][0]), "+v"(acc[r][1]));
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if ((uint32_t)r < e) {  // a target row: its body, nothing written at or past S
                        uint8_t* dst = p.target[r] + (oo + mixed::kRecHeader + cb) + l8;
                        const uint64_t v = (uint64_t)acc[r][0] | ((uint64_t)acc[r][1] << 32);
                        if (whole) st64_any(dst, v);
                        else st64_part(dst, v, l8, tail);
                        x[C + r] = make_uint2(acc[r][0], acc[r][1]);  // staged below: hashed as stored
                    } else {  // a surplus row against its record
                        diff = or_diff(diff, acc[r][0], x[C + r].x);
                        diff = or_diff(diff, acc[r][1], x[C + r].y);
                    }
                }
            }
            uint2 y[T];
            if (nxt) load_chunk(y, ch + 1);  // in flight across the barriers
            lds_barrier();  // A: the hashers are done with the previous chunk's rows
            if (act) {
#pragma unroll
                for (int row = 0; row < T; ++row) *(uint2*)(my_rows + row * kFusedPitch + lane * 8u) = x[row];
            }
            lds_barrier();  // B: this chunk's rows are ready
            if (nxt) {
#pragma unroll
                for (int row = 0; row < T; ++row)
                    if (is_read(row)) x[row] = y[row];
            }
        }
        // the stripe's mismatch word, written whole
        const bool bad = __builtin_amdgcn_ballot_w64(diff != 0u) != 0ull;
        if (glive && lane == 0) p.mismatch[gjob] = bad ? 1u : 0u;
    } else {
        // ------------------------------ hasher -------------------------------
        const uint32_t g = (wave - SPW) * 16u + (lane >> 2);  // stream of this quad
        const uint32_t ls = g / T, row = g - ls * T;          // local stripe, row
        const uint64_t idx = first + ls;
        const bool live = g < (uint32_t)(SPW * T) && idx < n;  // every row is hashed
        const bool tgt = row >= (uint32_t)C && row - (uint32_t)C < e;
        const uint32_t len = live ? desc[idx].len : 0u;
        const uint32_t job = live ? desc[idx].job : 0u;
        const uint64_t out_off = live && tgt ? desc[idx].out_off : 0;
        const uint32_t my_chunks = fused_chunks(len);                                // per quad
        const uint32_t tail = my_chunks ? len - (my_chunks - 1) * kFusedChunk : 0u;  // 1..512
        const uint8_t* row0 = rows + (live ? ls * kStripeRows + row * kFusedPitch : 0);
        const uint8_t* hdr = hdrs + (live ? (ls * T + row) * 32 : 0);
        uint8_t* flag = p.flags + (uint64_t)job * p.fstride + row;
        uint8_t* tbase = nullptr;  // the target arena of a target row
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (row == (uint32_t)(C + r)) tbase = p.target[r];
        HHQuad st;
        hhq_init(st, p.key, q);
        fused_hash_stream(st, row0, q, live, my_chunks, tail, wg_chunks, [&] {
            const uint64_t h = hhq_digest(st, q);
            if (tgt) {
                // the target record's header: 8 bytes per lane, any alignment
                st64_any(tbase + out_off + 8u * q, h);
            } else {
                // digest against the record's header; the quad's verdict, written whole
                uint32_t ok = h == *(const uint64_t*)(hdr + 8 * q) ? 1u : 0u;
                ok &= quad_swap_pairs(ok);
                ok &= quad_swap_halves(ok);
                if (q == 0) *flag = (uint8_t)ok;
            }
        });
    }
}

template <int C, int R>
static HealMixedPick heal_mixed_entry() {
    constexpr int spw = mixed::decode_spw_for(C + R);
    return {k_heal_mixed<C, R, spw>, spw, spw + (spw * (C + R) + 15) / 16};
}

#define RSG_MHEAL_CAT2(a, b) a##b
#define RSG_MHEAL_CAT(a, b) RSG_MHEAL_CAT2(a, b)

// this part's source counts: C = P + 1 + j*kMhealParts, j = 0..3
HealMixedPick RSG_MHEAL_CAT(pick_heal_mixed_part, RSG_MHEAL_PART)(int C, int R) {
    constexpr int P = RSG_MHEAL_PART;
    static_assert(P >= 0 && P < kMhealParts, "RSG_MHEAL_PART");
    return dispatch_int<0, 3>((C - 1 - P) / kMhealParts, HealMixedPick{}, [R](auto j) {
        return dispatch_int<1, mixed::kDecMaxR>(R, HealMixedPick{}, [](auto r) {
            return heal_mixed_entry<P + 1 + decltype(j)::value * kMhealParts, decltype(r)::value>();
        });
    });
}

#else  // the launchers

hipError_t launch_heal_mixed(const HealMixedParams& p, const mixed::DecDesc* d_desc, uint64_t n, hipStream_t stream) {
    const int C = (int)p.C, R = (int)p.R;
    if (!mixed::heal_kernel_shape(C, R) || p.e < 1 || p.e > p.R || !d_desc || !p.flags || !p.mismatch || n == 0 ||
        n > 0x7fffffffull)
        return hipErrorInvalidValue;
    for (uint32_t r = 0; r < p.e; ++r)
        if (!p.target[r]) return hipErrorInvalidValue;
    HealMixedPick f{nullptr, 0, 0};
    switch ((C - 1) % kMhealParts) {
        case 0: f = pick_heal_mixed_part0(C, R); break;
        case 1: f = pick_heal_mixed_part1(C, R); break;
        case 2: f = pick_heal_mixed_part2(C, R); break;
        case 3: f = pick_heal_mixed_part3(C, R); break;
    }
    if (!f.k) return hipErrorInvalidValue;
    const size_t lds = (size_t)C * R * 32 + (size_t)f.spw * (C + R) * (32 + kFusedPitch);
    const uint64_t blocks = (n + f.spw - 1) / f.spw;
    hipLaunchKernelGGL(f.k, dim3((uint32_t)blocks), dim3(64 * f.waves), lds, stream, p, d_desc, n);
    return hipGetLastError();
}

// The all-zero headers of failed stripes: one thread per 8 bytes of header,
// [offset][target][word], stored at any alignment.
__global__ __launch_bounds__(256) void k_heal_zero_headers(const HealZeroParams p, const uint64_t* __restrict__ offs,
                                                           const uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t per = (uint64_t)p.nt * 4u;
    if (i >= n * per) return;
    const uint64_t s = i / per;
    const uint32_t w = (uint32_t)(i - s * per), t = w >> 2, word = w & 3u;
    st64_any(p.target[t] + offs[s] + 8u * word, 0ull);
}

hipError_t launch_heal_zero_headers(const HealZeroParams& p, const uint64_t* d_offs, uint64_t n, hipStream_t stream) {
    if (p.nt < 1 || p.nt > 32 || !d_offs || n == 0 || n > 0x7fffffffull) return hipErrorInvalidValue;
    for (uint32_t t = 0; t < p.nt; ++t)
        if (!p.target[t]) return hipErrorInvalidValue;
    const uint64_t threads = n * p.nt * 4u;
    hipLaunchKernelGGL(k_heal_zero_headers, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, stream, p, d_offs, n);
    return hipGetLastError();
}

#endif

}  // namespace rsg
