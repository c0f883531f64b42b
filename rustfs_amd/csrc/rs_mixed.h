// rs_mixed.h — launchers of the mixed-length kernels: the fused encode +
// HH256S (rs_mixed.hip) and the verify + rebuild of record stripes
// (rs_mixed_decode.hip), their heal (rs_mixed_heal.hip) and the deep scan of
// record files (rs_mixed_verify.hip); internal to librsgpu.
#pragma once

#include "rs_kernels.h"
#include "rs_mixed_decode_plan.h"
#include "rs_mixed_heal_plan.h"
#include "rs_mixed_plan.h"
#include "rs_mixed_verify_plan.h"

namespace rsg {

#ifdef __HIPCC__
// Wave-uniform copies (scalar registers).  __builtin_amdgcn_readfirstlane
// returns int: widened as it is, a value with bit 31 set would sign-extend
// into the upper half (an offset or length of 2 GiB or more).
__device__ __forceinline__ uint32_t uniform32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    return (uint64_t)uniform32((uint32_t)v) | ((uint64_t)uniform32((uint32_t)(v >> 32)) << 32);
}
#endif

// One launch over the n stripes of the device table d_desc (planner order):
// p: the encode tables with base = the data arena and out_base = the parity
// arena (nothing else per stripe is read from p); h: key and digest output
// [n][C+R][32] in `job` order, or out = null for parity only.
// mixed::kernel_geometry(C, R) geometries only; any shard length, alignment
// and arena aliasing the planner accepts.
hipError_t launch_encode_hash_mixed(GfApplyParams p, HashParams h, const mixed::MixedDesc* d_desc, uint64_t n,
                                    hipStream_t stream);

// Kernel arguments of k_decode_mixed<C,R,SPW>: one launch serves the stripes
// of one mask group, which share the decode plan.  Row c < C is source c of
// the plan; row C + r belongs to computed row r: rows r < e rebuild data shard
// lost[r] into out (nothing is read for them), rows r >= e re-derive the
// surplus shard whose records lie in file[C + r] and compare.
struct DecodeMixedParams {
    const uint8_t* file[mixed::kDecMaxC + mixed::kDecMaxR];  // row -> record arena (null: not read)
    uint8_t* out;
    uint8_t* flags;      // [jobs][fstride]: flags[job*fstride + row] = 1 verified, 0 not, for every row read
    uint32_t* mismatch;  // [jobs]: nonzero where a re-derived surplus row differs from its record
    uint64_t key[4];
    uint32_t tab[mixed::kDecMaxR][mixed::kDecMaxC][5];  // v_perm tables of computed row r over source c
    uint32_t lost[mixed::kDecMaxR];
    uint32_t C, R, e, fstride;
};

// One launch over the n stripes of d_desc (planner order).
// mixed::decode_kernel_geometry(C, R) shapes only.
hipError_t launch_decode_mixed(const DecodeMixedParams& p, const mixed::DecDesc* d_desc, uint64_t n,
                               hipStream_t stream);

// Kernel arguments of k_heal_mixed<C,R,SPW>: one launch serves the stripes of
// one mask group, which share the heal plan.  Row c < C is source c of the
// plan; row C + r belongs to computed row r: rows r < e are the heal targets
// (the record [digest][shard] of stripe j is written at target[r] + out_off of
// its descriptor, nothing is read for them), rows r >= e re-derive the surplus
// shard whose records lie in file[C + r] and compare.
struct HealMixedParams {
    const uint8_t* file[mixed::kDecMaxC + mixed::kDecMaxR];  // row -> record arena (null: not read)
    uint8_t* target[mixed::kDecMaxR];                        // computed row r < e -> target arena
    uint8_t* flags;      // [jobs][fstride]: flags[job*fstride + row] = 1 verified, 0 not, for every row read
    uint32_t* mismatch;  // [jobs]: nonzero where a re-derived surplus row differs from its record
    uint64_t key[4];
    uint32_t tab[mixed::kDecMaxR][mixed::kDecMaxC][5];  // v_perm tables of computed row r over source c
    uint32_t C, R, e, fstride;
};

// One launch over the n stripes of d_desc (planner order).
// mixed::heal_kernel_shape(C, R) shapes only, 1 <= e <= R.
hipError_t launch_heal_mixed(const HealMixedParams& p, const mixed::DecDesc* d_desc, uint64_t n, hipStream_t stream);

// All-zero 32-byte headers at target[t] + d_offs[s] for every t < nt, s < n
// (the target records of failed stripes), any alignment, one launch.
struct HealZeroParams {
    uint8_t* target[32];
    uint32_t nt;
};
hipError_t launch_heal_zero_headers(const HealZeroParams& p, const uint64_t* d_offs, uint64_t n, hipStream_t stream);

// Kernel arguments of k_verify_mixed<DEPTH>: quad j hashes the body of unit[j]
// (device addresses, planner order) and writes flags[unit[j].flag] = 1 where
// the digest equals the 32 bytes in front of the body, 0 where not.
struct VerifyMixedParams {
    const mixed::VerifyUnit* unit;  // device table
    uint8_t* flags;
    uint64_t n;  // units
    uint64_t key[4];
};

// One launch over the n units; DEPTH from Tuning::hash_depth (RSG_HASH_DEPTH).
hipError_t launch_verify_mixed(const VerifyMixedParams& p, hipStream_t stream);

}  // namespace rsg
