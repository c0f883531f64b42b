// rs_blocks.h — launchers of the gathered block encode (rs_blocks.hip);
// internal to librsgpu.
#pragma once

#include "rs_blocks_plan.h"
#include "rs_kernels.h"

namespace rsg {

// Kernel arguments of k_encode_blocks<C,R> (C <= 8) and k_encode_blocks_loop<R,G>
// (C = 9..16, rolled over groups of G inputs): workgroup w handles tile
// w - tile0[i] of block i = the last block with tile0[i] <= w.
struct EncodeBlocksParams {
    const blocks::BlockDesc* desc;  // device-visible table, n entries
    const uint32_t* tile0;          // n + 1 prefix sums of the blocks' tile counts
    uint32_t n, C;  // C: set by the launcher
    uint32_t tab[blocks::kMaxR][blocks::kMaxC][5];  // GfApplyParams::tab layout (coef_tables)
};

// One launch over tiles = tile0[n] workgroups.  blocks::kernel_geometry(C, R)
// geometries only.
hipError_t launch_encode_blocks(EncodeBlocksParams p, int C, int R, uint32_t tiles, hipStream_t stream);

// Kernel arguments of k_hash_blocks<DEPTH>: quad j hashes unit[j]'s message
// and writes its 32 digest bytes at unit[j].out.
struct HashBlocksParams {
    const blocks::HashUnit* unit;  // device-visible table, planner order
    uint64_t n;
    uint64_t key[4];
};

// One launch over the n units; DEPTH from Tuning::hash_depth (RSG_HASH_DEPTH).
hipError_t launch_hash_blocks(const HashBlocksParams& p, hipStream_t stream);

}  // namespace rsg
