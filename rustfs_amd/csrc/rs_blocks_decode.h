// rs_blocks_decode.h — launcher of the gathered block reconstruct
// (rs_blocks_decode.hip); internal to librsgpu.
#pragma once

#include "rs_blocks_decode_plan.h"
#include "rs_kernels.h"

namespace rsg {

// Kernel arguments of k_reconstruct_blocks<C> (C <= 8) and
// k_reconstruct_blocks_loop<G> (C = 9..16): workgroup w handles tile
// w - tile0[e] of entry e = the last entry with tile0[e] <= w.
struct ReconBlocksParams {
    const blocks::RDesc* desc;  // device-visible table, n entries
    const uint32_t* tile0;      // n + 1 prefix sums of the entries' tile counts
    const uint32_t* tab;        // [tables][kMaxR][C][5], GfApplyParams::tab's layout per table (coef_tables)
    uint32_t n, C;
};

// One launch over tiles = tile0[n] workgroups, whatever the entries' row
// counts and tables.  C = 1..blocks::kMaxC.
hipError_t launch_reconstruct_blocks(const ReconBlocksParams& p, uint32_t tiles, hipStream_t stream);

}  // namespace rsg
