// rs_mixed.h — launcher of the mixed-length fused encode + HH256S kernel
// (rs_mixed.hip); internal to librsgpu.
#pragma once

#include "rs_kernels.h"
#include "rs_mixed_plan.h"

namespace rsg {

// One launch over the n stripes of the device table d_desc (planner order):
// p: the encode tables with base = the data arena and out_base = the parity
// arena (nothing else per stripe is read from p); h: key and digest output
// [n][C+R][32] in `job` order, or out = null for parity only.
// mixed::kernel_geometry(C, R) geometries only; any shard length, alignment
// and arena aliasing the planner accepts.
hipError_t launch_encode_hash_mixed(GfApplyParams p, HashParams h, const mixed::MixedDesc* d_desc, uint64_t n,
                                    hipStream_t stream);

}  // namespace rsg
