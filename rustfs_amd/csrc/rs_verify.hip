// rs_verify.hip — verify-only walks of BitrotWriter record files at unaligned
// pitches (the in-place GET with every data file present, the whole-file
// bitrot_verify: rsgpu.cpp launch_verify_group / bitrot_verify_dev) through
// the record kernels' LDS-DMA ring instead of k_hh256_quad's per-lane 8-byte
// loads.  At 1 MiB blocks most geometries put their records off 8-byte
// alignment (RS(12,4): 32 + 87382 bytes, records at 6 mod 8), and the quad
// kernel's unaligned loads cost it ~7 % against the same walk at 0 mod 32
// (tools/verify_align_probe.py: 1.122 against 1.045 ms for 16 files x 4096
// records); global_load_lds takes the unaligned sources and lands them in LDS
// in order, where the hash waves read them aligned (rs_records.h
// records_hash_wave).  The workgroup is the record ring of 4 stripes (records
// r, r+1, r+2, r+3 of every file) and NF files with hash waves only.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "rs_device.h"
#include "rs_kernels.h"
#include "rs_records.h"

namespace rsg {

namespace {

constexpr int kVG = 4;  // records per file per workgroup

// Up to 12 files: a 3-slot ring (two steps of DMA in flight), two workgroups
// a CU; 13-15 files: a 2-slot ring.  Which launches come here, and the
// measurements behind the thresholds: pick_verify_ring (rs_verify_pick.h).
template <int NF>
struct VerifyShape : RecRing<NF, kVG> {
    static constexpr int RD = NF <= 12 ? 3 : 2;
    static constexpr uint32_t LDS = RD * RecRing<NF, kVG>::DSLOT;
    static constexpr int PER_CU = (160 * 1024) / LDS > 8 ? 8 : (160 * 1024) / LDS;  // workgroups a CU holds
    static constexpr int WAVES = RecRing<NF, kVG>::HW;
    static constexpr int WPE = (PER_CU * WAVES + 3) / 4;
};

template <int NF>
__global__ __launch_bounds__(64 * VerifyShape<NF>::WAVES)
__attribute__((amdgpu_waves_per_eu(VerifyShape<NF>::WPE))) void k_verify_records_dma(const GfApplyParams p,
                                                                                     const HashParams h) {
    using L = VerifyShape<NF>;
    __shared__ __attribute__((aligned(16))) uint8_t ring[L::LDS];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t s0 = (uint64_t)blockIdx.x * kVG;
    (void)h;
    records_hash_wave<NF, kVG, 0, L::RD, false, L::WPE>(&karg_hash(), p.wave_prio, ring, wave, p.units, s0);
}

using VerifyLaunch = void (*)(uint64_t blocks, const GfApplyParams& p, const HashParams& h, hipStream_t stream);

template <int NF>
void launch_nf(uint64_t blocks, const GfApplyParams& p, const HashParams& h, hipStream_t stream) {
    static_assert(VerifyShape<NF>::LDS <= 160 * 1024, "the ring fits the LDS");
    hipLaunchKernelGGL((k_verify_records_dma<NF>), dim3((uint32_t)blocks), dim3(64 * VerifyShape<NF>::WAVES), 0,
                       stream, p, h);
}

constexpr int kMaxRingFiles = 15;
static_assert(VerifyShape<12>::LDS <= 80 * 1024 && VerifyShape<15>::LDS <= 80 * 1024, "two workgroups a CU");
const VerifyLaunch kLaunch[kMaxRingFiles + 1] = {
    nullptr,       launch_nf<1>,  launch_nf<2>,  launch_nf<3>,  launch_nf<4>,  launch_nf<5>,
    launch_nf<6>,  launch_nf<7>,  launch_nf<8>,  launch_nf<9>,  launch_nf<10>, launch_nf<11>,
    launch_nf<12>, launch_nf<13>, launch_nf<14>, launch_nf<15>};

}  // namespace

static_assert(kPickStep == dma::CH && kPickRingRecords == kVG && kPickMaxRingFiles == kMaxRingFiles &&
                  VerifyShape<12>::RD == 3 && VerifyShape<13>::RD == 2,
              "rs_verify_pick.h describes these kernels");

// A multi-file verify launch that pick_hash_launch (rs_verify_pick.h: which
// file counts, pitches and alignments) gave to the DMA ring: h.nbases files of
// h.per_base records at pitch h.stripe_stride, digest 32 bytes before each
// body, flags per file and record, no copies.  false: not a ring pick,
// nothing launched.
// The kernel writes each record's flag whole (1 verified, 0 not), whatever
// the flag held before; the quad kernel only clears a flag its caller set to 1.
bool launch_verify_records_dma(const HashParams& h, const HashPick& pick, hipStream_t stream) {
    if (pick.kind != kPickRing || pick.nf != (int)h.nbases || pick.nf < 1 || pick.nf > kMaxRingFiles) return false;
    GfApplyParams p;
    memset(&p, 0, sizeof(p));
    p.units = pick.steps;
    p.wave_prio = 0;
    HashParams q = h;
    q.n = h.per_base;  // the ring's stripes: the records of each file
    kLaunch[pick.nf](pick.blocks, p, q, stream);
    return true;
}

}  // namespace rsg
