// Stand-alone run of the hash launches' kernel choice
// (rustfs_amd/csrc/rs_verify_pick.h), built by the host compiler with
// AddressSanitizer + UBSan and run directly (tests/test_verify_shapes.py).
// Prints one line per input of a fixed table — the loops below are the ones of
// tests/verify_shapes.py table(), which restates the pick in Python and must
// print the same lines — and checks the structural facts on every input.
// With arguments it prints the picks of real call shapes instead:
//   verify_pick_main K M BLOCK_BYTES   (the all-present GET's data launch and a
//   whole-file verify of K + M files, 4096 records)
#include <stdio.h>
#include <stdlib.h>

#include "../../rustfs_amd/csrc/rs_verify_pick.h"

using namespace rsg;

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
            exit(1);                                                  \
        }                                                             \
    } while (0)

namespace {

constexpr uint64_t kOrigin = 0x7F0000000000ull;

uint64_t table_base(int place, uint32_t b) {
    const uint64_t res[5] = {0, 6, 1, (3 * b) % 16, b == 0 ? 2u : 0u};
    return kOrigin + (uint64_t)b * 0x100000 + res[place];
}

void print(const HashPick& p) {
    if (p.kind == kPickRing)
        printf("ring nf=%d rd=%d blocks=%llu steps=%u\n", p.nf, p.rd, (unsigned long long)p.blocks, p.steps);
    else if (p.kind == kPickQuad)
        printf("quad copy=%d depth=%d unal=%d blocks=%llu\n", p.copy, p.depth, (int)p.unal,
               (unsigned long long)p.blocks);
    else
        printf("%s\n", p.kind == kPickNone ? "none" : "invalid");
}

// What must hold of any pick, whatever the input.
void check(const HashPickIn& h, const HashPick& p) {
    bool copy = false, aligned = h.stripe_stride % 16 == 0, odd = h.stripe_stride % 2 != 0, all_flags = true;
    for (uint32_t b = 0; b < h.nbases; ++b) {
        copy = copy || h.has_copy[b];
        all_flags = all_flags && h.has_flag[b];
        aligned = aligned && h.base[b] % 16 == 0;
        odd = odd || h.base[b] % 2 != 0;
    }
    CHECK((p.kind == kPickNone) == (h.n == 0));
    if (p.kind == kPickRing) {
        CHECK(!copy);                                  // never with a copy target
        CHECK(!aligned);                               // never when every base and the pitch are 16-aligned
        CHECK(p.nf >= 1 && p.nf <= 15 && p.nf == (int)h.nbases);
        CHECK(p.nf <= 12 || !odd);                     // the 2-slot ring at even addresses only
        CHECK(p.rd == (p.nf <= 12 ? 3 : 2));
        CHECK(all_flags && !h.flags && h.digest_off == -32 && h.len > 0 && h.per_base > 0);
        // 32-bit limits: the workgroup count, the step count, the per-lane DMA offsets
        CHECK(p.blocks >= 1 && p.blocks <= 0x7fffffffull && p.blocks == (h.per_base + 3) / 4);
        CHECK(p.steps >= 1 && (uint64_t)p.steps == (h.len + 511) / 512);
        CHECK(3 * h.stripe_stride < (1ull << 32));
    }
    if (p.kind == kPickQuad) {
        CHECK(p.blocks >= 1 && p.blocks <= 0x7fffffffull && p.blocks == (h.n * 4 + 255) / 256);
        CHECK(p.depth >= 1 && p.depth <= 3 && p.depth == h.depth);
        CHECK((p.copy != 0) == copy && (p.copy == 1) == (copy && h.direct_copy));
        if (p.unal) CHECK(p.depth == 2 && h.unal && !copy && (h.nbases == 0 || odd));  // the funnel: depth 2 only
        if (h.nbases && !copy && h.depth == 2 && h.unal) CHECK(p.unal == odd);
    }
    if (p.kind == kPickInvalid) CHECK((h.n * 4 + 255) / 256 > 0x7fffffffull);
}

void run(const HashPickIn& h) {
    const HashPick p = pick_hash_launch(h);
    check(h, p);
    print(p);
}

void table() {
    const uint32_t nbases[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 32};
    const uint64_t per_base[] = {0, 1, 5};
    const uint64_t lens[] = {0, 1, 511, 512, 513, 87382};
    const uint64_t pads[] = {0, 1, 6, 16};
    const struct {
        int depth;
        bool unal, direct;
    } tunings[] = {{2, true, false}, {1, true, false}, {3, true, false}, {2, false, false}, {2, true, true},
                   {1, true, true}, {3, false, true}};
    for (uint32_t nb : nbases)
        for (uint64_t per : per_base)
            for (uint64_t len : lens)
                for (uint64_t pad : pads)
                    for (int place = 0; place < 5; ++place)
                        for (int v = 0; v < 5; ++v)
                            for (const auto& t : tunings) {
                                HashPickIn h = {};
                                h.nbases = nb;
                                h.per_base = per;
                                h.n = nb ? nb * per : per;
                                h.len = len;
                                h.stripe_stride = 32 + len + pad;
                                h.digest_off = v == 4 ? -16 : -32;
                                h.flags = v == 2;
                                h.data = table_base(place, 0);
                                h.shard_pitch = len + pad;
                                for (uint32_t b = 0; b < nb; ++b) {
                                    h.base[b] = table_base(place, b);
                                    h.has_copy[b] = v == 1 && b == 0;
                                    h.has_flag[b] = v != 2 && !(v == 3 && b == nb - 1);
                                }
                                h.depth = t.depth;
                                h.unal = t.unal;
                                h.direct_copy = t.direct;
                                run(h);
                            }
    // the ring's and the grid's 32-bit limits: (nbases, per_base, len, stride)
    const uint64_t limits[][4] = {
        {4, (1ull << 33) + 4, 100, 134}, {4, 1ull << 36, 100, 134}, {4, 1ull << 33, 100, 134},
        {4, 3, 1000, 1431655765}, {4, 3, 1000, 1431655766}, {4, 3, 1ull << 41, 38}, {4, 3, ((1ull << 32) - 1) * 512, 38},
        {1, 1ull << 37, 7, 39}, {1, (1ull << 37) - 64, 7, 39}, {16, 1ull << 33, 7, 39}, {13, 1ull << 20, 7, 38},
    };
    for (const auto& l : limits) {
        HashPickIn h = {};
        h.nbases = (uint32_t)l[0];
        h.per_base = l[1];
        h.n = l[0] * l[1];
        h.len = l[2];
        h.stripe_stride = l[3];
        h.digest_off = -32;
        for (uint32_t b = 0; b < h.nbases; ++b) {
            h.base[b] = table_base(1, b);
            h.has_flag[b] = true;
        }
        h.depth = 2;
        h.unal = true;
        run(h);
    }
}

// The picks of a real geometry: shard files of 4096 records in separate
// 256-byte aligned allocations, as the benchmark and the server hold them.
void real(int k, int m, uint64_t block) {
    const uint64_t S = (block + (uint64_t)k - 1) / (uint64_t)k, n = 4096;
    for (int whole = 0; whole < 2; ++whole) {
        const int files = whole ? k + m : k;
        HashPickIn h = {};
        h.nbases = (uint32_t)files;
        h.per_base = n;
        h.n = (uint64_t)files * n;
        h.len = S;
        h.stripe_stride = 32 + S;
        h.digest_off = -32;
        for (int b = 0; b < files; ++b) {
            h.base[b] = kOrigin + (uint64_t)b * (1ull << 32) + 32;
            h.has_flag[b] = true;
        }
        h.depth = 2;
        h.unal = true;
        printf("RS(%d,%d) S=%llu pitch=%llu %s of %d files: ", k, m, (unsigned long long)S,
               (unsigned long long)h.stripe_stride, whole ? "whole-file verify" : "all-present GET", files);
        run(h);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4) {
        real(atoi(argv[1]), atoi(argv[2]), strtoull(argv[3], nullptr, 10));
        return 0;
    }
    table();
    printf("verify pick ok\n");
    return 0;
}
