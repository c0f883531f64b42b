// The rounds of a record-stripe operation (mixed-length GET, mixed-length heal)
// run on a CPU: the planner's own round planning, flag translation and redo
// (rustfs_amd/csrc/rs_mixed_decode_plan.h), which are what record_rounds in
// rsgpu.cpp runs, around a fake kernel that fails the hash of the records a
// table calls rotten.  Shared by mixed_decode_plan_main.cpp and
// mixed_heal_plan_main.cpp.
#pragma once

#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "../../rustfs_amd/csrc/rs_mixed_decode_plan.h"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
            exit(1);                                                  \
        }                                                             \
    } while (0)

namespace rounds_check {

using namespace rsg::mixed;

// What one stripe must end with, worked out on its own: plan, drop every
// rotten record the plan reads, again, until a plan reads nothing rotten or
// there is no plan.
template <class PlanFn>
uint32_t settle(uint32_t mask, uint32_t rotten, PlanFn plan) {
    MaskPlan p;
    while (plan(mask, p) && (p.read_mask() & rotten)) mask &= ~(p.read_mask() & rotten);
    return mask;
}

// The stripes d[0 .. n) from masks[] to the end; rotten[s]: the shards whose
// record of stripe s fails its hash when read.  Returns the number of rounds.
// Checked in every round:
//   - a group has a launch exactly when its mask has a plan, and read[] says so;
//   - the launches' slices tile the table in launch order, and the table is a
//     partition of the todo stripes whose mask has a plan: every one once,
//     inside the slice of its own mask's launch, chunk counts descending there;
//   - row_shard[] is the sources, then -1 per written row, then the surplus:
//     the shards of read_mask() once each;
//   - redo is ascending, every redone stripe lost a bit, no mask gained one, and
//     a stripe without a launch is neither redone nor changed.
// At the end every mask is what settle() says.  *launching (optional): the
// rounds that had a launch, which is what record_rounds runs; the count
// returned is one higher when the last stripes end without a plan, in a round
// that only finds that out.
template <class PlanFn>
int run_rounds(int k, int m, const OutRule& rule, const std::vector<RecordDesc>& d, const uint32_t* rotten,
               uint32_t* masks, PlanFn plan, int* launching = nullptr) {
    const size_t n = d.size(), t = (size_t)(k + m);
    std::vector<uint32_t> want(n);
    for (size_t s = 0; s < n; ++s) want[s] = settle(masks[s], rotten[s], plan);
    std::vector<uint32_t> todo(n), redo;
    for (size_t i = 0; i < n; ++i) todo[i] = (uint32_t)i;
    std::vector<uint8_t> flags(n * t, 1);  // by shard
    Round r;
    int rounds = 0;
    while (!todo.empty()) {
        CHECK(++rounds <= (int)t + 1);  // the last round finds nothing to redo
        plan_round(rule, d.data(), 0, 0, 0, masks, todo, plan, r);
        CHECK(r.read.size() == r.groups.size());
        MaskPlan p;
        size_t li = 0, at = 0;
        std::set<uint32_t> tabled, launched;
        for (size_t g = 0; g < r.groups.size(); ++g) {
            const MaskGroup& gr = r.groups[g];
            if (!plan(gr.mask, p)) {
                CHECK(r.read[g] == 0);
                continue;
            }
            launched.insert(gr.stripes.begin(), gr.stripes.end());
            CHECK(li < r.launches.size());
            const RoundLaunch& l = r.launches[li++];
            CHECK(l.group == g && l.at == at && l.n == gr.stripes.size() && l.at + l.n <= r.table.size());
            at += l.n;
            CHECK(l.plan.src == p.src && l.plan.written == p.written && l.plan.surplus == p.surplus);
            CHECK(r.read[g] == p.read_mask() && r.read[g] != 0);
            std::set<uint32_t> jobs;
            for (size_t i = l.at; i < l.at + l.n; ++i) {
                const DecDesc& x = r.table[i];
                CHECK(x.job < n && masks[x.job] == gr.mask && x.len == d[x.job].shard_len);
                CHECK(i == l.at || chunks_of(r.table[i - 1].len) >= chunks_of(x.len));
                CHECK(jobs.insert(x.job).second && tabled.insert(x.job).second);
            }
            CHECK(jobs == std::set<uint32_t>(gr.stripes.begin(), gr.stripes.end()));
            CHECK(l.row_shard.size() == (size_t)k + (size_t)p.rows());
            uint32_t rows_read = 0;
            size_t unread = 0;
            for (size_t row = 0; row < l.row_shard.size(); ++row) {
                const int shard = l.row_shard[row];
                const bool written = row >= (size_t)k && row < (size_t)k + p.written.size();
                CHECK(written == (shard < 0));
                if (written) {
                    ++unread;
                    continue;
                }
                CHECK(shard < (int)t && !(rows_read >> shard & 1u));
                CHECK(shard == (row < (size_t)k ? p.src[row] : p.surplus[row - (size_t)k - p.written.size()]));
                rows_read |= 1u << shard;
            }
            CHECK(rows_read == p.read_mask() && unread == p.written.size());
        }
        CHECK(li == r.launches.size() && at == r.table.size() && tabled == launched);
        if (launching && !r.launches.empty()) ++*launching;
        // the fake kernel: of every launch, every stripe of its slice, every row read
        std::vector<uint8_t> rows(n * t, 0xaa);
        for (const RoundLaunch& l : r.launches)
            for (size_t i = l.at; i < l.at + l.n; ++i)
                for (size_t row = 0; row < l.row_shard.size(); ++row)
                    if (l.row_shard[row] >= 0)
                        rows[r.table[i].job * t + row] = !(rotten[r.table[i].job] >> l.row_shard[row] & 1u);
        const std::vector<uint32_t> before(masks, masks + n);
        shard_flags_from_rows(r, 0, rows.data(), t, flags.data());
        redo_from_flags((int)t, r.groups, r.read.data(), 0, flags.data(), t, masks, redo);
        for (size_t i = 0; i < redo.size(); ++i) {
            CHECK(i == 0 || redo[i - 1] < redo[i]);
            CHECK(launched.count(redo[i]) == 1);
            CHECK(popcount32(masks[redo[i]]) < popcount32(before[redo[i]]));  // at least one bit fewer
        }
        for (size_t s = 0; s < n; ++s) {
            CHECK((masks[s] & ~before[s]) == 0);
            if (!launched.count((uint32_t)s)) CHECK(masks[s] == before[s]);
        }
        todo = redo;
    }
    for (size_t s = 0; s < n; ++s) CHECK(masks[s] == want[s]);
    return rounds;
}

}  // namespace rounds_check
