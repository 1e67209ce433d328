// ivf_filter_plan_check.cpp — the two host plans of the IVF list filter (frankensearch_amd/csrc/ivf_filter_plan.hpp) on hand-made lists,
// counts and flags.  A plain program: tests/test_ivf_filter_contract.py builds it with the address and undefined-behaviour sanitizers
// and runs it as a child process.  Prints "ivf_filter_plan_check: ok" and exits 0, or names the first check that failed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ivf_filter_plan.hpp"

using namespace fsgpu;
using namespace fsgpu::ivf_filter;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("ivf_filter_plan_check: line %d: %s\n", __LINE__, #c); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

static std::vector<uint32_t> head_of(const std::vector<uint32_t>& members) {
    std::vector<uint32_t> head(members.size() + 1, 0u);
    for (size_t l = 0; l < members.size(); ++l) head[l + 1] = head[l] + members[l];
    return head;
}

int main() {
    // five lists: 17 rows, empty, 513 rows, 1 row, 40 rows; probed by 1, 3 (the empty one), 33, 0 and 2 queries
    const std::vector<uint64_t> offsets = {0, 17, 17, 530, 531, 571};
    const std::vector<uint32_t> members = {1, 3, 33, 0, 2};
    const std::vector<uint32_t> head = head_of(members);
    const uint32_t nlist = 5;
    uint64_t total = 0;
    const std::vector<uint64_t> first = pad_rows(nlist, offsets.data(), 16, &total);
    CHECK(first[0] == 0 && first[1] == 32 && first[2] == 32 && first[3] == 32 + 528 && first[4] == 32 + 528 + 16 && total == 32 + 528 + 16 + 48);

    {   // everything fits: one range; list 2 makes tiles of 16, 16 and 1 members with two items each
        const Caps caps{1ull << 26, 16, 16, 512, 128};
        const ScorePlan p = score_plan(nlist, offsets.data(), head.data(), first.data(), caps);
        CHECK(p.slots == 36 && p.tiles.size() == 6 && p.slot_tile.size() == 36 && p.ranges.size() == 1);
        CHECK(p.tiles[0].len == 17 && p.tiles[0].nmem == 1 && p.tiles[0].slot0 == 0 && p.tiles[0].item0 == 0 && p.tiles[0].scratch0 == 0);
        CHECK(p.tiles[1].len == 513 && p.tiles[1].nmem == 16 && p.tiles[1].slot0 == 1 && p.tiles[1].item0 == 1 && p.tiles[1].scratch0 == 32);
        CHECK(p.tiles[2].slot0 == 17 && p.tiles[2].item0 == 3 && p.tiles[2].scratch0 == 32 + 528 * 16);
        CHECK(p.tiles[3].nmem == 1 && p.tiles[3].slot0 == 33 && p.tiles[3].item0 == 5);
        CHECK(p.tiles[4].len == 40 && p.tiles[4].nmem == 2 && p.tiles[4].slot0 == 34 && p.tiles[4].item0 == 7 && p.tiles[4].ordered_row0 == first[4] &&
              p.tiles[4].list_pos0 == 531);
        CHECK(p.tiles[5].item0 == 8 && p.tiles[5].slot0 == 36);
        CHECK(p.slot_tile[0] == 0 && p.slot_tile[1] == 1 && p.slot_tile[16] == 1 && p.slot_tile[17] == 2 && p.slot_tile[33] == 3 && p.slot_tile[35] == 4);
        const Range& r = p.ranges[0];
        CHECK(r.tile_first == 0 && r.ntiles == 5 && r.item_first == 0 && r.nitems == 8 && r.slot_first == 0 && r.nslots == 36);
        CHECK(r.entries == 32 + 528 * 33 + 48 * 2);
    }
    {   // a scratch of 8,448 entries = one 16-member tile of list 2: four ranges, each restarting its scratch at 0
        const Caps caps{8448, 16, 16, 512, 128};
        const ScorePlan p = score_plan(nlist, offsets.data(), head.data(), first.data(), caps);
        CHECK(p.ranges.size() == 4);
        CHECK(p.ranges[0].ntiles == 1 && p.ranges[1].ntiles == 1 && p.ranges[2].ntiles == 1 && p.ranges[3].ntiles == 2);
        CHECK(p.ranges[1].tile_first == 1 && p.ranges[1].slot_first == 1 && p.ranges[1].nslots == 16 && p.ranges[1].item_first == 1 && p.ranges[1].nitems == 2);
        CHECK(p.ranges[3].slot_first == 33 && p.ranges[3].nslots == 3 && p.ranges[3].entries == 528 + 96);
        for (size_t t = 0; t < 5; ++t) CHECK(p.above[t] == 0);
        CHECK(p.tiles[1].scratch0 == 0 && p.tiles[2].scratch0 == 0 && p.tiles[3].scratch0 == 0 && p.tiles[4].scratch0 == 528);
    }
    {   // a scratch of 8,447 entries: the two full tiles of list 2 are above it, own no item and are in no range
        const Caps caps{8447, 16, 16, 512, 128};
        const ScorePlan p = score_plan(nlist, offsets.data(), head.data(), first.data(), caps);
        CHECK(p.above[0] == 0 && p.above[1] == 1 && p.above[2] == 1 && p.above[3] == 0 && p.above[4] == 0);
        CHECK(p.ranges.size() == 2 && p.ranges[0].ntiles == 1 && p.ranges[1].tile_first == 3 && p.ranges[1].ntiles == 2);
        CHECK(p.tiles[1].item0 == 1 && p.tiles[2].item0 == 1 && p.tiles[3].item0 == 1 && p.tiles[5].item0 == 4);
        CHECK(p.ranges[1].item_first == 1 && p.ranges[1].nitems == 3 && p.ranges[1].slot_first == 33 && p.ranges[1].nslots == 3);
    }
    {   // the second plan: slot 0 filtered with 5 candidates; of list 2's 33 slots, 3 .. 5 and 20 overflowed; list 4: one empty, one uncertified
        const Caps caps{1ull << 26, 16, 16, 512, 128};
        std::vector<uint32_t> counts(36, 7u), flags(36, 0u);
        counts[0] = 5;
        for (uint32_t s : {4u, 5u, 6u, 21u}) flags[s] = 1, counts[s] = 300;
        counts[34] = 0;
        flags[35] = 2, counts[35] = 0;
        const ScanPlan p = scan_plan(nlist, offsets.data(), head.data(), counts.data(), flags.data(), 10, 256, 64, caps);
        // groups: slot 0; slots 1 .. 3 (three), the run 4 .. 6, slots 7 .. 20 (fourteen), the run 21, slots 22 .. 33 (twelve); 34; the run 35
        CHECK(p.groups.size() == 1 + 3 + 1 + 14 + 1 + 12 + 1 + 1);
        CHECK(p.groups[0].from_cand == 1 && p.groups[0].rows_off == 0 && p.groups[0].n == 5 && p.groups[0].q0 == 0 && p.groups[0].nq == 1 && p.groups[0].nblocks == 1);
        const Group& run = p.groups[4];
        CHECK(run.from_cand == 0 && run.rows_off == 17 && run.n == 513 && run.q0 == 4 && run.nq == 3);
        CHECK(run.nblocks == 9);   // 513 rows are 9 tiles of 64; 4 x 256 CUs / 34 groups = 30 blocks at the most
        CHECK(p.groups[5].from_cand == 1 && p.groups[5].q0 == 7 && p.groups[5].rows_off == 7 * 128);
        const Group& one = p.groups[19];
        CHECK(one.from_cand == 0 && one.q0 == 21 && one.nq == 1 && one.n == 513);
        const Group& none = p.groups[32];
        CHECK(none.from_cand == 1 && none.q0 == 34 && none.n == 0 && none.nblocks == 1);
        const Group& unc = p.groups[33];
        CHECK(unc.from_cand == 0 && unc.rows_off == 531 && unc.n == 40 && unc.q0 == 35 && unc.nq == 1 && unc.nblocks == 1);
        CHECK(p.grid_x == 9);
        CHECK(p.rows_rescored == 5 + 7 * (3 + 14 + 12) + 513 * 4 + 0 + 40);
    }
    {   // nothing probed
        const std::vector<uint32_t> none(5, 0u), h = head_of(none);
        const Caps caps{1ull << 26, 16, 16, 512, 128};
        const ScorePlan p = score_plan(nlist, offsets.data(), h.data(), first.data(), caps);
        CHECK(p.slots == 0 && p.tiles.size() == 1 && p.ranges.empty());
        const ScanPlan s = scan_plan(nlist, offsets.data(), h.data(), nullptr, nullptr, 10, 256, 64, caps);
        CHECK(s.groups.empty() && s.grid_x == 0 && s.rows_rescored == 0);
    }
    std::printf("ivf_filter_plan_check: ok\n");
    return 0;
}
