// ivf_filter_plan.hpp — the two host plans of the IVF index's int8 list filter (ivf_index.cpp; ivf_filter_kernels.hip).
// Pure host code: no HIP header, no device call.  tests/host/ivf_filter_plan_check.cpp compiles this file alone and checks it under the
// host sanitizers; fsgpu_lab_ivf_filter_score_plan and fsgpu_lab_ivf_filter_scan_plan hand the two functions to tests/test_ivf_filter_contract.py.
//
// Slots are the probed-list search's own (ivf_index.cpp): the (list, query) pairs of the non-empty lists, by list, then by query, so
// the members of a list are consecutive slots.  `head` is the counting sort's table: list l has head[l + 1] - head[l] member queries.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ivf_filter_tile.hpp"

namespace fsgpu {

namespace ivf_filter {

struct Caps {
    uint64_t scratch_entries;   // scores resident at once
    uint32_t tile_queries, row_tile, item_rows, slot_cap;
};

struct Range {   // consecutive tiles whose scores fit the scratch together: one score launch and one selection launch
    uint32_t tile_first, ntiles, item_first, nitems, slot_first, nslots;
    uint64_t entries;
};

struct ScorePlan {
    std::vector<IvfFilterTile> tiles;   // [ntiles + 1]: the last entry carries the end of the items (item0) and of the slots (slot0)
    std::vector<uint32_t> slot_tile;    // [slots]
    std::vector<uint8_t> above;         // [ntiles] 1: the tile alone exceeds the scratch and is in no range; its slots are scanned whole
    std::vector<Range> ranges;
    uint32_t slots = 0;
};

inline uint64_t round_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// The ordered copy's layout: the first row of every list, a multiple of row_tile, and (*total) the rows of the copy.
inline std::vector<uint64_t> pad_rows(uint32_t nlist, const uint64_t* offsets, uint32_t row_tile, uint64_t* total) {
    std::vector<uint64_t> first(nlist, 0);
    uint64_t rows = 0;
    for (uint32_t l = 0; l < nlist; ++l) {
        first[l] = rows;
        rows += round_up(offsets[l + 1] - offsets[l], row_tile);
    }
    *total = rows;
    return first;
}

// offsets [nlist + 1], head [nlist + 1], pad_row0 [nlist]
inline ScorePlan score_plan(uint32_t nlist, const uint64_t* offsets, const uint32_t* head, const uint64_t* pad_row0, const Caps& caps) {
    ScorePlan p;
    uint32_t slots = 0, items = 0;
    for (uint32_t l = 0; l < nlist; ++l) {
        const uint32_t cnt = head[l + 1] - head[l];
        const uint64_t len = offsets[l + 1] - offsets[l];
        if (!cnt || !len) continue;
        for (uint32_t m0 = 0; m0 < cnt; m0 += caps.tile_queries) {
            IvfFilterTile t{};
            t.ordered_row0 = pad_row0[l];
            t.list_pos0 = offsets[l];
            t.len = (uint32_t)len;
            t.slot0 = slots + m0;
            t.nmem = std::min(caps.tile_queries, cnt - m0);
            t.item0 = items;
            const uint64_t entries = round_up(len, caps.row_tile) * t.nmem;
            const bool above = entries > caps.scratch_entries;
            if (!above) items += (uint32_t)((len + caps.item_rows - 1) / caps.item_rows);
            p.above.push_back(above ? 1 : 0);
            for (uint32_t j = 0; j < t.nmem; ++j) p.slot_tile.push_back((uint32_t)p.tiles.size());
            p.tiles.push_back(t);
        }
        slots += cnt;
    }
    IvfFilterTile end{};
    end.item0 = items;
    end.slot0 = slots;
    p.tiles.push_back(end);
    p.slots = slots;
    // the ranges: greedy, in tile order; a tile above the scratch ends the range before it and belongs to none
    const uint32_t ntiles = (uint32_t)p.tiles.size() - 1;
    uint32_t t = 0;
    while (t < ntiles) {
        if (p.above[t]) {
            ++t;
            continue;
        }
        Range r{};
        r.tile_first = t;
        r.item_first = p.tiles[t].item0;
        r.slot_first = p.tiles[t].slot0;
        uint64_t used = 0;
        while (t < ntiles && !p.above[t]) {
            const uint64_t entries = round_up(p.tiles[t].len, caps.row_tile) * p.tiles[t].nmem;
            if (used + entries > caps.scratch_entries) break;
            p.tiles[t].scratch0 = used;
            used += entries;
            ++t;
        }
        r.ntiles = t - r.tile_first;
        r.nitems = p.tiles[t].item0 - r.item_first;
        r.nslots = p.tiles[t].slot0 - r.slot_first;
        r.entries = used;
        p.ranges.push_back(r);
    }
    return p;
}

struct Group {   // a FilterGatherGroup before its pointer: rows at cand + rows_off (from_cand) or at list_rows + rows_off
    uint64_t rows_off;
    uint32_t from_cand, n, q0, nq, nblocks;
};

struct ScanPlan {
    std::vector<Group> groups;
    uint32_t grid_x = 0;
    uint64_t rows_rescored = 0;   // candidates of the filtered slots + whole lists of the others
};

// counts, flags: [slots] what the selection reported (flag != 0: the slot is scanned over its whole list).  A filtered slot is one
// single-member group over its candidates (none: a group without rows, whose list comes out empty); the other members of a list are
// grouped by runs of consecutive slots.  blocks per whole-list group: today's rule (ivf_index.cpp) over the number of groups.
inline ScanPlan scan_plan(uint32_t nlist, const uint64_t* offsets, const uint32_t* head, const uint32_t* counts, const uint32_t* flags, uint32_t k,
                          uint32_t num_cus, uint32_t gather_tile_rows, const Caps& caps) {
    ScanPlan p;
    uint32_t slots = 0;
    for (uint32_t l = 0; l < nlist; ++l) {
        const uint32_t cnt = head[l + 1] - head[l];
        const uint64_t len = offsets[l + 1] - offsets[l];
        if (!cnt || !len) continue;
        uint32_t i = 0;
        while (i < cnt) {
            const uint32_t s = slots + i;
            if (!flags[s]) {
                p.groups.push_back(Group{(uint64_t)s * caps.slot_cap, 1u, counts[s], s, 1u, 1u});
                p.rows_rescored += counts[s];
                ++i;
                continue;
            }
            uint32_t j = i;
            while (j < cnt && flags[slots + j]) ++j;
            p.groups.push_back(Group{offsets[l], 0u, (uint32_t)len, s, j - i, 0u});
            p.rows_rescored += len * (j - i);
            i = j;
        }
        slots += cnt;
    }
    const uint32_t ngroups = (uint32_t)p.groups.size();
    const uint32_t by_device = std::min<uint32_t>(1024, std::max<uint32_t>(1, 4 * num_cus / std::max<uint32_t>(ngroups, 1)));
    const uint32_t cap = std::max<uint32_t>(1, std::min<uint32_t>(by_device, 16384 / std::max<uint32_t>(k, 1)));
    for (Group& g : p.groups) {
        if (!g.from_cand) g.nblocks = std::min<uint32_t>((g.n + gather_tile_rows - 1) / gather_tile_rows, cap);
        p.grid_x = std::max(p.grid_x, g.nblocks);
    }
    return p;
}

}  // namespace ivf_filter
}  // namespace fsgpu
