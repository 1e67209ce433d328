"""The IVF index's int8 list filter (include/fsgpu.h, "IVF index") restated in plain Python: numpy and tests/ivf_ref.py.
The int8 codes, the bound delta and the exact scores come in as arguments — from the oracle (oracle.quantize_slab_i8,
oracle/filter_bound.py) where no GPU is at hand, from fsgpu_index_int8_filter_bound on the device — so that the rule itself is the
only thing restated here.  The device is held to it exactly: integers, row ids, counts and flags, no tolerance.

  slots       the (list, query) pairs of the non-empty probed lists, by list, then by query (the probed-list search's own)
  scores      s_r = the int32 dot of the query's codes with row r's; DEAD for a row that is not live now
  select      |L| <= k: every live row.  Otherwise t = the k-th largest s_r with multiplicity, m = ceil(2 delta) and the
              candidates are the live rows with s_r >= t - m, ascending; more than SLOT_CAP of them: the slot overflows
  plans       the two host plans of ivf_filter_plan.hpp"""
import math

import numpy as np

import ivf_ref as R

DEAD = -(1 << 31)
OVERFLOW, UNCERTIFIED, ABOVE_SCRATCH = 1, 2, 4


def margin(delta):
    """ceil(2.0 * (double)delta) as an integer; delta is the device's f32 (or the oracle's f64) bound, >= 0."""
    return int(math.ceil(2.0 * float(delta)))


def slots(index, probed):
    """probed [nq, nprobe] lists -> [(query, list)] of the non-empty lists, by list, then by query."""
    out = []
    nq = len(probed)
    by_list = {}
    for q in range(nq):
        for l in probed[q]:
            by_list.setdefault(int(l), []).append(q)
    for l in sorted(by_list):
        if index.list_rows(l).size:
            out.extend((q, l) for q in sorted(by_list[l]))
    return out


def scores(codes_q, slab_i8, rows, live):
    """-> int64 [len(rows)]: the exact integer dots, DEAD where the row is not live."""
    s = slab_i8[rows].astype(np.int64) @ np.asarray(codes_q, dtype=np.int64)
    return np.where(live[rows], s, DEAD)


def select(s, rows, k, delta, slot_cap, m=None):
    """s: scores(...) of a slot, rows: its list -> (t, m, count, flag, candidates).  m: a margin to use in the place of ceil(2 delta)."""
    m = margin(delta) if m is None else m
    alive = np.nonzero(s != DEAD)[0]
    if alive.size <= k:
        t, keep = DEAD, alive
    else:
        t = int(np.sort(s[alive])[::-1][k - 1])
        keep = alive[s[alive] >= t - m]
    return t, m, int(keep.size), (OVERFLOW if keep.size > slot_cap else 0), np.asarray(rows)[keep].astype(np.uint32)


def exact_top_k(oracle, slab_u16, query, rows, live, k, hreduce=0):
    """The slot's answer today: the best k of its live rows under the reference's order."""
    cand = np.asarray(rows)[live[rows]].astype(np.uint32)
    sc = oracle.gather_dot(slab_u16, query, cand, hreduce)
    order = np.argsort(R.order_keys(sc, cand), kind="stable")[::-1][:k]
    return cand[order]


# ---- the host plans (ivf_filter_plan.hpp) -----------------------------------------------------------------------------------------

def round_up(v, a):
    return (v + a - 1) // a * a


def pad_rows(offsets, row_tile):
    lens = np.diff(np.asarray(offsets, dtype=np.int64))
    first = np.concatenate([[0], np.cumsum(round_up(lens, row_tile))])
    return first[:-1], int(first[-1])


def score_plan(offsets, members, scratch_cap, tile_queries, row_tile, item_rows):
    """-> (tiles [[ordered_row0, list_pos0, scratch0, len, slot0, nmem, item0, above]], ranges [[tile_first, ntiles, item_first, nitems,
    slot_first, nslots, entries]], slots)."""
    first, _ = pad_rows(offsets, row_tile)
    tiles, slot, item = [], 0, 0
    for l, cnt in enumerate(members):
        ln = int(offsets[l + 1]) - int(offsets[l])
        if not cnt or not ln:
            continue
        for m0 in range(0, cnt, tile_queries):
            nmem = min(tile_queries, cnt - m0)
            above = int(round_up(ln, row_tile) * nmem > scratch_cap)
            tiles.append([int(first[l]), int(offsets[l]), 0, ln, slot + m0, nmem, item, above])
            if not above:
                item += (ln + item_rows - 1) // item_rows
        slot += cnt
    ends = tiles + [[0, 0, 0, 0, slot, 0, item, 0]]
    ranges, t = [], 0
    while t < len(tiles):
        if tiles[t][7]:
            t += 1
            continue
        t0, used = t, 0
        while t < len(tiles) and not tiles[t][7]:
            entries = round_up(tiles[t][3], row_tile) * tiles[t][5]
            if used + entries > scratch_cap:
                break
            tiles[t][2] = used
            used += entries
            t += 1
        ranges.append([t0, t - t0, tiles[t0][6], ends[t][6] - tiles[t0][6], tiles[t0][4], ends[t][4] - tiles[t0][4], used])
    return tiles, ranges, slot


def scan_plan(offsets, members, counts, flags, k, num_cus, slot_cap, gather_tile_rows):
    """-> (groups [[rows_off, from_cand, n, q0, nq, nblocks]], grid_x, rows_rescored)."""
    groups, slot, rescored = [], 0, 0
    for l, cnt in enumerate(members):
        ln = int(offsets[l + 1]) - int(offsets[l])
        if not cnt or not ln:
            continue
        i = 0
        while i < cnt:
            s = slot + i
            if not flags[s]:
                groups.append([s * slot_cap, 1, int(counts[s]), s, 1, 1])
                rescored += int(counts[s])
                i += 1
                continue
            j = i
            while j < cnt and flags[slot + j]:
                j += 1
            groups.append([int(offsets[l]), 0, ln, s, j - i, 0])
            rescored += ln * (j - i)
            i = j
        slot += cnt
    by_device = min(1024, max(1, 4 * num_cus // max(len(groups), 1)))
    cap = max(1, min(by_device, 16384 // k))
    for g in groups:
        if not g[1]:
            g[5] = min((g[2] + gather_tile_rows - 1) // gather_tile_rows, cap)
    return groups, max([g[5] for g in groups], default=0), rescored
