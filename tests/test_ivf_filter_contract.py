"""The IVF index's int8 list filter without a GPU: the rule of tests/ivf_filter_ref.py against the exact per-slot
answers on the CPU, with the oracle's int8 codes and its f64 bound (oracle/filter_bound.py); the fixtures of
tests/ivf_filter_cases.py against their own preconditions; the caps against kernels.hpp's constants; the two host plans of
ivf_filter_plan.hpp against their restatement, through the library and — under the host sanitizers — as a plain program."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ivf_filter_cases as FC
import ivf_filter_ref as FR
import ivf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frankensearch_amd", "csrc")


def lost_rows(slots):
    return sum(len(set(exact.tolist()) - set(sel[4].tolist())) for (_, _, _, _, _, sel, exact) in slots if sel is not None)


@pytest.fixture(scope="module")
def clustered(oracle):
    slab, queries, live = FC.clustered(oracle, nq=100)
    c = FC.CLUSTERED
    return slab, queries, live, R.build(oracle, slab, c["nlist"], c["iters"], live=live)


@pytest.fixture(scope="module")
def hashmix(oracle):
    slab, queries, live = FC.hashmix(oracle)
    c = FC.HASHMIX
    return slab, queries, live, R.build(oracle, slab, c["nlist"], c["iters"], live=live)


# ---- the rule keeps every slot's exact top k; without the margin it does not ----

def test_the_margin_is_what_keeps_the_exact_top_k_on_the_clustered_corpus(oracle, clustered):
    slab, queries, live, index = clustered
    c = FC.CLUSTERED
    queries = queries[:c["nq"]]
    without = FC.cpu_slots(oracle, slab, queries, index, live, c["k"], c["nprobe"], m=0)
    assert len(without) == 240 and lost_rows(without) == 28   # the k-th integer score as the cut loses true top-k rows
    held = FC.cpu_slots(oracle, slab, queries, index, live, c["k"], c["nprobe"])
    assert len(held) == 240 and lost_rows(held) == 0
    for (_, _, _, _, _, sel, exact) in held:
        assert set(exact.tolist()) <= set(sel[4].tolist())


def test_the_margin_is_what_keeps_the_exact_top_k_on_the_hashmix_rows(oracle, hashmix):
    slab, queries, live, index = hashmix
    c = FC.HASHMIX
    without = FC.cpu_slots(oracle, slab, queries, index, live, c["k"], c["nprobe"], m=0)
    assert len(without) == 76 and lost_rows(without) == 178
    held = FC.cpu_slots(oracle, slab, queries, index, live, c["k"], c["nprobe"])
    assert len(held) == 76 and lost_rows(held) == 0
    for (_, _, rows, s, _, sel, exact) in held:
        assert set(exact.tolist()) <= set(sel[4].tolist())
        assert (np.diff(sel[4].astype(np.int64)) > 0).all()          # ascending rows
        assert not (s[np.isin(rows, sel[4])] == FR.DEAD).any()       # no dead row among them


# ---- the fixtures' preconditions ----

def test_the_clustered_corpus_neither_overflows_nor_leaves_a_query_uncertified(oracle, clustered):
    slab, queries, live, index = clustered
    k = FC.CLUSTERED["k"]
    most, kept, total = 0, 0, 0
    for nprobe in (1, 4, 8):
        slots = FC.cpu_slots(oracle, slab, queries, index, live, k, nprobe)
        assert all(sel is not None and sel[3] == 0 for (_, _, _, _, _, sel, _) in slots), nprobe
        most = max(most, max(sel[2] for (_, _, _, _, _, sel, _) in slots))
        if nprobe == 8:
            kept, total = sum(sel[2] for (_, _, _, _, _, sel, _) in slots), sum(len(rows) for (_, _, rows, _, _, _, _) in slots)
    assert most <= 29 and most <= FC.SLOT_CAP
    assert kept < 0.1 * total   # a slot keeps a few rows in a hundred: the exact scan has little left to do


def test_the_hashmix_rows_overflow(oracle, hashmix):
    slab, queries, live, index = hashmix
    c = FC.HASHMIX
    slots = FC.cpu_slots(oracle, slab, queries, index, live, c["k"], c["nprobe"])
    counts = [sel[2] for (_, _, _, _, _, sel, _) in slots]
    # measured on these 40 queries: 54 of the 76 slots overflow, up to 439 candidates in a slot, 73.7 % of the probed rows kept (the
    # figures quoted for this fixture from other query draws: up to 445 and about 78 %)
    assert sum(sel[3] == FR.OVERFLOW for (_, _, _, _, _, sel, _) in slots) == 54 and max(counts) == 439
    kept = sum(counts) / sum(len(rows) for (_, _, rows, _, _, _, _) in slots)
    assert 0.73 < kept < 0.75   # the margin is wider than a bundle's score spread
    assert any(sel[3] == 0 for (_, _, _, _, _, sel, _) in slots)                       # ... and some slots still pass through the filter


def test_the_edge_corpus_makes_the_lists_it_promises(oracle):
    slab, init, lens = FC.edge_corpus()
    index = R.build(oracle, slab, len(lens), 0, init=init)
    assert np.diff(index.offsets.astype(np.int64)).tolist() == list(lens)
    for members in FC.MEMBER_COUNTS:
        q = FC.edge_queries(slab.shape[1], members)
        assert all(int(R.probe(oracle, index, x, 1)[0]) == 6 for x in q)


def test_the_caps_are_the_constants_of_kernels_hpp():
    text = open(os.path.join(CSRC, "kernels.hpp")).read()
    for name, want in FC.KERNELS_HPP.items():
        m = re.search(r"\b" + name + r"\s*=\s*([^;,]+)[;,]", text)
        assert m, name
        expr = m.group(1).replace("ull", "").replace("u", "").strip()
        assert eval(expr) == want, (name, m.group(1))
    assert re.search(r"kIvfFilterDead\s*=\s*INT32_MIN", text)
    flags = re.search(r"kIvfFilterFlagOverflow = (\d+), kIvfFilterFlagUncertified = (\d+), kIvfFilterFlagAboveScratch = (\d+)", text)
    assert tuple(int(x) for x in flags.groups()) == (FC.FLAG_OVERFLOW, FC.FLAG_UNCERTIFIED, FC.FLAG_ABOVE_SCRATCH)


# ---- the host plans ----

def _lib():
    from frankensearch_amd import _lib
    from frankensearch_amd.build import build
    build()
    return _lib.lib()


def library_score_plan(offsets, members, scratch_cap):
    L = _lib()
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    mem = np.ascontiguousarray(members, dtype=np.uint32)
    cap = int(mem.sum()) + 8
    tiles, ranges = np.zeros((cap, 8), np.uint64), np.zeros((cap, 7), np.uint64)
    nt, nr, slots = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    rc = L.fsgpu_lab_ivf_filter_score_plan(mem.size, off.ctypes.data, mem.ctypes.data, scratch_cap, cap, tiles.ctypes.data, C.byref(nt), cap,
                                           ranges.ctypes.data, C.byref(nr), C.byref(slots))
    assert rc == 0
    return tiles[:nt.value].astype(np.int64).tolist(), ranges[:nr.value].astype(np.int64).tolist(), slots.value


def library_scan_plan(offsets, members, counts, flags, k, num_cus):
    L = _lib()
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    mem = np.ascontiguousarray(members, dtype=np.uint32)
    cnt, flg = np.ascontiguousarray(counts, dtype=np.uint32), np.ascontiguousarray(flags, dtype=np.uint32)
    cap = int(mem.sum()) + 8
    groups = np.zeros((cap, 6), np.uint64)
    ng, gx, rr = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    rc = L.fsgpu_lab_ivf_filter_scan_plan(mem.size, off.ctypes.data, mem.ctypes.data, cnt.ctypes.data, flg.ctypes.data, k, num_cus, cap,
                                          groups.ctypes.data, C.byref(ng), C.byref(gx), C.byref(rr))
    assert rc == 0
    return groups[:ng.value].astype(np.int64).tolist(), gx.value, rr.value


HAND_OFFSETS, HAND_MEMBERS = [0, 17, 17, 530, 531, 571], [1, 3, 33, 0, 2]


@pytest.mark.parametrize("scratch,ranges,above", [(1 << 26, 1, 0), (8448, 4, 0), (8447, 2, 2), (623, 3, 2), (95, 1, 4), (31, 0, 5)])
def test_the_score_plan_is_its_restatement_on_both_sides_of_the_scratch_cap(scratch, ranges, above):
    got = library_score_plan(HAND_OFFSETS, HAND_MEMBERS, scratch)
    want = FR.score_plan(HAND_OFFSETS, HAND_MEMBERS, scratch, FC.TILE_QUERIES, FC.ROW_TILE, FC.ITEM_ROWS)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] == 36
    assert len(got[1]) == ranges and sum(t[7] for t in got[0]) == above
    covered = sorted(s for r in got[1] for s in range(r[4], r[4] + r[5]))
    in_no_range = sorted(s for t in got[0] if t[7] for s in range(t[4], t[4] + t[5]))
    assert sorted(covered + in_no_range) == list(range(36))   # every slot is in one range, or its tile is above the scratch
    for r in got[1]:
        assert r[6] <= scratch
        tiles = got[0][r[0]:r[0] + r[1]]
        assert tiles[0][2] == 0 and all(b[2] == a[2] + FR.round_up(a[3], FC.ROW_TILE) * a[5] for a, b in zip(tiles, tiles[1:]))


def test_the_scan_plan_is_its_restatement_on_hand_made_counts_and_flags():
    rng = np.random.default_rng(5)
    counts, flags = np.full(36, 7, np.uint32), np.zeros(36, np.uint32)
    counts[0], counts[34] = 5, 0
    flags[[4, 5, 6, 21]], flags[35] = FR.OVERFLOW, FR.UNCERTIFIED
    for k, cus in ((10, 256), (64, 256), (1, 8)):
        got = library_scan_plan(HAND_OFFSETS, HAND_MEMBERS, counts, flags, k, cus)
        assert got == tuple(FR.scan_plan(HAND_OFFSETS, HAND_MEMBERS, counts, flags, k, cus, FC.SLOT_CAP, 64))
    groups, grid_x, rescored = got
    assert sorted(s for g in groups for s in range(g[3], g[3] + g[4])) == list(range(36))   # every slot is scanned by one group
    # ... and on random lists, members, counts and flags, with enough groups for the scan's ranges of 65,535
    lens = rng.integers(0, 200, size=4000)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    members = rng.integers(0, 60, size=4000)
    slots = int(members[lens > 0].sum())
    counts, flags = rng.integers(0, 129, size=slots), rng.choice([0, 0, 0, 1, 2, 4], size=slots)
    got = library_scan_plan(offsets, members, counts, flags, 10, 256)
    assert got == tuple(FR.scan_plan(offsets, members, counts, flags, 10, 256, FC.SLOT_CAP, 64))
    assert len(got[0]) > 65535
    tiles, ranges, nslots = library_score_plan(offsets, members, 5000)
    assert (tiles, ranges, nslots) == FR.score_plan(offsets, members, 5000, FC.TILE_QUERIES, FC.ROW_TILE, FC.ITEM_ROWS) and nslots == slots


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_the_plan_header_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "ivf_filter_plan_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                            "-I", CSRC, os.path.join(ROOT, "tests", "host", "ivf_filter_plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ivf_filter_plan_check: ok" and not run.stderr, (run.returncode, run.stdout, run.stderr)
    text = open(os.path.join(CSRC, "ivf_filter_plan.hpp")).read()
    assert "#include <hip" not in text and "hip_runtime" not in text   # the header stays host-only
    assert "ivf_filter::scan_plan(" in open(os.path.join(CSRC, "ivf_index.cpp")).read()   # and the search goes through it
