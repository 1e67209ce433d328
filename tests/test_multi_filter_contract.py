"""A filter per query in one batched call, the part that needs no GPU: the entry points exist in the library, the
headers and the binding; the grouping and path decision (fsgpu_lab_multi_filter_plan, host code only) equals the plain restatement
of tests/multi_filter_ref.py at the 1/50 boundary and around it; the kernels of filter_gather_kernels.hip keep their state in
registers.  The answers themselves are checked on the GPU (tests/test_gpu_multi_filter.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import multi_filter_ref as R  # noqa: E402

PRODUCT = ("fsgpu_search_topk_batched_multi_filtered", "fsgpu_search_topk_batched_multi_filtered_device_queries",
           "fsgpu_allow_bitmap_rows", "fsgpu_index_multi_filter_stats")
LAB = ("fsgpu_lab_multi_filter_plan",)


@pytest.fixture(scope="module")
def L():
    from frankensearch_amd import _lib
    from frankensearch_amd.build import build

    build()
    return _lib.lib()


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fsgpu_[a-z0-9_]+)\s*\(", text))


def test_entry_points_are_exported_declared_and_bound(L):
    from frankensearch_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    for name in PRODUCT + LAB:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert set(PRODUCT) <= declared("fsgpu.h") and not set(LAB) & declared("fsgpu.h")
    assert set(LAB) <= declared("fsgpu_lab.h")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in PRODUCT:
        assert name in doc, name
    import frankensearch_amd as fa
    assert hasattr(fa.VectorIndex, "search_batched_per_query_filters") and hasattr(fa.VectorIndex, "multi_filter_stats")
    from frankensearch_amd.index import ResidentFilter
    assert hasattr(ResidentFilter, "rows")


def lab_plan(L, nrows, allowed, fq):
    allowed = np.ascontiguousarray(allowed, dtype=np.uint64)
    fq = np.ascontiguousarray(fq, dtype=np.int32)
    group = np.full(max(fq.size, 1), -7, dtype=np.int32)
    path = np.full(allowed.size + 1, -7, dtype=np.int32)
    ng = C.c_uint32(12345)
    st = L.fsgpu_lab_multi_filter_plan(nrows, allowed.ctypes.data, allowed.size, fq.ctypes.data, fq.size, group.ctypes.data,
                                       path.ctypes.data, C.byref(ng))
    return st, group[: fq.size].tolist(), path[: ng.value].tolist(), path[ng.value:].tolist()


def same_as_restatement(L, nrows, allowed, fq):
    st, group, path, untouched = lab_plan(L, nrows, allowed, fq)
    want_group, want_path, _ = R.plan(nrows, allowed, fq)
    assert st == 0 and group == want_group and path == want_path, (nrows, allowed, fq)
    assert all(v == -7 for v in untouched)   # nothing is written past the groups
    return group, path


def test_the_one_in_fifty_boundary(L):
    # allowed * 50 == nrows is dense, one row fewer is selective — at a corpus that divides by 50, one that does not, and a large one
    for nrows in (20_000, 4_099, 10_000_000, 50, 49, 51):
        edge = -(-nrows // 50)          # smallest allowed with allowed * 50 >= nrows
        _, path = same_as_restatement(L, nrows, [edge, edge - 1, edge + 1, 1, nrows], [0, 1, 2, 3, 4])
        assert path[0] == R.DENSE and path[2] == R.DENSE and path[4] == R.DENSE
        assert path[1] == (R.GATHER if edge - 1 > 0 else R.EMPTY)
        assert path[3] == (R.GATHER if 50 < nrows else R.DENSE)
    _, path = same_as_restatement(L, 20_000, [400, 399], [1, 0])
    assert path == [R.GATHER, R.DENSE]


def test_empty_filters_unfiltered_queries_and_unnamed_filters(L):
    group, path = same_as_restatement(L, 20_000, [0, 10, 0, 10_000], [-1, 0, 3, -1, 0, 1, -1])
    assert path == [R.UNFILTERED, R.EMPTY, R.DENSE, R.GATHER]       # filter 2 is named by no query: no group
    assert group == [0, 1, 2, 0, 1, 3, 0]
    group, path = same_as_restatement(L, 1_000, [], [-1, -1, -1])
    assert group == [0, 0, 0] and path == [R.UNFILTERED]
    st, group, path, _ = lab_plan(L, 1_000, [5], [])
    assert st == 0 and group == [] and path == []


def test_groups_keep_ascending_query_order_and_first_appearance_numbering(L):
    rng = np.random.default_rng(5)
    for trial in range(20):
        nf = int(rng.integers(1, 12))
        nrows = int(rng.integers(1, 100_000))
        allowed = rng.integers(0, max(2, nrows // 20), nf)
        fq = rng.integers(-1, nf, int(rng.integers(1, 300)))
        group, path = same_as_restatement(L, nrows, allowed, fq)
        firsts = [group.index(g) for g in range(len(path))]
        assert firsts == sorted(firsts)                      # numbered by first appearance
        for g in range(len(path)):
            members = [q for q in range(len(group)) if group[q] == g]
            assert members == sorted(members) and len({int(fq[q]) for q in members}) == 1
    fq = R.assignment()
    masks = R.filter_masks()
    group, path = same_as_restatement(L, R.N, [int(m.sum()) for m in masks], fq)
    sizes = sorted(group.count(g) for g in range(len(path)))
    assert sizes[0] == 1 and sizes[-1] == 40
    assert path.count(R.DENSE) == 1 and path.count(R.EMPTY) == 1 and path.count(R.UNFILTERED) == 1 and path.count(R.GATHER) == 35


def test_out_of_range_entries_are_refused(L):
    from frankensearch_amd import _lib
    for fq in ([0, 2], [-2], [0, 1, 5]):
        st, _, _, _ = lab_plan(L, 1_000, [3, 4], fq)
        assert st == _lib.ERR_INVALID_CONFIG, fq
        with pytest.raises(ValueError):
            R.plan(1_000, [3, 4], fq)


def test_no_kernel_of_the_gather_file_spills(L):
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "scripts", "list_spills.py"),
                                   os.path.join(ROOT, "frankensearch_amd", "libfsgpu.so"), r"filter_(gather|row_list)_"], timeout=300).decode()
    lines = [l for l in out.splitlines()[1:] if re.search(r"filter_(gather|row_list)_", l)]
    names = " ".join(lines)
    for kernel in ("filter_gather_scan_kernel<64>", "filter_gather_scan_kernel<256>", "filter_row_list_count_kernel",
                   "filter_row_list_scan_kernel", "filter_row_list_expand_kernel"):
        assert kernel in names, kernel
    for l in lines:
        m = re.match(r"vgpr\s+(\d+)\s+vgpr_spill\s+(\d+)\s+sgpr_spill\s+(\d+)\s+private\s+(\d+)", l)
        assert m and (int(m.group(2)), int(m.group(3)), int(m.group(4))) == (0, 0, 0), l


# ---- the cases of test_gpu_multi_filter_shapes.py (tests/multi_filter_cases.py) ----

import multi_filter_cases as M  # noqa: E402


def test_largest_gathered_dimensions_follow_from_the_lds_formula():
    """multi_filter_cases restates gather_row_pitch, filter_gather_lds_bytes and filter_gather_supported; the constants are read back
    from kernels.hpp, and the two limits are found again by trying every multiple of 8."""
    text = open(os.path.join(ROOT, "frankensearch_amd", "csrc", "kernels.hpp")).read()
    assert re.search(r"kGatherTileRows = (\d+);", text).group(1) == str(M.TILE_ROWS)
    assert re.search(r"kGatherMaxK = (\d+);", text).group(1) == str(M.MAX_K)
    assert re.search(r"kGatherLdsBudget = 160 \* 1024;", text) and M.LDS_BUDGET == 160 * 1024
    assert [M.row_pitch(d) for d in (64, 384, 8, 96, 104, 928, 1056)] == [320, 832, 64, 320, 320, 1856, 2112]   # 64 mod 256, >= the row
    dims = range(8, 4096, 8)
    assert max(d for d in dims if M.gather_supported(d, 64)) == M.MAX_DIM_K64 == 1056
    assert max(d for d in dims if M.gather_supported(d, 256)) == max(d for d in dims if M.gather_supported(d, 65)) == M.MAX_DIM_K256 == 928
    assert all(M.gather_supported(d, 64) for d in range(8, M.MAX_DIM_K64 + 8, 8))        # no gap below a limit
    assert all(M.gather_supported(d, 256) for d in range(8, M.MAX_DIM_K256 + 8, 8))
    assert (M.lds_bytes(1056, 64), M.lds_bytes(1064, 64), M.lds_bytes(928, 256), M.lds_bytes(936, 256)) == (156416, 172928, 150272, 166784)
    assert set(M.DIMS[d] for d in M.DIMS) >= {(0, 1), (0, 2), (0, 3), (1, 1)} and all(M.DIMS[d] == (d // 32, d // 8 % 4) for d in M.DIMS)


def test_a_plain_left_to_right_dot_differs_from_the_oracle_at_every_gathered_dimension(oracle):
    """Share of the filters' (query, row) pairs whose plain left-to-right f32 dot differs in bits from the oracle's, per dimension of
    the shape test, on that test's own rows and queries: printed; above dimension 8 it must not be zero (at 8 there is one product
    per accumulator and only the horizontal add's order is left: printed, not asserted)."""
    for dim in sorted(M.DIMS):
        c = M.shape_case(oracle, dim)
        rows = np.flatnonzero(np.any(c["masks"], axis=0)).astype(np.uint32)
        want = np.stack([oracle.gather_dot(c["slab"], q, rows) for q in c["queries"]])
        plain = M.left_to_right(c["slab"][rows], c["queries"])
        share = float((plain.view(np.uint32) != want.view(np.uint32)).mean())
        print(f"dimension {dim}: plain dot differs in {share:.4f} of the scores")
        if dim > 8:
            assert share > 0.0, dim


def test_tie_case_straddles_the_kth_place_and_holds_every_kind_of_score(oracle):
    for dim in (40, 384):
        c = M.tie_case(oracle, dim)
        nq = c["fq"].size // 2
        for f, k in ((0, 10), (1, 70)):
            rows = np.sort(np.flatnonzero(c["masks"][f]))
            assert np.array_equal(rows[list(M.TIE_DUPS)], c["dups"][f]) and rows.size == M.TIE_ALLOWED and M.TIE_ALLOWED * 50 < M.N
            assert 60 < M.TILE_ROWS <= 70                                            # the copies lie on both sides of the first tile's end
            assert np.unique(c["slab"][c["dups"][f]], axis=0).shape[0] == 1
            live = c["live"] & c["masks"][f]
            got, _ = oracle.search_top_k(c["slab"], c["queries"][f * nq], k, live=live)
            inside = np.isin(c["dups"][f], got)
            print(f"dim {dim} filter {f} k {k}: {int(inside.sum())} of {inside.size} equal rows inside the answer")
            assert 0 < inside.sum() < inside.size
            for i in range(nq):
                _, s = oracle.search_top_k(c["slab"], c["queries"][f * nq + i], 256, live=live)
                assert np.isnan(s).any() and (i >= 6 or (np.isposinf(s).any() and np.isneginf(s).any())), (dim, f, i)
