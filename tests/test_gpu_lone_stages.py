"""ONE launch of a per-query scan kernel or of merge_topk_kernel at a time, through fsgpu_lab_lone_stage (the product's launchers on host
arrays, the grid chosen by the case), against the plain reference of tests/lone_scan_ref.py over the tables of tests/lone_scan_cases.py.
Equality is exact: every block's list is the best-first top k of the rows that block visited, compared entry for entry as uint64 (a NaN
score as "a NaN at this place": its payload is the platform's); a merge's rows, score bits, packed entries, counts and padding are
compared as they are.  tests/test_lone_scan_contract.py holds the reference and the cases' regimes without a GPU.  The composition tests
feed the lab's block lists to the lab's merge and compare with the product's own answer on the same data: the lab route is the product's."""
import numpy as np
import pytest

import lone_scan_cases as T
import lone_scan_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def built():
    R.built()


def last_error():
    from frankensearch_amd import _lib
    return _lib.last_error()


def first_difference(got, want):
    where = np.argwhere(got != want)
    i = tuple(where[0])
    return f"{len(where)} entries differ, first at (query, block, slot) {i}: got {int(got[i]):#018x}, want {int(want[i]):#018x}"


@pytest.mark.parametrize("c", T.scan_cases(), ids=lambda c: c.name)
def test_scan_launch(c):
    call = T.lab_call(c)
    assert call.run() == R.OK, last_error()
    got = R.canon_nan(call.partial).reshape(c.nq, c.grid, c.k)
    want = R.canon_nan(T.expected_of(c))
    assert np.array_equal(got, want), first_difference(got, want)


@pytest.mark.parametrize("c", T.merge_cases(), ids=lambda c: c.name)
def test_merge_launch(c):
    call = T.merge_lab_call(c)
    assert call.run() == R.OK, last_error()
    lists = T.merge_lists(c)
    for q in range(c.nq):
        rows, bits, packed, n = R.merge_reference(lists[q], c.k, c.out_stride)
        span = slice(q * c.out_stride, (q + 1) * c.out_stride)
        if "out_counts" in c.outputs:
            assert call.out_counts[q] == n, (q, int(call.out_counts[q]), n)
        if "out_packed" in c.outputs:
            assert np.array_equal(call.out_packed[span], packed), q
        if "out_rows" in c.outputs:
            assert np.array_equal(call.out_rows[span], rows), q
        if "out_scores" in c.outputs:
            assert np.array_equal(call.out_scores[span], bits), q


# ---- the lab route is the product's route --------------------------------------------------------------------------------------------------

N, K, GRID = 3000, 10, 7


def lab_search(kind, nq, tier, dim, slab, queries, k=K, grid=GRID, n=N):
    """One scan launch, then one merge launch over its lists: (rows [nq, k], score bits [nq, k], counts [nq])."""
    scan = R.scan_call(kind, nq, tier, dim, n, k, grid, slab, queries)
    assert scan.run() == R.OK, last_error()
    merge = R.merge_call(scan.partial, nq, grid, k, k)
    assert merge.run() == R.OK, last_error()
    return merge.out_rows.reshape(nq, k), merge.out_scores.reshape(nq, k), merge.out_counts


@pytest.mark.parametrize("kind,nq,dim", [(R.F16, 2, 384), (R.F16, 4, 72), (R.F16_HOST_QUERY, 1, 384), (R.F16_MQ, 8, 384), (R.F16_MQ, 4, 128)],
                         ids=["f16-q2", "f16-q4-runtime-dim", "host-query", "mq-q8", "mq-q4"])
def test_f16_lists_merge_to_the_products_answer(kind, nq, dim):
    from frankensearch_amd import VectorIndex
    f16, _, _, _, q, _, _ = T.base()
    slab, queries = f16[:N, :dim].copy(), q[:nq, :dim].copy()
    rows, bits, counts = lab_search(kind, nq, 64, dim, slab, queries)
    prows, pscores, pcounts = VectorIndex.from_slab(slab).search_batch(queries, K, exact=True)
    assert np.array_equal(counts, pcounts) and np.array_equal(rows, prows) and np.array_equal(bits, pscores.view(np.uint32))


@pytest.mark.parametrize("nq,dim", [(1, 104), (4, 384)])
def test_f32_lists_merge_to_the_products_answer(nq, dim):
    from frankensearch_amd import VectorIndex
    _, f32, _, _, q, _, _ = T.base()
    slab, queries = f32[:N, :dim].copy(), q[:nq, :dim].copy()
    rows, bits, counts = lab_search(R.F32K, nq, 64, dim, slab, queries)
    prows, pscores, pcounts = VectorIndex.from_slab_f32(slab).search_batch(queries, K)
    assert np.array_equal(counts, pcounts) and np.array_equal(rows, prows) and np.array_equal(bits, pscores.view(np.uint32))


@pytest.mark.parametrize("kind", [R.I8, R.I4], ids=["int8", "4bit"])
def test_quantised_lists_merge_to_the_products_two_pass_answer(kind):
    """Pass 1 through the lab (the cc = k x multiplier best integer scores), the exact re-score from the oracle, the k best of those."""
    from frankensearch_amd import VectorIndex
    from oracle import oracle
    f16, _, _, _, q, _, _ = T.base()
    dim, mult = 384, 3
    slab, query = f16[:N, :dim].copy(), q[0, :dim].copy()
    if kind == R.I8:
        qslab, qquery = oracle.quantize_slab_i8(slab), oracle.quantize_query_i8(query)
    else:
        qslab, qquery = oracle.pack_slab_4bit(slab), oracle.pack_query_4bit(query)
    cand, _, counts = lab_search(kind, 1, 64, dim, qslab, qquery, k=K * mult)
    assert counts[0] == K * mult
    exact = oracle.gather_dot(slab, query, cand[0])
    best = R.best_first(R.pack(exact, cand[0]))[:K]
    idx = VectorIndex.from_slab(slab)
    hits = idx.search_top_k_int8_two_pass(query, K, mult) if kind == R.I8 else idx.search_top_k_4bit_two_pass(query, K, mult)
    assert [h.index for h in hits] == [R.row_of(e) for e in best]
    assert np.array_equal(np.array([h.score for h in hits], F32).view(np.uint32), np.array([R.score_bits(e) for e in best], np.uint32))
