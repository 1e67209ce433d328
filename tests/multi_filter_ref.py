"""Plain restatement of the grouping and path decision of fsgpu_search_topk_batched_multi_filtered, and the fixture
of tests/test_gpu_multi_filter.py.  numpy only; nothing here touches the library."""
import numpy as np

UNFILTERED, DENSE, GATHER, EMPTY = 0, 1, 2, 3
DIVISOR = 50   # GATHER_SELECTIVITY_DIVISOR (crates/frankensearch-index/src/search.rs:1667)


def path_of(nrows, allowed):
    if allowed == 0:
        return EMPTY
    return GATHER if allowed * DIVISOR < nrows else DENSE


def plan(nrows, allowed_per_filter, filter_of_query):
    """-> (group_of_query, path_of_group, filter_of_group).  Groups are numbered in the order their first query appears; no filter
    (-1) is a group like any other; a filter no query names forms none.  ValueError for an entry < -1 or >= the number of filters."""
    nf = len(allowed_per_filter)
    for f in filter_of_query:
        if f < -1 or f >= nf:
            raise ValueError(f)
    group_of_filter, group_of_query, path_of_group, filter_of_group = {}, [], [], []
    for f in filter_of_query:
        f = int(f)
        if f not in group_of_filter:
            group_of_filter[f] = len(path_of_group)
            path_of_group.append(UNFILTERED if f < 0 else path_of(nrows, int(allowed_per_filter[f])))
            filter_of_group.append(f)
        group_of_query.append(group_of_filter[f])
    return group_of_query, path_of_group, filter_of_group


# ---- the gather-scan fixture: N = 20,000 rows, 200 queries, 37 filters ------------------------------------------------------------
N, NQ, NF = 20_000, 200, 37
SIZES = (1, 7, 64, 65, 257, 399)          # all below N / 50 = 400: selective
DENSE_FILTER, EMPTY_FILTER = 35, 36
DUPLICATES = (100, 101, 5_000, 19_999)    # rows made equal to row 100: the row-asc tie-break
NAN_ROWS, PINF_ROWS, NINF_ROWS = (7, 3_001), (64, 12_345), (65, 9_000)
SPECIAL = DUPLICATES + NAN_ROWS + PINF_ROWS + NINF_ROWS + (0,)   # (row N - 1 is among the duplicates)


def doctor_slab(slab_u16):
    """Duplicated rows and rows holding f16 NaN / +inf / -inf, in place of a copy."""
    s = slab_u16.copy()
    for r in DUPLICATES[1:]:
        s[r] = s[DUPLICATES[0]]
    for r in NAN_ROWS:
        s[r, 3] = 0x7E00
    for r in PINF_ROWS:
        s[r, 5] = 0x7C00
    for r in NINF_ROWS:
        s[r, 5] = 0xFC00
    return s


def filter_masks(seed=11):
    """37 bool[N] masks: 35 selective ones of SIZES rows drawn from a pool of 2,500 rows (so that lists overlap), every third
    fourth holding the special rows as far as its size allows; one dense (every other row); one empty."""
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.choice(N, 2_500, replace=False))
    masks = []
    for f in range(35):
        size = SIZES[f % len(SIZES)]
        rows = []
        if f % 4 == 0:
            rows = list(SPECIAL[:size])
        cand = [int(r) for r in rng.permutation(pool) if int(r) not in rows]
        rows = rows + cand[: size - len(rows)]
        m = np.zeros(N, dtype=bool)
        m[rows] = True
        assert int(m.sum()) == size
        masks.append(m)
    dense = np.zeros(N, dtype=bool)
    dense[::2] = True
    masks.append(dense)
    masks.append(np.zeros(N, dtype=bool))
    return masks


def assignment(seed=12):
    """filter_of_query [200]: group sizes from 1 to 40, unfiltered queries, the dense and the empty filter, interleaved."""
    sizes = {0: 40, 1: 1, 2: 17, 3: 9, 4: 12, 5: 6, DENSE_FILTER: 11, EMPTY_FILTER: 3, -1: 19}
    left = NQ - sum(sizes.values())
    others = [f for f in range(6, 35)]
    for i in range(left):
        sizes[others[i % len(others)]] = sizes.get(others[i % len(others)], 0) + 1
    fq = np.concatenate([np.full(c, f, dtype=np.int32) for f, c in sizes.items()])
    assert fq.size == NQ
    return np.random.default_rng(seed).permutation(fq)


def tombstones(masks, seed=13):
    """live bool[N], set AFTER the filters were made: a tenth of every third filter's rows, one duplicate and one NaN row are deleted."""
    rng = np.random.default_rng(seed)
    live = np.ones(N, dtype=bool)
    for f in range(0, 35, 3):
        rows = np.flatnonzero(masks[f])
        live[rng.choice(rows, max(1, rows.size // 10), replace=False)] = False
    live[DUPLICATES[1]] = False
    live[NAN_ROWS[1]] = False
    live[rng.choice(N, 500, replace=False)] = False
    live[[DUPLICATES[0], DUPLICATES[2], DUPLICATES[3]]] = True   # three equal rows stay: ties inside the lists that hold them
    return live
