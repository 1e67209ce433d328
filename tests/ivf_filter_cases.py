"""Fixtures of the IVF list filter's tests, shared by tests/test_gpu_ivf_filter.py and the checks that need no GPU
(tests/test_ivf_filter_contract.py).  numpy, tests/ivf_cases.py and tests/ivf_filter_ref.py only; the oracle comes in as an argument."""
import numpy as np

import ivf_cases as CS
import ivf_filter_ref as FR
import ivf_ref as R

F32 = np.float32

# ---- the caps, from kernels.hpp's constants -------------------------------------------------------------------------------------
K_CAP, SLOT_CAP, SCRATCH_ENTRIES = 64, 128, 1 << 26
TILE_QUERIES, ROW_TILE, ITEM_ROWS, PITCH_ALIGN = 16, 16, 512, 64
FLAG_OVERFLOW, FLAG_UNCERTIFIED, FLAG_ABOVE_SCRATCH = FR.OVERFLOW, FR.UNCERTIFIED, FR.ABOVE_SCRATCH
KERNELS_HPP = {"kIvfFilterKCap": K_CAP, "kIvfFilterSlotCap": SLOT_CAP, "kIvfFilterScratchEntries": SCRATCH_ENTRIES,
               "kIvfFilterTileQueries": TILE_QUERIES, "kIvfFilterRowTile": ROW_TILE, "kIvfFilterItemRows": ITEM_ROWS,
               "kIvfFilterPitchAlign": PITCH_ALIGN}

# ---- the two corpora of the contract ----------------------------------------------------------------------------------------------
# clustered: the margin is far below the score spread, a slot keeps a few rows; hashmix: the rows lie in a few dozen bundles, the
# margin is wider than a bundle's spread and slots overflow
CLUSTERED = dict(nlist=64, iters=4, k=10, nprobe=4, nq=60)
HASHMIX = dict(nlist=16, iters=3, k=10, nprobe=2, nq=40, seed=3)


def clustered(oracle, nq=CLUSTERED["nq"]):
    slab, queries = CS.clustered(oracle, nq=nq)
    return slab, queries, None


def hashmix(oracle):
    slab = CS.hashmix(oracle)
    return slab, CS.noisy_queries(slab, HASHMIX["nq"], HASHMIX["seed"]), CS.one_in_seven_dead(slab.shape[0])


def cpu_slots(oracle, slab, queries, index, live, k, nprobe, m=None, hreduce=0):
    """Every slot of the call on the CPU, with the oracle's codes and its f64 bound -> [(q, list, rows, s, delta, select(...), exact top k)];
    a query whose bound is negative yields select None."""
    from oracle import filter_bound as FB
    stats = FB.slab_stats(slab)
    slab_i8 = oracle.quantize_slab_i8(slab)
    live_b = np.ones(slab.shape[0], dtype=bool) if live is None else np.asarray(live, dtype=bool)
    probed = [R.probe(oracle, index, q, nprobe) for q in queries]
    bounds = [FB.query_bound(q, stats, slab.shape[1]) for q in queries]
    out = []
    for q, l in FR.slots(index, probed):
        rows = index.list_rows(l)
        delta, _, codes = bounds[q]
        s = FR.scores(codes, slab_i8, rows, live_b)
        sel = FR.select(s, rows, k, delta, SLOT_CAP, m=m) if delta >= 0 else None
        out.append((q, l, rows, s, delta, sel, FR.exact_top_k(oracle, slab, queries[q], rows, live_b, k, hreduce)))
    return out


# ---- tile edges: caller's centroids that make lists of chosen lengths ---------------------------------------------------------------
EDGE_LENS = (1, 15, 16, 17, 10, 11, 513, 0)   # k = 10: k and k + 1; the last list is empty


def edge_corpus(dim=64, lens=EDGE_LENS):
    """List c holds lens[c] rows around the unit vector e_c (its centroid, the caller's); rows ascending by list.  The queries are
    e_c plus a little noise, so query c's best list is c and the others follow in an order the noise picks.
    -> (slab u16, init centroids, lens)"""
    rng = np.random.default_rng(43)
    n = sum(lens)
    rows = 0.05 * rng.standard_normal((n, dim)).astype(F32)
    at = 0
    for c, ln in enumerate(lens):
        rows[at:at + ln, c] += 1.0
        at += ln
    init = np.zeros((len(lens), dim), dtype=F32)
    for c in range(len(lens)):
        init[c, c] = 1.0
    return CS.f16(rows), init, lens


def edge_queries(dim, members, nlist=len(EDGE_LENS), target=6):
    """`members` queries around e_target (the 513-row list by default): that many member queries on one list."""
    rng = np.random.default_rng(47 + members)
    q = 0.02 * rng.standard_normal((members, dim)).astype(F32)
    q[:, target] += 1.0
    return q


MEMBER_COUNTS = (1, 15, 16, 17, 33)
