"""The stage contract of the batched scan (mfma_scan.hip's scan_mfma_kernel, mfma_wide.hip's scan_wide_kernel and the query preparation)
in plain numpy, f64 or integer: which (query, row) pairs ONE launch must report and with which score.  DESIGN.md, "The scan stage
contract", states it in words.  fsgpu_lab_scan_stage (include/fsgpu_lab.h) runs one such launch on host arrays; tests/test_gpu_scan_stages.py
compares the two, tests/test_scan_stage_contract.py checks this file against brute force without a GPU."""
import ctypes

import numpy as np

LDS, REG, PREPARE = 0, 1, 2
KEMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
UNWRITTEN = np.uint64(0xCDCDCDCDCDCDCDCD)      # what the lab entry prefills list, spill and dense areas with
UNWRITTEN32 = np.uint32(0xCDCDCDCD)
SPILL_COUNT_STRIDE = 16                        # kMfmaSpillCountStride
LDS_MAX_SLOTS, REG_MAX_SLOTS = 32, 32          # scan_mfma_max_slots (shapes 0 and 2), kWideSlots
LDS_DIMS = (64, 128, 256, 384)                 # scan_mfma_supported
LDS_SHAPES = {0: dict(nqt=4, wpb=4, rt=1), 2: dict(nqt=8, wpb=8, rt=2)}   # the shapes a shipped build contains
OK, INVALID_CONFIG, DEVICE_ERROR, NULL_ARGUMENT = 0, 2, 6, 8


# ---- the launchers' predicates, restated (test_scan_stage_contract.py holds them against the library's) ---------------------------------

def wide_supported(dim, eb):
    rowb = dim * eb
    return rowb in (768, 512) or (eb == 1 and rowb in (384, 256))


def wide_max_query_tiles(dim, eb):
    per_tile = dim * eb // 64 * 4
    fit = 144 // per_tile if per_tile else 0
    return min(fit, 3 if eb != 1 else 5)


def _wide_chunk_ksteps(ks, qt):
    if ks == 12:
        return 2 if qt >= 3 else 3
    if ks == 6:
        return 1 if qt >= 5 else 3
    if ks == 4:
        return 1 if qt >= 7 else 2
    return ks // 2 if ks >= 2 else 1


def wide_split(rowb, eb, qt):
    """The shape runs the query-tile-split loop (wide_split_ok with the shipped options)."""
    ks = rowb // 64
    room = qt * ks * 4 + 4 * _wide_chunk_ksteps(ks, qt) * 4 + 8 * qt <= 190
    return eb == 1 and room and rowb < 512 and qt >= 2 and qt * ks * 4 + 2 * ks * 4 + 9 * qt <= 200


def wide_group_maxima_supported(dim, qt):
    return dim in (384, 256) and 2 <= qt <= 5 and wide_split(dim, 1, qt)


def group_queries(kernel, variant):
    return LDS_SHAPES[variant]["nqt"] * 16 if kernel == LDS else 128 * variant


def tile_rows(kernel, variant, stage, dim, eb):
    """Rows per tile of the block-to-tile mapping."""
    if kernel == LDS:
        return 16 if stage == 0 else 16 * LDS_SHAPES[variant]["rt"]
    rowb = dim * eb
    if stage == 2 and wide_split(rowb, eb, variant):
        return 128
    return 32 if rowb >= 512 else 64


def instantiations(lab_only=True):
    """Every (kernel, dim, elem_bytes, variant, stage) the predicates accept: the LDS-query kernel at shapes 0 and 2 (what the batched
    planner selects: mf_shape_* = 2, the 64-query shape 0), the register-query kernel at 2..scan_wide_max_query_tiles.  lab_only: also
    int8 rows of 512 / 768 bytes, which scan_wide_supported admits and no search reaches (its sample stages need scan_mfma_supported)."""
    out = []
    for dim in LDS_DIMS:
        for eb in (2, 1):
            for shape in sorted(LDS_SHAPES):
                for stage in (0, 1, 2):
                    out.append((LDS, dim, eb, shape, stage))
    for eb in (2, 1):
        for dim in (64, 128, 256, 384, 512, 768):
            if not wide_supported(dim, eb) or (dim not in LDS_DIMS and not lab_only):
                continue
            for qt in range(2, wide_max_query_tiles(dim, eb) + 1):
                for stage in (1, 2, 3):
                    if stage == 3 and (eb != 1 or not wide_group_maxima_supported(dim, qt)):
                        continue
                    out.append((REG, dim, eb, qt, stage))
    return out


def inst_id(inst):
    kernel, dim, eb, variant, stage = inst
    return f"{'lds' if kernel == LDS else 'reg'}-d{dim}-{'f16' if eb == 2 else 'i8'}-{'s' if kernel == LDS else 'qt'}{variant}-st{stage}"


# ---- scores -----------------------------------------------------------------------------------------------------------------------------

def pack(score_f32, row):
    return (np.asarray(score_f32, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(row, np.uint64)


def unpack(entries):
    e = np.asarray(entries, np.uint64)
    return (e >> np.uint64(32)).astype(np.uint32).view(np.float32), (e & np.uint64(0xFFFFFFFF)).astype(np.int64)


def scores_int(slab_i8, q_i8):
    """[nq, nrows] int64 dot products of int8 rows (the first q.shape[1] elements of each) with int8 queries."""
    dim = q_i8.shape[1]
    # (in f64 through BLAS: every product and partial sum is an integer below 2^53, so the result is exact)
    return np.rint(q_i8.astype(np.float64) @ slab_i8[:, :dim].astype(np.float64).T).astype(np.int64)


def scores_f16(slab_u16, q_u16):
    """f64 dot products of the f16 rows with the f16 queries, and gamma = dim 2^-23 |q| |r|: the accumulation term of the bound in
    mfma_scan.hip's header (f32 accumulation of exact f16 x f16 products)."""
    dim = q_u16.shape[1]
    r = slab_u16[:, :dim].view(np.float16).astype(np.float64)
    q = q_u16.view(np.float16).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = q @ r.T
        gamma = dim * 2.0 ** -23 * np.sqrt((q * q).sum(axis=1))[:, None] * np.sqrt((r * r).sum(axis=1))[None, :]
    return s, gamma


# ---- rows ------------------------------------------------------------------------------------------------------------------------------

def bitmap_words(bits_bool):
    """bool [nrows] -> uint64 words, bit i of word w = row 64 w + i."""
    n = len(bits_bool)
    padded = np.zeros((n + 63) // 64 * 64, np.uint8)
    padded[:n] = bits_bool
    return np.packbits(padded.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint64).copy()


def valid_rows(nrows, live=None, allow=None):
    v = np.ones(nrows, bool)
    for words in (live, allow):
        if words is not None:
            bits = np.unpackbits(np.asarray(words, np.uint64).view(np.uint8), bitorder="little")[:nrows].astype(bool)
            v &= bits
    return v


def sample_rows(nrows, group_stride, group_count):
    """bool [nrows]: the rows of the 64-row groups {j group_stride : j < group_count}."""
    m = np.zeros(nrows, bool)
    for j in range(group_count):
        m[j * group_stride * 64:(j * group_stride + 1) * 64] = True
    return m


def visited_rows(kernel, stage, nrows, group_stride, group_count):
    if (kernel == LDS and stage < 2) or (kernel == REG and stage != 2):
        return sample_rows(nrows, group_stride, group_count)
    if kernel == REG:
        return np.ones(nrows, bool)
    return ~sample_rows(nrows, group_stride, group_count)       # tile_skipped: the groups of the stage-1 sample


def expected_rows(scores, tau, mask):
    """Per query the rows (ascending) a thresholded stage must report: visited, valid, score >= tau (a NaN on either side: not)."""
    with np.errstate(invalid="ignore"):
        return [np.flatnonzero(mask & (scores[q] >= np.float64(tau[q]))) for q in range(scores.shape[0])]


def gap_tau(scores_q, mask, rank, gamma_max, max_walk=64):
    """A threshold with no ambiguous row: from the rank-th best visited, valid score walk down to the first neighbours more than
    4 gamma_max apart; their midpoint, rounded to f32.  Returns (tau, ranks walked); ranks walked > max_walk raises."""
    s = scores_q[mask]
    s = np.sort(s[np.isfinite(s)])[::-1]
    assert len(s) > rank + max_walk, "too few rows for the rank"
    for step in range(max_walk + 1):
        hi, lo = s[rank - 1 + step], s[rank + step]
        if hi - lo > 4 * gamma_max:
            tau = np.float32((hi + lo) / 2)
            assert lo + gamma_max < np.float64(tau) < hi - gamma_max
            return tau, step
    raise AssertionError(f"no gap of 4 gamma within {max_walk} ranks of rank {rank}")


def tile_block(t, grid, ntiles, reverse):
    """The block that scans tile t: block b's n-th tile is n grid + ((b - n) mod grid), counted from the slab's end under reverse."""
    rounds = (ntiles + grid - 1) // grid
    f = rounds * grid - 1 - t if reverse else t
    n, j = divmod(f, grid)
    return (j + n) % grid


def row_block(row, kernel, variant, stage, dim, eb, grid, nrows, group_stride, group_count, reverse):
    """The block whose list row `row` (a visited row) lands in."""
    tr = tile_rows(kernel, variant, stage, dim, eb)
    if (kernel == LDS and stage < 2) or (kernel == REG and stage != 2):
        tpg = 64 // tr
        g = row // 64
        t = (g // group_stride) * tpg + (row % 64) // tr
        ntiles = group_count * tpg
    else:
        t = row // tr
        ntiles = (nrows + tr - 1) // tr
    return tile_block(t, grid, ntiles, reverse)


def dense_expected(scores_f32, valid, nrows, group_stride, group_count, row_base):
    """Stage 0: slot p of the sample is row (p // 64) group_stride 64 + p % 64; pack(score, row_base + row) or kEmpty for an invalid row.
    scores_f32 [nq, nrows] f32 (exact for int8 rows); returns (entries [nq, span], rows [span], ok [span])."""
    p = np.arange(group_count * 64)
    rows = (p // 64) * group_stride * 64 + p % 64
    ok = rows < nrows
    ok[ok] &= valid[rows[ok]]
    safe = np.where(rows < nrows, rows, 0)
    e = pack(scores_f32[:, safe], (row_base + rows)[None, :])
    e[:, ~ok] = KEMPTY
    return e, rows, ok


def group_maxima_expected(scores, valid, nrows, grid, group_stride, group_count, reverse):
    """Stage 3 (64-row tiles, one per sample group): per (query, block, row quarter fk) the largest integer score over the live, allowed
    rows g + fk 4 + {0..3}, g + 16 + fk 4 + {0..3} of every 32-row pair g of the block's tiles that lies wholly below nrows; None where
    there is none.  Returns (best [nq, grid, 4] int64 with a `have` mask, classes: (block, fk) -> list of g)."""
    nq = scores.shape[0]
    lowest = np.iinfo(np.int64).min
    best = np.full((nq, grid, 4), lowest, np.int64)
    classes = {(b, fk): [] for b in range(grid) for fk in range(4)}
    for t in range(group_count):
        b = tile_block(t, grid, group_count, reverse)
        for g in (t * group_stride * 64, t * group_stride * 64 + 32):
            if g + 32 > nrows:
                continue
            for fk in range(4):
                classes[(b, fk)].append(g)
                rows = np.array([g + fk * 4 + r for r in range(4)] + [g + 16 + fk * 4 + r for r in range(4)])
                rows = rows[valid[rows]]
                if len(rows):
                    best[:, b, fk] = np.maximum(best[:, b, fk], scores[:, rows].max(axis=1))
    return best, best != lowest, classes


# ---- query preparation -------------------------------------------------------------------------------------------------------------------

def prepare_delta_bound(q_f32, max_norm):
    """delta_q of mfma_scan.hip's header in f64 (the kernel may only be ABOVE it by its own f32 rounding; it inflates |q| by 1.0001)."""
    q = q_f32.astype(np.float64)
    dim = q.shape[1]
    return (2.0 ** -11 * (1 + 2.0 ** -11) + dim * 2.0 ** -23) * max_norm * np.sqrt((q * q).sum(axis=1)) + np.sqrt(dim) * 2.0 ** -25 * max_norm


def levels_4bit(packed):
    """oracle.pack_query_4bit's nibbles -> one signed level (-7..7) per dimension (low nibble = even dimension)."""
    p = np.asarray(packed, np.uint8)
    lo = ((p & 0x0F) ^ 0x08).astype(np.int16) - 8
    hi = ((p >> 4) ^ 0x08).astype(np.int16) - 8
    return np.stack([lo, hi], axis=1).reshape(-1).astype(np.int8)


# ---- the lab entry ----------------------------------------------------------------------------------------------------------------------

def _args(kernel, **kw):
    from frankensearch_amd import _lib
    a = _lib.ScanStageArgs()
    a.kernel = kernel
    for name, value in kw.items():
        setattr(a, name, value)
    return a


def check_args(kernel, **kw):
    """fsgpu_lab_scan_stage_check: the status the argument validation gives (0 = it would be launched); needs no device."""
    from frankensearch_amd import _lib
    return _lib.lib().fsgpu_lab_scan_stage_check(ctypes.byref(_args(kernel, **kw)))


def _stop_on_device_error(status):
    """A device error that is not the guard bands' ends the whole run: nothing more is started on a GPU that may have faulted."""
    from frankensearch_amd import _lib
    if status == DEVICE_ERROR and "guard band" not in _lib.last_error():
        import pytest
        pytest.exit(f"fsgpu_lab_scan_stage: device error ({_lib.last_error()}); no further launches", returncode=3)


def run_scan(kernel, variant, stage, eb, dim, slab, queries, tau, *, grid, slots=0, spill_cap=0, groups=0, live=None, allow=None,
             group_stride=1, group_count=0, row_stride=0, row_base=0, reverse=0, side_by_side=0, want_counts=0, nrows=None, expect=0):
    """One launch.  slab: the rows as the kernel reads them (uint16 / int8, [nrows, row elements]); queries [nq_pad, dim] likewise.
    Returns a dict of the outputs the stage writes, or the status when it is not `expect`ed to be FSGPU_OK."""
    from frankensearch_amd import _lib
    slab = np.ascontiguousarray(slab)
    queries = np.ascontiguousarray(queries)
    nrows = slab.shape[0] if nrows is None else nrows
    nq_pad = queries.shape[0]
    keep = [slab, queries]
    a = _args(kernel, variant=variant, stage=stage, elem_bytes=eb, dim=dim, nrows=nrows, row_stride=row_stride, row_base=row_base, grid=grid,
              groups=groups, side_by_side=side_by_side, reverse=reverse, group_stride=group_stride, group_count=group_count, slots=slots,
              spill_cap=spill_cap, nq_pad=nq_pad, want_counts=want_counts)
    a.slab, a.queries = slab.ctypes.data, queries.ctypes.data
    for name, arr, dt in (("live", live, np.uint64), ("allow", allow, np.uint64), ("tau", tau, np.float32)):
        if arr is not None:
            arr = np.ascontiguousarray(arr, dt)
            keep.append(arr)
            setattr(a, name, arr.ctypes.data)
    gmax = kernel == REG and stage == 3
    dense = kernel == LDS and stage == 0
    out = {}
    if dense:
        out["dense"] = np.zeros((nq_pad, group_count * 64), np.uint64)
    else:
        out["cand"] = np.zeros((nq_pad, grid, 4 if gmax else slots), np.uint64)
        if not gmax:
            out["spill"] = np.zeros((nq_pad, max(spill_cap, 1)), np.uint64)
            out["spill_count"] = np.zeros((nq_pad, SPILL_COUNT_STRIDE), np.uint32)
            out["overflow"] = np.zeros(nq_pad, np.uint32)
            if want_counts:
                out["cand_count"] = np.zeros((nq_pad, grid), np.uint32)
    for name, arr in out.items():
        setattr(a, name, arr.ctypes.data)
    status = _lib.lib().fsgpu_lab_scan_stage(0, ctypes.byref(a))
    _stop_on_device_error(status)
    if expect != 0 or status != 0:
        assert status == expect, (status, _lib.last_error())
        return status
    if "spill" in out:
        out["spill"] = out["spill"][:, :spill_cap]
    return out


def run_prepare(q_f32, nq_pad, eb, max_norm=None, bits=8, expect=0):
    """The query preparation: returns (prepared [nq_pad, dim] uint16 / int8, delta [nq_pad])."""
    from frankensearch_amd import _lib
    q = np.ascontiguousarray(q_f32, np.float32)
    nq, dim = q.shape
    prepared = np.zeros((nq_pad, dim), np.uint16 if eb == 2 else np.int8)
    delta = np.zeros(nq_pad, np.float32)
    mx = int(np.float32(max_norm if max_norm is not None else 0).view(np.uint32))
    a = _args(PREPARE, elem_bytes=eb, dim=dim, nq=nq, nq_pad=nq_pad, max_norm_bits=mx, bits=bits)
    a.queries_f32, a.prepared, a.delta = q.ctypes.data, prepared.ctypes.data, delta.ctypes.data
    status = _lib.lib().fsgpu_lab_scan_stage(0, ctypes.byref(a))
    _stop_on_device_error(status)
    if expect != 0 or status != 0:
        assert status == expect, (status, _lib.last_error())
        return status
    return prepared, delta


def collect(out, nq_pad, grid, slots, spill_cap):
    """What a thresholded launch reported: (taken [nq_pad, grid, slots] bool: the list slots that hold an entry, lens [nq_pad, grid],
    spills: per query the entries in its spill area).  Checks the lists' form on the way: at most `slots` entries, no hole before a
    list's end, kEmpty padding (with list lengths: the counted slots written, nothing said about the rest)."""
    cand = out["cand"]
    assert cand.shape == (nq_pad, grid, slots)
    slot = np.arange(slots)[None, None, :]
    if "cand_count" in out:
        lens = out["cand_count"].astype(np.int64)
        assert not np.any(out["cand_count"] == UNWRITTEN32), "a list length was not written"
        assert lens.max(initial=0) <= slots, "a list length beyond slots"
        taken = slot < lens[:, :, None]
        assert not np.any(cand[taken] == UNWRITTEN) and not np.any(cand[taken] == KEMPTY), "a counted slot was not written"
    else:
        filled = cand != KEMPTY
        lens = filled.sum(axis=2).astype(np.int64)
        taken = slot < lens[:, :, None]
        assert np.array_equal(filled, taken), "a hole before a list's end"
        assert not np.any(cand == UNWRITTEN), "a slot neither written nor padded"
    counts = out["spill_count"]
    assert np.all(counts[:, 1:] == 0), "a spill counter off its stride"
    spills = []
    for q in range(nq_pad):
        sp = out["spill"][q, :min(int(counts[q, 0]), spill_cap)]
        assert not np.any(sp == UNWRITTEN), ("a counted spill slot was not written", q)
        spills.append(sp)
    return taken, lens, spills
