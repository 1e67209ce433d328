"""What ONE launch of the per-query search path must write, in plain numpy and Python integers: the fused scan + top-k kernels
(scan_topk_kernel / scan_topk_kq_kernel, scan_mq_topk_kernel, scan_i8_topk_kernel<8 | 4>, scan_topk_f32_kernel) and merge_topk_kernel,
which finishes all of them.  fsgpu_lab_lone_stage (include/fsgpu_lab.h) runs one such launch on host arrays with an explicit grid;
tests/test_gpu_lone_stages.py compares the two, tests/test_lone_scan_contract.py holds this file to the oracle's whole-call answers without a
GPU.  Scores come from the oracle (gather_dot, dot_f32_bytes_f32) or are exact integers; the order is selection_ref's (rank_key,
best_first, pack).  What is restated from the kernels is only who visits which row (the tile walk) and which branch a merge takes."""
import ctypes
import functools

import numpy as np

from selection_ref import KEMPTY, best_first, pack, row_of, score_bits  # noqa: F401  (re-exported for the tests)

F16, F16_HOST_QUERY, F16_MQ, I8, I4, F32K, MERGE = 0, 1, 2, 3, 4, 5, 6
KIND_NAMES = {F16: "f16", F16_HOST_QUERY: "f16_host_query", F16_MQ: "f16_mq", I8: "i8", I4: "i4", F32K: "f32", MERGE: "merge"}
OK, INVALID_CONFIG, NULL_ARGUMENT = 0, 2, 8
WAVES_PER_BLOCK = 4
KERNARG_QUERY_DIMS = 512          # kKernargQueryDims
LDS_BUDGET = 160 * 1024
NT, U, HCAP = 1024, 4, 2048       # merge_topk_kernel: threads, entries per thread and round of the streaming pass, heads it can rank
F32 = np.float32


# ---- the launchers' predicates, restated (test_lone_scan_contract.py holds them against fsgpu_lab_lone_stage_check) ----------------------

def scan_lds_bytes(dim, nq, tier):
    return ((nq * dim * 4 + 15) & ~15) + WAVES_PER_BLOCK * nq * 2 * tier * 8


def row_bytes(kind, dim):
    return {F16: dim * 2, F16_HOST_QUERY: dim * 2, F16_MQ: dim * 2, I8: dim, I4: dim // 2, F32K: dim * 4}[kind]


def scan_ok(kind, nq, tier, dim, nrows, k, grid, row_stride=0, force_runtime_dim=0, plain_loads=0, hreduce=0):
    if tier not in (64, 256) or not 1 <= k <= tier or not 1 <= grid <= 4096 or not 1 <= nrows <= 1 << 22:
        return False
    if dim == 0 or dim > 4096 or dim % 8 or hreduce not in (0, 1, 2):
        return False
    if kind != F16 and (force_runtime_dim or plain_loads):
        return False
    strided = kind in (F16, F16_HOST_QUERY, F32K)
    if kind == F16:
        ok = nq in (1, 2, 4) and scan_lds_bytes(dim, nq, tier) <= LDS_BUDGET
    elif kind == F16_HOST_QUERY:
        ok = nq == 1 and dim <= KERNARG_QUERY_DIMS
    elif kind == F16_MQ:
        ok = nq in (4, 8) and dim in (128, 256, 384) and scan_lds_bytes(dim, nq, tier) <= LDS_BUDGET
    elif kind in (I8, I4):
        ok = nq == 1 and dim in (128, 256, 384, 512, 768)
    else:
        ok = nq in (1, 2, 4) and nq * dim * 4 <= 96 * 1024 and scan_lds_bytes(dim, nq, tier) <= LDS_BUDGET
    if not ok:
        return False
    rb = row_bytes(kind, dim)
    pitch = row_stride or rb
    if pitch < rb or pitch % 16 or pitch > 1 << 16 or (not strided and pitch != rb):
        return False
    return nrows * pitch <= 1 << 30


def merge_ok(nq, nlists, list_len, k, out_stride, l_stride, q_stride, lists_sorted=1):
    if not 1 <= nq <= 4096 or nlists == 0 or list_len == 0 or not 1 <= k <= 256 or out_stride < k or out_stride > 4096 or lists_sorted > 1:
        return False
    if nlists * list_len > 1 << 22 or l_stride < list_len or q_stride < (nlists - 1) * l_stride + list_len:
        return False
    return nq * q_stride <= 1 << 25


# ---- the order, vectorised (held to selection_ref.rank_key by the contract test) ---------------------------------------------------------

def sort_keys(entries):
    """The kernels' sortkey of packed entries as uint64: greater = better, 0 for kEmpty.  Sorting by it descending is best_first."""
    e = np.asarray(entries, np.uint64)
    bits = (e >> np.uint64(32)).astype(np.uint32)
    bits = np.where((bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0xFF800000), bits)
    ordv = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint64)
    key = (ordv << np.uint64(32)) | ((~e) & np.uint64(0xFFFFFFFF))
    return np.where(e == np.uint64(KEMPTY), np.uint64(0), key)


def canon_nan(entries):
    """Packed entries with every NaN score replaced by one NaN: a NaN's payload is the platform's, its place in a list is not."""
    e = np.asarray(entries, np.uint64).copy()
    bits = (e >> np.uint64(32)).astype(np.uint32)
    nan = ((bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)) & (e != np.uint64(KEMPTY))
    e[nan] = (np.uint64(0x7FC00000) << np.uint64(32)) | (e[nan] & np.uint64(0xFFFFFFFF))
    return e


# ---- scans -------------------------------------------------------------------------------------------------------------------------------

def tile_rows(kind, nq):
    """Rows of a wave tile: the lane-replicated f16 kernel shares its 16 quads among the queries of the pass."""
    return 16 // nq if kind in (F16, F16_HOST_QUERY) else 16


def unpack_nibbles(packed):
    """[n, dim / 2] bytes -> [n, dim] signed levels: low nibble = even dimension."""
    p = np.asarray(packed, np.uint8)
    lo = ((p & 0xF) ^ 8).astype(np.int32) - 8
    hi = ((p >> 4) ^ 8).astype(np.int32) - 8
    return np.stack([lo, hi], axis=-1).reshape(p.shape[:-1] + (p.shape[-1] * 2,))


def scores_of(kind, dim, hreduce, slab, queries):
    """[nq, nrows] f32: every row's score for every query of the pass, from the oracle (f16, F32) or exact integers (int8, 4-bit)."""
    from oracle import oracle
    n = slab.shape[0]
    if kind in (F16, F16_HOST_QUERY, F16_MQ):
        rows = np.ascontiguousarray(slab[:, :dim])
        q = np.asarray(queries, F32).reshape(-1, dim)
        return np.stack([oracle.gather_dot(rows, q[x], np.arange(n, dtype=np.uint32), hreduce) for x in range(q.shape[0])])
    if kind == F32K:
        q = np.asarray(queries, F32).reshape(-1, dim)
        return np.array([[oracle.dot_f32_bytes_f32(slab[r, :dim], q[x], hreduce) for r in range(n)] for x in range(q.shape[0])], F32)
    if kind == I8:
        dots = slab.astype(np.int64) @ np.asarray(queries, np.int8).astype(np.int64)
    else:
        dots = unpack_nibbles(slab).astype(np.int64) @ unpack_nibbles(np.asarray(queries, np.uint8)[None, :])[0].astype(np.int64)
    return dots.astype(F32)[None, :]


def block_of_rows(kind, nq, nrows, grid):
    """The block that visits each row: tile t belongs to wave t mod (4 grid), block b owns waves 4b .. 4b + 3."""
    tile = np.arange(nrows) // tile_rows(kind, nq)
    return (tile % (WAVES_PER_BLOCK * grid)) // WAVES_PER_BLOCK


def valid_rows(nrows, live, allow):
    v = np.ones(nrows, bool)
    if live is not None:
        v &= np.asarray(live, bool)[:nrows]
    if allow is not None:
        v &= np.asarray(allow, bool)[:nrows]
    return v


def expected_partial(kind, nq, nrows, grid, k, row_base, scores, live=None, allow=None):
    """[nq, grid, k] packed: per (query, block) the best-first top k of the block's valid rows, kEmpty padded."""
    out = np.full((nq, grid, k), np.uint64(KEMPTY))
    block = block_of_rows(kind, nq, nrows, grid)
    valid = valid_rows(nrows, live, allow)
    for b in range(grid):
        rows = np.flatnonzero((block == b) & valid)
        if rows.size == 0:
            continue
        for x in range(nq):
            best = best_first(pack(scores[x, rows], rows + row_base))[:k]
            out[x, b, :len(best)] = np.array(best, np.uint64)
    return out


def gate_walk(kind, nq, tier, nrows, grid, k, row_base, scores, live=None, allow=None, enough=None):
    """How often the busiest (wave, query) buffer compacts DURING its walk: a wave takes its tiles in order, a row is offered when its key
    beats the threshold, and a tile that does not fit the 2 tier slots sorts the buffer, keeps k and raises the threshold to the k-th.
    enough: stop looking once a wave has compacted that often."""
    cap, tr, nwaves = 2 * tier, tile_rows(kind, nq), WAVES_PER_BLOCK * grid
    valid = valid_rows(nrows, live, allow)
    ntiles = (nrows + tr - 1) // tr
    most = 0
    for x in range(nq):
        keys = [int(v) for v in sort_keys(pack(scores[x], np.arange(nrows) + row_base))]
        for w in range(min(nwaves, ntiles)):
            buf, thr, compactions = [], 0, 0
            for t in range(w, ntiles, nwaves):
                rows = [r for r in range(t * tr, min((t + 1) * tr, nrows)) if valid[r]]
                cand = [keys[r] for r in rows if keys[r] > thr]
                if not cand:
                    continue
                if len(buf) + len(cand) > cap:
                    compactions += 1
                    buf = sorted(buf, reverse=True)[:k]
                    thr = buf[k - 1] if len(buf) == k else 0
                    cand = [c for c in cand if c > thr]
                buf += cand
            most = max(most, compactions)
            if enough is not None and most >= enough:
                return most
    return most


def empty_blocks(kind, nq, nrows, grid):
    """Blocks none of whose waves has a tile."""
    return grid - len(set(block_of_rows(kind, nq, nrows, grid).tolist()))


# ---- merge -------------------------------------------------------------------------------------------------------------------------------

def merge_reference(lists, k, out_stride):
    """One query's answer: (rows u32 [out_stride], score bits u32 [out_stride], packed u64 [out_stride], count) — the k best real entries,
    best first, then the padding: row 0xffffffff, score bits of kEmpty's high word, packed kEmpty."""
    best = best_first(np.asarray(lists, np.uint64).ravel())[:k]
    packed = np.full(out_stride, np.uint64(KEMPTY))
    packed[:len(best)] = np.array(best, np.uint64)
    return (packed & np.uint64(0xFFFFFFFF)).astype(np.uint32), (packed >> np.uint64(32)).astype(np.uint32), packed, len(best)


def merge_regime(nlists, list_len, k, lists_sorted):
    """The branch of merge_topk_kernel a shape takes (launch_merge_topk and the kernel's own conditions)."""
    total = nlists * list_len
    mcap = 16384 if 8192 < total <= 16384 else 8192
    one_pass = total <= mcap
    use_heads = bool(lists_sorted) and k <= nlists <= HCAP
    ngroups = (nlists + 15) // 16
    return dict(mcap=mcap, one_pass=one_pass, per_thread=mcap // NT if one_pass else U, use_heads=use_heads,
                quick_heads=one_pass and use_heads and nlists <= NT and ngroups <= 64 and k <= ngroups,
                tail_bound=bool(lists_sorted) and list_len >= k)


def streaming_plan(lists, nlists, list_len, k, lists_sorted):
    """A streaming merge of one query's [nlists, list_len] entries: (entries that survive the pre-pass bound, in-loop re-sorts).  The
    pre-pass bound is the better of the best k-th entry of any list and the k-th largest head; a round takes NT x U entries in index order,
    and the buffer is sorted down to k (the threshold rising to the k-th) whenever it holds more than MCAP - NT x U."""
    reg = merge_regime(nlists, list_len, k, lists_sorted)
    assert not reg["one_pass"]
    keys = sort_keys(np.asarray(lists, np.uint64).reshape(nlists, list_len))
    thr = 0
    if lists_sorted:
        if reg["tail_bound"]:
            thr = int(keys[:, k - 1].max())
        if reg["use_heads"]:
            thr = max(thr, int(np.sort(keys[:, 0])[::-1][k - 1]))
        if thr:
            thr -= 1
    flat = keys.ravel()
    survivors = int(np.count_nonzero(flat > np.uint64(thr)))
    buf, resorts, room = [], 0, reg["mcap"] - NT * U
    for base in range(0, flat.size, NT * U):
        chunk = flat[base:base + NT * U]
        buf += [int(v) for v in chunk[chunk > np.uint64(thr)]]
        if len(buf) > room:
            resorts += 1
            buf = sorted(buf, reverse=True)[:k]
            if len(buf) >= k:
                thr = buf[k - 1]
    return survivors, resorts


# ---- the lab call ------------------------------------------------------------------------------------------------------------------------

def bitmap_words(mask):
    from oracle import oracle
    return oracle.live_bitmap(np.asarray(mask, bool))


class LabCall:
    """Fills a LoneStageArgs from keyword arguments; keeps every array alive until the call returns."""

    def __init__(self, **kw):
        from frankensearch_amd import _lib
        self.args = _lib.LoneStageArgs()
        self.keep = []
        for name, v in kw.items():
            if isinstance(v, np.ndarray):
                v = np.ascontiguousarray(v)
                self.keep.append(v)
                setattr(self, name, v)
                v = v.ctypes.data
            setattr(self.args, name, v)

    def check(self):
        from frankensearch_amd import _lib
        return _lib.lib().fsgpu_lab_lone_stage_check(ctypes.addressof(self.args))

    def run(self, device=0):
        from frankensearch_amd import _lib
        return _lib.lib().fsgpu_lab_lone_stage(device, ctypes.addressof(self.args))


def scan_call(kind, nq, tier, dim, nrows, k, grid, slab, queries, row_base=0, hreduce=0, row_stride=0, force_runtime_dim=0, plain_loads=0,
              live=None, allow=None):
    """The LabCall of one scan launch; .partial [nq * grid * k] receives the lists."""
    kw = dict(kind=kind, nq=nq, tier=tier, dim=dim, nrows=nrows, k=k, grid=grid, row_base=row_base, hreduce=hreduce, row_stride=row_stride,
              force_runtime_dim=force_runtime_dim, plain_loads=plain_loads, slab=slab, queries=queries,
              partial=np.zeros(nq * grid * k, np.uint64))
    for name, mask in (("live", live), ("allow", allow)):
        if mask is not None:
            kw[name] = bitmap_words(mask)
            kw["bitmap_words"] = kw[name].size
    return LabCall(**kw)


def merge_call(lists, nq, nlists, list_len, k, l_stride=0, q_stride=0, out_stride=0, lists_sorted=1,
               outputs=("out_rows", "out_scores", "out_packed", "out_counts")):
    """The LabCall of one merge launch; the outputs asked for are attributes of the call."""
    out_stride = out_stride or k
    l_stride = l_stride or list_len
    kw = dict(kind=MERGE, nq=nq, nlists=nlists, list_len=list_len, k=k, l_stride=l_stride, q_stride=q_stride or nlists * l_stride,
              out_stride=out_stride, lists_sorted=lists_sorted, lists=np.asarray(lists, np.uint64))
    shapes = dict(out_rows=(nq * out_stride, np.uint32), out_scores=(nq * out_stride, np.uint32), out_packed=(nq * out_stride, np.uint64),
                  out_counts=(nq, np.uint32))                # (scores travel as their bits)
    for name in outputs:
        kw[name] = np.zeros(*shapes[name])
    return LabCall(**kw)


@functools.lru_cache(maxsize=None)
def built():
    from frankensearch_amd.build import build
    from oracle import oracle
    build()
    oracle.build()
    return True
