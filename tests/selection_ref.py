"""The selection contract of the batched search (mfma_scan.hip's select_kernel, select_groups_kernel, list_cut_kernel and
two_pass_merge_kernel) in plain numpy and Python integers: what ONE launch must write.  DESIGN.md, "The selection contract", states it in
words.  fsgpu_lab_select (include/fsgpu_lab.h) runs one such launch on host arrays; tests/test_gpu_selection.py compares the two,
tests/test_selection_contract.py checks this file against brute force without a GPU.  No wave logic here: where a kernel promises only a
bound, the PARTITION that defines the bound is restated from the kernel's index arithmetic (quick_group, groups_wave) and nothing else."""
import ctypes

import numpy as np

SELECT, SELECT_GROUPS, LIST_CUT, TWO_PASS_MERGE = 0, 1, 2, 3
KEMPTY = 0xFFFFFFFFFFFFFFFF
UNWRITTEN = 0xCDCDCDCDCDCDCDCD           # what the lab entry prefills output areas with
UNWRITTEN32 = 0xCDCDCDCD
SPILL_COUNT_STRIDE = 16                  # kMfmaSpillCountStride
POOL = 1024                              # kSelectPool
SORT_CAP = 8192                          # kSelSortCap: live entries the sorted form holds; entries per pass of the extraction form
SORT_ABOVE = 32                          # ranks above it take the sorted form
SELECT_MAX_K, GROUPS_TAKEN, GROUPS_TAKEN_MAX, GROUPS_RANK_MAX, QUERY_LDS = 128, 24, 32, 128, 1024
OK, INVALID_CONFIG, DEVICE_ERROR, NULL_ARGUMENT = 0, 2, 6, 8
F32 = np.float32
NEG_INF, POS_INF = F32(-np.inf), F32(np.inf)


# ---- the launchers' predicates, restated (test_selection_contract.py holds them against fsgpu_lab_select_check) --------------------------

def select_ok(k, nlists=1, list_len=1, finish=False, k_out=1, dim=8, slab_f32=False, row_stride=0):
    if k < 1 or k > SELECT_MAX_K or nlists * list_len > 0x7FFFFFFF:
        return False
    if finish:
        if k_out < 1 or k_out > 64 or dim % 8:
            return False
        if slab_f32 and row_stride and row_stride != dim * 4:
            return False
    return True


def select_groups_ok(k, nentries, rank_only, dim=8):
    if k < 1 or nentries == 0 or nentries > 1024:
        return False
    if rank_only:
        return k <= GROUPS_RANK_MAX
    return k <= GROUPS_TAKEN_MAX and dim % 8 == 0 and dim <= QUERY_LDS


def list_cut_ok(nlists, list_len):
    return list_len != 0


def two_pass_merge_ok(nshards, cc, k):
    return not (cc == 0 or nshards * cc > 1024 or k > cc)


# ---- entries and their order ------------------------------------------------------------------------------------------------------------

def pack(score, row):
    return (np.asarray(score, F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(row, np.uint64)


def score_bits(e):
    return int(e) >> 32


def row_of(e):
    return int(e) & 0xFFFFFFFF


def score_of(e):
    return np.array([score_bits(e)], np.uint32).view(F32)[0]


def score_ord(bits):
    """The monotone integer image of f32::total_cmp with every NaN ranked as -inf."""
    if (bits & 0x7FFFFFFF) > 0x7F800000:
        bits = 0xFF800000
    return (~bits & 0xFFFFFFFF) if bits & 0x80000000 else bits | 0x80000000


def rank_key(e):
    """Sorting ascending by this key puts the best entry first: score descending under the order above, lower row first on ties."""
    return (-score_ord(score_bits(e)), row_of(e))


def best_first(entries):
    return sorted((int(e) for e in entries if int(e) != KEMPTY), key=rank_key)


def ranked_score(e):
    """The f32 score an entry ranks with: NaN reads as -inf."""
    s = score_of(e)
    return NEG_INF if s != s else s


def minus_2delta(a, delta):
    """a - 2 delta in f32 (the product 2 delta is exact, so fused or not the result rounds once); NaN becomes -inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = F32(np.float64(a) - 2.0 * np.float64(delta))
    return NEG_INF if t != t else t


# ---- select_kernel ----------------------------------------------------------------------------------------------------------------------

class SelectCase:
    """One launch's arguments (the fields of fsgpu_lab_select_args / SelectArgs); arrays are numpy, absent ones None."""

    def __init__(self, **kw):
        d = dict(nq=1, valid_queries=0, k=1, q_stride=0, l_stride=0, nlists=0, list_len=0, extra_len=0, spill_cap=0, reset_spill=1, take_topk=0,
                 heur_rank=0, big_pool=0, dim=0, nrows=0, row_base=0, row_stride=0, query_stride=0, hreduce=0, k_out=0, out_stride=0,
                 cand_out_stride=0, slab_f32=0, lists=None, list_counts=None, extra=None, spill=None, spill_count=None, delta=None,
                 anchor_unit=None, tau_floor_in=None, slab=None, queries=None, pool_flag=None, want_pool=False, want_counts=False,
                 want_tau=True, want_floor=False, want_cand_pairs=False)
        d.update(kw)
        self.__dict__.update(d)

    @property
    def finish(self):
        return self.slab is not None


def slots_of(c, q, nspill):
    """(slot index i, entry) of every slot query q's block reads, in the kernel's enumeration: the lists (list l, slot j: i = l list_len + j),
    then `extra`, then the first nspill spill slots.  A slot beyond its list's count is not read, whatever it holds."""
    out = []
    base = q * c.q_stride
    for l in range(c.nlists):
        n = c.list_len if c.list_counts is None else min(int(c.list_counts[q, l]), c.list_len)
        for j in range(n):
            out.append((l * c.list_len + j, int(c.lists[base + l * c.l_stride + j])))
    lists32 = c.nlists * c.list_len
    for x in range(c.extra_len):
        out.append((lists32 + x, int(c.extra[q, x])))
    for x in range(nspill):
        out.append((lists32 + c.extra_len + x, int(c.spill[q, x])))
    return out


def quick_group(i):
    """The group of the 64 'diagonal' groups that slot i of a single pass feeds: thread i mod 1024 holds the slots i, i + 1024, ...; thread t
    feeds group ((t >> 4) + (t & 15)) mod 64."""
    t = i % 1024
    return ((t >> 4) + (t & 15)) & 63


def is_sorted_form(c, big):
    return c.k > SORT_ABOVE or (big and c.finish and not c.take_topk)


def rescore(c, q, entry):
    """The exact entry of a candidate, or KEMPTY when its row lies outside [row_base, row_base + nrows)."""
    from oracle import oracle
    row = (row_of(entry) - c.row_base) & 0xFFFFFFFF
    if row >= c.nrows:
        return KEMPTY
    qv = np.ascontiguousarray(c.queries[q, :c.dim], F32)
    if c.slab_f32:
        s = F32(oracle.dot_f32_bytes_f32(c.slab[row, :c.dim], qv, c.hreduce))
    else:
        s = oracle.gather_dot(np.ascontiguousarray(c.slab[row:row + 1, :c.dim]), qv, np.zeros(1, np.uint32), c.hreduce)[0]
    return int(pack(s, row_of(entry)))


def anchor_f64(s_k, unit, delta):
    v = float(s_k) * float(unit)
    return v - float(delta) - abs(v) * 1e-6 - 1.0


def anchor_tolerance(s_k, unit, delta):
    """Four f32 operations, each within half an ulp of a value no larger than |S unit| + |delta| + 1."""
    return 4.0 * 2.0 ** -24 * (abs(float(s_k) * float(unit)) + abs(float(delta)) + 1.0)


def select_launch(c, q, state, big):
    """What one launch does for query q.  state: dict of the arrays a launch may write (tau_out, tau_floor_out, overflow, pool_flag,
    cand_counts, spill_count, ...), updated in place; entries the contract leaves open are recorded under state['open'][q].
    Returns the per-query facts the tests assert their regimes on."""
    info = dict(skipped=False)
    if big and int(state["pool_flag"][q]) == 0:
        info["skipped"] = True
        return info                                   # second chance: nothing of this query is touched
    nspill = 0
    if c.spill is not None:
        nspill = min(int(state["spill_count"][q * SPILL_COUNT_STRIDE]), c.spill_cap)
    slots = slots_of(c, q, nspill)
    total_slots = c.nlists * c.list_len + c.extra_len + nspill
    live = [(i, e) for i, e in slots if e != KEMPTY]
    ranked = best_first(e for _, e in live)
    d = F32(c.delta[q])
    k = c.k
    srt = is_sorted_form(c, big)
    info.update(entries=len(ranked), total_slots=total_slots, sorted=srt)
    opened = state["open"].setdefault(q, set())
    if srt and len(ranked) > SORT_CAP:
        # more live entries than the sort holds: the query is handed to the exact path; which 8,192 it kept is not defined
        state["overflow"][q] = 1
        opened.update(("tau", "floor", "cands", "answers"))
        info["regime"] = "sort_overflow"
        if c.reset_spill:
            state["spill_count"][q * SPILL_COUNT_STRIDE] = 0
        info["true_bound"] = POS_INF if d < 0 else (minus_2delta(ranked_score(ranked[k - 1]), d) if len(ranked) >= k else None)
        return info
    # the proven threshold (and the gate)
    gate_only = (not c.finish) and c.heur_rank != 0 and c.heur_rank <= k and not c.want_pool and not c.want_counts
    quick = (not srt) and not c.take_topk and total_slots <= SORT_CAP and k <= 32 and ((c.heur_rank == 0) if c.finish else gate_only)
    gmax = {}
    if quick:
        for i, e in live:
            g = quick_group(i)
            if g not in gmax or rank_key(e) < rank_key(gmax[g]):
                gmax[g] = e
        quick = len(gmax) >= k
    info["quick"] = quick
    info["nonempty_groups"] = len(gmax)
    basis = best_first(gmax.values()) if quick else ranked      # what the ranks are taken among
    gate = None
    if d < 0:
        proven = POS_INF
        state["overflow"][q] = 1
    elif len(basis) >= k:
        proven = minus_2delta(ranked_score(basis[k - 1]), d)
    elif c.tau_floor_in is not None:
        proven = F32(c.tau_floor_in[q])
    else:
        proven = NEG_INF
    tau = proven
    # the gate: the score at heur_rank WITHOUT a margin, where that rank exists (the extraction form keeps k ranks only)
    rank_exists = c.heur_rank != 0 and c.heur_rank <= len(basis) and (srt or c.heur_rank <= k)
    if d >= 0 and rank_exists:
        th = score_of(basis[c.heur_rank - 1])
        if th == th and th > tau:
            tau = th
            gate = th
    info.update(proven=proven, gate=gate)
    info["true_bound"] = POS_INF if d < 0 else (minus_2delta(ranked_score(ranked[k - 1]), d) if len(ranked) >= k else None)
    state["tau_floor_out"][q] = proven
    state["tau_out"][q] = tau
    if c.reset_spill:
        state["spill_count"][q * SPILL_COUNT_STRIDE] = 0
    if not c.finish and not c.want_pool and not c.want_counts:
        return info
    # candidates
    if c.take_topk:
        cands = ranked[:k]
    else:
        cands = [e for e in ranked if score_of(e) >= proven]     # (a NaN score never is)
    ncand = len(cands)
    cap = SORT_CAP if (big and srt and not c.take_topk) else POOL
    info.update(ncand=ncand, cap=cap)
    state["cand_counts"][q] = ncand
    if not big and c.pool_flag is not None:
        state["pool_flag"][q] = 1 if ncand > cap else 0
    elif ncand > cap:
        state["overflow"][q] = 1
    state["cands"][q] = cands
    if ncand > cap:
        opened.update(("answers",))      # which `cap` of the candidates were re-scored is not defined
    else:
        opened.discard("answers")
    opened.discard("tau")
    if not c.finish:
        return info
    if c.take_topk and c.want_cand_pairs:
        state["cand_approx"][q] = cands + [KEMPTY] * (k - len(cands))
    if ncand > cap:
        return info
    exact = [rescore(c, q, e) for e in cands]
    if c.take_topk and c.want_cand_pairs:
        state["cand_exact"][q] = exact + [KEMPTY] * (k - len(exact))
    answers = best_first(exact)[:c.k_out]
    state["answers"][q] = answers
    info["real"] = len([e for e in exact if e != KEMPTY])
    if c.anchor_unit is not None:
        # the exact anchor replaces the gate: tau_out = max(proven, S unit - delta - |S unit| 1e-6 - 1), S = the k_out-th best exact score
        tau = proven
        info["anchor"] = None
        if d >= 0 and len(answers) >= c.k_out:
            s_k = score_of(answers[c.k_out - 1])
            te = anchor_f64(s_k, c.anchor_unit[q], d)
            info["anchor"] = (te, anchor_tolerance(s_k, c.anchor_unit[q], d))
            if te == te and te > float(tau):
                tau = te
        state["tau_out"][q] = tau
    return info


def select_reference(c):
    """The state after the launch(es) of one fsgpu_lab_select call: (state, infos).  big_pool 1 = the first launch, then the second
    chance; 2 = the second chance alone on the given flags."""
    st = dict(tau_out=[None] * c.nq, tau_floor_out=[None] * c.nq, overflow=[0] * c.nq, cand_counts=[None] * c.nq,
              pool_flag=[int(x) for x in c.pool_flag] if c.pool_flag is not None else None,
              spill_count=[int(x) for x in c.spill_count] if c.spill_count is not None else [0] * (c.nq * SPILL_COUNT_STRIDE),
              cands={}, answers={}, cand_approx={}, cand_exact={}, open={})
    infos = []
    launches = {0: (False,), 1: (False, True), 2: (True,)}[c.big_pool]
    for big in launches:
        infos = [select_launch(c, q, st, big) for q in range(c.nq)] if not infos else \
            [dict(first=a, **select_launch(c, q, st, big)) for q, a in enumerate(infos)]
    return st, infos


# ---- select_groups_kernel ---------------------------------------------------------------------------------------------------------------

def groups_wave(i):
    """The wave (of 8) that holds entry i: 512 threads, thread t holds entries t and t + 512."""
    return (i % 512) >> 6


def group_rows(g):
    """The 8 rows of a group entry whose row field is g."""
    return [g + x for x in range(4)] + [g + 16 + x for x in range(4)]


def groups_picks(entries, k, rank_only):
    """The group entries the kernel ranks among, best first: every wave's PERW best, and of their union the best M (anchored) or k (rank
    form).  They are the true best unless one wave holds more than PERW of them."""
    kcap = 64 if k <= 64 else 128
    perw = kcap // 4 if rank_only else 8
    m = min(k, kcap) if rank_only else (GROUPS_TAKEN if k <= GROUPS_TAKEN else GROUPS_TAKEN_MAX)
    winners = []
    for w in range(8):
        winners += best_first(int(e) for i, e in enumerate(entries) if groups_wave(i) == w)[:perw]
    return best_first(winners)[:m]


def select_groups_reference(k, entries, delta, rank_only, valid=True, unit=None, slab=None, query=None, dim=0, nrows=0, row_base=0, hreduce=0,
                            slab_f32=False, live=None, allow=None):
    """(tau, overflow, info) of one query.  live / allow: boolean arrays over the slab's rows or None."""
    from oracle import oracle
    picks = groups_picks(entries, k, rank_only)
    info = dict(picks=picks, complete=picks == best_first(entries)[:len(picks)], rows=0)
    d = F32(delta)
    if d < 0 or not valid:
        return POS_INF, 1, info
    tau = NEG_INF
    if len(picks) >= k:
        tau = minus_2delta(ranked_score(picks[k - 1]), d)
    if rank_only:
        return tau, 0, info
    exact = []
    for g in picks:
        for grow in group_rows(row_of(g)):
            row = (grow - row_base) & 0xFFFFFFFF
            if row >= nrows or (live is not None and not live[row]) or (allow is not None and not allow[row]):
                continue
            qv = np.ascontiguousarray(query[:dim], F32)
            if slab_f32:
                s = F32(oracle.dot_f32_bytes_f32(slab[row, :dim], qv, hreduce))
            else:
                s = oracle.gather_dot(np.ascontiguousarray(slab[row:row + 1, :dim]), qv, np.zeros(1, np.uint32), hreduce)[0]
            exact.append(int(pack(s, grow & 0xFFFFFFFF)))
    exact = best_first(exact)
    info["rows"] = len(exact)
    info["anchor"] = None
    if len(exact) >= k:
        s_k = score_of(exact[k - 1])
        te = anchor_f64(s_k, unit, d)
        info["anchor"] = (te, anchor_tolerance(s_k, unit, d))
        if te == te and te > float(tau):
            tau = te
    return tau, 0, info


# ---- list_cut_kernel, two_pass_merge_kernel ---------------------------------------------------------------------------------------------

def list_cut_reference(lists):
    """lists [nlists, list_len]: the largest score at the last slot of the full lists (NaN reads as -inf), -inf when no list is full."""
    last = best_first(lists[:, -1]) if lists.shape[0] else []
    return ranked_score(last[0]) if last else NEG_INF


def two_pass_merge_reference(approx, exact, cc, k):
    """approx / exact [nshards, cc] of one query: the cc best pairs by the pass-1 order, of those with an exact entry the k best by the exact
    order."""
    pairs = [(int(a), int(e)) for a, e in zip(approx.ravel(), exact.ravel()) if int(a) != KEMPTY]
    pairs.sort(key=lambda p: rank_key(p[0]))
    return best_first(e for _, e in pairs[:cc])[:k]


# ---- the lab entry ----------------------------------------------------------------------------------------------------------------------

def _ptr(a):
    return a.ctypes.data if a is not None else None


class LabCall:
    """Fills a SelectLabArgs from keyword arguments; keeps every array alive until the call returns."""

    def __init__(self, **kw):
        from frankensearch_amd import _lib
        self.args = _lib.SelectLabArgs()
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
        return _lib.lib().fsgpu_lab_select_check(ctypes.addressof(self.args))

    def run(self, device=0):
        from frankensearch_amd import _lib
        return _lib.lib().fsgpu_lab_select(device, ctypes.addressof(self.args))


def run_select(c, device=0):
    """Runs a SelectCase through fsgpu_lab_select: (status, dict of output arrays)."""
    nq = c.nq
    kw = dict(kernel=SELECT, nq=nq, valid_queries=c.valid_queries, k=c.k, q_stride=c.q_stride, l_stride=c.l_stride, nlists=c.nlists,
              list_len=c.list_len, extra_len=c.extra_len, spill_cap=c.spill_cap, reset_spill=c.reset_spill, take_topk=c.take_topk,
              heur_rank=c.heur_rank, big_pool=c.big_pool, dim=c.dim, nrows=c.nrows, row_base=c.row_base, row_stride=c.row_stride,
              query_stride=c.query_stride, hreduce=c.hreduce, k_out=c.k_out, out_stride=c.out_stride, cand_out_stride=c.cand_out_stride,
              slab_f32=c.slab_f32)
    for name in ("lists", "list_counts", "extra", "spill", "delta", "anchor_unit", "tau_floor_in", "slab", "queries"):
        v = getattr(c, name)
        if v is not None:
            kw[name] = v
    out = dict(overflow=np.full(nq, UNWRITTEN32, np.uint32))
    out["spill_count"] = (c.spill_count if c.spill_count is not None else np.zeros(nq * SPILL_COUNT_STRIDE, np.uint32)).astype(np.uint32).copy()
    if c.pool_flag is not None:
        out["pool_flag"] = c.pool_flag.astype(np.uint32).copy()
    if c.want_tau:
        out["tau_out"] = np.zeros(nq, F32)
    if c.want_floor:
        out["tau_floor_out"] = np.zeros(nq, F32)
    if c.want_pool:
        out["pool_out"] = np.zeros(nq * POOL, np.uint64)
    if c.want_counts:
        out["cand_counts"] = np.zeros(nq, np.uint32)
    if c.finish:
        out["out_rows"] = np.zeros(nq * c.out_stride, np.uint32)
        out["out_scores"] = np.zeros(nq * c.out_stride, F32)
        out["out_packed"] = np.zeros(nq * c.out_stride, np.uint64)
        out["out_counts"] = np.zeros(nq, np.uint32)
        if c.want_cand_pairs:
            out["cand_approx_out"] = np.zeros(nq * c.cand_out_stride, np.uint64)
            out["cand_exact_out"] = np.zeros(nq * c.cand_out_stride, np.uint64)
    kw.update(out)
    call = LabCall(**kw)
    st = call.run(device)
    return st, {name: getattr(call, name) for name in out}
