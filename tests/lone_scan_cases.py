"""The case tables of the per-query scan and merge kernels: tests/test_lone_scan_contract.py (no GPU) and tests/test_gpu_lone_stages.py
iterate the same tables.  Every case names the regime it is there for; the contract test fails a case that is not in it.  Arrays are made
on demand from fixed seeds and never changed."""
import functools

import numpy as np

import lone_scan_ref as R

F32 = np.float32
NS = (1, 15, 16, 17, 63, 64, 65, 100, 5003)
KS = {64: (1, 10, 32, 33, 64), 256: (65, 128, 129, 256)}
NMAX = 5003
F16_KINDS = (R.F16, R.F16_HOST_QUERY, R.F16_MQ)


class ScanCase:
    def __init__(self, kind, nq, tier, dim, n, grid, k, data="random", regime="", live=None, allow=None, row_base=0, hreduce=0,
                 force_runtime_dim=0, plain_loads=0, row_stride=0):
        self.__dict__.update(kind=kind, nq=nq, tier=tier, dim=dim, n=n, grid=grid, k=k, data=data, regime=regime, live=live, allow=allow,
                             row_base=row_base, hreduce=hreduce, force_runtime_dim=force_runtime_dim, plain_loads=plain_loads,
                             row_stride=row_stride)

    @property
    def name(self):
        s = f"{R.KIND_NAMES[self.kind]}-q{self.nq}-t{self.tier}-d{self.dim}-n{self.n}-g{self.grid}-k{self.k}-{self.data}"
        for flag, tag in ((self.live, f"live_{self.live}"), (self.allow, f"allow_{self.allow}"), (self.row_base, f"base{self.row_base}"),
                          (self.hreduce, f"h{self.hreduce}"), (self.force_runtime_dim, "rt"), (self.plain_loads, "plain"),
                          (self.row_stride, f"stride{self.row_stride}"), (self.regime, self.regime.replace(" ", "_"))):
            if flag:
                s += "-" + tag
        return s


def tiles_of(kind, nq, n):
    tr = R.tile_rows(kind, nq)
    return (n + tr - 1) // tr


def grid_above(kind, nq, n):
    """A grid with more waves than tiles (and, from 4 tiles on, a block without any)."""
    return tiles_of(kind, nq, n) // 4 + 2


# ---- data --------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def base():
    """Random rows of every format and random queries, made once: f16 bits [NMAX, 768], f32 [NMAX, 1024], int8 [NMAX, 768], packed nibbles
    [NMAX, 384] (levels in -7..7), queries f32 [8, 1024], int8 / nibble queries."""
    rng = np.random.default_rng(2024)
    f16 = (rng.standard_normal((NMAX, 768)) / 8).astype(np.float16).view(np.uint16)
    f32 = (rng.standard_normal((NMAX, 1024)) / 8).astype(F32)
    i8 = rng.integers(-127, 128, (NMAX, 768)).astype(np.int8)
    lv = rng.integers(-7, 8, (NMAX, 768))
    q = rng.standard_normal((8, 1024)).astype(F32)
    qi8 = rng.integers(-127, 128, 768).astype(np.int8)
    qlv = rng.integers(-7, 8, 768)
    return f16, f32, i8, pack_nibbles(lv), q, qi8, pack_nibbles(qlv[None, :])[0]


def pack_nibbles(levels):
    """[n, dim] levels in -8..7 -> [n, dim / 2] bytes, low nibble = even dimension."""
    u = (np.asarray(levels, np.int64) & 0xF).astype(np.uint8)
    return (u[:, 0::2] | (u[:, 1::2] << 4)).astype(np.uint8)


def ordered_values(order, n, seed):
    """n integers whose order by row is the named one: asc, desc, equal, dup40 (every value 40 times, shuffled)."""
    rng = np.random.default_rng(seed)
    if order == "asc":
        return np.arange(n) - n // 2
    if order == "desc":
        return (np.arange(n) - n // 2)[::-1].copy()
    if order == "equal":
        return np.full(n, 3)
    if order == "dup40":
        return rng.permutation(np.arange(n) // 40 - n // 80)
    raise AssertionError(order)


def f16_of_int(v):
    """Distinct f16 values in the order of the integers v (|v| < 15000): the bit patterns of the normal numbers from 2^-14 up, signed."""
    mag = (np.abs(v) + 0x0400).astype(np.uint16)
    return np.where(v < 0, mag | np.uint16(0x8000), mag).astype(np.uint16)


def int_rows(values, dim, level, seed):
    """int rows [n, dim] and a query whose dots are `values`: the query is `level` in its first m dimensions, 1 in the next and 0 elsewhere
    (where the rows hold random levels); a row spreads value = level * A + b over them with |entries| <= level."""
    rng = np.random.default_rng(seed)
    n = len(values)
    m = 1 if level == 127 else 100
    rows = rng.integers(-level, level + 1, (n, dim))
    q = np.zeros(dim, np.int64)
    q[:m], q[m] = level, 1
    a_sum = np.rint(values / level).astype(np.int64)
    b = values - level * a_sum
    assert np.all(np.abs(b) <= level) and np.all(np.abs(a_sum) <= m * level)
    part = np.zeros((n, m), np.int64)
    left = a_sum.copy()
    for j in range(m):
        part[:, j] = np.clip(left, -level, level)
        left -= part[:, j]
    assert not left.any()
    rows[:, :m], rows[:, m] = part, b
    assert np.array_equal(rows @ q, values)
    return rows, q


def masks_of(c):
    """(live, allow) bool arrays or None.  'flips': random with the bits at rows 15|16 and 63|64 and at the last row set against their
    neighbours; 'none': nothing set."""
    out = []
    for which, pattern in ((0, c.live), (1, c.allow)):
        if pattern is None:
            out.append(None)
            continue
        if pattern == "none":
            out.append(np.zeros(c.n, bool))
            continue
        rng = np.random.default_rng(77 + which)
        m = rng.random(c.n) < 0.7
        for lo, hi in ((15, 16), (63, 64)):
            if hi < c.n:
                m[lo], m[hi] = bool(which), not which
        m[c.n - 1] = not which if c.n > 1 else True
        if c.n > 1:
            m[c.n - 2] = bool(which)
        out.append(m)
    return out


def arrays_of(c):
    """(slab as the kernel reads it [n, pitch], queries as the kernel reads them) of a case; cases that differ only in grid, k, bitmaps
    or row base share them."""
    return _arrays(c.kind, c.nq, c.dim, c.n, c.data, c.row_stride)


def scores_of(c):
    return _scores(c.kind, c.nq, c.dim, c.n, c.data, c.row_stride, c.hreduce)


@functools.lru_cache(maxsize=None)
def _scores(kind, nq, dim, n, data, row_stride, hreduce):
    slab, queries = _arrays(kind, nq, dim, n, data, row_stride)
    return R.scores_of(kind, dim, hreduce, slab, queries)


class _Shape:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@functools.lru_cache(maxsize=64)
def _arrays(kind, nq, dim, n, data, row_stride):
    c = _Shape(kind=kind, nq=nq, dim=dim, n=n, data=data, row_stride=row_stride)
    f16, f32, i8, i4, q, qi8, qi4 = base()
    seed = 1000 + n + dim
    if c.kind in F16_KINDS or c.kind == R.F32K:
        is16 = c.kind != R.F32K
        elems = (c.row_stride // (2 if is16 else 4)) if c.row_stride else dim
        if c.data == "random":
            slab = (f16 if is16 else f32)[:n, :elems].copy()
            return slab, q[:nq, :dim].copy()
        # one-hot queries: query x reads column x; even queries see the named order, odd ones its reverse
        slab = np.zeros((n, elems), np.uint16 if is16 else F32)
        queries = np.zeros((nq, dim), F32)
        for x in range(nq):
            queries[x, x] = 1.0
            if c.data == "special":
                rng = np.random.default_rng(seed + x)
                col = rng.standard_normal(n).astype(F32)
                pick = rng.random(n) < 0.25
                col[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5], F32), int(pick.sum()))
                slab[:, x] = col.astype(np.float16).view(np.uint16) if is16 else col
            else:
                v = ordered_values(c.data, n, seed)
                v = v if x % 2 == 0 else v[::-1]
                slab[:, x] = f16_of_int(v) if is16 else v.astype(F32) * F32(0.25)
        return slab, queries
    level = 127 if c.kind == R.I8 else 7
    if c.data == "random":
        return ((i8[:n, :dim].copy(), qi8[:dim].copy()) if c.kind == R.I8 else (i4[:n, :dim // 2].copy(), qi4[:dim // 2].copy()))
    if c.data == "extremes":
        rng = np.random.default_rng(seed)
        rows = rng.choice(np.array([-level, level]), (n, dim))
        qv = rng.choice(np.array([-level, level]), dim)
        rows[0], rows[n - 1] = qv, -qv          # the largest and the smallest dot a row can have
    else:
        rows, qv = int_rows(ordered_values(c.data, n, seed), dim, level, seed)
    if c.kind == R.I8:
        return rows.astype(np.int8), qv.astype(np.int8)
    return pack_nibbles(rows), pack_nibbles(qv[None, :])[0]


@functools.lru_cache(maxsize=None)
def expected_of(c):
    live, allow = masks_of(c)
    return R.expected_partial(c.kind, c.nq, c.n, c.grid, c.k, c.row_base, scores_of(c), live, allow)


def lab_call(c):
    slab, queries = arrays_of(c)
    live, allow = masks_of(c)
    return R.scan_call(c.kind, c.nq, c.tier, c.dim, c.n, c.k, c.grid, slab, queries, row_base=c.row_base, hreduce=c.hreduce,
                       row_stride=c.row_stride, force_runtime_dim=c.force_runtime_dim, plain_loads=c.plain_loads, live=live, allow=allow)


# ---- the scan tables ---------------------------------------------------------------------------------------------------------------------

def sweep(kind, nq, tier, dim, shift=0, orders=("asc", "desc", "equal", "dup40", "special"), **kw):
    """The full set of one configuration: every n (grids 1, 3 and one above the tile count in turn, every k of the tier in turn, both row
    bases), every k where a wave compacts, the empty blocks, every score order, the bitmaps."""
    ks = KS[tier]
    out = []
    for i, n in enumerate(NS):
        grid = (1, 3, grid_above(kind, nq, n))[(i + shift) % 3]
        out.append(ScanCase(kind, nq, tier, dim, n, grid, min(ks[(i + shift) % len(ks)], tier), row_base=1000 * (i % 2), **kw))
    out += k_sweep(kind, nq, tier, dim, **kw)
    out.append(empty_case(kind, nq, tier, dim, ks[1], **kw))
    fold = {64: (32, 33), 256: (128, 129)}[tier]
    for i, order in enumerate(orders):
        out.append(ScanCase(kind, nq, tier, dim, NMAX, 1, fold[i % 2], data=order, regime="compacts" if order in ("asc", "dup40") else "", **kw))
    out.append(ScanCase(kind, nq, tier, dim, 65, 3, ks[1], data="asc", row_base=1000, **kw))
    for live, allow in (("flips", None), (None, "flips"), ("flips", "flips"), (None, "none")):
        out.append(ScanCase(kind, nq, tier, dim, 100, 3, ks[1], live=live, allow=allow, **kw))
    out.append(ScanCase(kind, nq, tier, dim, 65, 1, ks[0], live="flips", allow="flips", row_base=1000, **kw))
    return out


def k_sweep(kind, nq, tier, dim, **kw):
    """Random rows, one block, every k of the tier: each wave meets more candidates than its 2 tier slots hold."""
    return [ScanCase(kind, nq, tier, dim, NMAX, 1, k, regime="compacts", **kw) for k in KS[tier]]


def empty_case(kind, nq, tier, dim, k, **kw):
    """n = 100 with more waves than tiles: 16-row tiles at grid 4 (16 waves, 7 tiles); the shorter tiles of a 2- or 4-query pass at grid 8."""
    return ScanCase(kind, nq, tier, dim, 100, 4 if R.tile_rows(kind, nq) == 16 else 8, k, regime="empty blocks", **kw)


def trio(kind, nq, tier, dim, i, data="random", **kw):
    """Three shapes of a configuration the sweeps do not take in full: compaction, empty blocks, an odd n on three blocks."""
    ks = KS[tier]
    return [ScanCase(kind, nq, tier, dim, NMAX, 1, ks[i % len(ks)], data=data, regime="compacts" if data == "random" else "", **kw),
            empty_case(kind, nq, tier, dim, ks[(i + 1) % len(ks)], **kw),
            ScanCase(kind, nq, tier, dim, (17, 65, 63)[i % 3], 3, ks[(i + 2) % len(ks)], data=data, row_base=1000, **kw)]


@functools.lru_cache(maxsize=None)
def scan_cases():
    out = []
    # F16: three full sweeps, the other (queries, tier) pairs where they compact, then every dimension and launcher flag
    out += sweep(R.F16, 1, 64, 384)
    out += sweep(R.F16, 2, 256, 128, shift=1)
    out += sweep(R.F16, 4, 64, 40, shift=2)
    for nq, tier, dim in ((1, 256, 256), (2, 64, 512), (4, 256, 72)):
        out += k_sweep(R.F16, nq, tier, dim)
    dims = [(d, {}) for d in (128, 256, 384, 512, 8, 24, 40, 72, 96, 768)] + [
        (384, dict(force_runtime_dim=1)), (384, dict(plain_loads=1)), (64, dict(row_stride=768))]
    for i, (dim, kw) in enumerate(dims):
        nq, tier = (1, 2, 4)[i % 3], (64, 256)[(i // 3) % 2]
        ks = KS[tier]
        out.append(ScanCase(R.F16, nq, tier, dim, NMAX, 3, ks[i % len(ks)], hreduce=i % 3, **kw))
        out.append(ScanCase(R.F16, nq, tier, dim, 65, grid_above(R.F16, nq, 65), ks[(i + 1) % len(ks)], hreduce=(i + 1) % 3, row_base=1000,
                            live="flips", **kw))
    for h in (1, 2):
        out.append(ScanCase(R.F16, 1, 64, 384, NMAX, 1, 33, hreduce=h, regime="compacts"))
    # the host-query form: one full sweep, the other tier, the runtime and the widest compile-time dimension
    out += sweep(R.F16_HOST_QUERY, 1, 64, 384, shift=1)
    out += k_sweep(R.F16_HOST_QUERY, 1, 256, 128)
    for i, dim in enumerate((8, 96, 512, 256)):
        out += trio(R.F16_HOST_QUERY, 1, (64, 256)[i % 2], dim, i, hreduce=i % 3)
    out.append(ScanCase(R.F16_HOST_QUERY, 1, 64, 64, NMAX, 3, 10, row_stride=768))
    # the multi-query kernel: every instantiation scan_mq_supported admits, one full sweep
    i = 0
    for nq in (4, 8):
        for tier in (64, 256):
            for dim in (128, 256, 384):
                assert R.scan_ok(R.F16_MQ, nq, tier, dim, 16, 1, 1)
                out += trio(R.F16_MQ, nq, tier, dim, i, hreduce=i % 3)
                i += 1
    out += sweep(R.F16_MQ, 4, 64, 256, shift=2)
    out += sweep(R.F16_MQ, 8, 256, 128, orders=("asc", "special"))
    # int8 and 4-bit: every dimension in both tiers, random rows and the extremes; one full sweep each
    for kind in (R.I8, R.I4):
        for i, dim in enumerate((128, 256, 384, 512, 768)):
            out += trio(kind, 1, (64, 256)[i % 2], dim, i)
            out += trio(kind, 1, (256, 64)[i % 2], dim, i + 1, data="extremes")
        out += sweep(kind, 1, 64, 128, orders=("asc", "desc", "equal", "dup40"))
        out += k_sweep(kind, 1, 256, 384)
    # F32: every dimension with 1, 2 and 4 queries, one full sweep, the other tier
    i = 0
    for dim in (8, 40, 104, 384, 1024):
        for nq in (1, 2, 4):
            n = NMAX if (i % 3) == (i // 3) % 3 else (65, 17)[i % 2]
            out.append(ScanCase(R.F32K, nq, (64, 256)[i % 2], dim, n, 1 if n == NMAX else 3, KS[(64, 256)[i % 2]][i % 4], hreduce=i % 3,
                                regime="compacts" if n == NMAX else ""))
            out.append(empty_case(R.F32K, nq, (256, 64)[i % 2], dim, KS[(256, 64)[i % 2]][(i + 1) % 4], row_base=1000))
            i += 1
    out += sweep(R.F32K, 2, 64, 104, shift=1)
    out += k_sweep(R.F32K, 4, 256, 40)
    out.append(ScanCase(R.F32K, 1, 64, 40, NMAX, 3, 10, row_stride=1024 * 4))
    unique = {}
    for c in out:          # (a sweep repeats a few shapes of the per-instantiation trios)
        unique.setdefault(c.name, c)
    return tuple(unique.values())


# ---- the merge table ---------------------------------------------------------------------------------------------------------------------

ALL_OUTPUTS = ("out_rows", "out_scores", "out_packed", "out_counts")


class MergeCase:
    """One merge launch.  regime: what merge_regime must say of the shape.  resorts (streaming shapes only): 0 = the loop never re-sorts,
    n > 0 = more than 4096 entries survive the pre-pass bound and the loop re-sorts at least n times, None = not claimed."""

    def __init__(self, name, nlists, list_len, k, regime, nq=1, lists_sorted=1, content="random", l_stride=0, q_pad=0, out_stride=0,
                 outputs=ALL_OUTPUTS, resorts=None):
        self.__dict__.update(name=name, nlists=nlists, list_len=list_len, k=k, regime=regime, nq=nq, lists_sorted=lists_sorted, content=content,
                             l_stride=l_stride or list_len, q_pad=q_pad, out_stride=out_stride or k, outputs=outputs, resorts=resorts)
        self.q_stride = nlists * self.l_stride + q_pad


def regime(mcap=8192, one_pass=True, use_heads=False, quick_heads=False, tail_bound=True):
    return dict(mcap=mcap, one_pass=one_pass, per_thread=mcap // R.NT if one_pass else R.U, use_heads=use_heads, quick_heads=quick_heads,
                tail_bound=tail_bound)


@functools.lru_cache(maxsize=None)
def merge_lists(c):
    """[nq, nlists, list_len] packed entries of a case (rows unique within a query, different contents per query)."""
    out = np.full((c.nq, c.nlists, c.list_len), np.uint64(R.KEMPTY))
    total = c.nlists * c.list_len
    for q in range(c.nq):
        rng = np.random.default_rng(500 + 31 * q + total + c.k)
        rows = rng.permutation(4 * total)[:total].astype(np.uint64).reshape(c.nlists, c.list_len) + np.uint64(1000)
        s = rng.standard_normal((c.nlists, c.list_len)).astype(F32)
        real = np.ones((c.nlists, c.list_len), bool)
        if c.content == "tails":
            real = np.arange(c.list_len)[None, :] < rng.integers(0, c.list_len + 1, c.nlists)[:, None]
        elif c.content == "empty":
            real[:] = False
        elif c.content == "few":
            real[:] = False
            real.ravel()[rng.permutation(total)[:max(c.k // 2, 1)]] = True
        elif c.content == "ties":
            s = rng.integers(-2, 3, (c.nlists, c.list_len)).astype(F32)
        elif c.content == "special":
            pick = rng.random((c.nlists, c.list_len)) < 0.5
            s[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 2.0, 2.0, -1.5, 1e-40, -1e-40], F32), int(pick.sum()))
        elif c.content == "adversarial":
            # k - 1 high entries and one very low one per list, the high ones rising with the list: the best k-th entry of any list is low,
            # and every round's entries beat whatever threshold the rounds before it left
            assert c.list_len == c.k
            s = (np.arange(c.nlists)[:, None] * F32(c.k) + rng.permutation(c.k - 1)[None, :].astype(F32) if c.k > 1 else s)
            s = np.concatenate([s.astype(F32), np.full((c.nlists, 1), F32(-1e30))], axis=1)
        elif c.content == "rising":
            s = (np.arange(total, dtype=F32).reshape(c.nlists, c.list_len) * F32(0.5))
        e = R.pack(s, rows)
        e[~real] = np.uint64(R.KEMPTY)
        if c.lists_sorted:
            order = np.argsort(R.sort_keys(e), axis=1, kind="stable")[:, ::-1]
            e = np.take_along_axis(e, order, axis=1)
        out[q] = e
    return out


def merge_buffer(c):
    """The lists as the launch reads them: [nq x q_stride], the slots between and behind the lists holding an entry that would win."""
    lists = merge_lists(c)
    buf = np.full((c.nq, c.q_stride), R.pack(F32(3e38), 7)[()], np.uint64)
    for l in range(c.nlists):
        buf[:, l * c.l_stride:l * c.l_stride + c.list_len] = lists[:, l]
    return buf.ravel()


def merge_lab_call(c):
    return R.merge_call(merge_buffer(c), c.nq, c.nlists, c.list_len, c.k, l_stride=c.l_stride, q_stride=c.q_stride, out_stride=c.out_stride,
                        lists_sorted=c.lists_sorted, outputs=c.outputs)


@functools.lru_cache(maxsize=None)
def merge_cases():
    M = MergeCase
    out = [
        # one-pass forms
        M("1x10", 1, 10, 10, regime()),
        M("1x256", 1, 256, 256, regime()),
        M("4x10", 4, 10, 10, regime()),
        M("64x10-ranked-heads", 64, 10, 10, regime(use_heads=True)),
        M("256x10-quick-heads", 256, 10, 10, regime(use_heads=True, quick_heads=True)),
        M("1024x8-exactly-8192", 1024, 8, 8, regime(use_heads=True, quick_heads=True)),
        M("1024x10-mcap-16384", 1024, 10, 10, regime(mcap=16384, use_heads=True, quick_heads=True)),
        M("1024x16-exactly-16384", 1024, 16, 16, regime(mcap=16384, use_heads=True, quick_heads=True)),
        # streaming forms
        M("1025x16-streaming", 1025, 16, 16, regime(one_pass=False, use_heads=True), resorts=0),
        M("2048x16-streaming-heads", 2048, 16, 16, regime(one_pass=False, use_heads=True), resorts=0),
        # (without the heads bound the best 16th entry of any list leaves half of random lists standing: one re-sort)
        M("2049x16-streaming-no-heads", 2049, 16, 16, regime(one_pass=False), resorts=1),
        M("2049x16-streaming-adversarial", 2049, 16, 16, regime(one_pass=False), content="adversarial", resorts=2),
        M("3x7000-streaming-unsorted-rising", 3, 7000, 256, regime(one_pass=False, tail_bound=False), lists_sorted=0, content="rising", resorts=2),
        # other shapes
        M("8x64-nlists-below-k", 8, 64, 64, regime()),
        M("256x32-k96-above-list-len", 256, 32, 96, regime(use_heads=True, tail_bound=False)),
        M("1x300-unsorted", 1, 300, 10, regime(tail_bound=False), lists_sorted=0),
        M("1x8192-unsorted-k256", 1, 8192, 256, regime(tail_bound=False), lists_sorted=0),
        # options
        M("4x10-l_stride", 4, 10, 10, regime(), l_stride=13),
        M("64x10-q_stride-nq8", 64, 10, 10, regime(use_heads=True), nq=8, q_pad=5, l_stride=11),
        M("256x10-out_stride", 256, 10, 10, regime(use_heads=True, quick_heads=True), nq=8, out_stride=17),
        M("1025x16-streaming-nq8", 1025, 16, 16, regime(one_pass=False, use_heads=True), nq=8, out_stride=20, resorts=0),
    ]
    out += [M(f"64x10-only-{name}", 64, 10, 10, regime(use_heads=True), outputs=(name,), out_stride=12) for name in ALL_OUTPUTS]
    # contents, on a one-pass shape of each heads form and on a streaming one
    for content in ("tails", "empty", "few", "ties", "special"):
        out.append(M(f"64x10-{content}", 64, 10, 10, regime(use_heads=True), content=content, nq=2))
        out.append(M(f"256x10-{content}", 256, 10, 10, regime(use_heads=True, quick_heads=True), content=content, nq=2))
        out.append(M(f"1x300-unsorted-{content}", 1, 300, 10, regime(tail_bound=False), lists_sorted=0, content=content))
        out.append(M(f"1025x16-streaming-{content}", 1025, 16, 16, regime(one_pass=False, use_heads=True), content=content,
                     resorts=None if content == "ties" else 0))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)
