"""No GPU: fsgpu_lab_scan_stage is declared, exported and bound; it refuses what the launchers' predicates refuse before a device is
looked for; the instantiations tests/test_gpu_scan_stages.py enumerates are exactly those the library accepts; a requested LDS-query
shape the build does not contain is never planned; and tests/scan_stage_ref.py agrees with brute force on tiny cases."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import scan_stage_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = np.zeros(64, np.uint64)


def valid_kw(inst, **over):
    """Arguments fsgpu_lab_scan_stage_check accepts for an instantiation (the pointers are never followed by the check)."""
    kernel, dim, eb, variant, stage = inst
    sample = (kernel == S.LDS and stage < 2) or (kernel == S.REG and stage != 2)
    p = DUMMY.ctypes.data
    kw = dict(variant=variant, stage=stage, elem_bytes=eb, dim=dim, nrows=1000, grid=3, slots=8, spill_cap=16, group_stride=2,
              group_count=4 if sample or kernel == S.LDS else 0, nq_pad=S.group_queries(kernel, variant) if (kernel != S.LDS or variant in S.LDS_SHAPES) else 128,
              slab=p, queries=p, tau=p, cand=p, spill=p, spill_count=p, overflow=p, dense=p)
    kw.update(over)
    return kw


def test_lab_entry_is_declared_exported_and_bound():
    from frankensearch_amd import _lib
    from frankensearch_amd.build import build
    build()
    text = open(os.path.join(ROOT, "include", "fsgpu_lab.h")).read()
    assert re.search(r"fsgpu_status fsgpu_lab_scan_stage\(int32_t device, const fsgpu_lab_scan_stage_args \*args\);", text)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("fsgpu_lab_scan_stage", "fsgpu_lab_scan_stage_check", "fsgpu_lab_scan_planner_shape"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    body = re.search(r"typedef struct fsgpu_lab_scan_stage_args \{(.*?)\}", text, re.S).group(1)
    names = re.findall(r"[\s*,]\*?([a-z_0-9]+)[,;]", body)
    assert names == [n for n, _ in _lib.ScanStageArgs._fields_], names
    assert ctypes.sizeof(_lib.ScanStageArgs) == 22 * 4 + 14 * 8
    for name, value in (("LDS", S.LDS), ("REG", S.REG), ("PREPARE", S.PREPARE)):
        assert re.search(rf"#define FSGPU_LAB_SCAN_{name} {value}\n", text)
    # the kernels' constants this file's reference restates
    hpp = open(os.path.join(ROOT, "frankensearch_amd", "csrc", "kernels.hpp")).read()
    assert f"kMfmaSpillCountStride = {S.SPILL_COUNT_STRIDE};" in hpp and f"kWideSlots = {S.REG_MAX_SLOTS};" in hpp and f"kMfmaMaxSlots = {S.LDS_MAX_SLOTS};" in hpp
    # the earlier entries' structures are untouched
    assert ctypes.sizeof(_lib.BertStageArgs) == 11 * 4 + 2 * 4 + 4 + 18 * 8 and ctypes.sizeof(_lib.BertShortArgs) == 10 * 4 + 2 * 4 + 14 * 8


def test_enumeration_is_what_the_predicates_accept():
    """Every (kernel, dim, elem_bytes, variant, stage) over a grid that contains all the launchers know, with otherwise valid arguments:
    the accepted ones are exactly scan_stage_ref.instantiations()."""
    accepted = []
    for kernel, eb, dim, variant, stage in itertools.product((S.LDS, S.REG), (2, 1), (32, 64, 96, 128, 192, 256, 320, 384, 512, 768, 1024),
                                                             range(0, 8), range(0, 5)):
        inst = (kernel, dim, eb, variant, stage)
        nq_pad = (S.group_queries(kernel, variant) if kernel == S.REG else {0: 64, 5: 160}.get(variant, 128)) or 128
        if S.check_args(kernel, **valid_kw(inst, nq_pad=nq_pad)) == S.OK:
            accepted.append(inst)
    assert sorted(accepted) == sorted(S.instantiations()), set(accepted) ^ set(S.instantiations())
    assert len(set(S.instantiations())) == len(S.instantiations()) == 48 + 8 + 16 + 7 + 10
    # the planner's share: everything but int8 rows of 512 / 768 bytes (scan_wide_supported admits them; the sample stages cannot serve them)
    lab_only = set(S.instantiations()) - set(S.instantiations(lab_only=False))
    assert lab_only == {(S.REG, d, 1, qt, st) for d, top in ((512, 4), (768, 3)) for qt in range(2, top + 1) for st in (1, 2)}
    # group maxima: 384-byte int8 rows at 2..4 query tiles, 256-byte ones at 2..5; 128-row tiles only in the main pass of split-loop shapes
    assert [i[3] for i in S.instantiations() if i[4] == 3 and i[1] == 384] == [2, 3, 4]
    assert [i[3] for i in S.instantiations() if i[4] == 3 and i[1] == 256] == [2, 3, 4, 5]
    assert S.tile_rows(S.REG, 4, 2, 384, 1) == 128 and S.tile_rows(S.REG, 5, 2, 384, 1) == 64 and S.tile_rows(S.REG, 4, 1, 384, 1) == 64
    assert S.tile_rows(S.REG, 2, 2, 384, 2) == 32 and S.tile_rows(S.REG, 3, 2, 768, 1) == 32 and S.tile_rows(S.LDS, 2, 2, 384, 2) == 32


def test_arguments_are_refused_before_a_device_is_needed():
    reg = (S.REG, 384, 1, 4, 2)
    lds = (S.LDS, 384, 2, 2, 1)
    gmx = (S.REG, 256, 1, 5, 3)
    assert S.check_args(S.REG, **valid_kw(reg)) == S.OK and S.check_args(S.LDS, **valid_kw(lds)) == S.OK and S.check_args(S.REG, **valid_kw(gmx)) == S.OK
    refused = [
        (reg, dict(nrows=0)), (reg, dict(grid=0)), (reg, dict(slots=0)), (reg, dict(slots=S.REG_MAX_SLOTS + 1)), (reg, dict(nq_pad=511)),
        (reg, dict(nq_pad=1024)), (reg, dict(groups=2)), (reg, dict(group_count=3)), (reg, dict(elem_bytes=4)), (reg, dict(row_stride=385)),
        (reg, dict(row_stride=256)), (reg, dict(variant=6)), (reg, dict(variant=1)), (reg, dict(stage=0)), (reg, dict(groups=9, nq_pad=9 * 512)),
        (lds, dict(slots=S.LDS_MAX_SLOTS + 1)), (lds, dict(variant=1)), (lds, dict(variant=3)), (lds, dict(variant=4)), (lds, dict(variant=5, nq_pad=160)),
        (lds, dict(group_count=0)), (lds, dict(group_stride=0)), (lds, dict(group_count=9, group_stride=2)),   # (a group that begins past row 999)
        (lds, dict(want_counts=1)), (lds, dict(side_by_side=1)), (lds, dict(stage=3)), (lds, dict(dim=192)), (lds, dict(nq_pad=64)),
        (gmx, dict(elem_bytes=2)), (gmx, dict(dim=384)), (gmx, dict(group_count=0)), (gmx, dict(want_counts=1)),
        ((S.LDS, 384, 2, 2, 2), dict(group_stride=0)), ((3, 384, 2, 2, 2), {}),
    ]
    for inst, over in refused:
        assert S.check_args(inst[0], **valid_kw(inst, **over)) == S.INVALID_CONFIG, (inst, over)
    for inst, over in ((reg, dict(slab=0)), (reg, dict(queries=0)), (reg, dict(tau=0)), (reg, dict(cand=0)), (reg, dict(spill_count=0)),
                       (reg, dict(overflow=0)), (reg, dict(spill=0)), (reg, dict(want_counts=1, cand_count=0)), ((S.LDS, 64, 1, 0, 0), dict(dense=0))):
        assert S.check_args(inst[0], **valid_kw(inst, **over)) == S.NULL_ARGUMENT, (inst, over)
    assert S.check_args(S.REG, **valid_kw(gmx, tau=0, spill=0, spill_count=0, overflow=0)) == S.OK      # group maxima: no tau, no spill
    assert S.check_args(S.REG, **valid_kw(reg, spill_cap=0, spill=0)) == S.OK
    # the entry itself refuses the same way, whatever the device ordinal (it is not looked at yet), and a null struct
    from frankensearch_amd import _lib
    a = S._args(S.REG, **valid_kw(reg, slots=33))
    assert _lib.lib().fsgpu_lab_scan_stage(-7, ctypes.byref(a)) == S.INVALID_CONFIG and "kWideSlots" in _lib.last_error()
    assert _lib.lib().fsgpu_lab_scan_stage(0, None) == S.NULL_ARGUMENT and _lib.lib().fsgpu_lab_scan_stage_check(None) == S.NULL_ARGUMENT
    # valid arguments, an ordinal that is no device (the device count itself): the failure the lab file reports from behind the argument
    # check is the thread's last error (FSGPU_ERR_NO_DEVICE on a host without one), not an empty or stale string; no pointer is followed
    n_dev = _lib.lib().fsgpu_device_count()
    assert (_lib.lib().fsgpu_lab_scan_stage(n_dev, ctypes.byref(S._args(S.REG, **valid_kw(reg)))), _lib.last_error()) == \
        ((S.INVALID_CONFIG, "device ordinal out of range") if n_dev else (7, "no HIP device visible"))
    # the prepare form
    p = DUMMY.ctypes.data
    prep = dict(elem_bytes=2, dim=384, nq=3, nq_pad=64, queries_f32=p, prepared=p, delta=p)
    assert S.check_args(S.PREPARE, **prep) == S.OK and S.check_args(S.PREPARE, **dict(prep, elem_bytes=1, bits=4)) == S.OK
    for over in (dict(nq=65), dict(nq_pad=0), dict(dim=0), dict(elem_bytes=1, bits=5), dict(elem_bytes=3)):
        assert S.check_args(S.PREPARE, **dict(prep, **over)) == S.INVALID_CONFIG, over
    for over in (dict(queries_f32=0), dict(prepared=0), dict(delta=0)):
        assert S.check_args(S.PREPARE, **dict(prep, **over)) == S.NULL_ARGUMENT, over


def test_a_requested_shape_the_build_lacks_is_never_planned():
    """FSGPU_MFMA_SHAPE / FSGPU_MFMA_SHAPE_I8 name shapes 1, 3 (and 4) that only experiments builds contain: batched_prepare plans what
    scan_mfma_planner_shape returns, and that is always a shape the lab entry would launch."""
    from frankensearch_amd import _lib
    shape = _lib.lib().fsgpu_lab_scan_planner_shape
    experiments = S.check_args(S.LDS, **valid_kw((S.LDS, 384, 2, 1, 2), nq_pad=128)) == S.OK     # an FSGPU_EXPERIMENTS build has shape 1
    for eb in (2, 1):
        for requested in range(-3, 9):
            got = shape(requested, eb)
            assert S.check_args(S.LDS, **valid_kw((S.LDS, 384, eb, got, 2), nq_pad=128)) == S.OK, (requested, eb, got)
            if not experiments:
                assert got == 2, (requested, eb, got)
        assert shape(0, eb) == 2 and shape(2, eb) == 2
    src = open(os.path.join(ROOT, "frankensearch_amd", "csrc", "vector_index_batched.cpp")).read()
    assert "mf_shape_ = scan_mfma_planner_shape(knobs().mfma_shape, 2);" in src and "mf_shape_i8_ = scan_mfma_planner_shape(knobs().mfma_shape_i8, 1);" in src
    assert not re.search(r"mf_shape(_i8)?_ = knobs\(\)", src)


# ---- the reference against brute force ----------------------------------------------------------------------------------------------

def test_pack_bitmaps_and_rows_against_brute_force():
    rng = np.random.default_rng(1)
    s = np.array([1.5, -2.0, 0.0, np.inf], np.float32)
    e = S.pack(s, [7, 0, 2 ** 32 - 2, 5])
    assert [int(x) for x in e] == [(int(np.float32(v).view(np.uint32)) << 32) | r for v, r in zip(s, [7, 0, 2 ** 32 - 2, 5])]
    sc, rows = S.unpack(e)
    assert np.array_equal(sc.view(np.uint32), s.view(np.uint32)) and list(rows) == [7, 0, 2 ** 32 - 2, 5]
    for n in (1, 63, 64, 65, 200):
        bits = rng.random(n) < 0.5
        w = S.bitmap_words(bits)
        assert len(w) == (n + 63) // 64
        assert all(((int(w[i >> 6]) >> (i & 63)) & 1) == int(bits[i]) for i in range(n))
        assert np.array_equal(S.valid_rows(n, w, None), bits) and np.array_equal(S.valid_rows(n, w, w), bits) and S.valid_rows(n).all()
    # visited rows: the sample's groups; the LDS-query main pass takes the rest, the register-query one everything
    n, stride, count = 1000, 3, 5
    want = np.array([(r // 64) % stride == 0 and (r // 64) // stride < count for r in range(n)])
    assert np.array_equal(S.sample_rows(n, stride, count), want)
    assert np.array_equal(S.visited_rows(S.LDS, 1, n, stride, count), want) and np.array_equal(S.visited_rows(S.REG, 3, n, stride, count), want)
    assert np.array_equal(S.visited_rows(S.LDS, 2, n, stride, count), ~want) and S.visited_rows(S.REG, 2, n, stride, count).all()


def test_scores_and_expected_set_against_brute_force():
    rng = np.random.default_rng(2)
    slab = rng.integers(-127, 128, (37, 64), dtype=np.int8)
    q = rng.integers(-127, 128, (5, 64), dtype=np.int8)
    s = S.scores_int(slab, q)
    assert all(int(s[a, b]) == sum(int(x) * int(y) for x, y in zip(q[a], slab[b])) for a in range(5) for b in range(37))
    assert np.array_equal(S.scores_int(np.concatenate([slab, slab], axis=1)[:, :128], q), s)       # an MRL view: the first dim elements
    f = rng.standard_normal((9, 64)).astype(np.float16)
    f[3, 5] = np.nan
    qf = rng.standard_normal((2, 64)).astype(np.float16)
    sf, gamma = S.scores_f16(f.view(np.uint16), qf.view(np.uint16))
    for a in range(2):
        for b in range(9):
            want = sum(float(x) * float(y) for x, y in zip(qf[a], f[b]))
            assert (np.isnan(sf[a, b]) and b == 3) or abs(sf[a, b] - want) < 1e-12
            if b != 3:
                g = 64 * 2.0 ** -23 * np.sqrt(sum(float(x) ** 2 for x in qf[a])) * np.sqrt(sum(float(x) ** 2 for x in f[b]))
                assert abs(gamma[a, b] - g) < 1e-15
    mask = np.ones(9, bool)
    mask[0] = False
    tau = np.array([-1e9, np.nan], np.float32)
    got = S.expected_rows(sf, tau, mask)
    assert list(got[0]) == [1, 2, 4, 5, 6, 7, 8] and list(got[1]) == []           # the NaN row never passes; a NaN tau passes nothing
    assert list(S.expected_rows(s.astype(np.float64), np.full(5, np.inf, np.float32), np.ones(37, bool))[0]) == []
    t = float(s[0, 11])
    assert 11 in S.expected_rows(s.astype(np.float64), np.full(5, t, np.float32), np.ones(37, bool))[0]     # >= : the score itself passes


def test_tile_mapping_and_dense_layout_against_brute_force():
    # block b's n-th tile is n grid + ((b - n) mod grid): every tile has one block, a block's tiles are one per round
    for grid, ntiles in ((1, 5), (3, 10), (8, 79), (40, 7), (5, 5)):
        for reverse in (0, 1):
            rounds = (ntiles + grid - 1) // grid
            seen = {}
            for b in range(grid):
                for n in range(rounds):
                    t = n * grid + ((b - n) % grid)
                    t = rounds * grid - 1 - t if reverse else t
                    if t < ntiles:
                        seen[t] = b
            assert sorted(seen) == list(range(ntiles))
            assert all(S.tile_block(t, grid, ntiles, reverse) == seen[t] for t in range(ntiles))
    # rows -> blocks: 128-row tiles in the register-query main pass of a split-loop shape, sample tiles inside their 64-row group
    assert S.row_block(129, S.REG, 4, 2, 384, 1, 3, 1000, 1, 0, 0) == 1 and S.row_block(640, S.REG, 4, 2, 384, 1, 3, 1000, 1, 0, 0) == (2 + 1) % 3
    assert S.row_block(3 * 64 + 40, S.REG, 2, 1, 384, 2, 4, 1000, 3, 5, 0) == S.tile_block(1 * 2 + 1, 4, 10, 0)
    assert S.row_block(3 * 64 + 40, S.LDS, 2, 1, 384, 2, 4, 1000, 3, 5, 1) == S.tile_block(1 * 2 + 1, 4, 10, 1)
    # dense layout
    n, stride, count = 300, 2, 3
    valid = np.ones(n, bool)
    valid[130] = False
    sc = np.arange(2 * n, dtype=np.float32).reshape(2, n)
    e, rows, ok = S.dense_expected(sc, valid, n, stride, count, 1000)
    assert e.shape == (2, 192) and list(rows[:2]) == [0, 1] and rows[64] == 128 and rows[191] == 256 + 63
    assert e[1, 64] == S.pack(sc[1, 128], 1128) and e[0, 66] == S.KEMPTY and not ok[66] and np.all(e[:, rows >= n] == S.KEMPTY) and (rows >= n).sum() == 20


def test_group_maxima_against_brute_force():
    rng = np.random.default_rng(3)
    n, grid, stride, count = 64 * 7 + 40, 3, 2, 4        # the last group (rows 384..447) is whole; a fifth would be ragged
    s = rng.integers(-50, 50, (4, n)).astype(np.int64)
    valid = rng.random(n) < 0.6
    valid[128:160] = False                                # a pair without a valid row
    for reverse in (0, 1):
        best, have, classes = S.group_maxima_expected(s, valid, n, grid, stride, count, reverse)
        for b in range(grid):
            tiles = [t for t in range(count) if S.tile_block(t, grid, count, reverse) == b]
            for fk in range(4):
                rows = [g + h * 16 + fk * 4 + r for t in tiles for g in (t * stride * 64, t * stride * 64 + 32) for h in (0, 1) for r in range(4)]
                rows = [r for r in rows if valid[r]]
                assert sorted(classes[(b, fk)]) == sorted(g for t in tiles for g in (t * stride * 64, t * stride * 64 + 32))
                for q in range(4):
                    assert bool(have[q, b, fk]) == bool(rows) and (not rows or best[q, b, fk] == max(s[q, r] for r in rows))
    # a pair that reaches past the last row stands for nothing
    _, have, classes = S.group_maxima_expected(s[:, :100], np.ones(100, bool), 100, 1, 1, 2, 0)
    assert classes[(0, 0)] == [0, 32, 64]


@pytest.mark.parametrize("dim", [64, 128, 256, 384])
def test_gap_walk_finds_an_unambiguous_threshold(dim):
    """Unit-norm rows and queries, 2,500 and 5,003 rows, ranks 1, 40 and n / 20: a gap of 4 gamma_max lies within 64 ranks (a failure,
    not a skip, otherwise), and no row is then within gamma of tau."""
    rng = np.random.default_rng(dim)
    worst = 0
    for n in (2500, 5003):
        rows = rng.standard_normal((n, dim))
        rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float16)
        q = rng.standard_normal((6, dim))
        q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float16)
        s, gamma = S.scores_f16(rows.view(np.uint16), q.view(np.uint16))
        mask = np.ones(n, bool)
        for qi in range(6):
            for rank in (1, 40, n // 20):
                tau, steps = S.gap_tau(s[qi], mask, rank, gamma[qi].max())
                worst = max(worst, steps)
                assert steps <= 64 and not np.any(np.abs(s[qi] - np.float64(tau)) <= gamma[qi])
                assert (s[qi] >= np.float64(tau)).sum() == rank + steps
    assert worst <= 64
    with pytest.raises(AssertionError):
        S.gap_tau(np.linspace(0, 1e-6, 500), np.ones(500, bool), 10, 1e-3)


def test_query_preparation_reference():
    rng = np.random.default_rng(5)
    q = rng.standard_normal((3, 384)).astype(np.float32)
    d = S.prepare_delta_bound(q, 1.25)
    qn = np.sqrt((q.astype(np.float64) ** 2).sum(axis=1))
    assert np.allclose(d, (2.0 ** -11 * (1 + 2.0 ** -11) + 384 * 2.0 ** -23) * 1.25 * qn + np.sqrt(384) * 2.0 ** -25 * 1.25, rtol=1e-15)
    packed = np.array([0x7F, 0x98, 0x01], np.uint8)     # 4-bit two's complement, low nibble first
    assert list(S.levels_4bit(packed)) == [-1, 7, -8, -7, 1, 0]
