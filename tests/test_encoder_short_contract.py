"""No GPU: fsgpu_lab_bert_short_stage is declared, exported and bound; the f64 references of tests/encoder_short_ref.py agree with the
f32 oracle (oracle.bert_oracle) to its precision at one and two layers; and the comparator is not blind — each fault of FAULTS, put in
place of the GPU output on the inputs of tests/test_gpu_encoder_short.py, reaches a ratio of at least 10 against bound x factor in the
check named next to it, or breaks the exact property named there."""
import ctypes
import os
import re

import numpy as np
import pytest

import encoder_stage_ref as R
import encoder_short_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLIND = 10.0


def test_lab_entry_is_declared_exported_and_bound():
    from frankensearch_amd import _lib
    from frankensearch_amd.build import build
    build()
    text = open(os.path.join(ROOT, "include", "fsgpu_lab.h")).read()
    assert re.search(r"fsgpu_status fsgpu_lab_bert_short_stage\(int32_t device, const fsgpu_lab_bert_short_args \*args\);", text)
    assert "fsgpu_lab_bert_short_stage" in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), "fsgpu_lab_bert_short_stage")
    # the binding's structure is the header's: ten u32, two floats, three pointers, eight inputs, the layer table, two outputs
    body = re.search(r"typedef struct fsgpu_lab_bert_short_args \{(.*?)\}", text, re.S).group(1)
    names = re.findall(r"[\s*,]\*?([a-z_0-9]+)(?:\[8\])?[,;]", body)
    assert names == [n.rstrip("_") for n, _ in _lib.BertShortArgs._fields_], names
    assert ctypes.sizeof(_lib.BertShortArgs) == 10 * 4 + 2 * 4 + 14 * 8
    for stage, value in (("Q_ATTN", S.Q_ATTN), ("Q_GEMM", S.Q_GEMM), ("Q_POOL", S.Q_POOL), ("DOCS", S.DOCS)):
        assert re.search(rf"#define FSGPU_LAB_BERT_{stage} {value}\n", text)
    # the earlier entry point's structure is untouched
    assert ctypes.sizeof(_lib.BertStageArgs) == 11 * 4 + 2 * 4 + 4 + 18 * 8
    # arguments are checked before a device is looked for: another model shape, too many tokens, a text of 33 tokens, seven layers
    a = np.zeros((1, S.H), np.float32)
    w = np.zeros((S.H, S.H), np.float32)
    assert S.run_short_stage(S.Q_GEMM, 0, [a, w], [(1, S.H)], [0, 1], hidden=256, expect=2) == 2
    assert S.run_short_stage(S.Q_GEMM, 0, [a, w], [(1, S.H)], [0, 1], inter=1024, expect=2) == 2
    assert S.run_short_stage(S.Q_GEMM, 0, [a, w], [(1, S.H)], [0, 1], heads=6, expect=2) == 2
    assert S.run_short_stage(S.Q_GEMM, 3, [a, w], [(1, S.H)], [0, 1], expect=2) == 2
    assert S.run_short_stage(S.Q_GEMM, 0, [np.zeros((33, S.H), np.float32), w], [(33, S.H)], [0, 33], expect=2) == 2
    wt = S.weights("random")
    assert S.run_docs(S.token_ids(34, 1), [0, 33, 34], wt, 1, expect=2) == 2
    assert S.run_short_stage(S.DOCS, 0, S.embedding_tensors(wt), [(2, S.H)], [0, 20, 40], ids=S.token_ids(40, 1),
                             layer_in=[S.layer_tensors(wt, 0)] * 7, vocab=S.VOCAB, max_pos=S.MAX_POS, expect=2) == 2
    assert S.run_short_stage(S.Q_GEMM, 0, [a], [(1, S.H)], [0, 1], expect=8) == 8     # a missing input: FSGPU_ERR_NULL_ARGUMENT


# ---- the references against the f32 oracle ----------------------------------------------------------------------------------------------

def texts_of(ids, offsets):
    return [ids[a:b].tolist() for a, b in zip(offsets[:-1], offsets[1:])]


@pytest.mark.parametrize("family", S.FAMILIES)
def test_forward_reference_agrees_with_the_f32_oracle(family):
    """One and two layers: the reference keeps f16 tiles where the kernel does, so it sits within a few 1e-4 of the f32 oracle on unit
    vectors (the oracle's own f32 arithmetic is good to ~1e-6), far inside the end-to-end tolerance."""
    from oracle import bert_oracle as O
    w = S.weights(family)
    emb = S.embedding_tensors(w)
    for lens in ([0, 5, 0, 27, 0], [32, 32, 1], [0, 0, 5, 0, 27, 6, 0, 0, 31, 2, 0]):
        offsets = S.offsets_of(lens)
        ids = S.token_ids(int(offsets[-1]), 11)
        for layers in (1, 2):
            pooled, bound, _ = S.docs_forward(ids, offsets, emb, [S.as_kernel_holds(S.layer_tensors(w, l)) for l in range(layers)])
            want = O.embed_forward(w, texts_of(ids, offsets), layers)
            assert np.max(np.abs(pooled - want)) < 4e-4, (family, lens, layers, np.max(np.abs(pooled - want)))
            assert np.all(pooled[np.array(lens) == 0] == 0) and np.all(bound[np.array(lens) == 0] == 0)


def test_stage_references_agree_with_the_f32_oracle():
    from oracle import bert_oracle as O
    f32 = np.float32
    w = S.weights("random")
    emb = S.embedding_tensors(w)
    t = S.layer_tensors(w, 0)
    offsets = S.offsets_of([0, 5, 0, 27, 0])
    ids, positions = S.token_ids(32, 3), S.positions_of(offsets)
    x, dx = S.embedding_ln(ids, positions, *emb)
    want_x = O.layer_norm((emb[0][ids] + emb[1][positions] + emb[2]).astype(f32), emb[3], emb[4])
    assert np.max(np.abs(x - want_x)) < 1e-5
    ctx, _ = S.q_attn(x, dx, R.h16(t[0]), t[1], offsets)
    qkv = (want_x @ t[0].T + t[1]).astype(f32)
    want = np.zeros_like(ctx)
    for a, b in zip(offsets[:-1], offsets[1:]):
        if b > a:
            want[a:b] = O.attention(qkv[a:b], S.H, S.ATTN_SCALE)
    # (f16 weights, Q, K and V of up to 5 — 2e-3 apiece — behind a softmax: 1e-2 at the worst element, a few 1e-4 at the typical one)
    assert np.max(np.abs(ctx - want)) < 1e-2 and np.median(np.abs(ctx - want)) < 5e-4
    # pending add + LayerNorm, FFN-up + GELU, FFN-down in four slabs, pooling
    x_in, parts, prev_bias = S.pending_inputs(17, 4, 5)
    x, dx = S.pending_ln(x_in, parts, prev_bias, t[10], t[11])
    want_x = O.layer_norm((x_in + parts.sum(axis=0) + prev_bias).astype(f32), t[10], t[11])
    assert np.max(np.abs(x - want_x) / (1 + np.abs(want_x))) < 1e-5
    g, _ = S.q_gemm_ln_gelu(x, dx, R.h16(t[6]), t[7])
    assert np.max(np.abs(g - O.gelu((want_x @ t[6].T + t[7]).astype(f32)))) < 5e-3
    a = S.activation_inputs(17, S.INTER, 7)
    slabs, _ = S.q_gemm_plain(a, R.h16(t[8]))
    assert slabs.shape == (4, 17, S.H) and np.max(np.abs(slabs.sum(axis=0) - a @ t[8].T)) < 2e-2   # (f16 weights against f32 ones)
    pooled, _ = S.pool_rows(x, dx, np.zeros_like(x), S.offsets_of([0, 5, 12, 0]))
    acc = want_x[:5].sum(axis=0, dtype=f32) / f32(5)
    assert np.max(np.abs(pooled[1] - acc / np.sqrt((acc * acc).sum()))) < 1e-5 and np.all(pooled[[0, 3]] == 0)
    # the fitted GELU of the one-launch kernel is within ERF_FIT of the 7.1.26 form on the error function, as its bound assumes
    xs = np.linspace(-9, 9, 20001)
    assert np.max(np.abs(S.docs_gelu_f64(xs) - R.gelu(xs)) / (0.5 * np.abs(xs) + 1e-30)) <= R.ERF_FIT


# ---- the comparator is not blind --------------------------------------------------------------------------------------------------------
# Each fault is applied where the kernels could have it, on the GPU tests' own inputs (both weight families; the worse of the two
# counts, a fault must be seen on each).  FAULTS: fault -> the check of tests/test_gpu_encoder_short.py that catches it.

def q_attn_faulty(x, dx, wqkv, bqkv, offsets, fault):
    """Q_ATTN's context with a faulty attention: 'neighbour_key' (a text's queries also see the first key of the text behind it),
    'last_key' (the last key of a text ignored)."""
    q, _, k, _, v, _ = S.qkv16(x, dx, np.zeros_like(x), wqkv, bqkv)
    out = np.zeros_like(q)
    for a, b in zip(offsets[:-1], offsets[1:]):
        a, b = int(a), int(b)
        if a == b:
            continue
        ka, kb = a, b
        if fault == "neighbour_key" and b < q.shape[0]:
            kb = b + 1
        if fault == "last_key" and b - a > 1:
            kb = b - 1
        for h in range(S.HEADS):
            c = slice(32 * h, 32 * h + 32)
            out[a:b, c] = R.attend(q[a:b, c], k[ka:kb, c], v[ka:kb, c], S.ATTN_SCALE)[0]
    return out


def worst_over_query_layouts(fn, min_tokens=2, multi=False):
    """min over the families of the max over the layouts of fn(family, lens) -> ratio."""
    worst = []
    for family in S.FAMILIES:
        ratios = [fn(family, lens) for lens in S.query_layouts() if sum(lens) >= min_tokens and (not multi or sum(1 for n in lens if n) > 1)]
        worst.append(max(ratios))
    return min(worst)


def attn_case(family, lens, form):
    w = S.weights(family)
    t = S.layer_tensors(w, 0)
    offsets = S.offsets_of(lens)
    m = int(offsets[-1])
    if form == 0:
        x, dx = S.embedding_ln(S.token_ids(m, 100 + m), S.positions_of(offsets), *S.embedding_tensors(w))
    else:
        x, dx = S.pending_ln(*S.pending_inputs(m, 4, 200 + m), t[10], t[11])
    return x, dx, R.h16(t[0]), t[1], offsets


def fault_neighbour_key():
    def ratio(family, lens):
        x, dx, wqkv, bqkv, offsets = attn_case(family, lens, 1)
        ref, bound = S.q_attn(x, dx, wqkv, bqkv, offsets)
        return S.compare(q_attn_faulty(x, dx, wqkv, bqkv, offsets, "neighbour_key"), ref, bound * S.SAFETY["q_attn"])
    return worst_over_query_layouts(ratio, multi=True)


def fault_last_key():
    def ratio(family, lens):
        x, dx, wqkv, bqkv, offsets = attn_case(family, lens, 1)
        ref, bound = S.q_attn(x, dx, wqkv, bqkv, offsets)
        return S.compare(q_attn_faulty(x, dx, wqkv, bqkv, offsets, "last_key"), ref, bound * S.SAFETY["q_attn"])
    return worst_over_query_layouts(ratio)


def fault_positions_run_on():
    """Positions not restarted at a text's start: the embedding prologue's x_out (f32 bound)."""
    def ratio(family, lens):
        w = S.weights(family)
        offsets = S.offsets_of(lens)
        m = int(offsets[-1])
        ids = S.token_ids(m, 100 + m)
        ref, bound = S.embedding_ln(ids, S.positions_of(offsets), *S.embedding_tensors(w))
        got, _ = S.embedding_ln(ids, np.arange(m), *S.embedding_tensors(w))
        return S.compare(got, ref, bound)
    return worst_over_query_layouts(ratio, multi=True)


def pending_fault(mutate, slabs=4):
    """A fault in the add + LayerNorm prologue: the x_out of Q_ATTN form 1 / Q_GEMM form 1 / the rows Q_POOL pools (f32 bound)."""
    def ratio(family, lens):
        t = S.layer_tensors(S.weights(family), 0)
        m = sum(lens)
        x_in, parts, prev_bias = S.pending_inputs(m, slabs, 200 + m)
        ref, bound = S.pending_ln(x_in, parts, prev_bias, t[10], t[11])
        got, _ = S.pending_ln(*mutate(x_in, parts, prev_bias, m), t[10], t[11])
        return S.compare(got, ref, bound)
    return worst_over_query_layouts(ratio, min_tokens=1)


def fault_rows_from_the_first_tile():
    """Rows 16..31 computed from rows 0..15: every output of more than 16 rows; here the GELU tile of Q_GEMM form 1 and the slabs."""
    worst = []
    for family in S.FAMILIES:
        t = S.layer_tensors(S.weights(family), 0)
        per_m = []
        for m in (17, 31, 32):
            x, dx = S.pending_ln(*S.pending_inputs(m, 1, 300 + m), t[4], t[5])
            ref, bound = S.q_gemm_ln_gelu(x, dx, R.h16(t[6]), t[7])
            got = ref.copy()
            got[16:] = ref[:m - 16]
            a = S.activation_inputs(m, S.INTER, 400 + m)
            slabs, sbound = S.q_gemm_plain(a, R.h16(t[8]))
            moved = slabs.copy()
            moved[:, 16:] = slabs[:, :m - 16]
            per_m.append(min(S.compare(got, ref, bound * S.SAFETY["q_gemm"]), S.compare(moved, slabs, sbound)))
        worst.append(min(per_m))
    return min(worst)


def fault_gelu_bias_shifted():
    worst = []
    for family in S.FAMILIES:
        t = S.layer_tensors(S.weights(family), 0)
        per_m = []
        for m in S.Q_TOKENS:
            x, dx = S.pending_ln(*S.pending_inputs(m, 1, 300 + m), t[4], t[5])
            ref, bound = S.q_gemm_ln_gelu(x, dx, R.h16(t[6]), t[7])
            got, _ = S.q_gemm_ln_gelu(x, dx, R.h16(t[6]), np.roll(t[7], 16))
            per_m.append(S.compare(got, ref, bound * S.SAFETY["q_gemm"]))
        worst.append(min(per_m))
    return min(worst)


def docs_case(family, lens, layers=1):
    w = S.weights(family)
    offsets = S.offsets_of(lens)
    ids = S.token_ids(int(offsets[-1]), 500 + len(lens))
    return ids, offsets, S.embedding_tensors(w), [S.as_kernel_holds(S.layer_tensors(w, l)) for l in range(layers)]


def block_starts(lens):
    """First text of each row block of the greedy packing (bert_docs_pack)."""
    starts, rows = [0], 0
    for i, n in enumerate(lens):
        if rows + n > 32:
            starts.append(i)
            rows = 0
        rows += n
    return starts + [len(lens)]


def fault_index_counts_empty_texts():
    """The in-block text index counting empty texts: in a block of more than 256 texts it no longer fits its 8 bits — the last text of
    [32, 2] + [0] * 255 + [30] gets index 256 = 0, the index of the 2-token text, and bit 8 lands in its positions: DOCS at one layer."""
    lens = S.DOCS_LAYOUTS[-1]
    assert block_starts(lens) == [0, 1, len(lens)] and len(lens) - 1 - 1 == 256
    worst = []
    for family in S.FAMILIES:
        ids, offsets, emb, layers = docs_case(family, lens)
        ref, bound, _ = S.docs_forward(ids, offsets, emb, layers)
        positions = S.positions_of(offsets)
        positions[34:] |= 1                                      # (256 >> 8) into the position field
        merged = np.array([0, 32, 64], np.uint32)                # the two texts of block 1 share a mask index
        x, det = S.embedding_ln(ids, positions, *emb)
        x, det, var, _ = S.docs_layer(x, det, np.zeros_like(x), layers[0], merged)
        got, _ = S.pool_rows(x, det, var, offsets)
        worst.append(S.compare(got, ref, bound * S.SAFETY["docs"]))
    return min(worst)


def fault_boundaries_of_the_text_before():
    """A text past in-block boundary 95 pooled with the boundaries of the text before it: DOCS on the layouts with such texts."""
    worst = []
    for family in S.FAMILIES:
        per_layout = []
        for lens in S.DOCS_LAYOUTS:
            starts = block_starts(lens)
            late = [i for b0, b1 in zip(starts[:-1], starts[1:]) for i in range(b0, b1) if i - b0 > 95 and (lens[i] or lens[i - 1])]
            if not late:
                continue
            ids, offsets, emb, layers = docs_case(family, lens)
            ref, bound, (x, _, _) = S.docs_forward(ids, offsets, emb, layers)
            got = ref.copy()
            for i in late:
                a, b = int(offsets[i - 1]), int(offsets[i])
                got[i] = 0 if a == b else x[a:b].mean(axis=0) / np.linalg.norm(x[a:b].mean(axis=0))
            per_layout.append(S.compare(got, ref, bound * S.SAFETY["docs"]))
        assert len(per_layout) >= 2
        worst.append(min(per_layout))
    return min(worst)


def fault_mean_over_n_plus_1():
    worst = []
    for family in S.FAMILIES:
        t = S.layer_tensors(S.weights(family), 0)
        per_layout = []
        for lens in S.query_layouts():
            m = sum(lens)
            x, dx = S.pending_ln(*S.pending_inputs(m, 4, 200 + m), t[10], t[11])
            offsets = S.offsets_of(lens)
            ref, bound = S.pool_rows(x, dx, np.zeros_like(x), offsets)
            got = ref.copy()
            for d, n in enumerate(lens):
                if n and offsets[d + 1] < m:   # the text takes the next row along
                    v = x[offsets[d]:offsets[d + 1] + 1].mean(axis=0)
                    got[d] = v / np.linalg.norm(v)
            if np.any(got != ref):
                per_layout.append(S.compare(got, ref, bound * S.SAFETY["q_pool"]))
        worst.append(min(per_layout))
    return min(worst)


FAULTS = {
    "a key of the neighbouring text attended at a boundary": ("Q_ATTN ctx against its bound (and neighbour independence)", fault_neighbour_key),
    "the last key of a text ignored": ("Q_ATTN ctx against its bound", fault_last_key),
    "positions not restarted at a text's start": ("Q_ATTN form 0 x_out against the f32 bound", fault_positions_run_on),
    "one FFN-down slab dropped": ("x_out of Q_ATTN form 1 against the f32 bound", lambda: pending_fault(lambda x, p, b, m: (x, p[:3], b))),
    "one FFN-down slab counted twice": ("x_out of Q_ATTN form 1 against the f32 bound",
                                        lambda: pending_fault(lambda x, p, b, m: (x, np.concatenate([p, p[3:]]), b))),
    "prev_bias omitted": ("x_out of Q_ATTN form 1 / Q_GEMM form 1 against the f32 bound", lambda: pending_fault(lambda x, p, b, m: (x, p, 0 * b))),
    "the residual taken from the other X buffer": ("x_out of Q_ATTN form 1 / Q_GEMM form 1 against the f32 bound",
                                                   lambda: pending_fault(lambda x, p, b, m: (S.pending_inputs(m, 4, 999)[0], p, b))),
    "rows 16..31 computed from rows 0..15": ("Q_GEMM form 1 GELU tile and form 2 slabs against their bounds", fault_rows_from_the_first_tile),
    "GELU bias 16 columns off": ("Q_GEMM form 1 GELU tile against its bound", fault_gelu_bias_shifted),
    "the in-block text index counting empty texts": ("DOCS, one layer, [32, 2] + [0] * 255 + [30] against its bound", fault_index_counts_empty_texts),
    "a text past boundary 95 pooled with the boundaries of the text before it": ("DOCS, one layer, the layouts of more than 95 texts", fault_boundaries_of_the_text_before),
    "a mean over n + 1": ("Q_POOL against its bound", fault_mean_over_n_plus_1),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_comparator_sees(fault):
    check, run = FAULTS[fault]
    ratio = run()
    print(f"{fault}: {ratio:.1f} x (bound x factor) in: {check}")
    assert ratio >= BLIND, (fault, check, ratio)


def test_slab_sum_property_sees_a_slab_of_the_wrong_k_slice():
    """Q_GEMM form 2's exact-sum property (the four slabs, summed in f64, are the unsplit product within the f32 dot-product bound)
    catches what a per-slab comparison against per-slab references would also catch, without trusting the split of the reference:
    slab 3 computed from K slice 2."""
    t = S.layer_tensors(S.weights("random"), 0)
    a = S.activation_inputs(17, S.INTER, 417)
    w = R.h16(t[8])
    slabs, _ = S.q_gemm_plain(a, w)
    whole, bound = R._dot(a, w, 0.0)
    assert S.compare(slabs.sum(axis=0), whole, bound) <= 1e-6
    slabs[3] = slabs[2]
    assert S.compare(slabs.sum(axis=0), whole, bound) >= BLIND


def test_store16_excludes_what_cannot_round_the_other_way():
    v = np.array([1.0 + 2.0 ** -12, 1.0 + 2.0 ** -11 - 1e-9, 0.3])
    h, var = S.store16(v, np.full(3, 1e-8), np.zeros(3))
    assert np.array_equal(h, R.r16(v)) and var[0] == 0 and var[1] > 0 and var[2] == 0
    _, var = S.store16(v, np.zeros(3), np.full(3, 1e-6))       # an error of a whole ulp's size: every element may disagree
    assert np.all(var >= 1e-6)
