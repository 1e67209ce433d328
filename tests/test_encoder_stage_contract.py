"""No GPU: fsgpu_lab_bert_stage is declared, exported and bound; the f64 references of tests/encoder_stage_ref.py agree with the f32
oracle (oracle.bert_oracle) to its precision; and the comparator is not blind — on the inputs of tests/test_gpu_encoder_stages.py a
mutated reference standing in for the GPU output must reach a ratio of at least 10 against the derived bound times the safety factor
the GPU tests pass under."""
import os
import re

import numpy as np
import pytest

import encoder_stage_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLIND = 10.0


def test_lab_entry_is_declared_exported_and_bound():
    import ctypes
    from frankensearch_amd import _lib
    from frankensearch_amd.build import build
    build()
    text = open(os.path.join(ROOT, "include", "fsgpu_lab.h")).read()
    assert re.search(r"fsgpu_status fsgpu_lab_bert_stage\(int32_t device, const fsgpu_lab_bert_stage_args \*args\);", text)
    assert "fsgpu_lab_bert_stage" in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), "fsgpu_lab_bert_stage")
    # the binding's structure is the header's: eleven u32, two floats, four pointers, twelve inputs, two outputs
    body = re.search(r"typedef struct fsgpu_lab_bert_stage_args \{(.*?)\}", text, re.S).group(1)
    names = re.findall(r"[\s*,]\*?([a-z_0-9]+)(?:\[12\])?[,;]", body)
    assert names == [n.rstrip("_") for n, _ in _lib.BertStageArgs._fields_], names
    assert ctypes.sizeof(_lib.BertStageArgs) == 11 * 4 + 2 * 4 + 4 + 18 * 8
    # arguments are checked before a device is looked for
    assert R.run_stage(R.LINEAR, 1, [np.zeros((1, 512), np.float32)] * 3, [(1, 512)], m=1, n=512, k=512, expect=2) == 2
    assert R.run_stage(R.POOL, 0, [np.zeros((1, 100), np.float32)], [(1, 100)], offsets=[0, 1], m=1, hidden=100, n_docs=1, expect=2) == 2


# ---- the references against the f32 oracle ----------------------------------------------------------------------------------------------

def test_references_agree_with_the_f32_oracle():
    from oracle import bert_oracle as O
    rng = np.random.default_rng(5)
    f32 = np.float32
    # attention: one document of 37 tokens, 4 heads
    qkv = R.attention_inputs("trained", [37], 128, 3)
    ref, _ = R.attention(qkv, [0, 37], 128)
    assert np.max(np.abs(ref - O.attention(qkv, 128, R.ATTN_SCALE))) < 2e-5
    cls, _ = R.attention(qkv, [0, 20, 37], 128, cls=True)
    assert np.max(np.abs(cls[1] - O.attention(qkv[20:], 128, R.ATTN_SCALE)[0])) < 2e-5
    # linear and GELU
    a, w, b = R.linear_inputs(256, 128, 1)
    y, _ = R.linear(a[:9], w, b)
    assert np.max(np.abs(y - (a[:9] @ w.T + b).astype(f32))) < 1e-4
    x = np.linspace(-9, 9, 4001)
    assert np.max(np.abs(R.gelu(x) - O.gelu(x.astype(f32)))) < 2e-6
    g, _ = R.linear(a[:9], w, b, epilogue=1)
    assert np.max(np.abs(g - O.gelu((a[:9] @ w.T + b).astype(f32)))) < 1e-4
    # LayerNorm (with the residual), embedding + LayerNorm
    a, w, b, xr, gam, beta = R.linear_ln_inputs(128, 256, 2)
    rows = [0, 1, 2, 5, 6, 7]   # (the rows of standard deviation 1e-3 amplify the oracle's own f32 rounding of the sum: left out)
    out, _, _ = R.linear_ln(a[rows], w, b, xr[rows], gam, beta)
    want = O.layer_norm((xr[rows] + (a[rows] @ w.T + b).astype(f32)).astype(f32), gam, beta)
    assert np.max(np.abs(out - want) / (1 + np.abs(want))) < 2e-4
    ids, positions, types, word, pos, type_emb, gam, beta = R.embed_inputs(17, 128, 4)
    out, _, _ = R.embed_ln(ids, positions, types, word, pos, type_emb, gam, beta)
    assert np.max(np.abs(out - O.layer_norm(((word[ids] + pos[positions]) + type_emb[types]).astype(f32), gam, beta))) < 1e-5
    # the post-attention block against the oracle's composition (the f16 tiles of the reference cost ~ 1e-3 of an O(1) value)
    ins = R.post_attn_inputs(128, 512, 6)
    ctx, w0, b0, ln0w, ln0b, w1, b1, w2, b2, lnw, lnb, xr = [np.asarray(v[:8]) if i in (0, 11) else v for i, v in enumerate(ins)]
    out = R.post_attn(ctx, w0, b0, ln0w, ln0b, w1, b1, w2, b2, lnw, lnb, xr)[0]
    x1 = O.layer_norm(xr + (ctx @ w0.T + b0).astype(f32), ln0w, ln0b)
    want = O.layer_norm(x1 + (O.gelu((x1 @ w1.T + b1).astype(f32)) @ w2.T + b2).astype(f32), lnw, lnb)
    assert np.max(np.abs(out - want)) < 5e-3
    # pooling: the oracle's last step
    x, offsets = R.pool_inputs(128, 8)
    out, _ = R.pool(x, offsets)
    for d in range(len(offsets) - 1):
        rows = x[offsets[d]:offsets[d + 1]]
        want = np.zeros(128, f32)
        if len(rows):
            acc = rows.sum(axis=0, dtype=f32) * f32(1.0 / len(rows))
            nsq = f32((acc * acc).sum(dtype=f32))
            if nsq > f32(1.1920929e-7):
                want = acc * f32(1.0 / np.sqrt(nsq))
        assert np.max(np.abs(out[d] - want)) < 1e-5, d
    assert rng is not None


# ---- the comparator is not blind ----------------------------------------------------------------------------------------------------------

def mutated_attention(qkv, offsets, hidden, mutation, cls=False):
    """The reference with one fault of the kind attention kernels have."""
    qkv = np.asarray(qkv, np.float64)
    n_docs = len(offsets) - 1
    out = np.zeros((n_docs if cls else qkv.shape[0], hidden))
    scale = R.ATTN_SCALE * (0.9 if mutation == "scale" else 1.0)
    for d in range(n_docs):
        a, b = int(offsets[d]), int(offsets[d + 1])
        if a == b:
            continue
        for h in range(hidden // 32):
            c = slice(32 * h, 32 * h + 32)
            k, v = qkv[a:b, hidden:][:, c], qkv[a:b, 2 * hidden:][:, c]
            if b - a > 1 and (mutation == "last_key_ignored" or (mutation == "last_key_ignored_head0" and h == 0)):
                k, v = k[:-1], v[:-1]
            if mutation == "last_key_twice":
                k, v = np.concatenate([k, k[-1:]]), np.concatenate([v, v[-1:]])
            if mutation == "next_document" and b < qkv.shape[0]:
                k, v = np.concatenate([k, qkv[b:b + 1, hidden:][:, c]]), np.concatenate([v, qkv[b:b + 1, 2 * hidden:][:, c]])
            o, _ = R.attend(qkv[a:a + 1, c] if cls else qkv[a:b, c], k, v, scale)
            if mutation == "last_query_stale" and not cls and b - a > 1:
                o[-1] = o[-2]
            if mutation == "last_tile_stale" and not cls and b - a > 16:
                t = (b - a - 1) // 16 * 16    # the last 16-query tile gets the context of the tile before it
                o[t:] = o[t - 16:t - 16 + (b - a - t)]
            out[slice(d, d + 1) if cls else slice(a, b), c] = o
    return out


ATTENTION_MUTATIONS = ["last_key_ignored", "last_key_ignored_head0", "last_key_twice", "next_document", "last_query_stale", "last_tile_stale",
                       "scale"]


@pytest.mark.parametrize("mutation", ATTENTION_MUTATIONS)
@pytest.mark.parametrize("cls", [False, True])
def test_attention_comparator_sees(mutation, cls):
    if cls and mutation in ("last_query_stale", "last_tile_stale"):
        mutation = "scale"   # (the [CLS] form has one query row)
    worst = 0.0
    for hidden in (128, 384):
        calls = [[s] for s in (300, 449, 512)] + R.attention_ragged(hidden // 32, cls)[:1]
        for family in R.ATTN_FAMILIES:
            for i, lens in enumerate(calls):
                seed = 1000 + lens[0] if len(lens) == 1 else 2000
                qkv = R.attention_inputs(family, lens, hidden, seed, rot=i)
                offsets = R.offsets_of(lens)
                ref, bound = R.attention(qkv, offsets, hidden, cls=cls)
                got = mutated_attention(qkv, offsets, hidden, mutation, cls)
                worst = max(worst, R.compare(got, ref, bound * R.SAFETY["attention"]))
        if worst >= BLIND:
            break
    assert worst >= BLIND, (mutation, worst)


def test_attention_comparator_sees_every_fault_on_long_documents():
    """The faults that pass the end-to-end tolerance at 300, 449 and 512 tokens, each on each of those lengths, in one family at least."""
    for s in (300, 449, 512):
        for mutation in ("last_key_ignored", "last_key_ignored_head0", "last_query_stale", "last_tile_stale"):
            worst = 0.0
            for family in R.ATTN_FAMILIES:
                qkv = R.attention_inputs(family, [s], 128, 1000 + s)
                ref, bound = R.attention(qkv, [0, s], 128)
                worst = max(worst, R.compare(mutated_attention(qkv, [0, s], 128, mutation), ref, bound * R.SAFETY["attention"]))
            assert worst >= BLIND, (s, mutation, worst)


@pytest.mark.parametrize("epilogue,packed", [(0, False), (1, False), (0, True), (1, True), (2, True)])
def test_linear_comparator_sees(epilogue, packed):
    n, k = (768, 768) if not packed else (768, 256)
    a, w, b = R.linear_inputs(n, k, 31 * n + k)
    m = 129
    ref, bound = R.linear(a[:m], w, b, epilogue, packed)
    bound = bound * R.SAFETY["linear"]
    dropped, _ = R.linear(a[:m, :-32], w[:, :-32], b, epilogue, packed)
    assert R.compare(dropped, ref, bound) >= BLIND
    for tile in (16, 32, 64):
        tail = m % tile
        moved = ref.copy()
        moved[m - tail:] = ref[m - tail - tile:m - tile]
        assert R.compare(moved, ref, bound) >= BLIND, tile
    shifted, _ = R.linear(a[:m], w, np.roll(b, 16), epilogue, packed)
    assert R.compare(shifted, ref, bound) >= BLIND


@pytest.mark.parametrize("hidden,k", [(128, 128), (384, 384), (1024, 1024)])
def test_layer_norm_comparator_sees(hidden, k):
    a, w, b, x, g, beta = R.linear_ln_inputs(hidden, k, 17 * hidden + k)
    m = 33
    ref, bound, bound_h = R.linear_ln(a[:m], w, b, x[:m], g, beta)
    unbiased = beta + (ref - beta) * np.sqrt((hidden - 1) / hidden)   # variance divided by H - 1
    assert R.compare(unbiased, ref, bound * R.SAFETY["linear_ln"]) >= BLIND
    dropped, _, _ = R.linear_ln(a[:m, :-32], w[:, :-32], b, x[:m], g, beta)
    assert R.compare(dropped, ref, bound * R.SAFETY["linear_ln"]) >= BLIND
    moved = ref.copy()
    moved[32:] = ref[0:1]
    assert R.compare(moved, ref, bound_h * R.SAFETY["linear_ln"]) >= BLIND
    shifted, _, _ = R.linear_ln(a[:m], w, np.roll(b, 16), x[:m], g, beta)
    assert R.compare(shifted, ref, bound_h * R.SAFETY["linear_ln"]) >= BLIND


def test_post_attention_comparator_sees():
    """Each fault must reach the ratio at one of the block's shapes at least; the LayerNorm invariant at every shape."""
    worst = {}
    safety = R.SAFETY["post_attn"]
    for hidden, inter in [(128, 512), (256, 768), (384, 1536)]:
        ins = list(R.post_attn_inputs(hidden, inter, 13 * hidden + inter))
        m = 33
        ins[0], ins[11] = ins[0][:m], ins[11][:m]
        ref, bound, bound_h, (tol_mean, tol_m2, m2) = R.post_attn(*ins)

        def seen(name, got):
            worst[name] = max(worst.get(name, 0.0), R.compare(got, ref, bound_h * safety))

        for which in (2, 6, 8):   # a bias of each of the three projections shifted by 16 columns
            mut = list(ins)
            mut[which] = np.roll(ins[which], 16)
            seen(f"bias {which} shifted", R.post_attn(*mut)[0])
        for which in (1, 5, 7):   # the last 32 columns of K of each projection dropped
            mut = list(ins)
            mut[which] = ins[which].copy()
            mut[which][:, -32:] = 0
            seen(f"K of {which} dropped", R.post_attn(*mut)[0])
        moved = ref.copy()
        moved[32:] = ref[0:1]    # the 33rd row from one tile earlier
        seen("tail rows from a tile earlier", moved)
        # a variance divided by H - 1 stays inside the block's bound; the invariant of the LayerNorm sees it
        unbiased = ins[10] + (ref - ins[10]) * np.sqrt((hidden - 1) / hidden)
        mean, second = R.ln_moments(ref, ins[9], ins[10])
        assert np.all(np.abs(mean) <= tol_mean) and np.all(np.abs(second - m2) <= tol_m2)
        mean, second = R.ln_moments(unbiased, ins[9], ins[10])
        assert np.all(np.abs(second - m2) >= BLIND * tol_m2 * safety)
        mean, _ = R.ln_moments(ref + 1e-4 * ins[9], ins[9], ins[10])     # a mean that is 1e-4 sigma off
        assert np.all(np.abs(mean) >= BLIND * tol_mean * safety)
    print(worst)
    assert min(worst.values()) >= BLIND, worst


def test_embedding_comparator_sees():
    for hidden in (128, 1024):
        ids, positions, types, word, pos, type_emb, g, beta = R.embed_inputs(17, hidden, 7 * hidden + 17)
        ref, bound, bound_h = R.embed_ln(ids, positions, types, word, pos, type_emb, g, beta)
        safety = R.SAFETY["embed_ln"]
        assert R.compare(beta + (ref - beta) * np.sqrt((hidden - 1) / hidden), ref, bound * safety) >= BLIND
        other, _, _ = R.embed_ln(ids, positions, 1 - types, word, pos, type_emb, g, beta)     # the other token type's row
        assert R.compare(other, ref, bound_h * safety) >= BLIND
        moved = ref.copy()
        moved[16:] = ref[0:1]                                                                  # the 17th token from another tile
        assert R.compare(moved, ref, bound_h * safety) >= BLIND


def test_pooling_comparator_sees():
    for hidden in (128, 1024):
        x, offsets = R.pool_inputs(hidden, hidden)
        ref, bound = R.pool(x, offsets)
        wider = offsets.copy()
        wider[1:-1] += 1    # every document takes the next one's first token along: a mean over n + 1
        got, _ = R.pool(x, wider)
        got[[0, 6, 7]] = ref[[0, 6, 7]]
        per_doc = [R.compare(got[d], ref[d], bound[d] * R.SAFETY["pool"]) for d in (1, 2, 3, 4, 5)]
        assert min(per_doc) >= BLIND, per_doc


def test_compare_treats_exact_bounds_and_non_finite_values():
    ref, bound = np.array([1.0, 0.0]), np.array([0.5, 0.0])
    assert R.compare(np.array([1.25, 0.0]), ref, bound) == 0.5
    assert R.compare(np.array([1.0, 1e-30]), ref, bound) == np.inf
    assert R.compare(np.array([np.nan, 0.0]), ref, bound) == np.inf
    assert R.is_rne_f16_of(np.float32([0.333251953125]), np.float32([1 / 3])) and not R.is_rne_f16_of(np.float32([0.3335]), np.float32([1 / 3]))
