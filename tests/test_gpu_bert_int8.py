"""GPU MiniLM-class encoder in the int8 dynamic-quant linear mode (FSGPU_BERT_LINEAR_INT8_DYNAMIC).
The kernel is held bit for bit to the numpy restatement of the contract (tests/int8_dynamic_ref.py) through the lab entry point;
the whole forward is held to cosine >= 0.995 and max-abs <= 6e-2 against the f32 oracle, and a text's vector to the same bits
whatever batch it is embedded in."""
import os
import threading

import numpy as np
import pytest

import int8_dynamic_ref as ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bert_golden.npz")
COS_MIN, ABS_MAX = 0.995, 6e-2
INT8 = "int8_dynamic"


@pytest.fixture(scope="module")
def fa():
    import frankensearch_amd as fa_mod
    from frankensearch_amd.build import build
    build()
    return fa_mod


def check(got, want):
    assert got.shape == want.shape
    err = float(np.max(np.abs(got - want)))
    nz = np.linalg.norm(want, axis=1) > 0
    cos = np.sum(got[nz] * want[nz], axis=1)
    print(f"int8 vs f32 oracle: min cosine {float(np.min(cos)) if cos.size else 1.0:.6f}, max-abs {err:.3e}")
    assert err <= ABS_MAX, err
    assert np.all(cos >= COS_MIN), float(np.min(cos))
    assert np.all(got[~nz] == 0)
    assert np.allclose(np.linalg.norm(got[nz], axis=1), 1.0, atol=1e-4)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def lab_linear(fa, x, w, b):
    from frankensearch_amd import _lib
    from frankensearch_amd.errors import check as ok
    x, w, b = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, w, b))
    y = np.empty((x.shape[0], w.shape[0]), np.float32)
    ok(_lib.lib().fsgpu_lab_linear_int8_dynamic(0, x.ctypes.data, w.ctypes.data, b.ctypes.data, x.shape[0], w.shape[0], x.shape[1],
                                                y.ctypes.data))
    return y


@pytest.mark.parametrize("n,k", [(1152, 384), (384, 384), (1536, 384), (384, 1536)])
def test_lab_linear_is_bit_identical_to_the_restatement(fa, n, k):
    rng = np.random.default_rng(n + k)
    w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
    w[3] = 0.0                                  # an all-zero output channel
    w[5] = 0.0
    w[5, k - 7] = -0.3                          # a one-hot channel
    w[:, [1, k // 2]] *= 1000.0                 # outlier input channels
    b = (rng.standard_normal(n) * 0.1).astype(np.float32)
    for m in (1, 5, 31, 32, 33, 257, 4096):
        x = rng.standard_normal((m, k)).astype(np.float32)
        if m > 1:
            x[1] = 0.0                          # a row of zeros
        if m > 2:
            x[2] = 0.0
            x[2, 11] = 3.0                      # a one-hot row
        x[:, [0, k - 1]] *= 1000.0              # outlier channels 1000 x the rest
        if m > 4:
            x[4] = np.round(x[4])               # integer rows: many exact .5 quotients
        got = lab_linear(fa, x, w, b)
        want = ref.linear_int8_dynamic(x, w, b)
        assert np.array_equal(bits(got), bits(want)), (m, int(np.sum(bits(got) != bits(want))))


@pytest.mark.parametrize("name", ["tiny", "minilm_shape"])
def test_golden_configs_within_tolerance_of_the_f32_oracle(fa, name):
    from oracle import bert_oracle
    g = np.load(GOLD)
    seed, vocab, hidden, layers, inter = (int(x) for x in g[f"{name}_config"])
    w = bert_oracle.random_weights(seed, vocab, hidden, layers, inter)
    m = fa.NativeEmbedder(w, linear=INT8)
    assert m.linear_format == INT8
    batch, o = [], 0
    for n in g["batch_lens"]:
        batch.append(g["batch_ids"][o:o + n].tolist())
        o += n
    check(m.embed_batch_token_ids(batch), bert_oracle.embed_forward(w, batch, layers))


def test_ragged_batches_with_empty_texts(fa):
    from oracle import bert_oracle
    rng = np.random.default_rng(7)
    w = bert_oracle.random_weights(21, 2000, 384, 6, 1536)
    m = fa.NativeEmbedder(w, linear=INT8)
    lens = [1, 2, 3, 8, 16, 17, 31, 32, 33, 63, 64, 65, 100, 128, 200, 0, 5, 0]
    batch = [[101] + rng.integers(1000, 2000, max(n - 2, 0)).tolist() + ([102] if n > 1 else []) if n else [] for n in lens]
    batch = [b[:n] for b, n in zip(batch, lens)]
    got = m.embed_batch_token_ids(batch)
    check(got, bert_oracle.embed_forward(w, batch, 6))
    assert np.all(got[15] == 0) and np.all(got[17] == 0)
    assert np.all(m.embed_batch_token_ids([[], []]) == 0)


def test_heavy_tailed_weights_and_512_token_documents(fa):
    from oracle import bert_oracle
    rng = np.random.default_rng(5)
    w = bert_oracle.heavy_tailed_weights(5, 3000, 384, 6, 1536)
    m = fa.NativeEmbedder(w, linear=INT8)
    batch = [[101] + rng.integers(1000, 3000, 510).tolist() + [102], [101, 2000, 102], [],
             [101] + rng.integers(1000, 3000, 300).tolist() + [102], [101] + rng.integers(1000, 3000, 20).tolist() + [102]]
    check(m.embed_batch_token_ids(batch), bert_oracle.embed_forward(w, batch, 6))


def test_int8_mode_is_not_the_f16_arithmetic(fa):
    from oracle import bert_oracle
    rng = np.random.default_rng(3)
    w = bert_oracle.random_weights(9, 1000, 384, 2, 1536)
    batch = [[101] + rng.integers(100, 1000, int(n)).tolist() + [102] for n in (5, 40, 200)]
    a = fa.NativeEmbedder(w).embed_batch_token_ids(batch)
    b = fa.NativeEmbedder(w, linear=INT8).embed_batch_token_ids(batch)
    assert fa.NativeEmbedder(w).linear_format == "f16"
    for i in range(len(batch)):
        assert not np.array_equal(bits(a[i]), bits(b[i])), i


def test_batch_invariance_bitwise(fa):
    """A text's vector has the same bits alone, in batches of 2, 31, 256 and 1,024 at shuffled positions, next to 512-token
    documents, and on a graph-replayed repeat of the same call."""
    from oracle import bert_oracle
    rng = np.random.default_rng(11)
    m = fa.NativeEmbedder(bert_oracle.random_weights(23, 30522, 384, 6, 1536), linear=INT8)
    pool = [[101] + rng.integers(1000, 30000, int(rng.integers(0, 31))).tolist() + [102] for _ in range(1024)]
    pool[17] = []
    probe = [int(i) for i in rng.choice(1024, 40, replace=False)] + [17]
    alone = {i: m.embed_token_ids(pool[i]) for i in probe}
    for i in probe[:3]:     # the same shape again: captured, then replayed from the graph
        for _ in range(2):
            assert np.array_equal(bits(m.embed_token_ids(pool[i])), bits(alone[i]))
    for size in (2, 31, 256, 1024):
        step = min(size, len(probe))
        for start in range(0, len(probe), step):
            members = probe[start:start + step]
            others = [i for i in rng.permutation(1024).tolist() if i not in members][:size - len(members)]
            order = rng.permutation(members + others).tolist()
            got = m.embed_batch_token_ids([pool[i] for i in order])
            for pos, i in enumerate(order):
                if i in alone:
                    assert np.array_equal(bits(got[pos]), bits(alone[i])), (size, i)
    docs = [[101] + rng.integers(1000, 30000, 510).tolist() + [102] for _ in range(3)]
    mixed = [docs[0], pool[probe[0]], docs[1], pool[probe[1]], pool[17], docs[2], pool[probe[2]]]
    got = m.embed_batch_token_ids(mixed)
    for pos, i in ((1, probe[0]), (3, probe[1]), (4, 17), (6, probe[2])):
        assert np.array_equal(bits(got[pos]), bits(alone[i]))
    doc_alone = m.embed_token_ids(docs[1])
    assert np.array_equal(bits(got[2]), bits(doc_alone))


def test_concurrent_callers_through_the_coalescer_get_their_lone_bits(fa):
    from oracle import bert_oracle
    rng = np.random.default_rng(13)
    m = fa.NativeEmbedder(bert_oracle.random_weights(24, 5000, 384, 2, 1536), linear=INT8)
    texts = [[101] + rng.integers(1000, 5000, int(rng.integers(1, 40))).tolist() + [102] for _ in range(96)]
    alone = [m.embed_token_ids(t) for t in texts]
    m.set_coalescing(32, 2000)
    got = [None] * len(texts)

    def worker(j):
        for i in range(j, len(texts), 16):
            got[i] = m.embed_token_ids(texts[i])

    threads = [threading.Thread(target=worker, args=(j,)) for j in range(16)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    m.set_coalescing(0, 0)
    for i in range(len(texts)):
        assert np.array_equal(bits(got[i]), bits(alone[i])), i


def test_safetensors_ex_equals_create_ex(fa):
    from oracle import bert_oracle
    from test_abi_symbols import _safetensors_blob
    rng = np.random.default_rng(19)
    w = bert_oracle.random_weights(4, 800, 384, 2, 1536, max_pos=512)
    a = fa.NativeEmbedder(w, linear=INT8)
    b = fa.NativeEmbedder.from_safetensors_bytes(_safetensors_blob(w), linear=INT8)
    assert b.linear_format == INT8 and b.dimension() == 384
    batch = [[101] + rng.integers(100, 800, int(n)).tolist() + [102] for n in (3, 30, 120, 0, 9)]
    assert np.array_equal(bits(a.embed_batch_token_ids(batch)), bits(b.embed_batch_token_ids(batch)))


def test_unsupported_widths_are_refused_at_create(fa):
    from oracle import bert_oracle
    for hidden, inter in ((96, 384), (384, 1000)):
        w = bert_oracle.random_weights(1, 100, hidden, 1, inter, max_pos=16)
        with pytest.raises(fa.InvalidConfig):
            fa.NativeEmbedder(w, linear=INT8)


@pytest.mark.parametrize("hidden,inter,layers", [(256, 1024, 2), (128, 384, 2), (384, 1280, 1)])
def test_other_widths(fa, hidden, inter, layers):
    from oracle import bert_oracle
    rng = np.random.default_rng(hidden + inter)
    w = bert_oracle.random_weights(31, 3000, hidden, layers, inter)
    m = fa.NativeEmbedder(w, linear=INT8)
    lens = [int(x) for x in rng.integers(3, 40, 40)] + [1, 129]
    batch = [[101] + rng.integers(1000, 3000, n - 1).tolist() for n in lens]
    got = m.embed_batch_token_ids(batch)
    check(got, bert_oracle.embed_forward(w, batch, layers))
    for i in (0, 7, 41):
        assert np.array_equal(bits(m.embed_token_ids(batch[i])), bits(got[i]))
