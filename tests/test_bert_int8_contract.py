"""CPU-side checks of the int8 dynamic-quant linear mode of the MiniLM-class encoder (FSGPU_BERT_LINEAR_INT8_DYNAMIC):
the C ABI declares and exports it, options are validated before a blob is parsed or a device looked for, the Python keyword
is checked, and the numpy restatement of the quantisation contract (tests/int8_dynamic_ref.py) gives hand-computed answers."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import int8_dynamic_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"fsgpu_bert_create_ex", "fsgpu_bert_create_safetensors_ex", "fsgpu_bert_linear_format"}


def _symbols(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(fsgpu_[a-z0-9_]+)\s*\(", text)), text


@pytest.fixture(scope="module")
def fa():
    import frankensearch_amd as fa_mod
    from frankensearch_amd.build import build
    build()
    return fa_mod


def test_headers_declare_the_int8_mode_and_the_library_exports_it(fa):
    from frankensearch_amd import _lib
    names, text = _symbols("fsgpu.h")
    assert NEW_ENTRIES <= names
    assert re.search(r"#define\s+FSGPU_BERT_LINEAR_F16\s+0\b", text)
    assert re.search(r"#define\s+FSGPU_BERT_LINEAR_INT8_DYNAMIC\s+1\b", text)
    assert re.search(r"typedef struct fsgpu_bert_options\s*\{\s*uint32_t linear_format;\s*uint32_t reserved\[7\];", text)
    lab, _ = _symbols("fsgpu_lab.h")
    assert "fsgpu_lab_linear_int8_dynamic" in lab
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES | {"fsgpu_lab_linear_int8_dynamic"}:
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert _lib.lib().fsgpu_bert_linear_format(None) == 0


def _options(fmt, reserved=None):
    from frankensearch_amd.embed import _BertOptions
    o = _BertOptions(fmt)
    for i, v in enumerate(reserved or []):
        o.reserved[i] = v
    return o


def test_create_safetensors_ex_validates_options_and_blob_without_a_device(fa):
    from frankensearch_amd import _lib
    from frankensearch_amd.errors import check
    from test_abi_symbols import _safetensors_blob, _tiny_bert_tensors   # (the tiny model-file images of the f16 test)

    lib = _lib.lib()
    good = np.frombuffer(_safetensors_blob(_tiny_bert_tensors(hidden=128, inter=256)), dtype=np.uint8).copy()
    bad = np.frombuffer(_safetensors_blob({"embeddings.position_ids": np.arange(4, dtype=np.int64)}), dtype=np.uint8).copy()

    def create(blob, opts, device=-1):
        h = C.c_void_p()
        st = lib.fsgpu_bert_create_safetensors_ex(device, blob.ctypes.data, blob.size, 0.0, C.byref(opts) if opts is not None else None,
                                                  C.byref(h))
        assert not h.value
        return st

    # a good blob in either format, or with no options: validated, then the device is asked for (none visible, or -1 out of range)
    for opts in (None, _options(0), _options(1)):
        with pytest.raises((fa.InvalidConfig, fa.NoDevice)):
            check(create(good, opts))
    # an unknown format or a non-zero reserved word: InvalidConfig before anything else, whatever the blob
    for opts in (_options(2), _options(0xFFFFFFFF), _options(1, [0, 0, 0, 0, 0, 0, 1]), _options(0, [5])):
        for blob in (good, bad):
            with pytest.raises(fa.InvalidConfig):
                check(create(blob, opts))
    # a malformed blob with valid options is the model-file error, as fsgpu_bert_create_safetensors reports it
    with pytest.raises(fa.ModelLoadFailed):
        check(create(bad, _options(1)))
    # the tensor-struct form rejects bad options the same way (before the config or a device is looked at)
    h = C.c_void_p()
    from frankensearch_amd.embed import _BertConfig, _BertWeights
    cfg, w = _BertConfig(), _BertWeights()
    with pytest.raises(fa.InvalidConfig):
        check(lib.fsgpu_bert_create_ex(0, C.byref(cfg), C.byref(w), C.byref(_options(7)), C.byref(h)))
    assert not h.value


def test_python_keyword_rejects_unknown_values(fa):
    from test_abi_symbols import _safetensors_blob, _tiny_bert_tensors
    from oracle import bert_oracle
    w = bert_oracle.random_weights(1, 50, 128, 1, 256, max_pos=16)
    blob = _safetensors_blob(_tiny_bert_tensors(hidden=128, inter=256))
    for bad in ("int8", "INT8_DYNAMIC", "bf16", "", None, 1):
        with pytest.raises(ValueError):
            fa.NativeEmbedder(w, linear=bad)
        with pytest.raises(ValueError):
            fa.NativeEmbedder.from_safetensors_bytes(blob, linear=bad)


def test_lab_linear_refuses_widths_that_are_not_multiples_of_64(fa):
    from frankensearch_amd import _lib
    from frankensearch_amd.errors import check
    x = np.zeros((2, 100), np.float32)
    w = np.zeros((96, 100), np.float32)
    b = np.zeros(96, np.float32)
    y = np.zeros((2, 96), np.float32)
    for (n, k) in ((96, 100), (64, 100), (96, 64), (0, 64)):
        with pytest.raises(fa.InvalidConfig):
            check(_lib.lib().fsgpu_lab_linear_int8_dynamic(0, x.ctypes.data, w.ctypes.data, b.ctypes.data, 2, n, k, y.ctypes.data))


# ---------------------------------------------------------------- the restatement, by hand
def test_rounding_is_half_away_from_zero_in_f64():
    v = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999997, -0.49999997, 126.5, 3.4999998], dtype=np.float32)
    assert ref.round_half_away(v).tolist() == [1, -1, 2, -2, 3, -3, 0, -0, 127, 3]
    # why f64: trunc(v + 0.5) in f32 rounds 0.49999997 up (0.49999997 + 0.5 rounds to 1.0 in f32)
    assert np.trunc(np.float32(0.49999997) + np.float32(0.5)) == 1.0


def test_known_answers_ties_zero_rows_and_clamping():
    q, s = ref.quantize_rows(ref.rust_quant_pin_matrix())
    # row 0: amax 127 -> inv = 1 exactly, every .5 is a tie and goes away from zero; 0.49999997 is not a tie
    assert q[0].tolist() == [127, 1, -1, 2, -2, 3, -3, 0] and s[0] == np.float32(1.0)
    # row 1: all zeros -> codes 0 and scale 0 (no division by zero)
    assert q[1].tolist() == [0] * 8 and s[1] == 0.0
    # row 2: amax 2.54 -> inv = f32(127 / 2.54) = 50; 0.01 * 50 = 0.5 (a tie after f32 rounding) -> 1, 1.27 * 50 = 63.5 -> 64
    assert np.float32(127.0) / np.float32(2.54) == np.float32(50.0)
    assert q[2].tolist() == [127, 1, -1, 2, -3, 64, -127, 0]
    assert s[2] == np.float32(2.54) / np.float32(127.0)
    # row 3: the amax element is -127 exactly, 500 * 0.127 = 63.5 -> 64; a code never leaves [-127, 127]
    assert q[3].tolist() == [-127, 1, -1, 2, 0, 0, 64, 32]
    big = np.array([[3.0e38, -3.0e38, 1.0, 1.7e38]], np.float32)
    qb, sb = ref.quantize_rows(big)
    assert qb.tolist() == [[127, -127, 0, 72]] and np.isfinite(sb[0])
    assert np.all(np.abs(ref.quantize_rows(np.random.default_rng(0).standard_normal((64, 384)).astype(np.float32))[0]) <= 127)


def test_known_answer_linear():
    # x row [2, -1, 0.5, 0 ...] (amax 2, inv 63.5): codes [127, -64 (-63.5 away from zero), 32 (31.75), 0]
    K = 64
    x = np.zeros((2, K), np.float32)
    x[0, :3] = [2.0, -1.0, 0.5]
    w = np.zeros((64, K), np.float32)
    w[0, :3] = [1.0, 1.0, 1.0]      # amax 1 -> codes 127, scale 1/127
    w[1, :3] = [0.0, -4.0, 0.0]     # codes [0, -127, 0], scale 4/127
    b = np.arange(64, dtype=np.float32)
    y = ref.linear_int8_dynamic(x, w, b)
    qx, sx = ref.quantize_rows(x)
    assert qx[0, :3].tolist() == [127, -64, 32] and sx[0] == np.float32(2.0) / np.float32(127.0)
    acc0 = 127 * 127 - 64 * 127 + 32 * 127
    acc1 = 64 * 127
    s0 = np.float32(sx[0] * (np.float32(1.0) / np.float32(127.0)))
    s1 = np.float32(sx[0] * (np.float32(4.0) / np.float32(127.0)))
    assert y[0, 0] == np.float32(np.float32(acc0) * s0) + np.float32(0.0)
    assert y[0, 1] == np.float32(np.float32(acc1) * s1) + np.float32(1.0)
    assert np.array_equal(y[1], b)      # a zero input row: the bias alone
    assert np.array_equal(y[0, 2:], b[2:])


def test_rust_int8_quant_golden_pins_the_rounding():
    """tests/golden/rust_int8_quant.json = {"codes": [...], "scale_bits": [...]} as printed by the Rust #[test] in INTEGRATION.md
    (quantize_per_output_channel_i8 of int8_dynamic_ref.rust_quant_pin_matrix()).  Absent here (frankentorch is not vendored):
    the rounding rule stays the contract of DESIGN §3.8 and the test is skipped."""
    path = os.path.join(os.path.dirname(__file__), "golden", "rust_int8_quant.json")
    if not os.path.exists(path):
        pytest.skip("tests/golden/rust_int8_quant.json not provided (see INTEGRATION.md)")
    got = json.load(open(path))
    q, s = ref.quantize_rows(ref.rust_quant_pin_matrix())
    assert [int(c) for c in got["codes"]] == q.reshape(-1).astype(int).tolist(), "the Rust codes differ from the contract"
    assert [int(b) for b in got["scale_bits"]] == s.view(np.uint32).astype(int).tolist(), "the Rust scales differ from the contract"


def test_whole_forward_restatement_stays_within_the_int8_tolerance():
    """embed_forward_int8 (the f32 oracle with only the linears replaced) against the f32 oracle on a small model: the arithmetic
    class alone, no GPU, inside the bounds tests/test_gpu_bert_int8.py holds the GPU to (cosine 0.995, max-abs 6e-2)."""
    from oracle import bert_oracle
    rng = np.random.default_rng(3)
    w = bert_oracle.random_weights(5, 500, 128, 2, 512)
    batch = [[101] + rng.integers(1, 500, int(n)).tolist() + [102] for n in (1, 10, 60)] + [[]]
    got = ref.embed_forward_int8(w, batch, 2)
    want = bert_oracle.embed_forward(w, batch, 2)
    assert np.max(np.abs(got - want)) <= 6e-2
    assert np.all(np.sum(got[:3] * want[:3], axis=1) >= 0.995) and np.all(got[3] == 0)
    assert not np.array_equal(got, want)
