"""Writes tests/golden/reranker_golden.npz: logits of transformers.BertForSequenceClassification(num_labels=1) in f32 on the CPU,
built from a config only (nothing is downloaded) and loaded with oracle.bert_oracle.random_weights + tests/reranker_ref.head_weights.
The fixture holds the configs, seeds, pairs (ids, type ids, lengths) and logits; the weights are regenerated from the seeds.

    python tests/golden/make_reranker_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name: (vocab, hidden, layers, inter, weight seed, head seed, pair seed)
CONFIGS = {"tiny": (500, 128, 2, 512, 11, 12, 13), "minilm": (30522, 384, 6, 1536, 21, 22, 23)}


def pairs_for(name: str):
    import reranker_ref as R
    vocab = CONFIGS[name][0]
    rng = np.random.default_rng(CONFIGS[name][6])
    pairs = [R.make_pair(rng, vocab, 6, 20), R.make_pair(rng, vocab, 9, 1), R.make_pair(rng, vocab, 0, 0),   # [CLS][SEP][SEP]-like
             R.make_pair(rng, vocab, 12, 90), R.make_pair(rng, vocab, 3, 40)]
    cls_sep_sep = ([pairs[2][0][0], pairs[2][0][1], pairs[2][0][1]], [0, 0, 1])
    pairs[2] = cls_sep_sep
    pairs.append(R.make_pair(rng, vocab, 20, 512 - 23))   # 512 tokens
    return pairs


def weights_for(name: str):
    import reranker_ref as R
    from oracle import bert_oracle
    vocab, hidden, layers, inter, ws, hs, _ = CONFIGS[name]
    w = bert_oracle.random_weights(ws, vocab, hidden, layers, inter)
    w.update(R.head_weights(hs, hidden))
    return w


def hf_logits(name: str, pairs):
    import torch
    from transformers import BertConfig, BertForSequenceClassification
    vocab, hidden, layers, inter, _, _, _ = CONFIGS[name]
    cfg = BertConfig(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=hidden // 32,
                     intermediate_size=inter, max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12,
                     hidden_act="gelu", num_labels=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = BertForSequenceClassification(cfg).eval()
    from oracle.bert_oracle import normalise_keys
    w = normalise_keys(weights_for(name))
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all("position_ids" in m or "token_type_ids" in m for m in missing), missing
    out = []
    with torch.no_grad():
        for ids, types in pairs:
            logit = model(input_ids=torch.tensor([ids]), token_type_ids=torch.tensor([types]),
                          attention_mask=torch.ones(1, len(ids), dtype=torch.long)).logits
            out.append(float(logit[0, 0]))
    return np.asarray(out, dtype=np.float32)


def main():
    data = {}
    for name, cfg in CONFIGS.items():
        pairs = pairs_for(name)
        data[f"{name}_config"] = np.asarray(cfg, dtype=np.int64)
        data[f"{name}_lengths"] = np.asarray([len(p[0]) for p in pairs], dtype=np.int32)
        data[f"{name}_ids"] = np.concatenate([np.asarray(p[0], dtype=np.int32) for p in pairs])
        data[f"{name}_types"] = np.concatenate([np.asarray(p[1], dtype=np.int8) for p in pairs])
        data[f"{name}_logits"] = hf_logits(name, pairs)
        print(name, data[f"{name}_logits"])
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "reranker_golden.npz"), **data)


if __name__ == "__main__":
    main()
