"""Golden fixture for teacher-forced scoring: the reference's own Translator._score_target
(translate/translator.py:928-941) on seeded synthetic models, written to tests/golden/score_target.npz
(data only, meta inside; index.json is untouched).  Needs the reference tree (oracle/_refimport.py); the
tests read only the fixture.

Two models (Transformer encoder with position encoding; NanoEncoder), each on the "ragged" chunk set of
oracle/make_golden.py (six chunks, T = 512 and tails 300 / 200 / 150 / 100 / 77, unsorted).  Target lengths
(EOS included) 1, 8, 32, 33, 65, 41: half random bases, half the CPU oracle's greedy tokens (likely paths);
none uses the -1e4-biased specials.

One shim: oracle/_refimport.py stubs inputters.make_features to return the batch tensor as it is; the real
one (inputters/inputter.py:192-217) adds the feature axis the decoder indexes (decoder/transformer.py:203),
so for side 'tgt' the stub is patched here to unsqueeze(2).

Regenerate with:  python tools/make_golden_score.py
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nanodecoder_amd import synth  # noqa: E402
from oracle import ref_cpu  # noqa: E402
from oracle._refimport import load_reference  # noqa: E402
from oracle.make_golden import build_reference_model, make_batch, make_translator, scenario_chunks  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "score_target.npz")
GOLD_LENS = (1, 8, 32, 33, 65, 41)  # EOS included
GREEDY_ROWS = (1, 3, 5)             # these take the oracle's greedy tokens, the others random bases
MODELS = {
    "transformer_pe": dict(cfg=dict(encoder_type="transformer", position_encoding=True), seed=21, eos_bias=-1.0),
    "nano": dict(cfg=dict(encoder_type="nano"), seed=22, eos_bias=-1.0),
}


def make_targets(cfg, W, chunks, seed):
    """gold [B, max(GOLD_LENS)] int32 (tokens, EOS, pad) and gold_len [B]."""
    B, L = len(chunks), max(GOLD_LENS)
    rng = np.random.default_rng(seed)
    bases = [i for i, w in enumerate(cfg.itos) if w not in ("<unk>", "<blank>", "<s>", "</s>")]
    src = np.zeros((B, max(len(c) for c in chunks)), np.float32)
    for i, c in enumerate(chunks):
        src[i, : len(c)] = c
    lens = np.array([len(c) for c in chunks], np.int32)
    # EOS barred for the whole run: every row yields max(GOLD_LENS) - 1 base tokens
    g = ref_cpu.greedy(ref_cpu.RefModel(cfg, W), src, lens, max_length=L - 1, min_length=L - 1)["tokens"]
    gold = np.full((B, L), cfg.pad_idx, np.int32)
    for i, n in enumerate(GOLD_LENS):
        toks = g[i, : n - 1] if i in GREEDY_ROWS else rng.choice(bases, n - 1)
        assert all(int(t) in bases for t in toks)
        gold[i, : n - 1] = toks
        gold[i, n - 1] = cfg.eos_idx
    return src, lens, gold, np.array(GOLD_LENS, np.int32)


def reference_scores(ns, cfg, W, chunks, gold, gold_len):
    """(score [B], logp [B, L, V]) from the reference's _run_encoder, decoder.init_state and _score_target,
    in the chunks' order."""
    model = build_reference_model(ns, cfg, W)
    tr = make_translator(ns, model, cfg, beam_size=1, max_length=100)
    mod = sys.modules[ns.Translator.__module__]
    stub = mod.inputters.make_features
    mod.inputters.make_features = lambda b, side, data_type="text": \
        getattr(b, side).unsqueeze(2) if side == "tgt" else stub(b, side, data_type)
    batch, order = make_batch(chunks)
    B, L = gold.shape
    tgt = np.full((L + 1, B), cfg.pad_idx, np.int64)  # BOS, tokens, EOS, pad
    tgt[0] = cfg.bos_idx
    for j, i in enumerate(order):
        tgt[1:, j] = gold[i]
    batch.tgt = torch.from_numpy(tgt)
    kept = []
    orig = tr._decode_and_generate

    def wrapped(*a, **k):
        lp, attn = orig(*a, **k)
        kept.append(lp.detach().clone())  # before _score_target zeroes the pad column
        return lp, attn

    tr._decode_and_generate = wrapped
    try:
        with torch.no_grad():
            src, enc_states, memory_bank, src_lengths = tr._run_encoder(batch, "nano")
            model.decoder.init_state(src, memory_bank, enc_states)
            sc = tr._score_target(batch, memory_bank, src_lengths, types.SimpleNamespace(data_type="nano"), None)
    finally:
        mod.inputters.make_features = stub
    inv = np.argsort(order)
    logp = kept[0].numpy().transpose(1, 0, 2)[inv].astype(np.float32)  # [L, B, V] -> [B, L, V]
    return sc.numpy().astype(np.float32)[inv], logp


def main():
    torch.manual_seed(0)
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    ns = load_reference()
    out, meta = {}, dict(models={}, gold_lens=list(GOLD_LENS), torch=torch.__version__, numpy=np.__version__)
    for name, spec in MODELS.items():
        cfg = synth.ModelConfig(**spec["cfg"])
        W = synth.make_weights(cfg, seed=spec["seed"], eos_bias=spec["eos_bias"])
        chunks = scenario_chunks("ragged", spec["seed"])
        src, lens, gold, gold_len = make_targets(cfg, W, chunks, spec["seed"])
        score, logp = reference_scores(ns, cfg, W, chunks, gold, gold_len)
        tok_logp = np.take_along_axis(logp, gold.astype(np.int64)[:, :, None], 2)[:, :, 0]
        tok_logp = np.where(np.arange(gold.shape[1])[None, :] < gold_len[:, None], tok_logp, 0.0).astype(np.float32)
        # the reference sums every position with the pad column zeroed: the same number
        assert np.allclose(tok_logp.sum(1), score, atol=1e-3, rtol=1e-5), (tok_logp.sum(1), score)
        for k, v in dict(src=src, lengths=lens, gold=gold, gold_len=gold_len, score=score, tok_logp=tok_logp,
                         logp=logp).items():
            out[f"{name}.{k}"] = v
        meta["models"][name] = spec
        print(name, "scores", score)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} B)")


if __name__ == "__main__":
    main()
