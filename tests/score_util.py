"""Teacher-forced scoring on the CPU oracle (test code; the oracle itself is unchanged): the gold tokens
forced through RefModel.decode_step one step at a time, which is what the scoring call computes in one
pass (Translator._score_target, translate/translator.py:928-941)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_target.npz")
MODELS = ("transformer_pe", "nano")


def load_fixture():
    """{model name: dict(cfg kwargs, seed, eos_bias, src, lengths, gold, gold_len, score, tok_logp, logp)}
    from tests/golden/score_target.npz (tools/make_golden_score.py)."""
    import json
    z = np.load(GOLDEN)
    meta = json.loads(bytes(z["meta"]).decode())
    out = {}
    for name in MODELS:
        d = {k: z[f"{name}.{k}"] for k in ("src", "lengths", "gold", "gold_len", "score", "tok_logp", "logp")}
        d.update(meta["models"][name])
        out[name] = d
    return out


def fixture_model(entry):
    """(cfg, weights) of a fixture entry."""
    from nanodecoder_amd import synth
    cfg = synth.ModelConfig(**entry["cfg"])
    return cfg, synth.make_weights(cfg, seed=entry["seed"], eos_bias=entry["eos_bias"])


def oracle_score(model, src, lengths, gold, gold_len):
    """Forced-token loop over RefModel.decode_step.  src [B, T] f32, lengths [B], gold [B, L] int (tokens,
    EOS, then padding), gold_len [B].  Returns (scores [B], tok_logp [B, L] (0 at i >= gold_len),
    logp [B, L, V]) as float32 numpy; logp rows at i >= gold_len follow whatever padding token gold holds."""
    cfg = model.cfg
    src_t = torch.as_tensor(np.asarray(src, np.float32))
    gold = np.asarray(gold, np.int64)
    gold_len = np.asarray(gold_len, np.int64)
    B, L = gold.shape
    with torch.no_grad():
        memory = model.encode(src_t, lengths)
        st = model.decoder_state(memory, src_t)
        tok = torch.full((B,), cfg.bos_idx, dtype=torch.long)
        lps = []
        for step in range(L):
            lps.append(model.decode_step(st, tok, step).clone())
            tok = torch.as_tensor(np.clip(gold[:, step], 0, cfg.vocab - 1))
    logp = torch.stack(lps, 1).numpy().astype(np.float32)  # [B, L, V]
    tok_logp = np.take_along_axis(logp, np.clip(gold, 0, cfg.vocab - 1)[:, :, None], 2)[:, :, 0]
    tok_logp = np.where(np.arange(L)[None, :] < gold_len[:, None], tok_logp, 0.0).astype(np.float32)
    return tok_logp.sum(1, dtype=np.float64).astype(np.float32), tok_logp, logp
