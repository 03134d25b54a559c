"""Forced alignment on the CPU oracle (test code; the oracle itself is unchanged): score_util.oracle_score's
forced-token loop over RefModel.decode_step that also keeps, after every step, the attention the step left in
its state (st["attn"]: the last decoder layer's context attention, head 0), which is what the scoring call
returns with return_attn."""
import numpy as np
import torch


def oracle_score_attn(model, src, lengths, gold, gold_len):
    """src [B, T] f32, lengths [B], gold [B, L] int (tokens, EOS, then padding), gold_len [B].  Returns
    (scores [B], tok_logp [B, L], logp [B, L, V], attn [B, L, T]) as float32 numpy: the first three are
    score_util.oracle_score's, attn[b, i] is the attention row of target position i (rows i >= gold_len
    follow whatever padding token gold holds)."""
    cfg = model.cfg
    src_t = torch.as_tensor(np.asarray(src, np.float32))
    gold = np.asarray(gold, np.int64)
    gold_len = np.asarray(gold_len, np.int64)
    B, L = gold.shape
    with torch.no_grad():
        memory = model.encode(src_t, lengths)
        st = model.decoder_state(memory, src_t)
        tok = torch.full((B,), cfg.bos_idx, dtype=torch.long)
        lps, attns = [], []
        for step in range(L):
            lps.append(model.decode_step(st, tok, step).clone())
            attns.append(st["attn"].clone())
            tok = torch.as_tensor(np.clip(gold[:, step], 0, cfg.vocab - 1))
    logp = torch.stack(lps, 1).numpy().astype(np.float32)  # [B, L, V]
    attn = torch.stack(attns, 1).numpy().astype(np.float32)  # [B, L, T]
    tok_logp = np.take_along_axis(logp, np.clip(gold, 0, cfg.vocab - 1)[:, :, None], 2)[:, :, 0]
    tok_logp = np.where(np.arange(L)[None, :] < gold_len[:, None], tok_logp, 0.0).astype(np.float32)
    return tok_logp.sum(1, dtype=np.float64).astype(np.float32), tok_logp, logp, attn
