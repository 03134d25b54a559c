"""Greedy layer-0 self-attention on the model's QKV table (needs an MI355X).

Key t < step of a greedy row r is a bit-for-bit copy of the k | v part of
table row t * V + tok_in(r, t), so the table-history form of
dec_self_attention_kernel (QkvRows.hist) reads the history from the table and
touches no cache.  The arithmetic after the loads is the cache form's, so
everything here is compared bitwise (torch.equal), except the oracle test
(the suite's 1e-3 log-prob / identical-token bar).

The op entry exposes the plain form (no fused head).  The head-fused form is
covered by the engine tests below: V = 8 models fuse the head, steps up to 23
run its <= 16 and <= 32 key instantiations bitwise against fresh engines and a
pool, and the oracle test runs all four of them, the second pass included (140
steps).
"""
import functools

import numpy as np
import pytest
import torch

from nanodecoder_amd import synth
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

LOGP_ATOL = 1e-3
TIE_MARGIN = 1e-4

# ----------------------------------------------------------------- op level
R, S = 5, 160
# the edges of every instantiation (<= 16 / 32 / 64 keys, else) and of the second pass (beyond 128 keys)
STEPS = [0, 1, 15, 16, 31, 32, 63, 64, 127, 128, 130]


@functools.lru_cache(maxsize=None)
def _op_case(V):
    """table [S * V, 768], hist [R, S] (the token each row picked at every step), tok0, and the cache the
    history selects: cache[r][t] = the k | v part of table row t * V + tok_in(r, t).  Built once per V."""
    g = torch.Generator().manual_seed(100 + V)
    table = torch.randn(S * V, 768, generator=g)
    hist = torch.randint(0, V, (R, S), generator=g, dtype=torch.int32)
    tok0 = 2
    tok_in = torch.cat([torch.full((R, 1), tok0, dtype=torch.int32), hist[:, :S - 1]], dim=1).long()  # [R, S]
    rows = torch.arange(S)[None, :] * V + tok_in
    cache = table[rows][:, :, 256:].contiguous()  # [R, S, 512]
    return table.cuda(), hist.cuda(), tok0, tok_in.cuda(), cache.cuda()


def _check_op(V, step):
    from nanodecoder_amd.engine import op_dec_self_attention, op_dec_self_attention_table
    table, hist, tok0, tok_in, cache = _op_case(V)
    tok = tok_in[:, step].to(torch.int32).contiguous()  # the row's token of this step (step 0: BOS)
    qkv = table[step * V + tok.long()].contiguous()
    ref_cache = cache.clone()
    ref_cache[:, step:] = 0.0  # the cache form appends the step's own key itself
    ref = op_dec_self_attention(qkv, ref_cache, step)
    sentinel = torch.full_like(cache, -7.25)
    out = op_dec_self_attention_table(table, V, tok, tok0, hist, step, cache=sentinel)
    torch.cuda.synchronize()
    assert torch.equal(out, ref), (V, step, (out - ref).abs().max().item())
    assert torch.equal(ref_cache[:, step], cache[:, step])  # (the reference appended what the table holds)
    assert bool((sentinel == -7.25).all()), "the table form wrote to the cache"


@pytest.mark.parametrize("step", STEPS)
def test_table_history_equals_cache_history(step):
    _check_op(7, step)


def test_table_history_vocab_9():
    """V = 9: more tokens than the head-fused form takes (the engine's plain form)."""
    _check_op(9, 40)


def test_table_history_rejects_what_it_does_not_cover():
    from nanodecoder_amd import _lib
    from nanodecoder_amd.engine import op_dec_self_attention_table
    table, hist, tok0, tok_in, cache = _op_case(7)
    tok = tok_in[:, 3].to(torch.int32).contiguous()
    with pytest.raises(_lib.NanodecError):  # a step the table has no rows for
        op_dec_self_attention_table(table, 7, tok, tok0, hist, S, max_steps=S + 1)
    with pytest.raises(_lib.NanodecError):  # a history shorter than the step needs
        op_dec_self_attention_table(table, 7, tok, tok0, hist[:, :8].contiguous(), 64)
    with pytest.raises(ValueError):
        op_dec_self_attention_table(table, 7, tok + 7, tok0, hist, 3)


# ----------------------------------------------------------------- engine level
B, T, MAX_STEPS = 3, 64, 32
KEYS = ("tokens", "scores", "logp")


@functools.lru_cache(maxsize=None)
def _model(pe=False):
    cfg = synth.ModelConfig(position_encoding=pe)
    return cfg, synth.make_weights(cfg, seed=11, eos_bias=-3.0)


def _batch():
    sig = synth.synth_chunk_batch(B, T, seed=41)
    return sig, np.full(B, T, np.int32)


def _engine(exact=False, max_steps=MAX_STEPS, pe=False):
    from nanodecoder_amd.engine import Engine
    cfg, W = _model(pe)
    e = Engine(cfg, W, device=0, max_batch=B, max_src_len=T, max_steps=max_steps)
    e.set_exact_fp32(exact)
    return e


def _call(e, max_len):
    sig, lens = _batch()
    r = e.translate_greedy(sig, lens, lens, max_len=max_len, min_len=4, return_logp=True)
    out = {k: r[k] for k in KEYS}
    if "event" in r:
        out["event"] = r["event"]
    return out


def _cpu(r):
    torch.cuda.synchronize()
    return {k: r[k].cpu() for k in KEYS}


@functools.lru_cache(maxsize=None)
def _fresh(max_len, exact=False):
    """The call's outputs from a new engine that runs nothing else."""
    e = _engine(exact)
    r = _cpu(_call(e, max_len))
    e.close()
    return r


def _same(a, b, what):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), (what, k)


def test_calls_of_different_lengths_on_one_context():
    """max_len 24, 10, 24 on one context: a shorter call reads a prefix of the model's table (row step * V +
    token does not depend on the call), and the token history's stride is the call's max_len."""
    e = _engine()
    got = [_cpu(_call(e, n)) for n in (24, 10, 24)]
    e.close()
    assert got[1]["tokens"].shape == (B, 10)
    _same(got[0], got[2], "call 1 vs call 3")
    for g, n in zip(got, (24, 10, 24)):
        _same(g, _fresh(n), f"max_len {n} vs a fresh engine")


def test_exact_fp32_switches_between_the_two_tables():
    """nd_set_exact_fp32 flips at run time between the table built in exact fp32 and the split-fp16 one."""
    e = _engine()
    got = []
    for exact in (True, False, True):
        e.set_exact_fp32(exact)
        got.append(_cpu(_call(e, 24)))
    e.close()
    _same(got[0], got[2], "exact, first vs second time")
    _same(got[0], _fresh(24, True), "exact vs a fresh engine")
    _same(got[1], _fresh(24, False), "split-fp16 vs a fresh engine")


def test_pool_lanes_read_the_owners_table():
    from nanodecoder_amd.engine import EnginePool
    cfg, W = _model()
    pool = EnginePool(cfg, W, device=0, lanes=2, max_batch=B, max_src_len=T, max_steps=MAX_STEPS)
    exp = _fresh(24)
    for rnd in range(2):
        got = [_call(pool, 24) for _ in range(4)]
        pool.synchronize()
        for k, g in enumerate(got):
            _same(_cpu(g), exp, (rnd, k))
    pool.close()


def test_greedy_vs_oracle_two_passes_position_encoding():
    """140 steps with position encoding on (the table's rows differ by step): the head-fused form's four
    instantiations and its second pass (beyond 128 keys) against the CPU oracle.  Exact tokens except after
    a genuine oracle near-tie (top-2 margin < 1e-4), log-probs within 1e-3."""
    from oracle import ref_cpu as ref
    n = 140
    cfg, W = _model(True)
    sig, lens = _batch()
    e = _engine(max_steps=n, pe=True)
    r = e.translate_greedy(sig, lens, lens, max_len=n, return_logp=True)
    got_tok, got_lp = r["tokens"].cpu().numpy(), r["logp"].cpu().numpy()
    e.close()
    o = ref.greedy(ref.RefModel(cfg, W), sig, lens, max_length=n)
    same = np.ones(B, bool)
    for b in range(B):
        for s in range(n):
            if got_tok[b, s] != o["tokens"][b, s]:
                top2 = np.sort(o["logp"][b, s])[-2:]
                assert top2[1] - top2[0] < TIE_MARGIN, (b, s, got_tok[b, s], o["tokens"][b, s], top2)
                same[b] = False
                break
    assert same.sum() >= B - 1
    assert gu.logp_close(got_lp[same], o["logp"][same], atol=LOGP_ATOL).all()
