"""Teacher-forced scoring on the GPU (needs an MI355X): the scoring pass's attention kernel against fp64,
nd_score_targets against the reference fixture (tests/golden/score_target.npz) and the CPU oracle's
forced-token loop, against the engine's own step-wise greedy decoder, its independence of the padding, the
pool, and the Translator surface."""
import ctypes
import types

import numpy as np
import pytest
import torch

from nanodecoder_amd import synth
from tests import golden_util as gu
from tests import score_util as su

pytestmark = pytest.mark.gpu

LOGP_ATOL = 1e-3
DEV = torch.device("cuda", 0)


def _engine(cfg, W, **kw):
    from nanodecoder_amd.engine import Engine
    return Engine(cfg, W, device=0, **kw)


# ----------------------------------------------------------------- attention op
def _attn_ref(q, k, v, allowed, filled):
    """fp64 attention of one chunk: q [Lq, 256], k / v [Lk, 256]; allowed [Lq, Lk] keys that exist for the
    row, filled [Lk] keys whose score is replaced by -1e18 (multi_headed_attn.py:167-177)."""
    Lq, Lk = q.shape[0], k.shape[0]
    qh = q.double().view(Lq, 8, 32).transpose(0, 1) / np.sqrt(32.0)
    kh = k.double().view(Lk, 8, 32).transpose(0, 1)
    vh = v.double().view(Lk, 8, 32).transpose(0, 1)
    s = qh @ kh.transpose(1, 2)
    s = s.masked_fill(filled[None, None, :], -1e18)
    s = s.masked_fill(~allowed[None, :, :], float("-inf"))
    return (torch.softmax(s, -1) @ vh).transpose(0, 1).reshape(Lq, 256)


@pytest.mark.parametrize("L", [1, 31, 32, 33, 64, 129])
def test_tf_attention_causal_vs_fp64(L):
    """Decoder self-attention over the target, operands in the [B * L, 768] q | k | v buffer: both sides of
    the 32-row query block, of the 128-key tile and of the diagonal tile.  B = 3; the kernel takes no
    target length (rows at or past a chunk's gold_len are rows like any other), so every row is held to
    the 2e-4 absolute bound of test_gemm_vs_fp64."""
    from nanodecoder_amd.engine import op_tf_attention
    B = 3
    g = torch.Generator().manual_seed(100 + L)
    qkv = torch.randn(B * L, 768, generator=g)
    out = op_tf_attention(qkv.to(DEV), qkv.to(DEV), B, L, L, 256, 512, True).cpu().double()
    tri = torch.tril(torch.ones(L, L, dtype=torch.bool))
    none = torch.zeros(L, dtype=torch.bool)
    err = 0.0
    for c in range(B):
        r = qkv[c * L:(c + 1) * L]
        ref = _attn_ref(r[:, :256], r[:, 256:512], r[:, 512:], tri, none)
        err = max(err, (out[c * L:(c + 1) * L] - ref).abs().max().item())
    print("causal L", L, "max abs err", err)
    assert err < 2e-4


@pytest.mark.parametrize("L,T,span", [(1, 77, 77), (33, 512, 300), (100, 512, 512), (129, 200, 150)])
def test_tf_attention_cross_vs_fp64(L, T, span):
    """Context attention: L query rows over the chunk's T memory keys of one layer of a three-layer K/V
    buffer, keys t < span[c], masked keys injected (signal == pad_val -> -1e18), and one chunk whose keys
    are all masked (a uniform row over its span).  B = 3 with ragged spans; 2e-4 absolute."""
    from nanodecoder_amd.engine import op_tf_attention
    B, pad_val = 3, 1.0
    g = torch.Generator().manual_seed(7 * L + T + span)
    q = torch.randn(B * L, 256, generator=g)
    kv = torch.randn(B * T, 1536, generator=g)
    sig = torch.randn(B, T, generator=g)
    sig[torch.rand(B, T, generator=g) < 0.1] = pad_val
    sig[2] = pad_val  # every key of chunk 2 masked
    spans = torch.tensor([span, max(1, span - 13), max(1, span // 2)], dtype=torch.int32)
    out = op_tf_attention(q.to(DEV), kv.to(DEV), B, L, T, 512, 768, False, signal=sig.to(DEV), span=spans.to(DEV),
                          pad_val=pad_val).cpu().double()
    assert torch.isfinite(out).all()
    err = 0.0
    for c in range(B):
        rows = kv[c * T:(c + 1) * T]
        allowed = (torch.arange(T) < int(spans[c]))[None, :].expand(L, T)
        ref = _attn_ref(q[c * L:(c + 1) * L], rows[:, 512:768], rows[:, 768:1024], allowed, sig[c] == pad_val)
        err = max(err, (out[c * L:(c + 1) * L] - ref).abs().max().item())
    uni = kv[2 * T: 2 * T + int(spans[2]), 768:1024].double().mean(0)
    assert (out[2 * L] - uni).abs().max().item() < 2e-4  # all keys masked: the mean of the span's values
    print("cross", (L, T, span), "max abs err", err)
    assert err < 2e-4


# ----------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def fixture():
    return su.load_fixture()


@pytest.fixture(scope="module")
def oracle(fixture):
    """The CPU oracle's forced-token scores of both fixture models, computed once."""
    from oracle import ref_cpu
    out = {}
    for name, z in fixture.items():
        cfg, W = su.fixture_model(z)
        out[name] = su.oracle_score(ref_cpu.RefModel(cfg, W), z["src"], z["lengths"], z["gold"], z["gold_len"])
    return out


def _score(eng, z, L=None, gold=None, **kw):
    """score_targets on a fixture batch: one reference batch, so every chunk's span is the batch's T."""
    gold = z["gold"] if gold is None else gold
    if L is not None and L > gold.shape[1]:
        gold = np.concatenate([gold, np.full((gold.shape[0], L - gold.shape[1]), 1, gold.dtype)], 1)
    B, T = z["src"].shape
    r = eng.score_targets(z["src"], z["lengths"], np.full(B, T, np.int32), gold=gold, gold_len=z["gold_len"], **kw)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", su.MODELS)
def test_score_targets_matches_reference_and_oracle(fixture, oracle, name, exact, graphs):
    z = fixture[name]
    cfg, W = su.fixture_model(z)
    eng = _engine(cfg, W, max_batch=8, max_steps=160, graphs=graphs)
    try:
        eng.set_exact_fp32(exact)
        r = _score(eng, z, return_tok_logp=True, return_logp=True)
        assert int(r["overflow"].item()) == 0
        sc, tl, lp = r["scores"].cpu().numpy(), r["tok_logp"].cpu().numpy(), r["logp"].cpu().numpy()
    finally:
        eng.close()
    L = z["gold"].shape[1]
    live = np.arange(L)[None, :] < z["gold_len"][:, None]
    o_sc, o_tl, o_lp = oracle[name]
    print(name, "exact" if exact else "split", "graphs" if graphs else "eager", "max |logp - ref| on live rows",
          np.abs(lp - z["logp"])[live][:, 4:].max(), "scores", sc, "ref", z["score"])
    assert gu.logp_close(lp, z["logp"], atol=LOGP_ATOL)[live].all()
    assert gu.logp_close(lp, o_lp, atol=LOGP_ATOL)[live].all()
    gathered = np.take_along_axis(lp, z["gold"].astype(np.int64)[:, :, None], 2)[:, :, 0]
    assert (tl[live] == gathered[live]).all()
    assert (tl[~live] == 0).all()
    assert gu.logp_close(sc, z["score"]).all()
    assert gu.logp_close(sc, o_sc).all()


@pytest.mark.parametrize("seed,eos_bias", [(31, 0.5), (32, -1.5)])
def test_score_targets_equals_the_stepwise_decoder(seed, eos_bias):
    """No oracle: 40 chunks of mixed lengths with masked samples decoded greedily for 40 steps; each
    chunk's own tokens up to and including its first EOS (or all 40), scored in one pass, must give the
    sum of the greedy call's own log-probabilities of those tokens, to 1e-3 + 1e-5 |x|.  The synthetic
    models decide on EOS almost independently of the signal, so the two cases are one model that ends
    its targets early (first EOS at step 1 or 3) and one that never emits EOS (all 40 positions)."""
    cfg = synth.ModelConfig()
    W = synth.make_weights(cfg, seed=seed, eos_bias=eos_bias)
    B, S = 40, 40
    sig = synth.synth_chunk_batch(B, 512, seed=5, inject_masks=True)
    lens = np.full(B, 512, np.int32)
    for i, n in enumerate((300, 77, 150, 411, 64, 1)):
        lens[3 * i + 1] = n
        sig[3 * i + 1, n:] = 0
    spans = np.full(B, 512, np.int32)
    eng = _engine(cfg, W, max_batch=B, max_steps=S)
    try:
        g = eng.translate_greedy(sig, lens, spans, max_len=S, return_logp=True)
        tok, lp = g["tokens"].cpu().numpy(), g["logp"].cpu().numpy()
        is_eos = tok == cfg.eos_idx
        gold_len = np.where(is_eos.any(1), is_eos.argmax(1) + 1, S).astype(np.int32)
        live = np.arange(S)[None, :] < gold_len[:, None]
        gold = np.where(live, tok, cfg.pad_idx).astype(np.int32)
        want_tl = np.where(live, np.take_along_axis(lp, tok.astype(np.int64)[:, :, None], 2)[:, :, 0], 0.0)
        r = eng.score_targets(sig, lens, spans, gold=gold, gold_len=gold_len, return_tok_logp=True)
        sc, tl = r["scores"].cpu().numpy(), r["tok_logp"].cpu().numpy()
    finally:
        eng.close()
    want = want_tl.sum(1)
    print("gold_len", gold_len, "max |score - stepwise|", np.abs(sc - want).max())
    assert (gold_len == S).all() if eos_bias < 0 else (gold_len < S).all()
    assert gu.logp_close(tl, want_tl).all()
    assert gu.logp_close(sc, want).all()


@pytest.mark.parametrize("exact", [False, True])
def test_score_is_independent_of_padding(fixture, exact):
    """The same batch scored with L = its longest target and with L = max_steps gives bit-identical
    scores, and garbage ids past gold_len (out-of-range ones included) change nothing."""
    z = fixture["transformer_pe"]
    cfg, W = su.fixture_model(z)
    eng = _engine(cfg, W, max_batch=8, max_steps=160)
    try:
        eng.set_exact_fp32(exact)
        a = _score(eng, z, return_tok_logp=True)
        b = _score(eng, z, L=160, return_tok_logp=True)
        junk = np.concatenate([z["gold"], np.zeros((6, 95), np.int32)], 1)
        rng = np.random.default_rng(3)
        dead = np.arange(160)[None, :] >= z["gold_len"][:, None]
        junk[dead] = rng.choice([0, 1, 2, 3, 4, 7, 8, 1000, -5, 2 ** 31 - 1], int(dead.sum()))
        c = _score(eng, z, gold=junk, return_tok_logp=True)
        L = z["gold"].shape[1]
        assert torch.equal(a["scores"], b["scores"]) and torch.equal(a["scores"], c["scores"])
        assert torch.equal(a["tok_logp"], b["tok_logp"][:, :L]) and torch.equal(b["tok_logp"], c["tok_logp"])
        assert (b["tok_logp"][:, L:] == 0).all()
    finally:
        eng.close()


def test_pool_scores_match_single_engine_bitwise(fixture):
    from nanodecoder_amd.engine import EnginePool
    z = fixture["transformer_pe"]
    cfg, W = su.fixture_model(z)
    B, T = z["src"].shape
    rev = np.arange(B)[::-1].copy()
    batches = [
        dict(src=z["src"], lengths=z["lengths"], gold=z["gold"], gold_len=z["gold_len"]),
        dict(src=z["src"][rev], lengths=z["lengths"][rev], gold=z["gold"][rev], gold_len=z["gold_len"][rev]),
        dict(src=z["src"][:4], lengths=z["lengths"][:4], gold=z["gold"][:4, :33], gold_len=z["gold_len"][:4]),
    ]
    eng = _engine(cfg, W, max_batch=8, max_steps=160)
    try:
        single = [_score(eng, b, return_tok_logp=True) for b in batches]
    finally:
        eng.close()
    pool = EnginePool(cfg, W, device=0, lanes=3, max_batch=8, max_steps=160)
    try:
        rs = [pool.score_targets(b["src"], b["lengths"], np.full(len(b["lengths"]), T, np.int32), gold=b["gold"],
                                 gold_len=b["gold_len"], return_tok_logp=True) for b in batches]
        pool.synchronize()
        torch.cuda.synchronize()
        assert sorted(r["lane"] for r in rs) == [0, 1, 2]
        for r, s in zip(rs, single):
            assert torch.equal(r["scores"], s["scores"]) and torch.equal(r["tok_logp"], s["tok_logp"])
    finally:
        pool.close()


def test_translator_gold_scores(fixture):
    """translate(src, tgt) on the fixture chunks: last_gold_scores are the reference's gold scores, and the
    predictions are those of translate(src)."""
    from nanodecoder_amd.translator import Translator
    z = fixture["transformer_pe"]
    cfg, W = su.fixture_model(z)
    opt = types.SimpleNamespace(gpu=0, beam_size=1, max_length=100, batch_size=6, engine_max_batch=8)
    tr = Translator(cfg, W, opt)
    try:
        chunks = gu.chunks_of(z)
        tgt = [z["gold"][i, : z["gold_len"][i] - 1].tolist() for i in range(len(chunks))]
        tgt[1] = " ".join(cfg.itos[t] for t in tgt[1])  # a token string among the id sequences
        plain = tr.translate(chunks, batch_size=6)
        assert tr.last_gold_scores is None
        got = tr.translate(chunks, tgt=tgt, batch_size=6)
        assert got == plain
        gold = np.array(tr.last_gold_scores, np.float32)
        print("gold scores", gold, "reference", z["score"])
        assert gu.logp_close(gold, z["score"]).all()
        per = tr.score(chunks, tgt, batch_size=6)
        assert [p[0] for p in per] == tr.last_gold_scores
        assert all(gu.logp_close(np.array(p[1], np.float32), z["tok_logp"][i, : z["gold_len"][i]]).all()
                   for i, p in enumerate(per))
    finally:
        tr.engine.close()


# ----------------------------------------------------------------- argument errors
def test_score_targets_argument_errors(fixture):
    """L > max_steps and an average-attention decoder are refused with ND_ERR_ARG (before any HIP call in
    nd_score_targets: they need a context, which only a device can give, so they run here)."""
    from nanodecoder_amd import _lib
    z = fixture["transformer_pe"]
    cfg, W = su.fixture_model(z)
    eng = _engine(cfg, W, max_batch=8, max_steps=40)
    try:
        with pytest.raises(_lib.NanodecError, match="L out of range"):
            _score(eng, z)  # gold is [6, 65]
    finally:
        eng.close()
    acfg = synth.ModelConfig(self_attn_type="average")
    aeng = _engine(acfg, synth.make_weights(acfg, seed=15), max_batch=8, max_steps=40)
    try:
        with pytest.raises(NotImplementedError):
            aeng.score_targets(z["src"], z["lengths"], gold=z["gold"][:, :8], gold_len=np.ones(6, np.int32))
        buf = torch.zeros(6 * 512, device=DEV)
        p = ctypes.c_void_p(buf.data_ptr())
        rc = aeng._L.nd_score_targets(aeng._h, p, p, p, p, p, 6, 512, 8, p, None, None, None)
        assert rc == _lib.ND_ERR_ARG and b"average-attention" in aeng._L.nd_last_error()
    finally:
        aeng.close()
