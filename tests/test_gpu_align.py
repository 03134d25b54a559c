"""Forced alignment on the GPU (needs an MI355X): the tapped form of the scoring pass's context attention
against fp64, nd_score_targets_attn against the CPU oracle's forced-token loop (tests/align_util.py) and
against the engine's own step-wise decoder, its independence of the padding, nd_token_positions on its
output, the pool, and Translator.score(moves=True)."""
import ctypes
import types

import numpy as np
import pytest
import torch

from nanodecoder_amd import frontend, synth
from tests import align_util as au
from tests import golden_util as gu
from tests import score_util as su

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = 777.0


def _engine(cfg, W, **kw):
    from nanodecoder_amd.engine import Engine
    return Engine(cfg, W, device=0, **kw)


# ----------------------------------------------------------------- the tapped attention op
# the three shapes the tap is specified on, dense, then a pitch above Lk on the 16-byte path (516) and one
# that sends a T % 4 == 0 shape down the scalar path (203)
@pytest.mark.parametrize("L,T,span,ld_tap", [(1, 77, 77, 77), (33, 512, 300, 512), (129, 200, 150, 200),
                                             (33, 512, 300, 516), (129, 200, 150, 203)])
def test_tf_attention_tap_vs_fp64(L, T, span, ld_tap):
    """The inputs of test_gpu_score.py::test_tf_attention_cross_vs_fp64 (B = 3, ragged spans, masked keys
    injected, chunk 2 masked whole).  Head 0's tapped scores: within 2e-4 absolute of fp64 at live keys (the
    bound that test holds the kernel's output to on the same randn operands), exactly -1e18 at masked keys,
    -inf or untouched past the span, untouched in the pad columns; a host softmax of chunk 2's rows is
    uniform; out is bit for bit the untapped launch's."""
    from nanodecoder_amd.engine import op_tf_attention, op_tf_attention_tap
    B, pad_val = 3, 1.0
    g = torch.Generator().manual_seed(7 * L + T + span)
    q = torch.randn(B * L, 256, generator=g)
    kv = torch.randn(B * T, 1536, generator=g)
    sig = torch.randn(B, T, generator=g)
    sig[torch.rand(B, T, generator=g) < 0.1] = pad_val
    sig[2] = pad_val  # every key of chunk 2 masked
    spans = torch.tensor([span, max(1, span - 13), max(1, span // 2)], dtype=torch.int32)
    dq, dkv, dsig, dsp = q.to(DEV), kv.to(DEV), sig.to(DEV), spans.to(DEV)
    buf = torch.full((B * L, ld_tap), SENTINEL, dtype=torch.float32, device=DEV)
    out, tap = op_tf_attention_tap(dq, dkv, B, L, T, 512, 768, signal=dsig, span=dsp, pad_val=pad_val, tap=buf,
                                   ld_tap=ld_tap)
    plain = op_tf_attention(dq, dkv, B, L, T, 512, 768, False, signal=dsig, span=dsp, pad_val=pad_val)
    torch.cuda.synchronize()
    assert tap.data_ptr() == buf.data_ptr()
    assert torch.equal(out, plain)
    tap = tap.cpu()
    assert (tap[:, T:] == SENTINEL).all()  # pad columns untouched
    tap = tap[:, :T].reshape(B, L, T)
    err, n_masked = 0.0, 0
    for c in range(B):
        n = int(spans[c])
        s = (q[c * L:(c + 1) * L, :32].double() / np.sqrt(32.0)) @ kv[c * T:(c + 1) * T, 512:544].double().T
        filled = (sig[c] == pad_val)[:n]
        got = tap[c, :, :n]
        err = max(err, (got.double() - s[:, :n])[:, ~filled].abs().max().item() if (~filled).any() else 0.0)
        assert (got[:, filled] == np.float32(-1e18)).all()
        n_masked += int(filled.sum())
        tail = tap[c, :, n:]
        assert ((tail == float("-inf")) | (tail == SENTINEL)).all()
    uni = torch.softmax(tap[2, :, : int(spans[2])].double(), -1)
    assert (uni.max(-1).values == uni.min(-1).values).all()
    assert (uni[:, 0] - 1.0 / int(spans[2])).abs().max().item() < 1e-12
    print("tap", (L, T, span, ld_tap), "max abs err at live keys", err, "masked keys", n_masked)
    assert n_masked > int(spans[2])  # chunk 2's whole span and the injected keys of the other chunks
    assert err < 2e-4


# ----------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def fixture():
    return su.load_fixture()


@pytest.fixture(scope="module")
def oracle(fixture):
    """The CPU oracle's forced-token scores and attention of both fixture models, computed once."""
    from oracle import ref_cpu
    out = {}
    for name, z in fixture.items():
        cfg, W = su.fixture_model(z)
        out[name] = au.oracle_score_attn(ref_cpu.RefModel(cfg, W), z["src"], z["lengths"], z["gold"], z["gold_len"])
    return out


@pytest.fixture(scope="module")
def pe_engine(fixture):
    """One engine on the position-encoding fixture model for the tests that need no setting of their own."""
    cfg, W = su.fixture_model(fixture["transformer_pe"])
    eng = _engine(cfg, W, max_batch=8, max_steps=160)
    yield eng
    eng.close()


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
def test_score_attention_matches_oracle(fixture, oracle, name, exact, graphs):
    """attn of score_targets(return_attn=True) on rows i < gold_len: within 1e-4 absolute of the oracle's
    forced-token loop (the bar test_gpu_parity.py holds the decode tap to), every row a probability row; and
    the call's other outputs are bit for bit those of the call without return_attn."""
    z = fixture[name]
    cfg, W = su.fixture_model(z)
    eng = _engine(cfg, W, max_batch=8, max_steps=160, graphs=graphs)
    try:
        eng.set_exact_fp32(exact)
        r = _score(eng, z, return_tok_logp=True, return_logp=True, return_attn=True)
        p = _score(eng, z, return_tok_logp=True, return_logp=True)
        again = _score(eng, z, return_tok_logp=True, return_logp=True, return_attn=True)
        assert int(r["overflow"].item()) == 0
        assert p["attn"] is None
        for k in ("scores", "tok_logp", "logp"):
            assert torch.equal(r[k], p[k]), k
        assert torch.equal(r["attn"], again["attn"])
        at = r["attn"].cpu().numpy()
    finally:
        eng.close()
    B, T = z["src"].shape
    L = z["gold"].shape[1]
    o_at = oracle[name][3]
    assert at.shape == (B, L, T) == o_at.shape
    live = np.arange(L)[None, :] < z["gold_len"][:, None]
    d = np.abs(at - o_at)[live]
    sums = at.sum(-1, dtype=np.float64)[live]
    print(name, "exact" if exact else "split", "graphs" if graphs else "eager", "max |attn - oracle| on live rows",
          d.max(), "max |row sum - 1|", np.abs(sums - 1).max())
    assert d.max() < 1e-4
    assert np.abs(sums - 1).max() < 1e-5
    assert np.isfinite(at[live]).all() and (at[live] >= 0).all()


@pytest.mark.parametrize("seed,eos_bias", [(31, 0.5), (32, -1.5)])
def test_score_attention_equals_the_stepwise_decoder(seed, eos_bias):
    """No oracle: chunks of mixed lengths and ragged spans with masked samples decoded greedily with
    return_attn; each chunk's own tokens up to and including its first EOS (or all of them), scored in one
    pass with return_attn, give the decoder's attention rows within 2e-4 (each side is within 1e-4 of the
    oracle), zero at t >= span on both sides.  One model ends its targets early, one never emits EOS."""
    cfg = synth.ModelConfig()
    W = synth.make_weights(cfg, seed=seed, eos_bias=eos_bias)
    B, S, T = 8, 24, 512
    sig = synth.synth_chunk_batch(B, T, seed=5, inject_masks=True)
    spans = np.array([512, 512, 300, 300, 448, 448, 100, 100], np.int32)
    lens = np.array([512, 411, 300, 77, 448, 150, 100, 1], np.int32)
    for i in range(B):
        sig[i, lens[i]:] = 0
    eng = _engine(cfg, W, max_batch=B, max_steps=S)
    try:
        g = eng.translate_greedy(sig, lens, spans, max_len=S, return_attn=True)
        tok, g_at = g["tokens"].cpu().numpy(), g["attn"].cpu().numpy()
        is_eos = tok == cfg.eos_idx
        gold_len = np.where(is_eos.any(1), is_eos.argmax(1) + 1, S).astype(np.int32)
        live = np.arange(S)[None, :] < gold_len[:, None]
        gold = np.where(live, tok, cfg.pad_idx).astype(np.int32)
        r = eng.score_targets(sig, lens, spans, gold=gold, gold_len=gold_len, return_attn=True)
        at = r["attn"].cpu().numpy()
    finally:
        eng.close()
    assert at.shape == g_at.shape == (B, S, T)
    d = np.abs(at - g_at)[live]
    print("gold_len", gold_len, "max |scoring attn - stepwise attn| on decoded rows", d.max())
    assert (gold_len == S).all() if eos_bias < 0 else (gold_len < S).all()
    assert d.max() < 2e-4
    past = np.arange(T)[None, None, :] >= spans[:, None, None]
    assert (at[live[:, :, None] & past] == 0).all() and (g_at[live[:, :, None] & past] == 0).all()
    assert np.abs(at.sum(-1, dtype=np.float64)[live] - 1).max() < 1e-5


def test_score_attention_is_independent_of_padding(fixture, pe_engine):
    """The same batch at L = its longest target and at L + 16 with padded gold rows: the live attention rows
    are bit for bit the same."""
    z = fixture["transformer_pe"]
    L = z["gold"].shape[1]
    a = _score(pe_engine, z, return_attn=True)
    b = _score(pe_engine, z, L=L + 16, return_attn=True)
    assert b["attn"].shape[1] == L + 16 and torch.equal(a["scores"], b["scores"])
    n = 0
    for i, gl in enumerate(z["gold_len"]):
        assert torch.equal(a["attn"][i, :gl], b["attn"][i, :gl]), i
        n += int(gl)
    assert n == int(z["gold_len"].sum()) > 100


def test_token_positions_of_the_scoring_attention(fixture, pe_engine):
    """Engine.token_positions on the scoring call's attention equals the host rule applied to the same device
    attention, exactly (as test_gpu_moves.py checks the decode path), with ragged spans."""
    z = fixture["transformer_pe"]
    B, T = z["src"].shape
    spans = np.maximum(z["lengths"], np.array([T, T, 300, 300, 77, 77], np.int32)[:B]).astype(np.int32)
    r = pe_engine.score_targets(z["src"], z["lengths"], spans, gold=z["gold"], gold_len=z["gold_len"],
                                return_attn=True)
    pos = pe_engine.token_positions(r["attn"], spans)
    torch.cuda.synchronize()
    assert pos.dtype == torch.int32 and tuple(pos.shape) == z["gold"].shape
    at = r["attn"].cpu().numpy()
    want = frontend.token_positions(at, spans)
    assert pos.cpu().numpy().tolist() == want.tolist()
    live = np.arange(z["gold"].shape[1])[None, :] < z["gold_len"][:, None]
    past = np.arange(T)[None, None, :] >= spans[:, None, None]
    assert (at[live[:, :, None] & past] == 0).all()
    assert (np.diff(want, axis=1) >= 0).all() and (want[live] < np.broadcast_to(spans[:, None], want.shape)[live]).all()
    assert want.max() > 0


def test_pool_attention_matches_single_engine_bitwise(fixture, pe_engine):
    from nanodecoder_amd.engine import EnginePool
    z = fixture["transformer_pe"]
    cfg, W = su.fixture_model(z)
    B, T = z["src"].shape
    single = _score(pe_engine, z, return_tok_logp=True, return_attn=True)
    pool = EnginePool(cfg, W, device=0, lanes=2, max_batch=8, max_steps=160)
    try:
        rs = [pool.score_targets(z["src"], z["lengths"], np.full(B, T, np.int32), gold=z["gold"],
                                 gold_len=z["gold_len"], return_tok_logp=True, return_attn=True) for _ in range(2)]
        pos = [pool.token_positions(r["attn"], np.full(B, T, np.int32), lane=r["lane"]) for r in rs]
        pool.synchronize()
        torch.cuda.synchronize()
        assert sorted(r["lane"] for r in rs) == [0, 1]
        want = pe_engine.token_positions(single["attn"], np.full(B, T, np.int32))
        for r, ps in zip(rs, pos):
            assert torch.equal(r["attn"], single["attn"]) and torch.equal(r["scores"], single["scores"])
            assert torch.equal(r["tok_logp"], single["tok_logp"]) and torch.equal(ps, want)
    finally:
        pool.close()


def test_translator_score_with_moves(fixture):
    """Translator.score(moves=True) on the fixture model: (score, tok_logp, positions) per chunk, the first
    two as without moves, positions = the host rule on the attention of the engine call it made (issued
    again here with the recorded arguments), one per target token, EOS included."""
    from nanodecoder_amd.translator import Translator
    z = fixture["transformer_pe"]
    cfg, W = su.fixture_model(z)
    opt = types.SimpleNamespace(gpu=0, beam_size=1, max_length=100, batch_size=6, engine_max_batch=8)
    tr = Translator(cfg, W, opt)
    try:
        chunks = gu.chunks_of(z)
        tgt = [z["gold"][i, : z["gold_len"][i] - 1].tolist() for i in range(len(chunks))]
        calls = []
        real = tr.engine.score_targets
        keep = lambda v: v.clone() if isinstance(v, torch.Tensor) else v  # noqa: E731

        def spy(*a, **kw):
            calls.append((tuple(keep(v) for v in a), {k: keep(v) for k, v in kw.items()}))
            return real(*a, **kw)
        tr.engine.score_targets = spy
        plain = tr.score(chunks, tgt, batch_size=6)
        assert len(calls) == 1 and "return_attn" not in calls[0][1]
        got = tr.score(chunks, tgt, batch_size=6, moves=True)
        assert len(calls) == 2 and calls[1][1]["return_attn"] is True
        assert all(len(p) == 2 for p in plain) and all(len(g) == 3 for g in got)
        assert [g[:2] for g in got] == plain
        a, kw = calls[1]
        r = real(*a, **kw)
        if "event" in r:
            r["event"].synchronize()
        torch.cuda.synchronize()
        spans = a[2].cpu().numpy()
        want = frontend.token_positions(r["attn"].cpu().numpy(), spans)
        for i, g in enumerate(got):
            n = int(z["gold_len"][i])
            assert len(g[2]) == len(g[1]) == n and all(isinstance(v, int) for v in g[2])
            assert g[2] == want[i, :n].tolist(), i
            assert g[2] == sorted(g[2]) and 0 <= g[2][0] and g[2][-1] < spans[i]
    finally:
        tr.engine.close()


# ----------------------------------------------------------------- refusals
def test_refusals(fixture, pe_engine):
    """A causal tap, ld_tap < Lk and a null d_attn return ND_ERR_ARG with a message; an average-attention
    context is refused by nd_score_targets_attn and by Engine.score_targets(return_attn=True)."""
    from nanodecoder_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(6 * 512, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    f0 = ctypes.c_float(0.0)
    rc = L.nd_op_tf_attention_tap(p, 768, p, 768, 256, 512, None, None, f0, p, 1, 8, 8, 1, p, 8, None)
    assert rc == _lib.ND_ERR_ARG and b"causal" in L.nd_last_error()
    rc = L.nd_op_tf_attention_tap(p, 256, p, 512, 0, 256, p, p, f0, p, 1, 2, 64, 0, p, 63, None)
    assert rc == _lib.ND_ERR_ARG and b"ld_tap" in L.nd_last_error()
    rc = L.nd_score_targets_attn(pe_engine._h, p, p, p, p, p, 6, 512, 8, p, None, None, None, None)
    assert rc == _lib.ND_ERR_ARG and b"null d_attn" in L.nd_last_error()
    torch.cuda.synchronize()
    assert (buf == 0).all()  # nothing ran
    z = fixture["transformer_pe"]
    acfg = synth.ModelConfig(self_attn_type="average")
    aeng = _engine(acfg, synth.make_weights(acfg, seed=15), max_batch=8, max_steps=40)
    try:
        with pytest.raises(NotImplementedError):
            aeng.score_targets(z["src"], z["lengths"], gold=z["gold"][:, :8], gold_len=np.ones(6, np.int32),
                               return_attn=True)
        rc = aeng._L.nd_score_targets_attn(aeng._h, p, p, p, p, p, 6, 512, 8, p, None, None, p, None)
        assert rc == _lib.ND_ERR_ARG and b"average-attention" in aeng._L.nd_last_error()
    finally:
        aeng.close()
