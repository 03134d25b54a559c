"""Forced alignment, host side (no GPU): what Translator.score(moves=...) asks of its engine, on a stand-in
engine as in tests/test_score_host.py, the oracle helper against the scoring fixture, and the two new entry
points' symbols and the refusals they make before any HIP call."""
import ctypes
import types

import numpy as np
import pytest
import torch

from nanodecoder_amd import frontend, synth
from nanodecoder_amd.translator import Translator
from oracle import ref_cpu
from tests import align_util as au
from tests import score_util as su


class AlignEngine:
    """Records every call Translator.score makes.  The score of a row is minus its gold length; with
    return_attn the attention row of (chunk b, position i) is one-hot at sample min(10 i + b, T - 1), so the
    positions the host rule gives are those samples.  ``overflow_first`` flags the first call's overflow word."""
    max_batch, max_src_len, max_steps = 4, 512, 12

    def __init__(self, overflow_first=False):
        self.calls, self.pos_calls, self.exact = [], [], []
        self.overflow_first = overflow_first

    def set_exact_fp32(self, on):
        self.exact.append(bool(on))

    def score_targets(self, sig, L, S, gold=None, gold_len=None, **kw):
        gold, gold_len = gold.numpy().copy(), gold_len.numpy().copy()
        self.calls.append(dict(kw=dict(kw), S=np.array(S).copy(), gold_len=gold_len, exact=self.exact[-1:] == [True]))
        B, T, n = sig.shape[0], sig.shape[1], gold.shape[1]
        tl = -(np.arange(n)[None, :] < gold_len[:, None]).astype(np.float32)
        r = dict(scores=torch.from_numpy(tl.sum(1)), tok_logp=torch.from_numpy(tl), logp=None,
                 overflow=torch.full((1,), int(self.overflow_first and len(self.calls) == 1), dtype=torch.int32))
        if kw.get("return_attn"):
            at = np.zeros((B, n, T), np.float32)
            for b in range(B):
                at[b, np.arange(n), np.minimum(10 * np.arange(n) + b, T - 1)] = 1.0
            r["attn"] = torch.from_numpy(at)
        return r

    def token_positions(self, attn, spans, hyp0=None, **kw):
        self.pos_calls.append(dict(shape=tuple(attn.shape), spans=np.array(spans).copy(), hyp0=hyp0, kw=dict(kw)))
        return torch.from_numpy(frontend.token_positions(attn.numpy(), np.asarray(spans)).astype(np.int32))


def make_translator(**kw):
    eng = AlignEngine(**kw)
    opt = types.SimpleNamespace(gpu=0, beam_size=1, max_length=12, batch_size=2)
    return Translator(synth.ModelConfig(), None, opt, engine=eng), eng


CHUNKS = [np.ones(n, np.float32) for n in (300, 200, 77)]
TARGETS = ["A C G T", "A A C", ""]


def test_score_without_moves_passes_no_new_keyword():
    tr, eng = make_translator()
    out = tr.score(CHUNKS, TARGETS, batch_size=2)
    assert [c["kw"] for c in eng.calls] == [dict(return_tok_logp=True)]
    assert not eng.pos_calls
    assert all(len(o) == 2 for o in out) and [o[0] for o in out] == [-5.0, -4.0, -1.0]
    assert out == tr.score(CHUNKS, TARGETS, batch_size=2, moves=False)
    assert all("return_attn" not in c["kw"] for c in eng.calls)


def test_score_with_moves_asks_for_the_attention_and_cuts_at_gold_len():
    tr, eng = make_translator()
    plain = tr.score(CHUNKS, TARGETS, batch_size=2)
    del eng.calls[:]
    out = tr.score(CHUNKS, TARGETS, batch_size=2, moves=True)
    assert [c["kw"] for c in eng.calls] == [dict(return_tok_logp=True, return_attn=True)]
    # one token_positions call over the call's whole attention with the batch's spans (the engine's four rows:
    # chunks 0 and 1 share their reference batch's span, the padding row keeps the stage's)
    assert len(eng.pos_calls) == 1
    p = eng.pos_calls[0]
    assert p["shape"] == (4, 8, 320) and list(p["spans"][:3]) == [300, 300, 77] and p["spans"].shape == (4,)
    assert (p["spans"] == eng.calls[0]["S"]).all()
    assert [o[:2] for o in out] == plain
    assert [len(o[2]) for o in out] == [5, 4, 1] and [len(o[2]) for o in out] == [len(o[1]) for o in out]
    assert out[0][2] == [0, 10, 20, 30, 40] and out[1][2] == [1, 11, 21, 31] and out[2][2] == [2]
    assert all(isinstance(v, int) for o in out for v in o[2])


def test_overflow_rerun_carries_the_request():
    tr, eng = make_translator(overflow_first=True)
    out = tr.score(CHUNKS, TARGETS, batch_size=2, moves=True)
    assert [c["kw"] for c in eng.calls] == [dict(return_tok_logp=True, return_attn=True)] * 2
    assert [c["exact"] for c in eng.calls] == [False, True] and eng.exact == [True, False]
    assert len(eng.pos_calls) == 1  # positions of the rerun only
    assert [len(o) for o in out] == [3, 3, 3] and out[0][2] == [0, 10, 20, 30, 40]
    # and without moves the rerun stays today's
    tr, eng = make_translator(overflow_first=True)
    out = tr.score(CHUNKS, TARGETS, batch_size=2)
    assert [c["kw"] for c in eng.calls] == [dict(return_tok_logp=True)] * 2 and not eng.pos_calls
    assert [len(o) for o in out] == [2, 2, 2]


def test_average_attention_config_is_refused():
    eng = AlignEngine()
    opt = types.SimpleNamespace(gpu=0, beam_size=1, max_length=12, batch_size=2)
    tr = Translator(synth.ModelConfig(self_attn_type="average"), None, opt, engine=eng)
    for kw in (dict(), dict(moves=True)):
        with pytest.raises(NotImplementedError):
            tr.score(CHUNKS, TARGETS, batch_size=2, **kw)
    assert not eng.calls and not eng.pos_calls


def test_oracle_helper_repeats_oracle_score_and_stacks_attention():
    """align_util.oracle_score_attn: the same scores as score_util.oracle_score (same loop, bit for bit), and
    attention rows that are probability rows over the chunk's samples."""
    z = su.load_fixture()["transformer_pe"]
    cfg, W = su.fixture_model(z)
    sl = slice(0, 3)  # gold_len 1, 8, 32
    gold = z["gold"][sl, :32]
    model = ref_cpu.RefModel(cfg, W)
    sc, tl, lp, at = au.oracle_score_attn(model, z["src"][sl], z["lengths"][sl], gold, z["gold_len"][sl])
    sc0, tl0, lp0 = su.oracle_score(model, z["src"][sl], z["lengths"][sl], gold, z["gold_len"][sl])
    assert (sc == sc0).all() and (tl == tl0).all() and (lp == lp0).all()
    assert at.shape == (3, 32, z["src"].shape[1]) and at.dtype == np.float32
    assert np.abs(at.sum(-1) - 1.0).max() < 1e-5 and (at >= 0).all()


def test_symbols_and_refusals_without_gpu():
    """Both entry points are exported and bound, and refuse before any HIP call: a null context, a causal
    tap, a null tap, ld_tap below Lk (no device is touched; the checks that need a context run in
    tests/test_gpu_align.py)."""
    from nanodecoder_amd import _lib, build
    build.build()
    L = _lib.lib()
    assert "nd_score_targets_attn" in _lib.SIGNATURES and "nd_op_tf_attention_tap" in _lib.SIGNATURES
    rc = L.nd_score_targets_attn(None, None, None, None, None, None, 1, 64, 8, None, None, None, None, None)
    assert rc == _lib.ND_ERR_ARG and b"null ctx" in L.nd_last_error()
    f0, one = ctypes.c_float(0.0), ctypes.c_void_p(16)  # never dereferenced: refused first
    rc = L.nd_op_tf_attention_tap(None, 256, None, 768, 256, 512, None, None, f0, None, 1, 8, 8, 1, one, 8, None)
    assert rc == _lib.ND_ERR_ARG and b"causal" in L.nd_last_error()
    rc = L.nd_op_tf_attention_tap(None, 256, None, 512, 0, 256, None, None, f0, None, 1, 8, 64, 0, one, 63, None)
    assert rc == _lib.ND_ERR_ARG and b"ld_tap" in L.nd_last_error()
    rc = L.nd_op_tf_attention_tap(None, 256, None, 512, 0, 256, None, None, f0, None, 1, 8, 64, 0, None, 64, None)
    assert rc == _lib.ND_ERR_ARG and b"null tap" in L.nd_last_error()
