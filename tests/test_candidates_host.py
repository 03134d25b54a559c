"""Candidate scoring, host side (no GPU): the two entry points' symbols and the refusals they make before any
HIP call, the fp64 posterior rule against a direct logsumexp, and what Translator.score_candidates asks of
its engine, on a stand-in engine as in tests/test_align_host.py."""
import types

import numpy as np
import pytest
import torch

from nanodecoder_amd import frontend, synth
from nanodecoder_amd.translator import Translator
from tests import cand_util as cu


# ----------------------------------------------------------------- C ABI
def test_symbols_and_refusals_without_gpu():
    from nanodecoder_amd import _lib, build
    build.build()
    L = _lib.lib()
    assert "nd_score_candidates" in _lib.SIGNATURES and "nd_cand_posterior" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["nd_score_candidates"][1]) == 16 and len(_lib.SIGNATURES["nd_cand_posterior"][1]) == 8
    assert hasattr(L, "nd_score_candidates") and hasattr(L, "nd_cand_posterior")
    rc = L.nd_score_candidates(None, None, None, None, None, None, 1, 64, 2, 8, None, None, None, None, None, None)
    assert rc == _lib.ND_ERR_ARG and b"null ctx" in L.nd_last_error()
    p = 16  # never dereferenced: refused first
    for args in ((None, p, 2, 4, p, p, p), (p, None, 2, 4, p, p, p), (p, p, 2, 4, None, p, p)):
        assert L.nd_cand_posterior(*args, None) == _lib.ND_ERR_ARG and b"null buffer" in L.nd_last_error()
    for B, K in ((2, 0), (2, -1), (-1, 4)):
        assert L.nd_cand_posterior(p, p, B, K, p, p, p, None) == _lib.ND_ERR_ARG
        assert b"cand_posterior" in L.nd_last_error()
    assert L.nd_cand_posterior(None, None, 0, 4, None, None, None, None) == 0  # B == 0: nothing to do


def test_header_declares_both_entry_points():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nanodec.h")).read()
    assert "int nd_score_candidates(nd_ctx* ctx," in hdr and "int nd_cand_posterior(const float* d_score," in hdr


# ----------------------------------------------------------------- the rule
def test_candidate_posterior_matches_direct_logsumexp():
    scores, cand_len, want_best = cu.scripted_rows()
    post, best = frontend.candidate_posterior(scores, cand_len)
    assert post.dtype == np.float64 and post.shape == scores.shape and best.shape == (5,)
    assert best.tolist() == want_best.tolist()
    want = cu.logsumexp_posterior(scores, cand_len)
    assert np.isnan(post[4, :3]).all() and np.isnan(want[4, :3]).all() and post[4, 3] == -np.inf
    assert (post[1] == -np.inf).all() and post[2].tolist() == [-np.inf, 0.0, -np.inf, -np.inf]
    assert (np.isneginf(post[:4]) == np.isneginf(want[:4])).all()
    fin = np.isfinite(want[:4])
    assert np.abs(post[:4][fin] - want[:4][fin]).max() < 1e-12
    # a posterior: the live slots of a row sum to 1; scores 1e-3 apart near -400 are told apart
    assert np.abs(np.exp(post[[0, 2, 3]]).sum(-1) - 1.0).max() < 1e-12
    assert post[3, 2] > post[3, 0] > post[3, 1] > post[3, 3]
    # one row is the [K] case
    p1, b1 = frontend.candidate_posterior(scores[0], cand_len[0])
    assert (p1 == post[0]).all() and int(b1) == 1
    with pytest.raises(ValueError):
        frontend.candidate_posterior(scores, cand_len[:, :3])


# ----------------------------------------------------------------- Translator.score_candidates
class CandEngine:
    """Records every call Translator.score_candidates makes.  The score of a slot is minus its candidate's
    length (EOS counted) minus a tenth of its first token; post and best follow frontend.candidate_posterior.
    ``overflow_first`` flags the first call's overflow word."""
    max_batch, max_src_len, max_steps = 8, 512, 12

    def __init__(self, overflow_first=False):
        self.calls, self.exact = [], []
        self.overflow_first = overflow_first

    def set_exact_fp32(self, on):
        self.exact.append(bool(on))

    def score_candidates(self, sig, L, S, cand=None, cand_len=None, **kw):
        cand, cand_len = cand.numpy().copy(), cand_len.numpy().copy()
        self.calls.append(dict(kw=dict(kw), B=sig.shape[0], T=sig.shape[1], S=np.array(S).copy(), cand=cand,
                               cand_len=cand_len, exact=self.exact[-1:] == [True]))
        sc = np.where(cand_len > 0, -cand_len - 0.1 * cand[:, :, 0], -np.inf).astype(np.float32)
        post, best = frontend.candidate_posterior(sc, cand_len)
        return dict(scores=torch.from_numpy(sc), post=torch.from_numpy(post.astype(np.float32)),
                    best=torch.from_numpy(best.astype(np.int32)), tok_logp=None, logp=None,
                    overflow=torch.full((1,), int(self.overflow_first and len(self.calls) == 1), dtype=torch.int32))


def make_translator(cfg=None, **kw):
    eng = CandEngine(**kw)
    opt = types.SimpleNamespace(gpu=0, beam_size=1, max_length=12, batch_size=2)
    return Translator(cfg or synth.ModelConfig(), None, opt, engine=eng), eng


CHUNKS = [np.ones(n, np.float32) for n in (300, 200, 77, 120, 64, 500, 10)]
CANDS = [["A C G T", [5, 6]], ["A A C"], [[4], [5], [6]], ["T", "G", "C", "A", ""], [[7, 7]], ["C C", "C"],
         [[6, 5, 4], [6, 5]]]


def _want(cl):
    ids = [[synth.DEFAULT_ITOS.index(w) for w in t.split()] if isinstance(t, str) else list(t) for t in cl]
    sc = np.array([-(len(t) + 1) - 0.1 * (t[0] if t else 3) for t in ids], np.float32)  # "" is a lone EOS (id 3)
    post, best = frontend.candidate_posterior(sc, np.ones(len(ids)))
    return sc.tolist(), post.astype(np.float32).tolist(), int(best)


def test_translator_packs_calls_and_trims_results():
    tr, eng = make_translator()
    out = tr.score_candidates(CHUNKS, CANDS, batch_size=2)
    assert len(out) == len(CHUNKS)
    for o, cl in zip(out, CANDS):
        sc, post, best = o
        assert len(sc) == len(cl) and len(post) == len(cl) and isinstance(best, int)
        w_sc, w_post, w_best = _want(cl)
        assert sc == w_sc and best == w_best and np.allclose(post, w_post, atol=1e-6)
        assert all(np.isfinite(sc)) and all(np.isfinite(post))  # no padding slot leaks into a result
    # no call exceeds max_batch sequences; K is uniform within a call (the array is rectangular) and a power
    # of two; several calls were needed; the chunks go in input order
    assert len(eng.calls) > 1
    seen = 0
    for c in eng.calls:
        B, K, L = c["cand"].shape
        assert B == c["B"] and B * K <= eng.max_batch and K & (K - 1) == 0 and L % 8 == 0 and L <= eng.max_steps
        assert c["kw"] == {} and c["cand_len"].shape == (B, K)
        n = int((c["cand_len"][:, 0] > 0).sum())  # real chunks: slot 0 is always filled
        assert (c["cand_len"][n:] == 0).all()     # padding chunks hold empty slots only
        for b in range(n):
            filled = int((c["cand_len"][b] > 0).sum())
            assert filled == len(CANDS[seen + b]) and (c["cand_len"][b, :filled] > 0).all()
            assert K >= filled
        seen += n
    assert seen == len(CHUNKS)
    # spans as score() assigns them: the longest chunk of each reference batch of two
    spans = np.concatenate([c["S"][: int((c["cand_len"][:, 0] > 0).sum())] for c in eng.calls])
    assert spans.tolist() == [300, 300, 120, 120, 500, 500, 10]
    # a candidate row: tokens, EOS, then pad
    c0 = eng.calls[0]
    assert c0["cand"][0, 0, :6].tolist() == [4, 5, 6, 7, 3, 1] and c0["cand_len"][0, :2].tolist() == [5, 3]


def test_overflow_rerun_goes_through_exact_fp32_and_restores_the_mode():
    tr, eng = make_translator(overflow_first=True)
    out = tr.score_candidates(CHUNKS[:2], CANDS[:2], batch_size=2)
    assert [c["exact"] for c in eng.calls] == [False, True] and eng.exact == [True, False]
    assert (eng.calls[0]["cand"] == eng.calls[1]["cand"]).all()
    assert [o[0] for o in out] == [_want(cl)[0] for cl in CANDS[:2]]


def test_refusals():
    acfg = synth.ModelConfig(self_attn_type="average")
    tr, eng = make_translator(acfg)
    with pytest.raises(NotImplementedError):
        tr.score_candidates(CHUNKS[:2], CANDS[:2], batch_size=2)
    tr, eng = make_translator()
    with pytest.raises(ValueError, match="no candidates"):
        tr.score_candidates(CHUNKS[:2], [["A"], []], batch_size=2)
    with pytest.raises(ValueError, match="special token"):
        tr.score_candidates(CHUNKS[:2], [["A"], [[4, 3]]], batch_size=2)
    with pytest.raises(ValueError, match="longer than max_steps - 1"):
        tr.score_candidates(CHUNKS[:2], [["A"], [[4] * 12]], batch_size=2)
    with pytest.raises(ValueError, match="one candidate list per chunk"):
        tr.score_candidates(CHUNKS[:2], [["A"]], batch_size=2)
    assert not eng.calls
