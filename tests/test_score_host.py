"""Teacher-forced scoring, host side (no GPU): the CPU oracle's forced-token loop against the fixture recorded
from the reference's Translator._score_target (tools/make_golden_score.py), the Translator's target parsing
and validation, and nd_score_targets' exported symbol and argument errors."""
import ctypes
import types

import numpy as np
import pytest
import torch

from nanodecoder_amd import synth
from nanodecoder_amd.translator import Translator
from oracle import ref_cpu
from tests import golden_util as gu
from tests import score_util as su


@pytest.fixture(scope="module")
def fixture():
    return su.load_fixture()


@pytest.mark.parametrize("name", su.MODELS)
def test_oracle_score_matches_reference(fixture, name):
    """The step-wise oracle with forced tokens equals the reference's one-pass _score_target: log-probs
    within test_oracle.py's bound for log-probs (atol 1e-4, rtol 1e-6), scores within logp_close."""
    z = fixture[name]
    cfg, W = su.fixture_model(z)
    sc, tl, lp = su.oracle_score(ref_cpu.RefModel(cfg, W), z["src"], z["lengths"], z["gold"], z["gold_len"])
    assert list(z["gold_len"]) == [1, 8, 32, 33, 65, 41]
    live = np.arange(z["gold"].shape[1])[None, :] < z["gold_len"][:, None]
    d = np.abs(lp - z["logp"])[live]
    print(name, "max |logp - ref| over live rows", d.max(), "scores", sc, z["score"])
    assert gu.logp_close(lp, z["logp"], atol=1e-4, rtol=1e-6)[live].all()
    assert gu.logp_close(tl, z["tok_logp"], atol=1e-4, rtol=1e-6).all()
    assert (tl[~live] == 0).all() and (z["tok_logp"][~live] == 0).all()
    assert gu.logp_close(sc, z["score"]).all()
    # the reference sums every position with the pad column zeroed: the sum of the live positions
    assert gu.logp_close(z["tok_logp"].sum(1), z["score"]).all()


class ScoreEngine:
    """Records what Translator.score hands to Engine.score_targets; the score of a row is minus its gold
    length, each summand -1."""
    max_batch, max_src_len, max_steps = 4, 512, 12

    def __init__(self):
        self.calls = []

    def translate_greedy(self, sig, L, S, max_len, min_len=0, return_attn=False):
        B = sig.shape[0]
        tok = torch.full((B, max_len), 3, dtype=torch.int32)  # "A" then EOS
        tok[:, 0] = 4
        return {"tokens": tok, "scores": torch.zeros(B), "logp": None, "attn": None}

    def score_targets(self, sig, L, S, gold=None, gold_len=None, return_tok_logp=False, return_logp=False):
        gold, gold_len = gold.numpy().copy(), gold_len.numpy().copy()
        self.calls.append(dict(shape=tuple(sig.shape), L=np.array(L).copy(), S=np.array(S).copy(), gold=gold,
                               gold_len=gold_len))
        tl = -(np.arange(gold.shape[1])[None, :] < gold_len[:, None]).astype(np.float32)
        return dict(scores=torch.from_numpy(tl.sum(1)), tok_logp=torch.from_numpy(tl), logp=None,
                    overflow=torch.zeros(1, dtype=torch.int32))


def make_translator():
    eng = ScoreEngine()
    opt = types.SimpleNamespace(gpu=0, beam_size=1, max_length=12, batch_size=2)
    return Translator(synth.ModelConfig(), None, opt, engine=eng), eng


def test_score_parses_targets_and_keeps_reference_spans():
    tr, eng = make_translator()
    cfg = tr.cfg
    rng = np.random.default_rng(0)
    chunks = [rng.standard_normal(n).astype(np.float32) for n in (300, 200, 77, 512, 100)]
    A, C, G, T = (cfg.itos.index(w) for w in "ACGT")
    out = tr.score(chunks, ["A C G T", [A, A, C], "A N G", "", np.array([T] * 11)], batch_size=2)
    # five chunks on an engine of max_batch 4: two calls
    assert [c["shape"][0] for c in eng.calls] == [4, 4]
    c0, c1 = eng.calls
    # spans: consecutive batch_size = 2 chunks share their longer length, as stream_reads assigns them
    assert list(c0["S"][:4]) == [300, 300, 512, 512] and list(c1["S"][:1]) == [100]
    assert list(c0["L"][:4]) == [300, 200, 77, 512]
    E, P, U = cfg.eos_idx, cfg.pad_idx, cfg.unk_idx
    assert c0["gold"].shape[1] == 8  # longest target + EOS = 5, padded to a multiple of 8 positions
    assert list(c0["gold"][0]) == [A, C, G, T, E, P, P, P] and c0["gold_len"][0] == 5   # EOS appended
    assert list(c0["gold"][1][:5]) == [A, A, C, E, P] and c0["gold_len"][1] == 4        # id sequence
    assert list(c0["gold"][2][:4]) == [A, U, G, E]                                      # unknown word -> <unk>
    assert list(c0["gold"][3][:2]) == [E, P] and c0["gold_len"][3] == 1                 # empty target: EOS alone
    assert c1["gold"].shape[1] == 12 and c1["gold_len"][0] == 12                        # max_steps - 1 tokens + EOS
    assert [o[0] for o in out] == [-5.0, -4.0, -4.0, -1.0, -12.0]
    assert [len(o[1]) for o in out] == [5, 4, 4, 1, 12]


@pytest.mark.parametrize("target,what", [
    ([4, 99], "outside the vocabulary"),
    ([4, -1], "outside the vocabulary"),
    ("A <blank> C", "special token"),
    ([4, 2, 5], "special token"),           # BOS inside
    ("A </s>", "special token"),            # EOS inside
    ("A " * 12, "longer than max_steps - 1"),
])
def test_score_rejects_bad_targets(target, what):
    tr, eng = make_translator()
    with pytest.raises(ValueError, match=what):
        tr.score([np.ones(64, np.float32)], [target], batch_size=1)
    assert not eng.calls  # refused before any engine call


def test_score_needs_one_target_per_chunk():
    tr, _ = make_translator()
    with pytest.raises(ValueError, match="one target per chunk"):
        tr.score([np.ones(64, np.float32)] * 2, ["A"], batch_size=1)


def test_translate_with_tgt_keeps_gold_scores_and_logs_them():
    """translate(src, tgt): the return value is translate(src)'s, the per-chunk gold scores stay on
    last_gold_scores, and -verbose logs GOLD / GOLD SCORE after PRED SCORE (translation.py:147-150)."""
    tr, eng = make_translator()
    tr.verbose = True
    lines = []
    tr.logger = types.SimpleNamespace(info=lines.append)
    chunks = [np.ones(n, np.float32) for n in (128, 64, 100)]
    plain = tr.translate(chunks, batch_size=2)
    assert tr.last_gold_scores is None and not eng.calls and not any("GOLD" in m for m in lines)
    del lines[:]
    got = tr.translate(chunks, tgt=["A C", "G", "T T T"], batch_size=2)
    assert got == plain
    assert tr.last_gold_scores == [-3.0, -2.0, -4.0]
    assert len(lines) == 3
    assert "PRED SCORE: 0.0000\nGOLD 1: A C\nGOLD SCORE: -3.0000\n" in lines[0]
    assert "GOLD 3: T T T\nGOLD SCORE: -4.0000\n" in lines[2]


def test_score_targets_symbol_and_argument_errors_without_gpu():
    """nd_score_targets is exported and bound, and refuses a call before any HIP call (a null context:
    no device is touched).  The checks that need a context (L > max_steps, an average-attention
    configuration) cannot run here, since nd_create itself opens the device: tests/test_gpu_score.py."""
    from nanodecoder_amd import _lib, build
    build.build()
    L = _lib.lib()
    assert "nd_score_targets" in _lib.SIGNATURES and "nd_op_tf_attention" in _lib.SIGNATURES
    rc = L.nd_score_targets(None, None, None, None, None, None, 1, 64, 8, None, None, None, None)
    assert rc == _lib.ND_ERR_ARG and b"null ctx" in L.nd_last_error()
    rc = L.nd_op_tf_attention(None, 256, None, 768, 256, 512, None, None, ctypes.c_float(0.0), None, 1, 8, 8, 1, None)
    assert rc == _lib.ND_ERR_ARG and b"tf_attention" in L.nd_last_error()
