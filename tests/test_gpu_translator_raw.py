"""Translator.stream_raw_reads / translate_raw_reads on a two-lane EnginePool, for every combination of the
optional outputs: the ``arrays`` rows against the per-chunk results, and both against the run without outputs.
More calls are made than lanes, so results are collected while other calls are in flight.  Every comparison
is exact equality.

The module's name makes it the last of the GPU modules: a pool opened before tests/test_gpu_score.py brings out an
engine defect there (the open item under "Engine streams are recycled")."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(batch_size=4, normalization="median", src_seq_length=300, src_seq_stride=60)
MAX_LENGTH = 30
LENGTHS = (700, 0, 1300, 1000)  # 8, 0, 18 and 13 windows of 300 samples at stride 60
CASES = [dict(), dict(qualities=True), dict(mods=True), dict(moves=True), dict(qualities=True, moves=True),
         dict(mods=True, moves=True)]


@pytest.fixture(scope="module")
def raw_run():
    """(translator over a two-lane pool, raw reads, translate_raw_reads' result without outputs)."""
    from nanodecoder_amd import synth
    from nanodecoder_amd.engine import EnginePool
    from nanodecoder_amd.translator import Translator
    cfg = synth.ModelConfig(itos=list(synth.DEFAULT_ITOS) + ["M"])
    pool = EnginePool(cfg, synth.make_weights(cfg, seed=11, eos_bias=-1.0), device=0, lanes=2, max_batch=8,
                      max_steps=MAX_LENGTH)
    try:
        opt = types.SimpleNamespace(gpu=0, n_best=1, max_length=MAX_LENGTH, min_length=4, beam_size=1, fast=False,
                                    alpha=0.0, beta=0.0, batch_size=4)
        tr = Translator(cfg, None, opt, engine=pool)
        raws = [synth.synth_raw_read(i, n).astype(np.float64) if n else np.zeros(0) for i, n in enumerate(LENGTHS)]
        calls = []
        greedy = pool.translate_greedy
        pool.translate_greedy = lambda *a, **k: (calls.append(k), greedy(*a, **k))[1]
        plain = tr.translate_raw_reads(raws, **KW)
        del pool.translate_greedy
        assert [len(p[1]) for p in plain] == [8, 0, 18, 13] and len(calls) == 5  # 39 chunks, 8 per call
        assert all(len(p) == 2 for p in plain) and plain[1] == ([], [])
        yield tr, raws, plain
    finally:
        pool.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "+".join(c) or "none")
def test_raw_reads_arrays_rows_equal_the_per_chunk_results(raw_run, case):
    tr, raws, plain = raw_run
    per_read = tr.translate_raw_reads(raws, **case, **KW)
    assert [p[:2] for p in per_read] == plain  # the same scores and strings as without outputs
    dtypes = [np.uint16] * (2 if case.get("mods") else int(bool(case.get("qualities")))) + \
        [np.int32] * int(bool(case.get("moves")))
    seen, n_checked = [], 0
    for ri, tok, sc, *cols in tr.stream_raw_reads(raws, arrays=True, **case, **KW):
        seen.append(ri)
        n = len(plain[ri][1])
        assert tok.dtype == np.int32 and tok.shape == (n, MAX_LENGTH) and sc.dtype == np.float32 and sc.shape == (n,)
        assert [c.dtype for c in cols] == dtypes and all(c.shape == tok.shape for c in cols)
        assert [[float(s)] for s in sc] == plain[ri][0]
        assert [[" ".join(tr._tokens_to_sent(t))] for t in tok.tolist()] == plain[ri][1]
        w, mw, ps = tr.split_result(per_read[ri], **case)[2:]
        named = [x for x in (w, mw, ps) if x is not None]
        assert len(named) == len(dtypes) and all(a is b for a, b in zip(named, per_read[ri][2:]))
        assert (mw is not None) == bool(case.get("mods")) and (ps is not None) == bool(case.get("moves"))
        for col, chunks, dtype in zip(cols, per_read[ri][2:], dtypes):
            assert len(chunks) == n
            for ci in range(n):
                want = tr._char_weights(tok[ci].tolist(), col[ci], dtype)
                assert chunks[ci].dtype == dtype and chunks[ci].tolist() == want.tolist()
                n_checked += len(want)
    assert sorted(seen) == [0, 1, 2, 3] and seen[0] == 1  # the empty read comes at once, with zero-row arrays
    assert n_checked > 0 or not dtypes
