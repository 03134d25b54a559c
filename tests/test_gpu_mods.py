"""Per-base methylation probabilities on the device: nd_token_mod_weights against fp64 numpy,
nd_assemble_reads_m against the host function frontend.assemble_read_m (byte identity) and against
nd_assemble_reads_q (sequence, quality and status), the Translator's modification weights on the golden CpG
model (greedy and --fast beam), and translate.py -mod_probs with both assemblies and both front ends."""
import ctypes
import math
import os
import random
import types

import numpy as np
import pytest
import torch

from nanodecoder_amd import frontend
from tests import golden_util as gu
from tests.test_mods_host import HAND_M, parse_record, random_group_m, random_mod_weights
from tests.test_quality_host import HAND, random_weights, spaced

pytestmark = pytest.mark.gpu
LEN, STRIDE = 300, 60
C_ID, M_ID = 5, 8  # "C" and "M" in the nine-token vocabulary


# ---------------------------------------------------------------- nd_token_mod_weights
def mod_case(B, S, V, seed):
    """(tokens [B, S] int32, logp [B, S, V] float32): half the tokens C or M, the rest anything; planted at the
    front: token ids -1 and V, +-inf and NaN log-probs, both -inf, and one p = 1."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, S, V)) * 2.5
    lp = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)
    tok = np.where(rng.random((B, S)) < 0.5, rng.choice([C_ID, M_ID], (B, S)), rng.integers(0, V, (B, S))).astype(np.int32)
    flat, lpf = tok.reshape(-1), lp.reshape(B * S, V)
    inf, nan = np.inf, np.nan
    planted = {1: (-1, None, None, 0), 9: (V, None, None, 0),
               2: (C_ID, None, -inf, 0),          # d = +inf
               3: (M_ID, -inf, None, 65535),      # d = -inf
               4: (M_ID, nan, None, 65535),       # NaN: the hard call
               5: (C_ID, None, nan, 0),
               6: (C_ID, -inf, -inf, 0),          # both infinite with the same sign: NaN
               7: (M_ID, -inf, -inf, 65535),
               8: (M_ID, -50.0, 0.0, 65535),      # p = 1 in fp64
               10: (C_ID, inf, None, 0), 11: (4, -inf, nan, 0)}  # 11: neither C nor M, whatever the log-probs
    for i, (t, a, b, _) in planted.items():
        flat[i] = t
        if a is not None:
            lpf[i, C_ID] = a
        if b is not None:
            lpf[i, M_ID] = b
    return tok, lp, {i: v[3] for i, v in planted.items()}


def expected_mod_weights(tok, lp):
    """The definition in fp64 numpy; asserts first that no element sits within 1e-9 of a rounding boundary."""
    with np.errstate(all="ignore"):
        d = lp[..., C_ID].astype(np.float64) - lp[..., M_ID].astype(np.float64)
        y = 65535.0 * (1.0 / (1.0 + np.exp(d)))
    cm = (tok == C_ID) | (tok == M_ID)
    ok = cm & ~np.isnan(d)
    assert (np.abs(y[ok] - np.floor(y[ok]) - 0.5) > 1e-9).all()
    mw = np.zeros(tok.shape, np.uint16)
    mw[ok] = np.minimum(65535.0, np.floor(y[ok] + 0.5)).astype(np.uint16)
    mw[cm & np.isnan(d) & (tok == M_ID)] = 65535
    return mw


@pytest.mark.parametrize("B,S,V,seed", [(3, 5, 9, 1), (70, 100, 9, 2)])
def test_token_mod_weights_equal_fp64_numpy(B, S, V, seed):
    from nanodecoder_amd import _lib
    tok, lp, planted = mod_case(B, S, V, seed)
    want = expected_mod_weights(tok, lp)
    for i, v in planted.items():
        assert want.reshape(-1)[i] == v, i
    cm = (tok == C_ID) | (tok == M_ID)
    assert not want[~cm].any() and cm.sum() >= 8
    if B * S > 1000:
        assert len(np.unique(want)) > 1000
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    tok_d, lp_d = torch.from_numpy(tok).to(dev), torch.from_numpy(lp).to(dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    mw_d = torch.full((B, S), -1, dtype=torch.int16, device=dev)
    _lib.check(L.nd_token_mod_weights(p(tok_d), p(lp_d), B, S, V, C_ID, M_ID, p(mw_d), stream), "nd_token_mod_weights")
    got = mw_d.cpu().numpy().view(np.uint16)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    # the host restatement is the same function
    host = [frontend.token_mod_weight(lp.reshape(-1, V)[i, C_ID], lp.reshape(-1, V)[i, M_ID], t == M_ID)
            if t in (C_ID, M_ID) else 0 for i, t in enumerate(tok.reshape(-1).tolist()[:1500])]
    assert host == want.reshape(-1)[:1500].tolist()


def test_engine_token_mod_weights_method():
    from nanodecoder_amd import synth
    from nanodecoder_amd.engine import Engine, EnginePool
    cfg = synth.ModelConfig(itos=list(synth.DEFAULT_ITOS) + ["M"])
    tok, lp, _ = mod_case(3, 5, cfg.vocab, 1)
    want = expected_mod_weights(tok, lp)
    W = synth.make_weights(cfg, seed=1)
    eng = Engine(cfg, W, device=0, max_batch=4, max_steps=8)
    try:
        mw = eng.token_mod_weights(torch.from_numpy(tok), torch.from_numpy(lp), C_ID, M_ID)
        assert mw.dtype == torch.int16 and tuple(mw.shape) == (3, 5)
        assert (mw.cpu().numpy().view(np.uint16) == want).all()
        with pytest.raises(ValueError):
            eng.token_mod_weights(torch.from_numpy(tok), torch.from_numpy(lp[..., :8]), C_ID, M_ID)
        from nanodecoder_amd._lib import NanodecError
        with pytest.raises(NanodecError):
            eng.token_mod_weights(torch.from_numpy(tok), torch.from_numpy(lp), C_ID, C_ID)
    finally:
        eng.close()
    pool = EnginePool(cfg, W, device=0, lanes=2, max_batch=4, max_steps=8)
    try:
        mw = pool.token_mod_weights(torch.from_numpy(tok), torch.from_numpy(lp), C_ID, M_ID, lane=1)
        pool.engines[1].stream.synchronize()
        assert (mw.cpu().numpy().view(np.uint16) == want).all()
    finally:
        pool.close()


# ---------------------------------------------------------------- nd_assemble_reads_m
def host_m(reads, ws, ms):
    return [frontend.assemble_read_m(p, w, m, LEN, STRIDE) for p, w, m in zip(reads, ws, ms)]


def same(a, b):
    """Two (sequence, quality, ml) results, or None."""
    if a is None or b is None:
        return a is b
    return a[:2] == b[:2] and a[2].dtype == b[2].dtype == np.uint8 and a[2].tobytes() == b[2].tobytes()


def device_raw_m(reads, ws, ms):
    """One nd_assemble_reads_m call and one nd_assemble_reads_q call on the same input: ((sequence, quality,
    ml) or None where status != 0, status, seq bytes, qual bytes, ml bytes); the q call's seq, qual, lengths
    and status are asserted identical."""
    bases, chunk_off, read_off, kept, qw, mw = frontend.pack_assembly_input(reads, ws, ms)[:6]
    assert kept == []
    seq, seq_len, status, qual, ml = frontend._assemble_device(bases, chunk_off, read_off, 0, qw, mw)[:5]
    seq0, seq_len0, status0, qual0 = frontend._assemble_device(bases, chunk_off, read_off, 0, qw)[:4]
    assert (status == status0).all() and (seq_len == seq_len0).all()
    assert seq.tobytes() == seq0.tobytes() and qual.tobytes() == qual0.tobytes()
    start, end = chunk_off[read_off[:-1]], chunk_off[read_off[1:]]
    out = []
    for r in range(len(reads)):
        assert (seq_len[r] == -1) == (status[r] != 0)
        if status[r]:
            out.append(None)
            continue
        a, n = start[r], seq_len[r]
        assert not ml[a + n: end[r]].any()  # 0 past the read's length
        out.append((seq[a: a + n].tobytes().decode(), frontend.quality_string(qual[a: a + n]), ml[a: a + n].copy()))
    return out, status, seq, qual, ml


def test_assemble_m_hand_made_reads():
    names = [h[0] for h in HAND_M] + [h[0] for h in HAND]
    reads = [h[1] for h in HAND_M] + [h[1] for h in HAND]
    ws = [h[2] for h in HAND_M] + random_weights([h[1] for h in HAND], seed=5)
    ms = [h[3] for h in HAND_M] + random_mod_weights([h[1] for h in HAND], seed=6)
    exp = host_m(reads, ws, ms)
    got, status, _, _, _ = device_raw_m(reads, ws, ms)
    assert not status.any()
    for name, g, e in zip(names, got, exp):
        assert same(g, e), (name, g, e)
    for (name, _, _, _, seq, ml), g in zip(HAND_M, got):  # the values worked out by hand
        assert g[0] == seq and g[2].tolist() == ml, name
    stats = {}
    grp = frontend.assemble_reads(reads, LEN, STRIDE, device=0, stats=stats, weights=ws, mod_weights=ms)
    assert all(same(g, e) for g, e in zip(grp, exp)) and stats == {"reads": len(reads), "fallback": 0}
    # nothing to assemble at all
    none = frontend.assemble_reads([[], [[""]]], LEN, STRIDE, device=0, weights=[[], [[]]], mod_weights=[[], [[]]])
    assert [n[:2] for n in none] == [("", ""), ("", "")] and all(n[2].shape == (0,) for n in none)


def test_assemble_m_random_group_matches_host():
    reads = random_group_m()
    ws, ms = random_weights(reads), random_mod_weights(reads)
    assert 35 <= len(reads) <= 45 and max(len(x[0].replace(" ", "")) for p in reads for x in p) == 199
    exp = host_m(reads, ws, ms)
    got, status, _, _, _ = device_raw_m(reads, ws, ms)
    assert not status.any()
    bad = [r for r in range(len(reads)) if not same(got[r], exp[r])]
    assert not bad, bad
    sites = np.concatenate([e[2][[c in "CM" for c in e[0]]] for e in exp])
    assert sites.size > 1500 and len(np.unique(sites)) > 200  # many sites, most ML levels
    stats = {}
    grp = frontend.assemble_reads(reads, LEN, STRIDE, device=0, stats=stats, weights=ws, mod_weights=ms)
    assert all(same(g, e) for g, e in zip(grp, exp)) and stats == {"reads": len(reads), "fallback": 0}
    # without the modification weights the calls are the ones they were
    assert frontend.assemble_reads(reads, LEN, STRIDE, device=0, weights=ws) == [e[:2] for e in exp]
    assert frontend.assemble_reads(reads, LEN, STRIDE, device=0) == [e[0] for e in exp]


def test_assemble_m_fallback_reads_get_their_ml():
    rng = random.Random(5)
    t = "".join(rng.choice("ACGTM") for _ in range(400))
    long_read = [[spaced(t[0:150])], [spaced(t[100:300])], [spaced(t[250:400])]]  # one 200-char chunk
    odd_read = [["A C G G"], ["N T M A C G G M"]]  # an N in the clipped part: the host assembles it
    plain = [["A C G T A"], ["G T A M C"]]
    reads = [plain, long_read, odd_read, plain]
    ws, ms = random_weights(reads, seed=9), random_mod_weights(reads, seed=10)
    got, status, _, _, _ = device_raw_m(reads, ws, ms)
    assert list(status) == [0, frontend.ASM_STATUS_LONG, frontend.ASM_STATUS_CHAR, 0]
    exp = host_m(reads, ws, ms)
    assert exp[2][0] == "ACGGM" and len(exp[1][0]) > 200 and exp[1][2].any() and exp[2][2].shape == (5,)
    stats = {}
    grp = frontend.assemble_reads(reads, LEN, STRIDE, device=0, stats=stats, weights=ws, mod_weights=ms)
    assert all(same(g, e) for g, e in zip(grp, exp)) and stats == {"reads": 4, "fallback": 2}
    assert same(got[0], exp[0]) and same(got[3], exp[3]) and got[0][0] == "ACGTAMC"


def test_assemble_m_no_reads_and_no_chunks():
    from nanodecoder_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    off = torch.zeros(4, dtype=torch.int32, device=dev)  # chunk_off [0] and read_off [0, 0, 0]
    out = torch.full((2, 2), 7, dtype=torch.int32, device=dev)
    assert L.nd_assemble_reads_m_work_bytes(0, 0) == 0
    # R == 0: ND_OK at once, nothing written
    _lib.check(L.nd_assemble_reads_m(None, None, None, p(off), p(off[1:]), 0, 0, 0, None, None, None, None, None,
                                     None, 0, stream), "nd_assemble_reads_m")
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [[7, 7], [7, 7]]
    # C == 0: every read is empty, status 0, as nd_assemble_reads
    _lib.check(L.nd_assemble_reads_m(None, None, None, p(off), p(off[1:]), 2, 0, 0, None, None, None, p(out[0]),
                                     p(out[1]), None, 0, stream), "nd_assemble_reads_m")
    assert out.cpu().tolist() == [[0, 0], [0, 0]]
    ref = torch.full((2, 2), 7, dtype=torch.int32, device=dev)
    _lib.check(L.nd_assemble_reads(None, p(off), p(off[1:]), 2, 0, 0, None, p(ref[0]), p(ref[1]), None, 0, stream),
               "nd_assemble_reads")
    assert ref.cpu().tolist() == out.cpu().tolist()


def test_assemble_m_repeatable_and_stream_independent():
    from nanodecoder_amd import synth
    from nanodecoder_amd.engine import Engine
    reads = random_group_m(seed=11, n_reads=30)
    ws, ms = random_weights(reads, seed=12), random_mod_weights(reads, seed=14)
    a = device_raw_m(reads, ws, ms)
    b = device_raw_m(reads, ws, ms)
    cfg = synth.ModelConfig()
    eng = Engine(cfg, synth.make_weights(cfg, seed=1), device=0, max_batch=4, max_steps=8)
    try:
        assert eng.stream != torch.cuda.default_stream(0)
        with torch.cuda.stream(eng.stream):
            c = device_raw_m(reads, ws, ms)
        eng.stream.synchronize()
    finally:
        eng.close()
    for other in (b, c):
        assert all(same(x, y) for x, y in zip(other[0], a[0])) and (other[1] == a[1]).all()
        assert all(other[k].tobytes() == a[k].tobytes() for k in (2, 3, 4))
    assert all(same(x, y) for x, y in zip(a[0], host_m(reads, ws, ms)))


# ---------------------------------------------------------------- the Translator's modification weights
# make_weights seed of the synthetic nine-token model of the tests below.  Chosen on the CPU oracle (oracle.ref_cpu
# over the CLI test's windows): its three reads assemble to 43 C / M letters, both kinds; seeds 3, 5, 11, 13 and
# 23 give none
CLI_SEED = 19


def eps(lp):
    """The project's log-prob tolerance (golden_util.logp_close)."""
    return 1e-3 + 1e-5 * abs(float(lp))


def mod_bound(lp_c, lp_m):
    """|d - d_golden| <= eps(lp_c) + eps(lp_m), the logistic's slope is at most 1 / 4, plus one rounding step."""
    return math.ceil(65535.0 * 0.25 * (eps(lp_c) + eps(lp_m))) + 1


def _translator(cfg, eng, **kw):
    from nanodecoder_amd.translator import Translator
    opt = dict(gpu=0, n_best=1, max_length=100, min_length=0, beam_size=1, fast=False, alpha=0.0, beta=0.0,
               batch_size=8)
    opt.update(kw)
    return Translator(cfg, None, types.SimpleNamespace(**opt), engine=eng)


def test_greedy_mod_weights_vs_golden():
    from nanodecoder_amd.engine import Engine, pad_chunks
    z, meta = gu.load("transformer_cpg")
    cfg, W = gu.model_for(meta)
    assert (cfg.itos.index("C"), cfg.itos.index("M")) == (C_ID, M_ID)
    g = meta["greedy"]
    chunks = gu.chunks_of(z)
    eng = Engine(cfg, W, device=0, max_batch=8, max_steps=g["max_length"])
    try:
        tr = _translator(cfg, eng, max_length=g["max_length"], min_length=g.get("min_length", 0))
        (scores, preds, ws, ms), = tr.translate_reads([chunks], batch_size=len(chunks), mods=True)
        (scores0, preds0, ws0), = tr.translate_reads([chunks], batch_size=len(chunks), qualities=True)
        sig, lens = pad_chunks(chunks, int(z["T"]))
        r = eng.translate_greedy(sig, lens, np.full(len(chunks), int(z["T"]), np.int32), max_len=g["max_length"],
                                 min_len=g.get("min_length", 0), return_logp=True)
        mw_all = eng.token_mod_weights(r["tokens"], r["logp"], C_ID, M_ID).cpu().numpy().view(np.uint16)
        tok_all = r["tokens"].cpu().numpy()
    finally:
        eng.close()
    # tokens, strings and quality weights are those of a qualities=True call
    assert preds == preds0 and scores == scores0 and [w.tolist() for w in ws] == [w.tolist() for w in ws0]
    assert (tok_all == z["tokens"]).all()
    # engine level, all 6 x 60 steps
    n_all = 0
    for i, s in np.ndindex(*tok_all.shape):
        t, lc, lm = int(tok_all[i, s]), z["logp"][i, s, C_ID], z["logp"][i, s, M_ID]
        if t not in (C_ID, M_ID):
            assert mw_all[i, s] == 0
            continue
        want, bound = frontend.token_mod_weight(lc, lm, t == M_ID), mod_bound(lc, lm)
        assert abs(int(mw_all[i, s]) - want) <= bound, (i, s, int(mw_all[i, s]), want, bound)
        n_all += 1
    # through the Translator, up to EOS
    n_checked = 0
    for i in range(len(chunks)):
        toks = z["tokens"][i].tolist()
        words = tr._tokens_to_sent(toks)
        assert preds[i][0] == " ".join(words)
        want, bound = [], []
        for s, t in enumerate(toks[: len(words)]):
            lc, lm = z["logp"][i, s, C_ID], z["logp"][i, s, M_ID]
            cm = t in (C_ID, M_ID)
            want += [frontend.token_mod_weight(lc, lm, t == M_ID) if cm else 0] * len(cfg.itos[t])
            bound += [mod_bound(lc, lm) if cm else 0] * len(cfg.itos[t])
            n_checked += cm
        got = ms[i]
        assert got.dtype == np.uint16 and len(got) == len(ws[i]) == len(want)
        diff = np.abs(got.astype(np.int64) - np.asarray(want, np.int64))
        print("cpg", i, "max |mw - mw_golden|", int(diff.max(initial=0)), "bound", max(bound, default=0))
        assert (diff <= np.asarray(bound, np.int64)).all(), (i, diff.tolist(), bound)
    print("cpg: C/M tokens checked, all steps", n_all, "before EOS", n_checked)
    assert n_all >= 100 and n_checked >= 40  # the fixture holds 146 and 49


def test_beam_mod_weights_vs_score_of_the_hypothesis():
    from nanodecoder_amd.engine import Engine, pad_chunks
    z, meta = gu.load("transformer_cpg")
    cfg, W = gu.model_for(meta)
    kw = meta["beam"]
    chunks = gu.chunks_of(z)
    # room for the scoring pass of a hypothesis that ran to max_length without EOS (score() appends one)
    eng = Engine(cfg, W, device=0, max_batch=8, max_steps=kw["max_length"] + 4, max_beam=kw["beam_size"])
    try:
        tr = _translator(cfg, eng, max_length=kw["max_length"], min_length=kw.get("min_length", 0),
                         beam_size=kw["beam_size"], n_best=kw["n_best"], fast=True)
        (scores, preds, ws, ms), = tr.translate_reads([chunks], batch_size=len(chunks), mods=True)
        (scores0, preds0), = tr.translate_reads([chunks], batch_size=len(chunks))
        assert preds == preds0 and scores == scores0
        # a separate scoring pass of each best hypothesis, with its full log-probs
        n_checked = 0
        for i, p in enumerate(preds):
            ids = [cfg.itos.index(w) for w in p[0].split()]
            assert len(ms[i]) == len(ws[i]) == len(ids)
            if not ids:
                continue
            L = min(eng.max_steps, (len(ids) + 1 + 7) // 8 * 8)
            gold = np.full((1, L), cfg.pad_idx, np.int32)
            gold[0, : len(ids)], gold[0, len(ids)] = ids, cfg.eos_idx
            sig, lens = pad_chunks([chunks[i]], int(z["T"]))
            r = eng.score_targets(sig, lens, np.full(1, int(z["T"]), np.int32), gold=torch.from_numpy(gold),
                                  gold_len=torch.tensor([len(ids) + 1], dtype=torch.int32), return_logp=True)
            want = eng.token_mod_weights(torch.from_numpy(gold), r["logp"], C_ID, M_ID).cpu().numpy().view(np.uint16)[0]
            lp = r["logp"].cpu().numpy()[0]
            for s, t in enumerate(ids):
                if t not in (C_ID, M_ID):
                    assert ms[i][s] == 0 == want[s]
                    continue
                bound = mod_bound(lp[s, C_ID], lp[s, M_ID])
                assert abs(int(ms[i][s]) - int(want[s])) <= bound, (i, s, int(ms[i][s]), int(want[s]), bound)
                n_checked += 1
        print("cpg beam: C/M tokens checked", n_checked)
        assert n_checked > 20
    finally:
        eng.close()


def test_raw_reads_arrays_carry_the_same_mod_weights():
    """stream_raw_reads(arrays=True, mods=True): a fifth array, one modification weight per token; spread over
    the characters it is what translate_raw_reads(mods=True) returns per chunk."""
    from nanodecoder_amd import synth
    from nanodecoder_amd.engine import Engine
    cfg = synth.ModelConfig(itos=list(synth.DEFAULT_ITOS) + ["M"])
    eng = Engine(cfg, synth.make_weights(cfg, seed=CLI_SEED, eos_bias=-1.0), device=0, max_batch=8, max_steps=30)
    try:
        tr = _translator(cfg, eng, max_length=30, min_length=4)
        raws = [np.asarray(synth.synth_raw_read(i, n), np.float64) for i, n in enumerate((400, 700))]
        per_read = tr.translate_raw_reads(raws, batch_size=4, src_seq_length=300, src_seq_stride=60, mods=True)
        n_cm = 0
        for ri, tok, sc, w, mw in tr.stream_raw_reads(raws, 4, "median", 300, 60, arrays=True, mods=True):
            assert mw.dtype == np.uint16 and mw.shape == w.shape == tok.shape
            cm = (tok == C_ID) | (tok == M_ID)
            assert not mw[~cm].any()
            n_cm += int(cm.sum())
            for c in range(len(tok)):
                assert tr._char_weights(tok[c].tolist(), mw[c]).tolist() == per_read[ri][3][c].tolist()
                assert tr._char_weights(tok[c].tolist(), w[c]).tolist() == per_read[ri][2][c].tolist()
        assert n_cm > 10
    finally:
        eng.close()


# ---------------------------------------------------------------- translate.py -mod_probs
def test_cli_mod_probs_gpu_assembly_matches_host(tmp_path):
    """-mod_probs -fastq with -assembly cpu against -assembly gpu and -assembly gpu -frontend gpu on a few short
    reads with overlapping windows: the same result/*.mod.fastq, *.fastq and *.fasta bytes."""
    import nanodecoder_amd.translator as T
    from nanodecoder_amd import checkpoint, cli, opts, synth
    built = []
    orig = T.Translator.__init__

    def spy(self, *a, **k):
        orig(self, *a, **k)
        built.append(self.engine)
    cfg = synth.ModelConfig(itos=list(synth.DEFAULT_ITOS) + ["M"])
    W = synth.make_weights(cfg, seed=CLI_SEED, eos_bias=-1.0)
    ck = tmp_path / "m.pt"
    checkpoint.save_synthetic(str(ck), cfg, W)
    src = tmp_path / "reads"
    src.mkdir()
    sizes = (400, 1300, 700)
    for i, n in enumerate(sizes):
        raw = synth.synth_raw_read(i, n)
        (src / f"read{i}.signal").write_text(" ".join(str(int(v)) for v in raw))
    files = {}
    try:
        T.Translator.__init__ = spy
        for m, asm, fe in (("cpu", "cpu", "cpu"), ("gpu", "gpu", "cpu"), ("gpu_fe", "gpu", "gpu")):
            out = tmp_path / ("out_" + m)
            o = opts.parse_translate_opts(["-model", str(ck), "-src_dir", str(src), "-save_data", str(out), "-gpu",
                                           "0", "-beam_size", "1", "-batch_size", "4", "-thread", "2", "-max_length",
                                           "30", "-min_length", "4", "-engine_max_batch", "8", "-engine_lanes", "1",
                                           "-src_seq_length", "300", "-src_seq_stride", "60", "-assembly", asm,
                                           "-frontend", fe, "-fastq", "-mod_probs"])
            assert cli.main(o) == len(sizes)
            files[m] = {f: (out / "result" / f).read_bytes() for f in sorted(os.listdir(out / "result"))}
    finally:
        T.Translator.__init__ = orig
    for e in built:
        e.close()
    assert sorted(files["cpu"]) == sorted(f"read{i}.{ext}" for i in range(len(sizes))
                                          for ext in ("fasta", "fastq", "mod.fastq"))
    for m in ("gpu", "gpu_fe"):
        assert set(files[m]) == set(files["cpu"])
        for name in files["cpu"]:
            assert files[m][name] == files["cpu"][name], (m, name)
    n_cm = 0
    for i in range(len(sizes)):
        fasta = files["cpu"][f"read{i}.fasta"].decode()
        n_cm += sum(fasta.split("\n")[1].count(c) for c in "CM")
        name, seq, qual, vals = parse_record(files["gpu"][f"read{i}.mod.fastq"].decode())
        assert name == f"read{i}" and fasta.split("\n")[1].replace("M", "C") == seq
        assert files["gpu"][f"read{i}.fastq"].decode().split("\n")[3] == qual
        assert len(vals) == seq.count("C")
    print("C / M letters in the -assembly cpu leg's .fasta files:", n_cm)
    assert n_cm >= 10
