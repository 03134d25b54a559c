"""Per-base qualities on the device: nd_token_weights against fp64 numpy, nd_assemble_reads_q against the
host function frontend.assemble_read_q (byte identity) and against nd_assemble_reads (sequence and status),
the Translator's weights on the golden greedy and beam cases, and translate.py -fastq with both assemblies."""
import math
import os
import types

import numpy as np
import pytest
import torch

from nanodecoder_amd import frontend
from tests import golden_util as gu
from tests.test_quality_host import HAND, random_group, random_weights, spaced

pytestmark = pytest.mark.gpu
LEN, STRIDE = 300, 60


# ---------------------------------------------------------------- nd_token_weights
def weights_case(B, S, V, seed):
    """(tokens [B, S] int32, logp [B, S, V] float32) with -inf and NaN entries and token ids -1 and V."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, S, V)) * 2.0
    lp = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)
    tok = rng.integers(0, V, (B, S)).astype(np.int32)
    flat = tok.reshape(-1)
    flat[1], flat[B * S // 2] = -1, V
    lpf = lp.reshape(B * S, V)
    lpf[3, flat[3]] = -np.inf
    lpf[4, flat[4]] = np.nan
    lpf[B * S - 1, flat[B * S - 1]] = 0.0  # probability 1
    return tok, lp


def expected_weights(tok, picked):
    """The definition in fp64 numpy; asserts first that no element sits within 1e-9 of a rounding boundary."""
    ok = (tok >= 0) & np.isfinite(picked)
    y = 65535.0 * np.exp(picked[ok].astype(np.float64))
    assert (np.abs(y - np.floor(y) - 0.5) > 1e-9).all()
    w = np.zeros(tok.shape, np.uint16)
    w[ok] = np.minimum(65535.0, np.floor(y + 0.5)).astype(np.uint16)
    return w


@pytest.mark.parametrize("B,S,V,seed", [(3, 5, 8, 1), (70, 100, 9, 2)])
def test_token_weights_equal_fp64_numpy(B, S, V, seed):
    import ctypes
    from nanodecoder_amd import _lib
    tok, lp = weights_case(B, S, V, seed)
    valid = (tok >= 0) & (tok < V)
    picked = np.where(valid, np.take_along_axis(lp, np.clip(tok, 0, V - 1)[..., None], -1)[..., 0], np.float32(0))
    want = expected_weights(np.where(valid, tok, -1), picked)
    assert want.reshape(-1)[[1, B * S // 2, 3, 4]].tolist() == [0, 0, 0, 0] and want.reshape(-1)[-1] == 65535
    assert len(np.unique(want)) > min(B * S, 1000) // 2
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    tok_d, lp_d, pk_d = (torch.from_numpy(a).to(dev) for a in (tok, lp, picked))
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for name, a, b in (("logp", p(lp_d), None), ("tok_logp", None, p(pk_d))):
        w_d = torch.full((B, S), -1, dtype=torch.int16, device=dev)
        _lib.check(L.nd_token_weights(p(tok_d), a, b, B, S, V, p(w_d), stream), "nd_token_weights")
        got = w_d.cpu().numpy().view(np.uint16)
        assert (got == want).all(), (name, np.argwhere(got != want)[:5])


def test_engine_token_weights_method():
    from nanodecoder_amd import synth
    from nanodecoder_amd.engine import Engine
    cfg = synth.ModelConfig()
    tok, lp = weights_case(3, 5, cfg.vocab, 1)
    eng = Engine(cfg, synth.make_weights(cfg, seed=1), device=0, max_batch=4, max_steps=8)
    try:
        w = eng.token_weights(torch.from_numpy(tok), logp=torch.from_numpy(lp))
        assert w.dtype == torch.int16 and tuple(w.shape) == (3, 5)
        valid = (tok >= 0) & (tok < cfg.vocab)
        picked = np.where(valid, np.take_along_axis(lp, np.clip(tok, 0, cfg.vocab - 1)[..., None], -1)[..., 0], 0)
        assert (w.cpu().numpy().view(np.uint16) == expected_weights(np.where(valid, tok, -1), picked)).all()
        with pytest.raises(ValueError):
            eng.token_weights(torch.from_numpy(tok))
    finally:
        eng.close()


# ---------------------------------------------------------------- nd_assemble_reads_q
def host_q(reads, ws):
    return [frontend.assemble_read_q(p, w, LEN, STRIDE) for p, w in zip(reads, ws)]


def device_raw_q(reads, ws):
    """One nd_assemble_reads_q call and one nd_assemble_reads call on the same input: ((sequence, quality) or
    None where status != 0, status, seq bytes, qual bytes); the plain call's status and seq are asserted
    identical."""
    bases, chunk_off, read_off, kept, qw = frontend.pack_assembly_input(reads, ws)[:5]
    assert kept == []
    seq, seq_len, status, qual = frontend._assemble_device(bases, chunk_off, read_off, 0, qw)[:4]
    seq0, seq_len0, status0 = frontend._assemble_device(bases, chunk_off, read_off, 0)[:3]
    assert (status == status0).all() and (seq_len == seq_len0).all() and seq.tobytes() == seq0.tobytes()
    start = chunk_off[read_off[:-1]]
    end = chunk_off[read_off[1:]]
    out = []
    for r in range(len(reads)):
        assert (seq_len[r] == -1) == (status[r] != 0)
        if status[r]:
            out.append(None)
            continue
        a, n = start[r], seq_len[r]
        assert not qual[a + n: end[r]].any() and qual[a: a + n].max(initial=0) <= 40  # 0 past the read's length
        out.append((seq[a: a + n].tobytes().decode(), frontend.quality_string(qual[a: a + n])))
    return out, status, seq, qual


def test_assemble_q_hand_made_reads():
    reads = [h[1] for h in HAND]
    ws = random_weights(reads, seed=5)
    exp = host_q(reads, ws)
    got, status, _, _ = device_raw_q(reads, ws)
    assert not status.any()
    for (name, _), g, e in zip(HAND, got, exp):
        assert g == e, name
    stats = {}
    assert frontend.assemble_reads(reads, LEN, STRIDE, device=0, stats=stats, weights=ws) == exp
    assert stats == {"reads": len(reads), "fallback": 0}
    # by hand: full weights agree -> 40; 2 to 1 -> 4; 0.99 alone -> 20
    one = [[["A C G T"], ["A C G T"], ["A C G A"]], [["A C G T"], ["G T A A"]]]
    w1 = [[[65535] * 4] * 3, [[65535] * 4, [65535, 65535, 64880, 0]]]
    assert frontend.assemble_reads(one, LEN, STRIDE, device=0, weights=w1) == [("ACGT", "III%"), ("ACGTAA", "IIII5!")]
    # nothing to assemble at all
    assert frontend.assemble_reads([[], [[""]]], LEN, STRIDE, device=0, weights=[[], [[]]]) == [("", ""), ("", "")]


def test_assemble_q_random_group_matches_host():
    reads = random_group()
    ws = random_weights(reads)
    exp = host_q(reads, ws)
    assert [e[0] for e in exp] == [frontend.assemble_read(p, LEN, STRIDE) for p in reads]
    got, status, _, _ = device_raw_q(reads, ws)
    assert not status.any()
    bad = [r for r in range(len(reads)) if got[r] != exp[r]]
    assert not bad, bad
    stats = {}
    assert frontend.assemble_reads(reads, LEN, STRIDE, device=0, stats=stats, weights=ws) == exp
    assert stats == {"reads": 60, "fallback": 0}
    # without weights the call is the one it was
    assert frontend.assemble_reads(reads, LEN, STRIDE, device=0) == [e[0] for e in exp]


def test_assemble_q_fallback_reads_get_their_quality():
    import random
    rng = random.Random(5)
    t = "".join(rng.choice("ACGT") for _ in range(400))
    long_read = [[spaced(t[0:150])], [spaced(t[100:300])], [spaced(t[250:400])]]      # one 200-char chunk
    # an N in the part of the second chunk that lies left of the read (clipped): the host assembles it,
    # the device flags the character
    odd_read = [["A C G G"], ["N T T A C G G C"]]
    plain = [["A C G T A"], ["G T A C C"]]
    reads = [plain, long_read, odd_read, plain]
    ws = random_weights(reads, seed=9)
    got, status, _, _ = device_raw_q(reads, ws)
    assert list(status) == [0, frontend.ASM_STATUS_LONG, frontend.ASM_STATUS_CHAR, 0]
    exp = host_q(reads, ws)
    assert exp[2][0] == "ACGGC" and exp[1][0] == frontend.assemble_read(long_read, LEN, STRIDE)
    assert len(exp[1][1]) == len(exp[1][0]) > 200
    stats = {}
    assert frontend.assemble_reads(reads, LEN, STRIDE, device=0, stats=stats, weights=ws) == exp
    assert stats == {"reads": 4, "fallback": 2}
    assert got[0] == exp[0] and got[3] == exp[3] and got[0][0] == got[3][0] == "ACGTACC"


def test_assemble_q_repeatable_and_stream_independent():
    from nanodecoder_amd import synth
    from nanodecoder_amd.engine import Engine
    reads = random_group(seed=11)[:30]
    ws = random_weights(reads, seed=12)
    a = device_raw_q(reads, ws)
    b = device_raw_q(reads, ws)
    # the non-default stream is an engine context's own, as in tests/test_gpu_assembly.py
    cfg = synth.ModelConfig()
    eng = Engine(cfg, synth.make_weights(cfg, seed=1), device=0, max_batch=4, max_steps=8)
    try:
        assert eng.stream != torch.cuda.default_stream(0)
        with torch.cuda.stream(eng.stream):
            c = device_raw_q(reads, ws)
        eng.stream.synchronize()
    finally:
        eng.close()
    for other in (b, c):
        assert other[0] == a[0] and (other[1] == a[1]).all()
        assert other[2].tobytes() == a[2].tobytes() and other[3].tobytes() == a[3].tobytes()
    assert a[0] == host_q(reads, ws)


# ---------------------------------------------------------------- the Translator's weights
def weight_bound(lp):
    """The project's log-prob tolerance (golden_util.logp_close: 1e-3 + 1e-5 |lp|) carried through exp, plus
    one rounding step."""
    return math.ceil(65535.0 * math.exp(lp) * (math.exp(1e-3 + 1e-5 * abs(lp)) - 1.0)) + 1


def _translator(cfg, eng, **kw):
    from nanodecoder_amd.translator import Translator
    opt = dict(gpu=0, n_best=1, max_length=100, min_length=0, beam_size=1, fast=False, alpha=0.0, beta=0.0,
               batch_size=8)
    opt.update(kw)
    return Translator(cfg, None, types.SimpleNamespace(**opt), engine=eng)


@pytest.mark.parametrize("name", ["transformer_greedy", "transformer_pe_short", "nano_greedy", "transformer_aan",
                                  "transformer_cpg"])
def test_greedy_weights_vs_golden(name):
    from nanodecoder_amd.engine import Engine
    z, meta = gu.load(name)
    cfg, W = gu.model_for(meta)
    g = meta["greedy"]
    chunks = gu.chunks_of(z)
    assert max(len(c) for c in chunks) == int(z["T"])  # the golden run's span is the batch's longest chunk
    eng = Engine(cfg, W, device=0, max_batch=8, max_steps=g["max_length"])
    try:
        tr = _translator(cfg, eng, max_length=g["max_length"], min_length=g.get("min_length", 0))
        (scores, preds, ws), = tr.translate_reads([chunks], batch_size=len(chunks), qualities=True)
        (scores0, preds0), = tr.translate_reads([chunks], batch_size=len(chunks))
        # the same call at the engine: every step's token, past the first EOS too
        from nanodecoder_amd.engine import pad_chunks
        sig, lens = pad_chunks(chunks, int(z["T"]))
        r = eng.translate_greedy(sig, lens, np.full(len(chunks), int(z["T"]), np.int32), max_len=g["max_length"],
                                 min_len=g.get("min_length", 0), return_logp=True)
        w_all = eng.token_weights(r["tokens"], logp=r["logp"]).cpu().numpy().view(np.uint16)
        tok_all = r["tokens"].cpu().numpy()
    finally:
        eng.close()
    assert preds == preds0 and scores == scores0
    assert (tok_all == z["tokens"]).all()
    lp_all = np.take_along_axis(z["logp"], z["tokens"][..., None].astype(np.int64), -1)[..., 0]
    want_all = np.vectorize(frontend.token_weight)(lp_all)
    bound_all = np.vectorize(weight_bound)(lp_all.astype(np.float64))
    diff_all = np.abs(w_all.astype(np.int64) - want_all)
    print(name, "all steps: max |w - w_golden|", int(diff_all.max()), "largest bound", int(bound_all.max()))
    assert (diff_all <= bound_all).all(), np.argwhere(diff_all > bound_all)[:5]
    n_checked = 0
    for i in range(len(chunks)):
        toks = z["tokens"][i].tolist()
        words = tr._tokens_to_sent(toks)
        assert preds[i][0] == " ".join(words)  # the tokens the parity tests pin
        want, bound = [], []
        for s, t in enumerate(toks[: len(words)]):
            lp = float(z["logp"][i, s, t])
            want += [frontend.token_weight(lp)] * len(cfg.itos[t])
            bound += [weight_bound(lp)] * len(cfg.itos[t])
        got = ws[i]
        assert got.dtype == np.uint16 and len(got) == len(preds[i][0].replace(" ", "")) == len(want)
        diff = np.abs(got.astype(np.int64) - np.asarray(want, np.int64))
        print(name, i, "max |w - w_golden|", int(diff.max(initial=0)), "bound", max(bound, default=0))
        assert (diff <= np.asarray(bound, np.int64)).all(), (i, diff.tolist(), bound)
        n_checked += len(want)
    assert n_checked > 0  # these models reach EOS after a few bases; the engine-level check above has every step


def test_beam_weights_vs_score_of_the_hypothesis():
    from nanodecoder_amd.engine import Engine
    z, meta = gu.load("transformer_beam")
    cfg, W = gu.model_for(meta)
    kw = meta["beam"]
    chunks = gu.chunks_of(z)
    # room for the scoring pass of a hypothesis that ran to max_length without EOS (score() appends one)
    eng = Engine(cfg, W, device=0, max_batch=8, max_steps=kw["max_length"] + 4, max_beam=kw["beam_size"])
    try:
        tr = _translator(cfg, eng, max_length=kw["max_length"], min_length=kw.get("min_length", 0),
                         beam_size=kw["beam_size"], n_best=kw["n_best"], fast=True)
        (scores, preds, ws), = tr.translate_reads([chunks], batch_size=len(chunks), qualities=True)
        (scores0, preds0), = tr.translate_reads([chunks], batch_size=len(chunks))
        assert preds == preds0 and scores == scores0
        targets = [p[0] for p in preds]
        scored = tr.score(chunks, targets, batch_size=len(chunks))
        n_checked = 0
        for i, (_, tok_logp) in enumerate(scored):
            n = len(targets[i].split())
            assert len(tok_logp) == n + 1 and len(ws[i]) == n
            if n == 0:
                continue
            ids = torch.tensor([[cfg.itos.index(w) for w in targets[i].split()]], dtype=torch.int32)
            lp = torch.tensor([tok_logp[:n]], dtype=torch.float32)
            want = eng.token_weights(ids, tok_logp=lp).cpu().numpy().view(np.uint16)[0]
            diff = np.abs(ws[i].astype(np.int64) - want.astype(np.int64))
            bound = np.asarray([weight_bound(float(v)) for v in tok_logp[:n]], np.int64)
            print("beam", i, "max |w - w_score|", int(diff.max()), "bound", int(bound.max()))
            assert (diff <= bound).all(), (i, diff.tolist())
            n_checked += n
        assert n_checked > 20
    finally:
        eng.close()


# ---------------------------------------------------------------- translate.py -fastq
def test_cli_fastq_gpu_assembly_matches_host(tmp_path):
    """-fastq with -assembly cpu against -assembly gpu (and the device front end) on a few short reads with
    overlapping windows: the same result/*.fastq and result/*.fasta bytes."""
    import nanodecoder_amd.translator as T
    from nanodecoder_amd import checkpoint, cli, opts, synth
    built = []
    orig = T.Translator.__init__

    def spy(self, *a, **k):
        orig(self, *a, **k)
        built.append(self.engine)
    cfg = synth.ModelConfig()
    W = synth.make_weights(cfg, seed=11, eos_bias=-1.0)
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
                                           "-frontend", fe, "-fastq"])
            assert cli.main(o) == len(sizes)
            files[m] = {f: (out / "result" / f).read_bytes() for f in sorted(os.listdir(out / "result"))}
    finally:
        T.Translator.__init__ = orig
    for e in built:
        e.close()
    assert sorted(files["cpu"]) == sorted(f"read{i}.{ext}" for i in range(len(sizes)) for ext in ("fasta", "fastq"))
    for m in ("gpu", "gpu_fe"):
        assert set(files[m]) == set(files["cpu"])
        for name in files["cpu"]:
            assert files[m][name] == files["cpu"][name], (m, name)
    for i in range(len(sizes)):
        head, seq, plus, qual = files["gpu"][f"read{i}.fastq"].decode().split("\n")[:4]
        assert head == f"@read{i}" and plus == "+" and len(seq) == len(qual)
        assert files["gpu"][f"read{i}.fasta"].decode() == f">read{i}\n{seq}"
    assert any(len(files["gpu"][f"read{i}.fastq"]) > 20 for i in range(len(sizes)))  # not only empty reads
