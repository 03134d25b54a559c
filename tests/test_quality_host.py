"""Per-base qualities on the host (CPU only): the column rule and its table, frontend.assemble_read_q against
assemble_read, the Translator's opt-in with a stand-in engine, translate.py -fastq end to end, and the new
entry points' argument errors."""
import ctypes
import os
import random
import types

import numpy as np
import pytest
import torch

from nanodecoder_amd import checkpoint, cli, frontend, opts, synth
from nanodecoder_amd.translator import Translator
from tests.test_translator_host import FakeEngine, chunks

LEN, STRIDE = 300, 60
M1 = frontend.WEIGHT_ONE


def spaced(s):
    return " ".join(s)


# the kinds of hand-made reads tests/test_gpu_assembly.py lists
HAND = [
    ("no shared char", [["A A A"], ["C C"]]),
    ("nested second chunk", [["A C G T A C"], ["G T"]]),
    ("negative position", [["A C G G"], ["T T T A C G G C"]]),
    ("homopolymer tie", [["A A A A"], ["A A A"]]),
    ("earliest in a before earliest in b", [["A C T G T"], ["G T C A C"]]),
    ("earliest in b", [["T A C"], ["A C G A C"]]),
    ("lower case matches case-sensitively", [["a c g t"], ["A C G T"], ["c g t t"]]),
    ("lower case votes as upper", [["A c G"], ["c G t"]]),
    ("an M base", [["A C M T"], ["C M T T"]]),
    ("single chunk", [["A C G T"]]),
    ("only empty chunks", [[""], [""], [""]]),
    ("zero chunks", []),
    ("empty chunks between", [[""], ["A C G T"], [""], [""], ["G T A A"], [""]]),
    ("three chunks drifting left", [["G G A C"], ["T T G G A"], ["C C T T G"]]),
    ("a two-way tie in a column", [["A C G T"], ["A C G A"]]),
]


def random_group(seed=7):
    """As tests/test_gpu_assembly.py's: about 60 reads, chunk lengths from {1, 2, 63, 64, 65, 128, 199}."""
    rng = random.Random(seed)
    reads = []
    counts = [0, 1, 2, 3, 9, 40]
    for i in range(60):
        alpha = ["A", "AC", "ACGT"][i % 3]
        truth = "".join(rng.choice(alpha) for _ in range(700))
        st = rng.randrange(200, 300)
        preds = []
        for _ in range(counts[(i // 3) % len(counts)]):
            if rng.random() < 0.15:
                preds.append([""])
                continue
            n = rng.choice([1, 2, 63, 64, 65, 128, 199])
            st = max(0, min(len(truth) - n, st + rng.randint(-40, 60)))
            w = [rng.choice(alpha) if rng.random() < 0.07 else ch for ch in truth[st: st + n]]
            preds.append([spaced(w), spaced("ACGT")])
        reads.append(preds)
    return reads


def random_weights(reads, seed=3):
    """Per read, per chunk, one uint16 per base: the whole range, 0 and 65535 included."""
    rng = np.random.default_rng(seed)
    out = []
    for preds in reads:
        ws = []
        for x in preds:
            n = len(x[0].replace(" ", ""))
            w = rng.integers(0, 65536, n).astype(np.uint16)
            w[rng.random(n) < 0.1] = 0
            w[rng.random(n) < 0.3] = 65535
            ws.append(w)
        out.append(ws)
    return out


def test_column_rule_by_hand():
    for (n, S), q in [((1, 65535), 40), ((1, 0), 0), ((1, 64880), 20), ((2, 2 * 64880), 20), ((3, 2 * 65535), 4),
                      ((0, 0), 0)]:
        assert frontend.column_quality(n, S) == q, (n, S)
    got = frontend.column_quality(np.array([1, 1, 3, 0]), np.array([65535, 0, 2 * 65535, 0]))
    assert got.dtype == np.uint8 and got.tolist() == [40, 0, 4, 0]
    # the definition, spelled out: the largest k with float(E) * RATIO[k] <= float(65535 n)
    rng = np.random.default_rng(1)
    seen = set()
    for _ in range(3000):
        n = int(rng.integers(1, 6))
        S = int(rng.integers(0, 65535 * n + 1)) if rng.random() < 0.5 else 65535 * n - int(rng.integers(0, 700))
        e, f = float(65535 * n - S), float(65535 * n)
        want = max(k for k in range(41) if e * frontend.PHRED_RATIO[k] <= f)
        assert frontend.column_quality(n, S) == want, (n, S)
        seen.add(want)
    assert seen == set(range(41))
    assert frontend.quality_string([0, 20, 40]) == "!5I"


def test_table_is_the_powers_of_ten_bit_for_bit():
    want = [10.0 ** (k / 10.0) for k in range(41)]
    assert len(frontend.PHRED_RATIO) == 41
    assert np.asarray(frontend.PHRED_RATIO, np.float64).tobytes() == np.asarray(want, np.float64).tobytes()
    from nanodecoder_amd import _lib, build
    build.build()
    L = _lib.lib()  # loads without a GPU, as in tests/test_abi.py
    out = (ctypes.c_double * 41)()
    assert L.nd_phred_ratios(out, 41) == 0
    assert np.asarray(list(out), np.float64).tobytes() == np.asarray(want, np.float64).tobytes()
    assert L.nd_phred_ratios(out, 42) == _lib.ND_ERR_ARG and L.nd_phred_ratios(None, 4) == _lib.ND_ERR_ARG


def test_token_weight_definition():
    assert frontend.token_weight(0.0) == 65535 and frontend.token_weight(np.log(0.99)) == 64880
    assert frontend.token_weight(-np.inf) == 0 and frontend.token_weight(np.nan) == 0
    assert frontend.token_weight(np.inf) == 0 and frontend.token_weight(3.0) == 65535
    assert frontend.token_weight(-30.0) == 0 and frontend.token_weight(np.float32(-0.5)) == \
        int(np.floor(65535 * np.exp(np.float64(np.float32(-0.5))) + 0.5))


def _check_read(preds, ws, name=""):
    seq, qual = frontend.assemble_read_q(preds, ws, LEN, STRIDE)
    assert seq == frontend.assemble_read(preds, LEN, STRIDE), name
    assert len(qual) == len(seq), name
    assert all(33 <= ord(c) <= 73 for c in qual), name
    return seq, qual


def test_host_function_on_hand_made_reads():
    reads = [h[1] for h in HAND]
    for (name, preds), ws in zip(HAND, random_weights(reads)):
        _check_read(preds, ws, name)
    one = lambda preds, ws: frontend.assemble_read_q(preds, ws, LEN, STRIDE)  # noqa: E731
    assert one([["A C G T"]], [[M1] * 4]) == ("", "")
    # two chunks agree with weight 1: n = 2, S = 2 * 65535 -> 40; where only one votes, its own weight
    assert one([["A C G T"], ["G T A A"]], [[M1] * 4, [M1, M1, 64880, 0]]) == ("ACGTAA", "IIII5!")
    # a column split 2 to 1 with every weight 65535 -> 4; the lone loser's weight does not count
    assert one([["A C G T"], ["A C G T"], ["A C G A"]], [[M1] * 4] * 3) == ("ACGT", "III%")
    # a tie goes to the lowest class, whose weight alone is S: n = 2, S = 64880 -> E / full just above 1 / 2
    seq, qual = one([["A C G T"], ["A C G A"]], [[M1] * 4, [M1, M1, M1, 64880]])
    assert seq == "ACGA" and qual == "III" + chr(33 + frontend.column_quality(2, 64880))
    # negative position: the clipped bases' weights are dropped with them
    assert one([["A C G G"], ["T T T A C G G C"]], [[M1] * 4, [0, 0, 0, M1, M1, M1, M1, 64880]]) == ("ACGGC", "IIII5")
    # what assemble_read raises is raised here, and weights that do not fit the text are refused
    bad = [["A C G T"], ["C G <unk> T"]]
    with pytest.raises(KeyError) as a:
        frontend.assemble_read(bad, LEN, STRIDE)
    with pytest.raises(KeyError) as b:
        one(bad, [[1] * 4, [1] * 8])
    assert a.value.args == b.value.args
    with pytest.raises(ValueError):
        one([["A C G T"], ["G T A"]], [[1] * 4, [1] * 2])
    with pytest.raises(ValueError):
        one([["A C G T"], ["G T A"]], [[1] * 4])


def test_host_function_on_a_random_group():
    reads = random_group()
    ws = random_weights(reads)
    seen = set()
    n_bases = 0
    for r, (preds, w) in enumerate(zip(reads, ws)):
        seq, qual = _check_read(preds, w, r)
        seen.update(qual)
        n_bases += len(seq)
    assert n_bases > 4000 and len(seen) > 20  # the fixture is not trivial: many bases, most quality levels
    # the group function without a device is the host function per read
    assert frontend.assemble_reads(reads, LEN, STRIDE, device=None, weights=ws) == \
        [frontend.assemble_read_q(p, w, LEN, STRIDE) for p, w in zip(reads, ws)]
    assert frontend.assemble_reads(reads, LEN, STRIDE, device=None) == \
        [frontend.assemble_read(p, LEN, STRIDE) for p in reads]


def test_host_function_in_the_concatenation_branch():
    preds = [["A C G"], [""], ["T T", "A"], ["m"]]
    ws = [[65535, 64880, 0], [], [1, 40000], [65000]]
    seq, qual = frontend.assemble_read_q(preds, ws, 512, 512)
    assert seq == frontend.assemble_read(preds, 512, 512) == "ACGTTm"
    flat = [65535, 64880, 0, 1, 40000, 65000]
    assert qual == "".join(chr(33 + frontend.column_quality(1, w)) for w in flat)
    assert qual[:3] == "I5!"
    assert frontend.assemble_reads([preds], 512, 512, device=0, weights=[ws]) == [(seq, qual)]  # no device call
    with pytest.raises(ValueError):
        frontend.assemble_read_q(preds, [[1] * 3, [], [1], [1]], 512, 512)


def test_pack_assembly_input_with_weights():
    reads = [[["A C"], [""], ["G G T"]], [["é"]], [["T"]]]
    ws = [[[1, 2], [], [3, 4, 65535]], [[7]], [[9]]]
    plain = frontend.pack_assembly_input(reads)
    bases, chunk_off, read_off, host, qw = frontend.pack_assembly_input(reads, ws)[:5]
    assert plain.qw is None and host == plain.host == [1]
    assert bases.tobytes() == plain.bases.tobytes() == b"ACGGTT"
    assert (chunk_off == plain.chunk_off).all() and (read_off == plain.read_off).all()
    assert qw.dtype == np.uint16 and qw.tolist() == [1, 2, 3, 4, 65535, 9]
    with pytest.raises(ValueError):
        frontend.pack_assembly_input(reads, [[[1, 2], [], [3, 4]], [[7]], [[9]]])


# ---------------------------------------------------------------- Translator with a stand-in engine
def known_logp(B, S, V):
    b, s, v = np.meshgrid(np.arange(B), np.arange(S), np.arange(V), indexing="ij")
    return (-0.003 * b - 0.02 * s - 0.11 * v).astype(np.float32)


class QualityEngine(FakeEngine):
    """FakeEngine that also takes return_logp (a known logp) and weighs tokens on the host."""

    def translate_greedy(self, sig, L, S, max_len, min_len=0, return_attn=False, return_logp=False):
        out = super().translate_greedy(sig, L, S, max_len, min_len, return_attn)
        self.calls[-1] = self.calls[-1] + (("return_logp", True),) if return_logp else self.calls[-1]
        if return_logp:
            out["logp"] = torch.from_numpy(known_logp(len(L), max_len, 8))
        return out

    def translate_sample(self, sig, L, S, temp, keep_topk, seed, max_len, min_len=0, return_attn=False,
                         return_logp=False):
        out = self.translate_greedy(sig, L, S, max_len, min_len, return_attn, return_logp)
        self.calls[-1] = ("sample",) + self.calls[-1][1:]
        return out

    def token_weights(self, tokens, logp=None, tok_logp=None):
        tok = tokens.numpy()
        w = np.zeros(tok.shape, np.uint16)
        for i in np.ndindex(*tok.shape):
            if 0 <= tok[i] < 8:
                w[i] = frontend.token_weight(logp.numpy()[i + (tok[i],)] if tok_logp is None else tok_logp.numpy()[i])
        return torch.from_numpy(w.view(np.int16))


def make_tr(engine_cls, **over):
    opt = dict(gpu=0, n_best=1, max_length=10, min_length=0, beam_size=1, random_sampling_temp=1.0,
               random_sampling_topk=1, block_ngram_repeat=0, dump_beam="", replace_unk=False, verbose=False,
               fast=False, alpha=0.0, beta=0.0, batch_size=3)
    opt.update(over)
    eng = engine_cls()
    return Translator(synth.ModelConfig(), None, types.SimpleNamespace(**opt), engine=eng), eng


def test_translator_weights_line_up_with_the_strings():
    reads = [chunks([512, 512, 77], seed=1), chunks([512, 300], seed=2), chunks([60], seed=3)]
    tr, eng = make_tr(QualityEngine)
    got = tr.translate_reads(reads, batch_size=2, qualities=True)
    tr0, eng0 = make_tr(FakeEngine)
    plain = tr0.translate_reads(reads, batch_size=2)
    assert [g[:2] for g in got] == plain  # scores and strings are today's
    assert len(eng.calls) == 1 and eng.calls[0][-1] == ("return_logp", True)
    lp = known_logp(8, 10, 8)
    row = 0
    for (sc, preds, ws), read in zip(got, reads):
        assert len(ws) == len(preds) == len(read)
        for p, w in zip(preds, ws):
            s = p[0].replace(" ", "")
            assert w.dtype == np.uint16 and len(w) == len(s) == 3  # FakeEngine: three bases, then EOS
            toks = [synth.DEFAULT_ITOS.index(c) for c in s]
            assert w.tolist() == [frontend.token_weight(lp[row, t, tok]) for t, tok in enumerate(toks)]
            row += 1
    # the generator carries the same weights per chunk, as its third entry
    tr, eng = make_tr(QualityEngine)
    for ri, res in tr.stream_reads(reads, 2, qualities=True):
        assert [r[2].tolist() for r in res] == [w.tolist() for w in got[ri][2]]
    # sampling takes the same path
    tr, eng = make_tr(QualityEngine, random_sampling_topk=3, random_sampling_temp=0.7, seed=5)
    smp = tr.translate_reads(reads, batch_size=2, qualities=True)
    assert eng.calls[0][0] == "sample" and [w.tolist() for w in smp[0][2]] == [w.tolist() for w in got[0][2]]


def test_translator_default_is_unchanged():
    reads = [chunks([512, 512, 77], seed=1), chunks([512, 300], seed=2)]
    # FakeEngine takes no return_logp and has no token_weights: the default path never asks for either
    tr0, eng0 = make_tr(FakeEngine)
    plain = tr0.translate_reads(reads, batch_size=2)
    tr, eng = make_tr(QualityEngine)
    same = tr.translate_reads(reads, batch_size=2)
    assert same == plain and all(len(r) == 2 for r in same)
    assert len(eng.calls) == len(eng0.calls) == 1
    for a, b in zip(eng.calls[0], eng0.calls[0]):
        assert np.array_equal(a, b)
    assert [r for _, r in tr.stream_reads(reads, 2)] == [r for _, r in tr0.stream_reads(reads, 2)]
    assert tr.translate(reads[0], batch_size=2) == tr0.translate(reads[0], batch_size=2)
    # refusals: with attention dumps, and beam search on an average-attention decoder
    with pytest.raises(ValueError):
        tr.translate_reads(reads, batch_size=2, attn_debug=True, qualities=True)
    cfg = synth.ModelConfig(self_attn_type="average")
    opt = types.SimpleNamespace(gpu=0, n_best=1, max_length=10, beam_size=4, fast=True, batch_size=2)
    aan = Translator(cfg, None, opt, engine=QualityEngine())
    with pytest.raises(NotImplementedError):
        aan.translate_reads(reads, batch_size=2, qualities=True)
    aan.translate_reads(reads, batch_size=2)  # without qualities it decodes as before


class OverflowEngine(QualityEngine):
    """Flags the split-fp16 range guard until exact fp32 is on; the exact rerun's log-probs are shifted."""

    exact = False

    def set_exact_fp32(self, on):
        self.exact = bool(on)

    def translate_greedy(self, *a, **k):
        out = super().translate_greedy(*a, **k)
        out["overflow"] = torch.tensor([0 if self.exact else 1], dtype=torch.int32)
        if self.exact and out["logp"] is not None:
            out["logp"] = out["logp"] - 0.5
        return out


def test_overflow_rerun_carries_the_request():
    reads = [chunks([512, 300], seed=2)]
    tr, eng = make_tr(OverflowEngine)
    (sc, preds, ws), = tr.translate_reads(reads, batch_size=2, qualities=True)
    assert [c[0] for c in eng.calls] == ["greedy", "greedy"] and eng.exact is False
    assert all(c[-1] == ("return_logp", True) for c in eng.calls)
    lp = known_logp(8, 10, 8) - np.float32(0.5)  # the rerun's weights replace the flagged call's
    for row, (p, w) in enumerate(zip(preds, ws)):
        toks = [synth.DEFAULT_ITOS.index(c) for c in p[0].replace(" ", "")]
        assert w.tolist() == [frontend.token_weight(lp[row, t, tok]) for t, tok in enumerate(toks)]


# ---------------------------------------------------------------- translate.py -fastq
class _Eng(QualityEngine):
    def __init__(self, cfg, W, device=0, max_batch=8, max_src_len=512, max_steps=100, max_beam=1):
        super().__init__(max_batch=max_batch, max_src_len=max_src_len)


@pytest.mark.parametrize("window", [("512", "512"), ("300", "100")])
def test_cli_fastq_end_to_end(tmp_path, monkeypatch, window):
    import nanodecoder_amd.translator as T
    monkeypatch.setattr(T, "Engine", _Eng)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    cfg = synth.ModelConfig()
    ck = tmp_path / "m.pt"
    checkpoint.save_synthetic(str(ck), cfg, synth.make_weights(cfg, seed=1))
    src = tmp_path / "reads"
    src.mkdir()
    for i, n in enumerate((1300, 700, 400)):
        raw = synth.synth_raw_read(i, n)
        (src / f"read{i}.signal").write_text(" ".join(str(int(v)) for v in raw))
    files = {}
    for mode in ("plain", "fastq"):
        out = tmp_path / mode
        argv = ["-model", str(ck), "-src_dir", str(src), "-save_data", str(out), "-gpu", "0", "-beam_size", "1",
                "-batch_size", "2", "-thread", "2", "-max_length", "10", "-pack_reads", "2", "-src_seq_length",
                window[0], "-src_seq_stride", window[1]] + (["-fastq"] if mode == "fastq" else [])
        assert cli.main(opts.parse_translate_opts(argv)) == 3
        files[mode] = {os.path.join(d, f): (out / d / f).read_bytes() for d in ("result", "segment")
                       for f in sorted(os.listdir(out / d))}
        files[mode]["speed names"] = [ln.split("\t")[0] for ln in (out / "speed.txt").read_text().splitlines()]
    fq = {k: v for k, v in files["fastq"].items() if str(k).endswith(".fastq")}
    assert len(fq) == 3 and not any(str(k).endswith(".fastq") for k in files["plain"])
    assert {k: v for k, v in files["fastq"].items() if k not in fq} == files["plain"]
    some = False
    for k, v in fq.items():
        name = os.path.basename(k)[: -len(".fastq")]
        text = v.decode("ascii")
        assert text.endswith("\n") and text.count("\n") == 4
        head, seq, plus, qual = text.split("\n")[:4]
        assert head == "@" + name and plus == "+" and len(qual) == len(seq)
        assert all(33 <= ord(c) <= 73 for c in qual)
        assert files["plain"][os.path.join("result", name + ".fasta")].decode() == ">%s\n%s" % (name, seq)
        some = some or len(seq) > 0
    assert some


def test_cli_fastq_refuses_attn_debug(tmp_path):
    o = opts.parse_translate_opts(["-model", "m.pt", "-src_dir", str(tmp_path), "-save_data", str(tmp_path / "o"),
                                   "-gpu", "0", "-fastq", "-attn_debug"])
    assert o.fastq is True
    with pytest.raises(ValueError):
        cli.main(o)
    assert opts.parse_translate_opts(["-model", "m.pt", "-src_dir", "x", "-save_data", "y"]).fastq is False


# ---------------------------------------------------------------- argument errors, no device
def test_new_entry_points_argument_errors_without_gpu():
    from nanodecoder_amd import _lib, build
    build.build()
    L = _lib.lib()
    ERR = _lib.ND_ERR_ARG
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before any HIP call
    # nd_token_weights
    assert L.nd_token_weights(None, p, None, 2, 3, 8, p, None) == ERR
    assert L.nd_token_weights(p, p, None, 2, 3, 8, None, None) == ERR
    assert L.nd_token_weights(p, None, None, 2, 3, 8, p, None) == ERR  # neither log-prob input
    assert b"exactly one" in L.nd_last_error()
    assert L.nd_token_weights(p, p, p, 2, 3, 8, p, None) == ERR  # both
    assert L.nd_token_weights(p, p, None, -1, 3, 8, p, None) == ERR
    assert L.nd_token_weights(p, None, p, 2, -3, 8, p, None) == ERR
    assert L.nd_token_weights(p, None, p, 2, 3, 0, p, None) == ERR
    assert L.nd_token_weights(p, None, p, 70000, 70000, 8, p, None) == ERR
    assert L.nd_token_weights(None, None, p, 0, 5, 8, None, None) == 0  # nothing to do
    # nd_assemble_reads_q
    need = L.nd_assemble_reads_q_work_bytes(3, 100)
    assert need == L.nd_assemble_reads_work_bytes(3, 100) + 5 * 100 * 8 == 2 * 3 * 4 + 5 * 100 * 4 + 5 * 100 * 8
    assert L.nd_assemble_reads_q_work_bytes(0, 0) == 0 and L.nd_assemble_reads_q_work_bytes(-1, 5) < 0
    q = lambda *a: L.nd_assemble_reads_q(*a)  # noqa: E731
    assert q(None, None, None, None, 2, 3, 100, None, None, None, None, None, need, None) == ERR
    assert q(p, None, p, p, 2, 3, 100, p, p, p, p, p, need, None) == ERR  # no weights
    assert q(p, p, p, p, 2, 3, 100, p, None, p, p, p, need, None) == ERR  # no quality output
    assert q(p, p, p, p, 2, 3, 100, p, p, p, p, None, need, None) == ERR  # no work buffer
    assert q(p, p, p, p, 2, 3, 100, p, p, p, p, p, need - 1, None) == ERR
    assert b"work_bytes" in L.nd_last_error()
    assert q(p, p, p, p, 2, 3, 100, p, p, p, p, p, L.nd_assemble_reads_work_bytes(3, 100), None) == ERR
    assert q(p, p, p, p, -1, 3, 100, p, p, p, p, p, need, None) == ERR
    assert q(p, p, p, p, 2, -3, 100, p, p, p, p, p, need, None) == ERR
    assert q(p, p, p, p, 2, 3, 2 ** 31, p, p, p, p, p, 2 ** 40, None) == ERR
    assert q(None, None, p, p, 0, 0, 0, None, None, None, None, None, 0, None) == 0  # R == 0: at once
