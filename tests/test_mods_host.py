"""Per-base methylation probabilities on the host (CPU only): the token rule and its edge cases, the column
rule, frontend.assemble_read_m against assemble_read_q and against values worked out by hand, the .mod.fastq
record, the new entry points' argument errors, the Translator's opt-in with a stand-in engine and translate.py
-mod_probs end to end."""
import ctypes
import math
import os
import random
import types

import numpy as np
import pytest
import torch

from nanodecoder_amd import checkpoint, cli, frontend, opts, synth
from nanodecoder_amd.translator import Translator
from tests.test_quality_host import HAND, random_group, random_weights, spaced
from tests.test_translator_host import FakeEngine, chunks

LEN, STRIDE = 300, 60
M1 = frontend.WEIGHT_ONE
ITOS9 = list(synth.DEFAULT_ITOS) + ["M"]
C_ID, M_ID = ITOS9.index("C"), ITOS9.index("M")


def ml_of(n_cm, W):
    """The column rule, spelled out on Python integers."""
    return min(255, (256 * W) // (65535 * n_cm))


# the hand-made reads of the issue: (name, predictions, weights, modification weights, sequence, ml)
HAND_M = [
    # column 1: a C vote (mw 100) against an M vote (mw 65000): the tie goes to the lower class, C, and the site
    # still carries both votes: (256 * 65100) // (65535 * 2) = 127
    ("a 1:1 C/M tie", [["A C G T"], ["A M G T"]], [[M1] * 4] * 2, [[0, 100, 0, 0], [0, 65000, 0, 0]],
     "ACGT", [0, ml_of(2, 65100), 0, 0]),
    # column 1: one C vote, one M vote, three G votes: the call is G, no site, although C / M votes came in
    ("C/M votes that lose", [["A C G T"], ["A M G T"], ["A G G T"], ["A G G T"], ["A G G T"]], [[M1] * 4] * 5,
     [[0, 65535, 0, 0], [0, 65535, 0, 0], [0] * 4, [0] * 4, [0] * 4], "AGGT", [0, 0, 0, 0]),
    # the second chunk sits at position -3: its first three bases (an M of full weight among them) are clipped
    # with their weights; column 1 gets C (mw 10) and C (mw 30000), column 4 the lone M (mw 65535)
    ("negative position", [["A C G G"], ["T M T A C G G M"]], [[M1] * 4, [M1] * 8],
     [[0, 10, 0, 0], [0, 65535, 0, 0, 30000, 0, 0, 65535]], "ACGGM", [0, ml_of(2, 30010), 0, 0, 255]),
    # M wins 2:1 over C: a site called M, all three votes count
    ("M outvotes C", [["A M T"], ["A M T"], ["A C T"]], [[M1] * 3] * 3,
     [[0, 60000, 0], [0, 50000, 0], [0, 2000, 0]], "AMT", [0, ml_of(3, 112000), 0]),
    ("no C or M", [["A G T A"], ["G T A A"]], [[M1] * 4] * 2, [[7] * 4, [9] * 4], "AGTAA", [0] * 5),
    ("no chunks", [], [], [], "", []),
    ("only empty chunks", [[""], [""]], [[], []], [[], []], "", []),
    ("a single chunk assembles to nothing", [["A C M T"]], [[M1] * 4], [[0, 1, 2, 0]], "", []),
]


def test_token_mod_weight_against_the_fp64_formula():
    rng = np.random.default_rng(4)
    lp = (rng.normal(size=(4000, 2)) * 4.0 - 3.0).astype(np.float32)
    seen = set()
    for a, b in lp:
        d = np.float64(a) - np.float64(b)
        want = int(min(65535.0, np.floor(65535.0 * (1.0 / (1.0 + np.exp(d))) + 0.5)))
        for is_mod in (False, True):
            assert frontend.token_mod_weight(a, b, is_mod) == want, (a, b)
        seen.add(want)
    assert len(seen) > 1500 and 0 in seen and 65535 in seen
    assert frontend.token_mod_weight(-1.0, -1.0, False) == 32768  # p = 1 / 2: floor(32767.5 + 0.5)
    # float64 inputs are rounded to float32 first, as the device reads them
    assert frontend.token_mod_weight(-0.1 - 1e-12, -2.0, False) == frontend.token_mod_weight(np.float32(-0.1), -2.0, True)


def test_token_mod_weight_edge_cases():
    inf, nan = math.inf, math.nan
    one = frontend.token_mod_weight
    for is_mod in (False, True):
        assert one(0.0, -inf, is_mod) == 0        # d = +inf
        assert one(-inf, 0.0, is_mod) == M1       # d = -inf
        assert one(inf, 0.0, is_mod) == 0 and one(0.0, inf, is_mod) == M1
        assert one(-40.0, 0.0, is_mod) == M1      # p = 1 in fp64: 1 + exp(-40) == 1
        assert one(-30.0, 0.0, is_mod) == M1 and one(0.0, -30.0, is_mod) == 0
        assert one(2000.0, -2000.0, is_mod) == 0  # exp overflows to +inf
    # a NaN d falls back to the hard call
    for lp_c, lp_m in ((nan, 0.0), (0.0, nan), (nan, nan), (-inf, -inf), (inf, inf)):
        assert one(lp_c, lp_m, True) == M1 and one(lp_c, lp_m, False) == 0


def test_column_ml_rule():
    for n in (1, 2, 3, 17, 2 ** 31 - 1):
        assert frontend.column_ml(n, 0) == 0 and frontend.column_ml(n, M1 * n) == 255
    assert frontend.column_ml(0, 0) == 0
    assert frontend.column_ml(1, 32768) == 128 and frontend.column_ml(1, 32767) == 127
    assert frontend.column_ml(1, 65280) == 255 and frontend.column_ml(1, 65279) == 254
    got = frontend.column_ml(np.array([1, 2, 0, 3]), np.array([M1, M1, 0, 0]))
    assert got.dtype == np.uint8 and got.tolist() == [255, 128, 0, 0]  # (256 * 65535) // (65535 * 2) = 128
    rng = np.random.default_rng(2)
    for n in (1, 2, 5):
        W = np.sort(rng.integers(0, M1 * n + 1, 3000))
        ml = frontend.column_ml(np.full(W.size, n), W)
        assert (np.diff(ml.astype(int)) >= 0).all()  # monotone in W
        assert ml.tolist() == [ml_of(n, int(w)) for w in W]
        assert len(set(ml.tolist())) > 200


def random_mod_weights(reads, seed=13):
    return random_weights(reads, seed=seed)


def random_group_m(seed=17, n_reads=42):
    """As tests/test_quality_host.py's random_group with C and M in every alphabet: about 40 reads of 0 to 40
    chunks, chunk lengths from {1, 2, 63, 64, 65, 128, 199}, some chunks empty."""
    rng = random.Random(seed)
    reads = []
    counts = [0, 1, 2, 3, 9, 40]
    for i in range(n_reads):
        alpha = ["CM", "ACM", "ACGTM"][i % 3]
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


def _check_read(preds, ws, ms, length, stride, name=""):
    seq, qual, ml = frontend.assemble_read_m(preds, ws, ms, length, stride)
    assert (seq, qual) == frontend.assemble_read_q(preds, ws, length, stride), name
    assert ml.dtype == np.uint8 and ml.shape == (len(seq),), name
    off = np.array([c not in "CMcm" for c in seq], bool)
    assert not ml[off].any(), name
    return seq, qual, ml


def test_assemble_read_m_by_hand():
    for name, preds, ws, ms, seq, ml in HAND_M:
        got = _check_read(preds, ws, ms, LEN, STRIDE, name)
        assert got[0] == seq and got[2].tolist() == ml, (name, got)
    assert ml_of(2, 65100) == 127 and ml_of(2, 30010) == 58 and ml_of(3, 112000) == 145
    # the tie's column is called C and yet carries more than the hard call would: the sequence is never changed
    tie = frontend.assemble_read_m([["A C"], ["A M"]], [[M1] * 2] * 2, [[0, 65535], [0, 65535]], LEN, STRIDE)
    assert tie[0] == "AC" and tie[2].tolist() == [0, 255]
    # weights that do not fit the text are refused, and what assemble_read raises is raised here
    with pytest.raises(ValueError):
        frontend.assemble_read_m([["A C G T"], ["G T A"]], [[1] * 4, [1] * 3], [[1] * 4, [1] * 2], LEN, STRIDE)
    with pytest.raises(ValueError):
        frontend.assemble_read_m([["A C G T"], ["G T A"]], [[1] * 4, [1] * 3], [[1] * 4], LEN, STRIDE)
    with pytest.raises(KeyError):
        frontend.assemble_read_m([["A C G T"], ["C G <unk> T"]], [[1] * 4, [1] * 8], [[1] * 4, [1] * 8], LEN, STRIDE)


def test_assemble_read_m_on_the_quality_fixtures():
    reads = [h[1] for h in HAND] + random_group()[:20] + random_group_m()
    ws, ms = random_weights(reads), random_mod_weights(reads)
    sites, seen = 0, set()
    for r, (preds, w, m) in enumerate(zip(reads, ws, ms)):
        seq, _, ml = _check_read(preds, w, m, LEN, STRIDE, r)
        sites += sum(c in "CM" for c in seq)
        seen.update(ml[[c in "CM" for c in seq]].tolist())
    assert sites > 2000 and len(seen) > 200  # the fixture is not trivial: many sites, most ML levels
    # the group function without a device is the host function per read
    got = frontend.assemble_reads(reads, LEN, STRIDE, device=None, weights=ws, mod_weights=ms)
    for g, (preds, w, m) in zip(got, zip(reads, ws, ms)):
        e = frontend.assemble_read_m(preds, w, m, LEN, STRIDE)
        assert g[:2] == e[:2] and g[2].tobytes() == e[2].tobytes()
    with pytest.raises(ValueError):
        frontend.assemble_reads(reads, LEN, STRIDE, device=None, mod_weights=ms)


def test_assemble_read_m_in_the_concatenation_branch():
    preds = [["A C M"], [""], ["T C", "A"], ["m"]]
    ws = [[65535, 64880, 0], [], [1, 40000], [65000]]
    ms = [[500, 100, 65535], [], [65535, 32768], [65279]]
    seq, qual, ml = _check_read(preds, ws, ms, 512, 512)
    assert seq == "ACMTCm"
    # every base is its own column: n_cm = 1, W = its own weight; A and T get 0 whatever their weight
    assert ml.tolist() == [0, ml_of(1, 100), 255, 0, 128, 254]
    got, = frontend.assemble_reads([preds], 512, 512, device=0, weights=[ws], mod_weights=[ms])  # no device call
    assert got[:2] == (seq, qual) and got[2].tolist() == ml.tolist()
    assert frontend.assemble_read_m([], [], [], 512, 512)[2].shape == (0,)
    with pytest.raises(ValueError):
        frontend.assemble_read_m(preds, ws, [[1] * 3, [], [1], [1]], 512, 512)


def test_pack_assembly_input_with_mod_weights():
    reads = [[["A C"], [""], ["G M T"]], [["é"]], [["T"]]]
    ws = [[[1, 2], [], [3, 4, 65535]], [[7]], [[9]]]
    ms = [[[5, 6], [], [7, 65535, 0]], [[1]], [[2]]]
    five = frontend.pack_assembly_input(reads, ws)
    six = frontend.pack_assembly_input(reads, ws, ms)
    assert five.qw is not None and five.mw is None and five.bp is None and six.bp is None
    for a, b in zip(five[:5], six[:5]):
        assert np.array_equal(a, b)
    assert six.mw.dtype == np.uint16 and six.mw.tolist() == [5, 6, 7, 65535, 0, 2]
    with pytest.raises(ValueError):
        frontend.pack_assembly_input(reads, ws, [[[5, 6], [], [7, 8]], [[1]], [[2]]])
    with pytest.raises(ValueError):
        frontend.pack_assembly_input(reads, None, ms)


def parse_record(text):
    """(name, sequence, quality, ML list) of a .mod.fastq record; asserts its form."""
    assert text.endswith("\n") and text.count("\n") == 4
    head, seq, plus, qual = text.split("\n")[:4]
    assert head.startswith("@") and plus == "+" and len(qual) == len(seq) and "M" not in seq
    fields = head[1:].split("\t")
    if len(fields) == 1:
        assert seq.count("C") == 0
        return fields[0], seq, qual, []
    name, mm, mlf = fields
    assert mm.startswith("MM:Z:C+m.") and mm.endswith(";") and mlf.startswith("ML:B:C")
    skips = mm[len("MM:Z:C+m."):-1].split(",")[1:]
    vals = [int(v) for v in mlf[len("ML:B:C"):].split(",")[1:]]
    assert skips == ["0"] * len(vals) and len(vals) == seq.count("C") > 0
    assert all(0 <= v <= 255 for v in vals)
    return name, seq, qual, vals


def test_mod_fastq_record():
    text = frontend.mod_fastq_record("read7", "ACMTCG", "I5!I5!", [0, 3, 255, 0, 128, 0])
    assert text == "@read7\tMM:Z:C+m.,0,0,0;\tML:B:C,3,255,128\nACCTCG\n+\nI5!I5!\n"
    assert parse_record(text) == ("read7", "ACCTCG", "I5!I5!", [3, 255, 128])
    assert frontend.mod_fastq_record("r", "AGT", "III", [0, 0, 0]) == "@r\nAGT\n+\nIII\n"
    assert frontend.mod_fastq_record("r", "", "", []) == "@r\n\n+\n\n"
    with pytest.raises(ValueError):
        frontend.mod_fastq_record("r", "ACG", "III", [0, 1])
    for name, preds, ws, ms, seq, ml in HAND_M:
        got = frontend.assemble_read_m(preds, ws, ms, LEN, STRIDE)
        rec = parse_record(frontend.mod_fastq_record("x", *got))
        assert rec[1] == seq.replace("M", "C") and rec[3] == [v for c, v in zip(seq, ml) if c in "CM"]


# ---------------------------------------------------------------- argument errors, no device
def test_new_entry_points_argument_errors_without_gpu():
    from nanodecoder_amd import _lib, build
    build.build()
    L = _lib.lib()
    ERR = _lib.ND_ERR_ARG
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before any HIP call
    t = L.nd_token_mod_weights
    assert t(None, p, 2, 3, 9, 5, 8, p, None) == ERR
    assert t(p, None, 2, 3, 9, 5, 8, p, None) == ERR
    assert t(p, p, 2, 3, 9, 5, 8, None, None) == ERR
    assert b"null buffer" in L.nd_last_error()
    assert t(p, p, -1, 3, 9, 5, 8, p, None) == ERR
    assert t(p, p, 2, -3, 9, 5, 8, p, None) == ERR
    assert t(p, p, 2, 3, 0, 0, 0, p, None) == ERR
    assert t(p, p, 70000, 70000, 9, 5, 8, p, None) == ERR
    assert t(p, p, 2, 3, 9, -1, 8, p, None) == ERR
    assert t(p, p, 2, 3, 9, 5, 9, p, None) == ERR
    assert t(p, p, 2, 3, 9, 9, 5, p, None) == ERR
    assert t(p, p, 2, 3, 9, 5, 5, p, None) == ERR
    assert b"two different ids" in L.nd_last_error()
    assert t(None, None, 0, 5, 9, 5, 8, None, None) == 0  # nothing to do
    need = L.nd_assemble_reads_m_work_bytes(3, 100)
    assert need == L.nd_assemble_reads_q_work_bytes(3, 100) + 100 * 8
    assert L.nd_assemble_reads_m_work_bytes(0, 0) == 0 and L.nd_assemble_reads_m_work_bytes(-1, 5) < 0
    assert L.nd_assemble_reads_m_work_bytes(3, -5) < 0
    m = L.nd_assemble_reads_m
    assert m(None, None, None, None, None, 2, 3, 100, None, None, None, None, None, None, need, None) == ERR
    for hole in (0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13):  # each buffer in turn
        a = [p, p, p, p, p, 2, 3, 100, p, p, p, p, p, p, need, None]
        a[hole] = None
        assert m(*a) == ERR, hole
        assert b"null buffer" in L.nd_last_error()
    assert m(p, p, p, p, p, 2, 3, 100, p, p, p, p, p, p, need - 1, None) == ERR
    assert b"work_bytes" in L.nd_last_error()
    assert m(p, p, p, p, p, 2, 3, 100, p, p, p, p, p, p, L.nd_assemble_reads_q_work_bytes(3, 100), None) == ERR
    assert m(p, p, p, p, p, -1, 3, 100, p, p, p, p, p, p, need, None) == ERR
    assert m(p, p, p, p, p, 2, -3, 100, p, p, p, p, p, p, need, None) == ERR
    assert m(p, p, p, p, p, 2, 3, -100, p, p, p, p, p, p, need, None) == ERR
    assert m(p, p, p, p, p, 2, 3, 2 ** 31, p, p, p, p, p, p, 2 ** 40, None) == ERR
    assert m(None, None, None, p, p, 0, 0, 0, None, None, None, None, None, None, 0, None) == 0  # R == 0: at once


# ---------------------------------------------------------------- Translator with a stand-in engine
def known_logp9(B, S):
    b, s, v = np.meshgrid(np.arange(B), np.arange(S), np.arange(9), indexing="ij")
    return (-0.003 * b - 0.02 * s - 0.11 * v + 0.9 * ((b + s) % 3) * (v == M_ID)).astype(np.float32)


class ModEngine(FakeEngine):
    """FakeEngine over the nine-token vocabulary: the second token of a row is M for odd spans, C for even, the
    third always C; takes return_logp (a known logp) and weighs tokens on the host."""

    def _tok(self, L, S, n):
        row = [4 + (L % 4), M_ID if S % 2 else C_ID, C_ID, 3] + [6] * (n - 4)
        return row[:n]

    def translate_greedy(self, sig, L, S, max_len, min_len=0, return_attn=False, return_logp=False):
        out = super().translate_greedy(sig, L, S, max_len, min_len, return_attn)
        self.calls[-1] = self.calls[-1] + (("return_logp", True),) if return_logp else self.calls[-1]
        if return_logp:
            out["logp"] = torch.from_numpy(known_logp9(len(L), max_len))
        return out

    def translate_sample(self, sig, L, S, temp, keep_topk, seed, max_len, min_len=0, return_attn=False,
                         return_logp=False):
        out = self.translate_greedy(sig, L, S, max_len, min_len, return_attn, return_logp)
        self.calls[-1] = ("sample",) + self.calls[-1][1:]
        return out

    def token_weights(self, tokens, logp=None, tok_logp=None):
        tok, lp = tokens.numpy(), logp.numpy()
        w = np.zeros(tok.shape, np.uint16)
        for i in np.ndindex(*tok.shape):
            w[i] = frontend.token_weight(lp[i + (tok[i],)])
        return torch.from_numpy(w.view(np.int16))

    def token_mod_weights(self, tokens, logp, canon_id, mod_id):
        assert (canon_id, mod_id) == (C_ID, M_ID)
        self.calls.append(("token_mod_weights",))
        tok, lp = tokens.numpy(), logp.numpy()
        mw = np.zeros(tok.shape, np.uint16)
        for i in np.ndindex(*tok.shape):
            if tok[i] in (C_ID, M_ID):
                mw[i] = frontend.token_mod_weight(lp[i + (C_ID,)], lp[i + (M_ID,)], tok[i] == M_ID)
        return torch.from_numpy(mw.view(np.int16))


def make_tr(engine_cls, itos=ITOS9, **over):
    opt = dict(gpu=0, n_best=1, max_length=10, min_length=0, beam_size=1, random_sampling_temp=1.0,
               random_sampling_topk=1, block_ngram_repeat=0, dump_beam="", replace_unk=False, verbose=False,
               fast=False, alpha=0.0, beta=0.0, batch_size=3)
    opt.update(over)
    eng = engine_cls()
    return Translator(synth.ModelConfig(itos=list(itos)), None, types.SimpleNamespace(**opt), engine=eng), eng


def test_translator_mod_weights_line_up_with_the_strings():
    reads = [chunks([512, 512, 77], seed=1), chunks([511, 300], seed=2), chunks([60], seed=3)]
    tr, eng = make_tr(ModEngine)
    got = tr.translate_reads(reads, batch_size=2, mods=True)
    trq, engq = make_tr(ModEngine)
    qual = trq.translate_reads(reads, batch_size=2, qualities=True)
    assert [g[:2] for g in got] == [q[:2] for q in qual]
    assert [[w.tolist() for w in g[2]] for g in got] == [[w.tolist() for w in q[2]] for q in qual]
    # one engine call with return_logp, then one token_mod_weights: no second decode
    assert [c[0] for c in eng.calls] == ["greedy", "token_mod_weights"] and eng.calls[0][-1] == ("return_logp", True)
    assert [c[0] for c in engq.calls] == ["greedy"]
    lp = known_logp9(8, 10)
    row, seen = 0, set()
    for (sc, preds, ws, ms), read in zip(got, reads):
        assert len(ms) == len(ws) == len(preds) == len(read)
        for p, w, m in zip(preds, ws, ms):
            s = p[0].replace(" ", "")
            assert m.dtype == np.uint16 and len(m) == len(w) == len(s) == 3  # three bases, then EOS
            want = [frontend.token_mod_weight(lp[row, t, C_ID], lp[row, t, M_ID], c == "M") if c in "CM" else 0
                    for t, c in enumerate(s)]
            assert m.tolist() == want and s[2] == "C" and s[1] in "CM"
            seen.add(s[1])
            row += 1
    assert seen == {"C", "M"}
    # the generator carries the same arrays per chunk, as its fourth entry; mods implies qualities
    tr, eng = make_tr(ModEngine)
    for ri, res in tr.stream_reads(reads, 2, mods=True):
        assert [r[3].tolist() for r in res] == [m.tolist() for m in got[ri][3]]
        assert [r[2].tolist() for r in res] == [w.tolist() for w in got[ri][2]]
    # sampling takes the same path
    tr, eng = make_tr(ModEngine, random_sampling_topk=3, random_sampling_temp=0.7, seed=5)
    smp = tr.translate_reads(reads, batch_size=2, mods=True)
    assert eng.calls[0][0] == "sample" and [m.tolist() for m in smp[0][3]] == [m.tolist() for m in got[0][3]]


def test_translator_refusals_and_default():
    reads = [chunks([512, 300], seed=2)]
    tr, eng = make_tr(ModEngine, itos=synth.DEFAULT_ITOS)  # no M in the vocabulary
    with pytest.raises(ValueError, match="C and M"):
        tr.translate_reads(reads, batch_size=2, mods=True)
    with pytest.raises(ValueError, match="C and M"):
        list(tr.stream_reads(reads, 2, mods=True))
    assert eng.calls == []
    tr, eng = make_tr(ModEngine)
    with pytest.raises(ValueError):
        tr.translate_reads(reads, batch_size=2, attn_debug=True, mods=True)
    # the average-attention beam refusal is the qualities' own
    opt = types.SimpleNamespace(gpu=0, n_best=1, max_length=10, beam_size=4, fast=True, batch_size=2)
    aan = Translator(synth.ModelConfig(self_attn_type="average", itos=list(ITOS9)), None, opt, engine=ModEngine())
    with pytest.raises(NotImplementedError):
        aan.translate_reads(reads, batch_size=2, mods=True)
    # without mods the engine sees today's arguments: FakeEngine takes no return_logp and has no weights at all
    class Plain9(FakeEngine):
        _tok = ModEngine._tok
    tr0, eng0 = make_tr(Plain9)
    plain = tr0.translate_reads(reads, batch_size=2)
    tr, eng = make_tr(ModEngine)
    assert tr.translate_reads(reads, batch_size=2) == plain and len(eng.calls) == len(eng0.calls) == 1
    for a, b in zip(eng.calls[0], eng0.calls[0]):
        assert np.array_equal(a, b)


class BeamModEngine(ModEngine):
    """ModEngine whose scoring pass records what it was asked for and returns known log-probs."""

    max_steps = 16

    def score_targets(self, sig, L, S, gold, gold_len, return_tok_logp=False, return_logp=False):
        self.calls.append(("score", bool(return_tok_logp), bool(return_logp)))
        B, Lg = gold.shape
        lp = known_logp9(B, Lg)
        tl = np.take_along_axis(lp, gold.numpy().astype(np.int64)[..., None], -1)[..., 0]
        out = {"scores": torch.from_numpy(tl.sum(-1)), "tok_logp": torch.from_numpy(tl)}
        if return_logp:
            out["logp"] = torch.from_numpy(lp)
        return out

    def token_weights(self, tokens, logp=None, tok_logp=None):
        return torch.from_numpy(np.vectorize(frontend.token_weight)(tok_logp.numpy()).astype(np.uint16).view(np.int16))


def test_beam_mods_use_one_scoring_pass():
    reads = [chunks([512, 511, 77], seed=1)]
    tr, eng = make_tr(BeamModEngine, beam_size=4, fast=True)
    (sc, preds, ws, ms), = tr.translate_reads(reads, batch_size=1, mods=True)  # spans 512, 511, 77: C, M, M
    assert [c[0] for c in eng.calls] == ["beam", "score", "token_mod_weights"]
    assert eng.calls[1] == ("score", True, True)  # the one pass gives tok_logp and logp
    trq, engq = make_tr(BeamModEngine, beam_size=4, fast=True)
    (sc0, preds0, ws0), = trq.translate_reads(reads, batch_size=1, qualities=True)
    assert engq.calls[1] == ("score", True, False)  # with qualities alone: today's arguments
    assert (sc, preds) == (sc0, preds0) and [w.tolist() for w in ws] == [w.tolist() for w in ws0]
    lp = known_logp9(8, 8)
    for row, (p, m) in enumerate(zip(preds, ms)):
        s = p[0].replace(" ", "")
        want = [frontend.token_mod_weight(lp[row, t, C_ID], lp[row, t, M_ID], c == "M") if c in "CM" else 0
                for t, c in enumerate(s)]
        assert len(s) == 3 and m.tolist() == want
    assert [p[0].split()[1] for p in preds] == ["C", "M", "M"]


# ---------------------------------------------------------------- translate.py -mod_probs
class _Eng(ModEngine):
    def __init__(self, cfg, W, device=0, max_batch=8, max_src_len=512, max_steps=100, max_beam=1):
        super().__init__(max_batch=max_batch, max_src_len=max_src_len)


def _cli_setup(tmp_path, monkeypatch, itos):
    import nanodecoder_amd.translator as T
    monkeypatch.setattr(T, "Engine", _Eng)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    cfg = synth.ModelConfig(itos=list(itos))
    ck = tmp_path / "m.pt"
    checkpoint.save_synthetic(str(ck), cfg, synth.make_weights(cfg, seed=1))
    src = tmp_path / "reads"
    src.mkdir()
    for i, n in enumerate((1300, 700, 400)):
        raw = synth.synth_raw_read(i, n)
        (src / f"read{i}.signal").write_text(" ".join(str(int(v)) for v in raw))
    return ck, src


@pytest.mark.parametrize("window", [("512", "512"), ("300", "100")])
def test_cli_mod_probs_end_to_end(tmp_path, monkeypatch, window):
    ck, src = _cli_setup(tmp_path, monkeypatch, ITOS9)
    files = {}
    for mode, extra in (("plain", []), ("mods", ["-mod_probs"]), ("both", ["-mod_probs", "-fastq"]),
                        ("fastq", ["-fastq"])):
        out = tmp_path / mode
        argv = ["-model", str(ck), "-src_dir", str(src), "-save_data", str(out), "-gpu", "0", "-beam_size", "1",
                "-batch_size", "2", "-thread", "2", "-max_length", "10", "-pack_reads", "2", "-src_seq_length",
                window[0], "-src_seq_stride", window[1]] + extra
        assert cli.main(opts.parse_translate_opts(argv)) == 3
        files[mode] = {os.path.join(d, f): (out / d / f).read_bytes() for d in ("result", "segment")
                       for f in sorted(os.listdir(out / d))}
    is_mod = lambda k: k.endswith(".mod.fastq")  # noqa: E731
    is_fq = lambda k: k.endswith(".fastq") and not is_mod(k)  # noqa: E731
    assert sum(map(is_mod, files["mods"])) == 3 and not any(map(is_fq, files["mods"]))
    assert not any(k.endswith(".fastq") for k in files["plain"])
    # the other outputs are byte for byte those of a run without the flag
    assert {k: v for k, v in files["mods"].items() if not is_mod(k)} == files["plain"]
    assert {k: v for k, v in files["both"].items() if not is_mod(k)} == files["fastq"]
    assert {k: v for k, v in files["both"].items() if is_mod(k)} == {k: v for k, v in files["mods"].items() if is_mod(k)}
    n_sites = 0
    for k, v in files["both"].items():
        if not is_mod(k):
            continue
        name = os.path.basename(k)[: -len(".mod.fastq")]
        rname, seq, qual, vals = parse_record(v.decode("ascii"))
        fasta = files["plain"][os.path.join("result", name + ".fasta")].decode()
        assert rname == name and fasta.replace("M", "C") == ">%s\n%s" % (name, seq)
        assert files["both"][os.path.join("result", name + ".fastq")].decode().split("\n")[3] == qual
        n_sites += len(vals)
    assert n_sites > 0


def test_cli_mod_probs_refusals(tmp_path, monkeypatch):
    o = opts.parse_translate_opts(["-model", "m.pt", "-src_dir", str(tmp_path), "-save_data", str(tmp_path / "o"),
                                   "-gpu", "0", "-mod_probs", "-attn_debug"])
    assert o.mod_probs is True
    with pytest.raises(ValueError, match="attn_debug"):
        cli.main(o)
    assert opts.parse_translate_opts(["-model", "m.pt", "-src_dir", "x", "-save_data", "y"]).mod_probs is False
    # a vocabulary without M: refused before any read is touched
    ck, src = _cli_setup(tmp_path, monkeypatch, synth.DEFAULT_ITOS)
    out = tmp_path / "out"
    with pytest.raises(ValueError, match="C and M"):
        cli.main(opts.parse_translate_opts(["-model", str(ck), "-src_dir", str(src), "-save_data", str(out), "-gpu",
                                            "0", "-beam_size", "1", "-mod_probs"]))
    assert not os.path.exists(out / "result") or os.listdir(out / "result") == []
