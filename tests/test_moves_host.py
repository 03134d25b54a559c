"""Per-base signal positions on the host (CPU only): the token rule by hand, frontend.assemble_read_p against
assemble_read and hand-worked columns, the Translator's opt-in with a stand-in engine that returns scripted
attention, translate.py -moves end to end, and the new entry points' argument errors.  Every comparison is exact."""
import ctypes
import math
import os
import random

import numpy as np
import pytest
import torch

from nanodecoder_amd import cli, frontend, opts, synth
from tests.test_mods_host import ITOS9, ModEngine, _cli_setup, make_tr
from tests.test_quality_host import HAND, random_group
from tests.test_translator_host import FakeEngine, chunks

ONE = 1 << 24


# ---------------------------------------------------------------- the token rule
def slow_positions(rows, span):
    """The rule of DESIGN.md §1.6 in Python integers, one entry at a time: m [S] of rows [S, T]."""
    out, m = [], 0
    for row in np.asarray(rows, np.float32):
        Q = M = 0
        for t in range(min(max(int(span), 0), len(row))):
            a = float(row[t])
            if not a > 0:
                q = 0
            elif a >= 1:
                q = ONE
            else:
                q = math.floor(a * 16777216.0 + 0.5)
            Q += q
            M += q * t
        c = (2 * M + Q) // (2 * Q) if Q else 0
        m = c if not out else max(m, c)
        out.append(m)
    return out


def one(row, span):
    return int(frontend.token_positions(np.asarray([row], np.float32), span)[0])


def hot(T, *at, v=1.0):
    row = np.zeros(T, np.float32)
    for t in at:
        row[t] = v
    return row


def test_token_rule_by_hand():
    T = 16
    assert one(hot(T, 0, v=0.75), T) == 0                      # one-hot at t = 0
    assert one(hot(T, T - 1, v=0.75), T) == T - 1              # one-hot at t = span - 1
    assert one(hot(T, 10, v=0.75), 11) == 10
    assert one(hot(T, 6, 7, v=0.5), T) == 7                    # two equal peaks at t and t + 1: half up, t + 1
    assert one(hot(T, 0, 1, v=0.25), T) == 1
    assert one(np.zeros(T, np.float32), T) == 0                # an all-zero row: Q = 0
    row = hot(T, 9, v=0.25)
    row[3] = np.nan                                            # a NaN entry counts nothing
    assert one(row, T) == 9
    row = hot(T, 4, v=1.0)                                     # an entry of 1.0 is 2^24; 3.0 is clamped to it
    row[8] = 3.0
    assert one(row, T) == 6
    row[8] = np.inf
    assert one(row, T) == 6
    row = np.full(T, 2.0 ** -26, np.float32)                   # below 2^-25: floor(0.25 + 0.5) = 0
    assert one(row, T) == 0
    row[12] = 2.0 ** -25                                       # exactly 2^-25: floor(0.5 + 0.5) = 1
    assert one(row, T) == 12
    row[2] = 2.0 ** -24                                        # q = 1 at t = 2 and at t = 12: centroid 7
    assert one(row, T) == 7
    row = hot(T, 5, v=0.5)                                     # negatives and -0 count nothing
    row[1], row[2] = -1.0, -0.0
    assert one(row, T) == 5
    # three quarters at t = 2 and one quarter at t = 5: M / Q = 2.75 -> 3; the other way round 4.25 -> 4
    row = hot(T, 2, v=0.75)
    row[5] = 0.25
    assert one(row, T) == 3
    row[2], row[5] = 0.25, 0.75
    assert one(row, T) == 4


def test_garbage_past_the_span_is_ignored():
    T = 16
    row = hot(T, 3, v=0.5)
    row[8:] = [np.nan, np.inf, 7.0, -3.0, 1.0, 0.5, 1e30, 2.0]
    assert one(row, 8) == 3 and one(row, 4) == 3
    assert one(row, 3) == 0 and one(row, 0) == 0 and one(row, -5) == 0  # nothing inside the span
    assert one(row, 9) == 3                                              # the NaN at t = 8 counts nothing
    assert one(row, 11) == (2 * (3 * (ONE // 2) + 10 * ONE) + 3 * (ONE // 2)) // (2 * 3 * (ONE // 2))  # 7.0 -> 2^24
    assert one(row, 99) == one(row, T)                                   # min(span, T)


def test_running_maximum_over_the_steps():
    T = 32
    rows = np.stack([hot(T, 20), hot(T, 10), np.zeros(T, np.float32), hot(T, 5), hot(T, 30), hot(T, 29)])
    assert frontend.token_positions(rows, T).tolist() == [20, 20, 20, 20, 30, 30]
    # m[0] = c[0]: a leading zero row is 0, and a zero row keeps the position before it
    rows = np.stack([np.zeros(T, np.float32), hot(T, 4), np.zeros(T, np.float32)])
    assert frontend.token_positions(rows, T).tolist() == [0, 4, 4]
    got = frontend.token_positions(rows, T)
    assert got.dtype == np.int32 and got.shape == (3,)


def scripted_rows(T, span):
    """Nine rows that walk through the rule's cases at a given span, with garbage at every t >= span."""
    s1 = max(int(span) - 1, 0)
    t0 = max(min(10, int(span) - 2), 0)
    rows = np.zeros((9, T), np.float32)
    rows[0, 0] = 0.75                                   # one-hot at t = 0
    rows[2, t0] = rows[2, min(t0 + 1, T - 1)] = 0.5     # row 1 stays zero; two equal peaks
    rows[3, min(5, s1)], rows[3, min(20, s1)] = np.nan, 0.25
    rows[4, min(7, s1)], rows[4, min(9, s1)] = 1.0, 1.5
    rows[5, :] = 2.0 ** -26
    rows[5, min(30, s1)] = 2.0 ** -24
    rows[6, s1] = 0.75                                  # one-hot at t = span - 1
    rows[7, s1 // 2] = 0.75                             # a smaller centroid: the running maximum holds
    rows[8, min(2, s1)], rows[8, min(4, s1)], rows[8, min(6, s1)] = -0.0, -1.0, 0.5
    rows[:, int(span):] = np.resize(np.asarray([np.nan, np.inf, 7.0, 0.9, -2.0], np.float32), max(T - int(span), 0))
    return rows


def softmax_rows(B, S, T, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, S, T)).astype(np.float32) * rng.uniform(0.5, 6.0, size=(B, S, 1)).astype(np.float32)
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("T", [64, 100])
def test_numpy_rule_equals_the_integer_restatement(T):
    for span in (T, 37, 1):
        rows = scripted_rows(T, span)
        got = frontend.token_positions(rows, span).tolist()
        assert got == slow_positions(rows, span)
        assert got[0] == 0 and got[1] == 0 and got[6] == span - 1 and got[7] == span - 1 and got[8] == span - 1
    a = softmax_rows(3, 5, T, seed=T)
    spans = np.asarray([T, 37, 9])
    got = frontend.token_positions(a, spans)
    assert got.shape == (3, 5)
    for b in range(3):
        assert got[b].tolist() == slow_positions(a[b], spans[b])
    assert (np.diff(got, axis=1) >= 0).all() and (got < spans[:, None]).all()


# ---------------------------------------------------------------- assemble_read_p
LEN, STRIDE = 100, 50


def test_column_rule_by_hand():
    assert frontend.column_position(0, 0) == 0          # a column nobody voted on
    assert frontend.column_position(1, 77) == 77
    assert frontend.column_position(2, 125) == 62       # integer division
    assert frontend.column_position(3, 2 ** 33) == 2 ** 33 // 3
    assert frontend.column_position(np.asarray([0, 2, 1]), np.asarray([0, 7, 2 ** 32 - 1])).tolist() == \
        [0, 3, 2 ** 32 - 1]


def test_assemble_read_p_hand_worked():
    """The placement rule keeps consecutive chunks touching (disp <= la), so a vote always reaches every column
    below the read's length: the no-vote column of the rule is covered by test_column_rule_by_hand."""
    # an empty chunk in the middle: the third chunk's offset is 2 * STRIDE, not 1 * STRIDE.
    # ACGTA / GTACC share GTA: disp 2, columns 2..4 have two votes
    preds = [["A C G T A"], [""], ["G T A C C"]]
    pos = [[0, 10, 20, 30, 40], [], [5, 15, 25, 35, 45]]
    seq, r = frontend.assemble_read_p(preds, pos, LEN, STRIDE)
    assert seq == "ACGTACC" == frontend.assemble_read(preds, LEN, STRIDE)
    assert r.dtype == np.uint32
    assert r.tolist() == [0, 10, (20 + 105) // 2, (30 + 115) // 2, (40 + 125) // 2, 135, 145]
    # a negative placement: ACGG sits at b's offset 3, b's first three chars fall off the left edge
    preds = [["A C G G"], ["T T T A C G G C"]]
    pos = [[1, 2, 3, 4], [0, 1, 2, 3, 4, 5, 6, 7]]
    seq, r = frontend.assemble_read_p(preds, pos, LEN, STRIDE)
    assert seq == "ACGGC" == frontend.assemble_read(preds, LEN, STRIDE)
    assert r.tolist() == [(1 + 53) // 2, (2 + 54) // 2, (3 + 55) // 2, (4 + 56) // 2, 57]
    # a vote that lost the call still counts: column 3 is T, T, A -> T, and A's position is in the mean
    preds = [["A C G T"], ["A C G T"], ["A C G A"]]
    pos = [[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 30]]
    seq, r = frontend.assemble_read_p(preds, pos, LEN, STRIDE)
    assert seq == "ACGT" and r.tolist() == [50, 51, 52, (3 + 53 + 130) // 3]
    # the running maximum along the read: the second chunk's own columns lie before the shared ones
    preds = [["A C G T"], ["G T C C"]]
    pos = [[60, 61, 90, 91], [0, 1, 2, 3]]
    seq, r = frontend.assemble_read_p(preds, pos, LEN, STRIDE)
    assert seq == "ACGTCC" and r.tolist() == [60, 61, 70, 71, 71, 71]
    # a read of one valid chunk is "" (simple_assembly's length only counts the chunks after the first)
    seq, r = frontend.assemble_read_p([[""], ["A C G T"], [""]], [[], [1, 2, 3, 4], []], LEN, STRIDE)
    assert seq == "" and r.size == 0 and r.dtype == np.uint32
    seq, r = frontend.assemble_read_p([], [], LEN, STRIDE)
    assert seq == "" and r.size == 0


def test_assemble_read_p_concatenation_branch():
    preds = [["A C"], [""], ["G T A"]]
    pos = [[3, 9], [], [2, 1, 8]]
    seq, r = frontend.assemble_read_p(preds, pos, 100, 100)
    assert seq == "ACGTA" == frontend.assemble_read(preds, 100, 100)
    assert r.tolist() == [3, 9, 202, 202, 208] and r.dtype == np.uint32
    seq, r = frontend.assemble_read_p([[""]], [[]], 100, 100)
    assert seq == "" and r.size == 0
    with pytest.raises(ValueError):
        frontend.assemble_read_p(preds, [[3], [], [2, 1, 8]], 100, 100)
    with pytest.raises(ValueError):
        frontend.assemble_read_p(preds, pos[:2], 100, 100)


def random_positions(reads, seed=5, span=300):
    """Chunk-relative positions as a decoder gives them: non-decreasing inside a chunk, below the span."""
    rng = random.Random(seed)
    return [[sorted(rng.randrange(span) for _ in p[0].replace(" ", "")) for p in preds] for preds in reads]


def test_assemble_read_p_sequence_is_assemble_reads():
    reads = [h[1] for h in HAND] + random_group()[:25]
    pos = random_positions(reads)
    some = 0
    for preds, ps in zip(reads, pos):
        for L, S in ((300, 60), (300, 300)):
            seq, r = frontend.assemble_read_p(preds, ps, L, S)
            assert seq == frontend.assemble_read(preds, L, S)
            assert r.dtype == np.uint32 and r.size == len(seq)
            assert (np.diff(r.astype(np.int64)) >= 0).all()
            if r.size:
                assert int(r[-1]) < (len(preds) - 1) * S + 300
            some += r.size
    assert some > 1000
    with pytest.raises(ValueError):
        frontend.assemble_read_p([["A C"], ["C G"]], [[1, 2], [3]], 300, 60)
    with pytest.raises(KeyError):  # what assemble_read raises is raised here
        frontend.assemble_read_p([["A X"], ["X G"]], [[1, 2], [3, 4]], 300, 60)


def test_pack_assembly_input_with_positions_and_host_group():
    reads = [[["A C"], [""], ["C G T"]], [["G"]], []]
    pos = [[[1, 2], [], [0, 5, 9]], [[7]], []]
    packed = frontend.pack_assembly_input(reads, positions=pos, src_seq_stride=60)
    (bases, chunk_off, read_off, host), bp = packed[:4], packed.bp
    assert packed.qw is None and packed.mw is None
    assert bases.tobytes() == b"ACCGTG" and host == []
    assert bp.dtype == np.uint32 and bp.tolist() == [1, 2, 120, 125, 129, 7]  # the empty chunk counts in ci
    assert chunk_off.tolist() == [0, 2, 2, 5, 6] and read_off.tolist() == [0, 3, 4, 4]
    with pytest.raises(ValueError):
        frontend.pack_assembly_input(reads, positions=pos)  # no stride
    with pytest.raises(ValueError):
        frontend.pack_assembly_input(reads, positions=[[[1], [], [0, 5, 9]], [[7]], []], src_seq_stride=60)
    # assemble_reads without a device is the per-read host function, also beside weights
    got = frontend.assemble_reads(reads, 300, 60, positions=pos)
    for g, preds, ps in zip(got, reads, pos):
        seq, r = frontend.assemble_read_p(preds, ps, 300, 60)
        assert g[0] == seq and g[1].tolist() == r.tolist()
    ws = [[[9, 8], [], [7, 6, 5]], [[4]], []]
    both = frontend.assemble_reads(reads, 300, 60, weights=ws, positions=pos)
    for b, g, preds, w in zip(both, got, reads, ws):
        assert b[:2] == frontend.assemble_read_q(preds, w, 300, 60) and b[2].tolist() == g[1].tolist()


def test_moves_record_text():
    assert frontend.moves_record("read7", "ACGT", np.asarray([0, 5, 5, 4000000000], np.uint32)) == \
        ">read7\nACGT\n0,5,5,4000000000\n"
    assert frontend.moves_record("r", "A", [3]) == ">r\nA\n3\n"
    assert frontend.moves_record("e", "", np.zeros(0, np.uint32)) == ">e\n\n\n"
    with pytest.raises(ValueError):
        frontend.moves_record("r", "AC", [1])


# ---------------------------------------------------------------- Translator with a stand-in engine
class MovesEngine(ModEngine):
    """ModEngine whose attention (FakeEngine's: row t uniform over the first t + 1 samples; the beam's 1000 t + x)
    is reduced on the host by the rule, and which records that it was asked."""

    def token_positions(self, attn, spans, hyp0=False):
        self.calls.append(("token_positions", tuple(attn.shape), bool(hyp0)))
        a = attn.numpy()
        return torch.from_numpy(frontend.token_positions(a[:, 0] if hyp0 else a, np.asarray(spans)))


def test_translator_positions_line_up_with_the_strings():
    reads = [chunks([512, 512, 77], seed=1), chunks([511, 300], seed=2), chunks([60], seed=3)]
    tr0, eng0 = make_tr(MovesEngine)
    plain = tr0.translate_reads(reads, batch_size=2)
    tr, eng = make_tr(MovesEngine)
    got = tr.translate_reads(reads, batch_size=2, moves=True)
    assert [g[:2] for g in got] == plain and all(len(g) == 3 for g in got)
    # one engine call with its attention, then one reduction: no second decode, no log-probs
    assert [c[0] for c in eng.calls] == ["greedy", "token_positions"]
    assert eng.calls[1] == ("token_positions", (8, 10, 512), False)
    for (sc, preds, ps), read in zip(got, reads):
        assert len(ps) == len(preds) == len(read)
        for p, m in zip(preds, ps):
            # row t is uniform over t + 1 samples: the centroid t / 2 rounds half up
            assert m.dtype == np.int32 and m.tolist() == [0, 1, 1] and len(p[0].replace(" ", "")) == 3
    # the trailing entry comes after the weights and the modification weights
    trq, engq = make_tr(MovesEngine)
    q = trq.translate_reads(reads, batch_size=2, qualities=True, moves=True)
    assert [c[0] for c in engq.calls] == ["greedy", "token_positions"]
    assert engq.calls[0][-1] == ("return_logp", True)
    trm, engm = make_tr(MovesEngine)
    m = trm.translate_reads(reads, batch_size=2, mods=True, moves=True)
    assert [c[0] for c in engm.calls] == ["greedy", "token_mod_weights", "token_positions"]
    trw, _ = make_tr(MovesEngine)
    w_only = trw.translate_reads(reads, batch_size=2, mods=True)
    for g, a, b, c in zip(got, q, m, w_only):
        assert len(a) == 4 and len(b) == 5 and a[:2] == b[:2] == g[:2]
        assert [x.tolist() for x in a[3]] == [x.tolist() for x in b[4]] == [x.tolist() for x in g[2]]
        assert [x.tolist() for x in a[2]] == [x.tolist() for x in b[2]] == [x.tolist() for x in c[2]]
        assert [x.tolist() for x in b[3]] == [x.tolist() for x in c[3]]
        assert all(x.dtype == np.uint16 for x in a[2] + b[2] + b[3]) and all(x.dtype == np.int32 for x in a[3] + b[4])
    # the generator carries the same arrays per chunk as its last entry
    tr, eng = make_tr(MovesEngine)
    for ri, res in tr.stream_reads(reads, 2, moves=True):
        assert all(len(r) == 3 for r in res)
        assert [r[2].tolist() for r in res] == [x.tolist() for x in got[ri][2]]
    tr, eng = make_tr(MovesEngine)
    for ri, res in tr.stream_reads(reads, 2, mods=True, moves=True):
        assert all(len(r) == 5 for r in res)
        assert [r[4].tolist() for r in res] == [x.tolist() for x in got[ri][2]]
    # sampling takes the same path
    tr, eng = make_tr(MovesEngine, random_sampling_topk=3, random_sampling_temp=0.7, seed=5)
    smp = tr.translate_reads(reads, batch_size=2, moves=True)
    assert [c[0] for c in eng.calls] == ["sample", "token_positions"]
    assert [x.tolist() for x in smp[0][2]] == [x.tolist() for x in got[0][2]]


@pytest.mark.parametrize("fast", [True, False])
def test_translator_beam_positions_use_hypothesis_0(fast):
    reads = [chunks([512, 511, 77], seed=1)]
    tr, eng = make_tr(MovesEngine, beam_size=4, n_best=2, fast=fast)
    (sc, preds, ps), = tr.translate_reads(reads, batch_size=1, moves=True)
    tr0, eng0 = make_tr(MovesEngine, beam_size=4, n_best=2, fast=fast)
    (sc0, preds0), = tr0.translate_reads(reads, batch_size=1)
    assert (sc, preds) == (sc0, preds0)
    assert [c[0] for c in eng.calls] == ["beam" if fast else "classic", "token_positions"]  # no scoring pass
    assert eng.calls[1] == ("token_positions", (8, 2, 10, 512), True)
    # the stand-in's rows hold 1000 t + x >= 1 everywhere but (0, 0): 2^24 each, over the chunk's span
    for i, span in enumerate((512, 511, 77)):
        row0 = (2 * sum(range(1, span)) + (span - 1)) // (2 * (span - 1))
        rows = (2 * sum(range(span)) + span) // (2 * span)
        assert ps[i].dtype == np.int32 and ps[i].tolist() == [row0, max(row0, rows), max(row0, rows)]


def test_translator_refusal_and_default():
    reads = [chunks([512, 300], seed=2)]
    tr, eng = make_tr(MovesEngine)
    with pytest.raises(ValueError, match="attn_debug"):
        tr.translate_reads(reads, batch_size=2, attn_debug=True, moves=True)
    with pytest.raises(ValueError, match="attn_debug"):
        list(tr.stream_reads(reads, 2, attn_debug=True, moves=True))
    assert eng.calls == []

    # without moves the engine sees today's arguments: FakeEngine has no token_positions at all
    class Plain9(FakeEngine):
        _tok = ModEngine._tok
    tr0, eng0 = make_tr(Plain9)
    plain = tr0.translate_reads(reads, batch_size=2)
    tr, eng = make_tr(MovesEngine)
    assert tr.translate_reads(reads, batch_size=2) == plain and len(eng.calls) == len(eng0.calls) == 1
    for a, b in zip(eng.calls[0], eng0.calls[0]):
        assert np.array_equal(a, b)
    asked = []

    class Spy(Plain9):
        def translate_greedy(self, sig, L, S, max_len, min_len=0, **kw):
            asked.append(kw)
            return super().translate_greedy(sig, L, S, max_len, min_len, **kw)
    tr, eng = make_tr(Spy)
    tr.translate_reads(reads, batch_size=2)
    assert asked == [{"return_attn": False}]


class OverflowMoves(MovesEngine):
    """Flags the split-fp16 range guard until exact fp32 is on; the exact rerun's attention is shifted right."""

    exact = False

    def set_exact_fp32(self, on):
        self.exact = bool(on)

    def translate_greedy(self, *a, **k):
        out = super().translate_greedy(*a, **k)
        out["overflow"] = torch.tensor([0 if self.exact else 1], dtype=torch.int32)
        if self.exact and out["attn"] is not None:
            out["attn"] = torch.roll(out["attn"], 40, dims=-1)
        return out


def test_overflow_rerun_carries_the_request():
    reads = [chunks([512, 300], seed=2)]
    tr, eng = make_tr(OverflowMoves)
    (sc, preds, ps), = tr.translate_reads(reads, batch_size=2, moves=True)
    assert [c[0] for c in eng.calls] == ["greedy", "token_positions", "greedy", "token_positions"]
    assert eng.exact is False
    assert all(m.tolist() == [40, 41, 41] for m in ps)  # the rerun's positions replace the flagged call's


# ---------------------------------------------------------------- translate.py -moves
class _Eng(MovesEngine):
    def __init__(self, cfg, W, device=0, max_batch=8, max_src_len=512, max_steps=100, max_beam=1):
        super().__init__(max_batch=max_batch, max_src_len=max_src_len)


def test_opts_parse_moves(tmp_path):
    base = ["-model", "m.pt", "-src_dir", str(tmp_path), "-save_data", str(tmp_path / "o"), "-gpu", "0"]
    assert opts.parse_translate_opts(base).moves is False
    o = opts.parse_translate_opts(base + ["-moves", "-fastq", "-mod_probs", "-assembly", "gpu", "-frontend", "gpu"])
    assert o.moves is True and o.fastq is True and o.mod_probs is True
    o = opts.parse_translate_opts(base + ["-moves", "-attn_debug"])
    with pytest.raises(ValueError, match="-moves"):
        cli.main(o)


@pytest.mark.parametrize("window", [("512", "512"), ("300", "100")])
def test_cli_moves_end_to_end(tmp_path, monkeypatch, window):
    import nanodecoder_amd.translator as T
    ck, src = _cli_setup(tmp_path, monkeypatch, ITOS9)
    monkeypatch.setattr(T, "Engine", _Eng)
    sizes = {"read0": 1300, "read1": 700, "read2": 400}
    files = {}
    for mode, flags in (("plain", ["-fastq"]), ("moves", ["-fastq", "-moves"]), ("only", ["-moves"]),
                        ("all", ["-fastq", "-mod_probs", "-moves"])):
        out = tmp_path / mode
        argv = ["-model", str(ck), "-src_dir", str(src), "-save_data", str(out), "-gpu", "0", "-beam_size", "1",
                "-batch_size", "2", "-thread", "2", "-max_length", "10", "-pack_reads", "2", "-src_seq_length",
                window[0], "-src_seq_stride", window[1]] + flags
        assert cli.main(opts.parse_translate_opts(argv)) == 3
        files[mode] = {os.path.join(d, f): (out / d / f).read_bytes() for d in ("result", "segment")
                       for f in sorted(os.listdir(out / d))}
    mv = {k: v for k, v in files["moves"].items() if k.endswith(".moves")}
    assert len(mv) == 3 and not any(k.endswith(".moves") for k in files["plain"])
    assert {k: v for k, v in files["moves"].items() if k not in mv} == files["plain"]  # .fasta, .fastq, segment
    assert {k: v for k, v in files["only"].items() if k.endswith(".moves")} == mv
    assert {k: v for k, v in files["all"].items() if k.endswith(".moves")} == mv
    assert {k: v for k, v in files["only"].items() if k not in mv} == \
        {k: v for k, v in files["plain"].items() if not k.endswith(".fastq")}
    some = False
    for k, v in mv.items():
        name = os.path.basename(k)[: -len(".moves")]
        text = v.decode("ascii")
        assert text.endswith("\n") and text.count("\n") == 3
        head, seq, pos = text.split("\n")[:3]
        assert head == ">" + name
        assert files["plain"][os.path.join("result", name + ".fasta")].decode() == ">%s\n%s" % (name, seq)
        vals = [int(x) for x in pos.split(",")] if pos else []
        assert len(vals) == len(seq) and vals == sorted(vals)
        assert all(0 <= x < sizes[name] for x in vals)
        some = some or len(seq) > 0
    assert some


# ---------------------------------------------------------------- argument errors, no device
def test_new_entry_points_argument_errors_without_gpu():
    from nanodecoder_amd import _lib, build
    build.build()
    L = _lib.lib()
    ERR = _lib.ND_ERR_ARG
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before any HIP call
    tp = lambda *a: L.nd_token_positions(*a)  # noqa: E731
    assert tp(None, 9 * 64, p, 3, 9, 64, p, None) == ERR
    assert tp(p, 9 * 64, None, 3, 9, 64, p, None) == ERR
    assert tp(p, 9 * 64, p, 3, 9, 64, None, None) == ERR
    assert b"null" in L.nd_last_error()
    assert tp(p, 9 * 64, p, -1, 9, 64, p, None) == ERR
    assert tp(p, 9 * 64, p, 3, -9, 64, p, None) == ERR
    assert tp(p, 9 * 64, p, 3, 9, 0, p, None) == ERR
    assert tp(p, 9 * 64 - 1, p, 3, 9, 64, p, None) == ERR
    assert b"ld_chunk" in L.nd_last_error()
    assert tp(p, 2 ** 40, p, 70000, 70000, 64, p, None) == ERR
    assert tp(p, 2 ** 40, p, 3, 9, 2 ** 19 + 1, p, None) == ERR
    assert tp(None, 9 * 64, None, 0, 9, 64, None, None) == 0  # nothing to do
    need = L.nd_assemble_reads_p_work_bytes(3, 100)
    assert need == L.nd_assemble_reads_work_bytes(3, 100) + 100 * 8
    assert L.nd_assemble_reads_p_work_bytes(0, 0) == 0 and L.nd_assemble_reads_p_work_bytes(-1, 5) < 0
    a = lambda *x: L.nd_assemble_reads_p(*x)  # noqa: E731
    assert a(None, None, None, None, 2, 3, 100, None, None, None, None, None, need, None) == ERR
    assert a(p, None, p, p, 2, 3, 100, p, p, p, p, p, need, None) == ERR  # no positions
    assert a(p, p, p, p, 2, 3, 100, p, None, p, p, p, need, None) == ERR  # no position output
    assert a(p, p, p, p, 2, 3, 100, p, p, p, p, None, need, None) == ERR  # no work buffer
    assert a(p, p, p, p, 2, 3, 100, p, p, p, p, p, need - 1, None) == ERR
    assert b"work_bytes" in L.nd_last_error()
    assert a(p, p, p, p, 2, 3, 100, p, p, p, p, p, L.nd_assemble_reads_work_bytes(3, 100), None) == ERR
    assert a(p, p, p, p, -1, 3, 100, p, p, p, p, p, need, None) == ERR
    assert a(p, p, p, p, 2, -3, 100, p, p, p, p, p, need, None) == ERR
    assert a(p, p, p, p, 2, 3, 2 ** 31, p, p, p, p, p, 2 ** 40, None) == ERR
    assert a(None, None, p, p, 0, 0, 0, None, None, None, None, None, 0, None) == 0  # R == 0: at once
