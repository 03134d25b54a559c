"""The annotated forms of read assembly on the host (CPU only): frontend.assemble_read_annotated with every
annotation at once against assemble_read and the _q / _m / _p wrappers, the vote's sums against a restatement
over the chunks' positions, what the wrappers raise, and pack_assembly_input with all three arrays."""
import difflib
import random

import numpy as np
import pytest

from nanodecoder_amd import frontend

BRANCHES = ((300, 60), (300, 300))  # the overlap vote, and translate.py's concatenation branch


def spaced(s):
    return " ".join(s)


def make_group(seed=11):
    """Six reads of 0 to 8 chunks of 5 to 40 bases over ACGTM: two random ones built as test_gpu_assembly's
    random group is (windows of one truth that drift both ways, 7 % substitutions), with empty chunks and
    lower-case bases, then the planted cases."""
    rng = random.Random(seed)
    reads = []
    for n_chunks in (8, 6):
        truth = "".join(rng.choice("ACGTM") for _ in range(300))
        st = rng.randrange(100, 160)
        preds = []
        for j in range(n_chunks):
            if j in (2, 5):
                preds.append([""])
                continue
            n = rng.choice([5, 17, 33, 40])
            st = max(0, min(len(truth) - n, st + rng.randint(-12, 20)))
            w = [rng.choice("ACGTM") if rng.random() < 0.07 else ch for ch in truth[st: st + n]]
            w = [ch.lower() if rng.random() < 0.1 else ch for ch in w]
            preds.append([spaced(w), spaced("ACGT")])  # n-best: the second is never used
        reads.append(preds)
    reads.append([[""], [spaced("ACGMTac")], [""]])                                    # one valid chunk
    reads.append([[spaced("AAAAA")], [spaced("CCMCCC")], [spaced("CMCCGT")]])          # no shared char: la - lb
    reads.append([[spaced("ACGGT")], [spaced("TTTMACGGTC")], [spaced("GGTCAa")]])      # the placement goes to -4
    reads.append([])
    rng = np.random.default_rng(seed)
    sizes = [[len(x[0].replace(" ", "")) for x in preds] for preds in reads]
    ws = [[rng.integers(0, 65536, n) for n in ns] for ns in sizes]
    ms = [[rng.integers(0, 65536, n) for n in ns] for ns in sizes]
    ps = [[np.sort(rng.integers(0, 300, n)) for n in ns] for ns in sizes]
    return reads, ws, ms, ps


@pytest.fixture(scope="module")
def group():
    return make_group()


def positions_by_difflib(valid):
    pos = [0] * len(valid)
    for i in range(1, len(valid)):
        a, b, _ = max(difflib.SequenceMatcher(None, valid[i - 1], valid[i]).get_matching_blocks(), key=lambda t: t[2])
        pos[i] = pos[i - 1] + a - b
    return pos


def test_the_group_holds_its_planted_cases(group):
    reads = group[0]
    assert len(reads) == 6 and [len(p) for p in reads] == [8, 6, 3, 3, 3, 0]
    strs = [x[0].replace(" ", "") for p in reads for x in p]
    assert all(5 <= len(s) <= 40 for s in strs if s) and sum(1 for s in strs if not s) >= 5
    assert any(ch.islower() for s in strs for ch in s) and set("".join(strs).upper()) == set("ACGTM")
    assert positions_by_difflib([x[0].replace(" ", "") for x in reads[3]])[1] == 5 - 6
    assert min(positions_by_difflib([x[0].replace(" ", "") for x in reads[4]])) < 0
    assert frontend.assemble_read(reads[2], 300, 60) == "" and frontend.assemble_read(reads[2], 300, 300) == "ACGMTac"


@pytest.mark.parametrize("length,stride", BRANCHES)
def test_all_annotations_at_once_equal_each_form(group, length, stride):
    some = 0
    for preds, w, m, p in zip(*group):
        a = frontend.assemble_read_annotated(preds, length, stride, weights=w, mod_weights=m, positions=p)
        assert a.sequence == frontend.assemble_read(preds, length, stride)
        assert (a.sequence, a.quality) == frontend.assemble_read_q(preds, w, length, stride)
        seq, qual, ml = frontend.assemble_read_m(preds, w, m, length, stride)
        assert (a.sequence, a.quality) == (seq, qual) and a.ml.dtype == ml.dtype == np.uint8
        assert a.ml.tolist() == ml.tolist() and len(ml) == len(seq) == len(qual)
        seq, rpos = frontend.assemble_read_p(preds, p, length, stride)
        assert a.sequence == seq and a.rpos.dtype == rpos.dtype == np.uint32 and a.rpos.tolist() == rpos.tolist()
        plain = frontend.assemble_read_annotated(preds, length, stride)
        assert plain == (a.sequence, None, None, None)
        some += int(a.ml.astype(bool).sum())
    assert some > 20  # sites with a methylation value: the ml comparison is not one of zeros


@pytest.mark.parametrize("length,stride", BRANCHES)
def test_assemble_reads_on_the_host_is_the_per_read_composition(group, length, stride):
    reads, ws, ms, ps = group
    got = frontend.assemble_reads(reads, length, stride, device=None, weights=ws, mod_weights=ms, positions=ps)
    assert len(got) == len(reads)
    for g, preds, w, m, p in zip(got, reads, ws, ms, ps):
        seq, qual, ml = frontend.assemble_read_m(preds, w, m, length, stride)
        rpos = frontend.assemble_read_p(preds, p, length, stride)[1]
        assert len(g) == 4 and g[:2] == (seq, qual) and g[2].tolist() == ml.tolist() and g[3].tolist() == rpos.tolist()
    # every other combination keeps its shape: a string, or a tuple in the order quality, ml, positions
    assert frontend.assemble_reads(reads, length, stride) == [frontend.assemble_read(p, length, stride) for p in reads]
    both = frontend.assemble_reads(reads, length, stride, weights=ws, positions=ps)
    for b, g in zip(both, got):
        assert len(b) == 3 and b[:2] == g[:2] and b[2].tolist() == g[3].tolist()


def test_the_sums_of_the_vote_are_exact(group):
    stride, some = 60, 0
    for preds, w, m, p in zip(*group):
        consensus, wsum, msum, psum = frontend.simple_assembly_annotated(preds, w, m, p, stride)
        # for every vote that lands on column x >= 0: count, wsum[class], msum if C or M, psum
        valid = [(ci, x[0].replace(" ", "")) for ci, x in enumerate(preds) if x[0] != ""]
        pos = positions_by_difflib([s for _, s in valid])
        length = max([0] + [pos[i] + len(valid[i][1]) for i in range(1, len(valid))])
        width = max([length] + [pos[i] + len(s) for i, (_, s) in enumerate(valid)])
        count, ws_ = [[0] * width for _ in range(5)], [[0] * width for _ in range(5)]
        ms_, ps_ = [0] * width, [0] * width
        for i, (ci, s) in enumerate(valid):
            for x, ch in enumerate(s):
                if pos[i] + x >= 0:
                    k = "ACGTM".index(ch.upper())
                    count[k][pos[i] + x] += 1
                    ws_[k][pos[i] + x] += int(w[ci][x])
                    ms_[pos[i] + x] += int(m[ci][x]) if k in (1, 4) else 0
                    ps_[pos[i] + x] += int(p[ci][x]) + ci * stride
        assert consensus.shape == wsum.shape == (5, length) and msum.shape == psum.shape == (length,)
        assert wsum.dtype == msum.dtype == psum.dtype == np.int64
        assert consensus.tolist() == [row[:length] for row in count]
        assert wsum.tolist() == [row[:length] for row in ws_]
        assert msum.tolist() == ms_[:length] and psum.tolist() == ps_[:length]
        some += int(consensus.sum())
        # a subset of the arrays gives the same sums, and None for the rest
        only = frontend.simple_assembly_annotated(preds, positions=p, src_seq_stride=stride)
        assert only[1] is None and only[2] is None and only[3].tolist() == psum.tolist()
        assert only[0].tolist() == frontend.simple_assembly(preds).tolist() == consensus.tolist()
    assert some > 200  # votes counted over the group


GOOD = [["A C G T A"], ["G T A C C"]]
W_GOOD = [[1, 2, 3, 4, 5], [6, 7, 8, 9, 10]]
WITH_N = [["A C G T A"], ["G T N C C"]]
WRAPPERS = [
    ("weights", lambda preds, a, b, L, S: frontend.assemble_read_q(preds, a, L, S)),
    ("modification weights", lambda preds, a, b, L, S: frontend.assemble_read_m(preds, b, a, L, S)),
    ("positions", lambda preds, a, b, L, S: frontend.assemble_read_p(preds, a, L, S)),
]


@pytest.mark.parametrize("what,call", WRAPPERS, ids=["q", "m", "p"])
def test_what_the_wrappers_raise(what, call):
    """``a`` is the wrapper's own array (for _m the modification weights, beside good weights ``b``)."""
    short = [W_GOOD[0], W_GOOD[1][:4]]
    assert call(GOOD, W_GOOD, W_GOOD, 300, 60)[0] == frontend.assemble_read(GOOD, 300, 60)
    for L, S in BRANCHES:
        with pytest.raises(ValueError, match="array per chunk"):  # a wrong number of arrays
            call(GOOD, W_GOOD[:1], W_GOOD, L, S)
    with pytest.raises(ValueError, match="a chunk of 5 bases with 4 " + what):
        call(GOOD, short, W_GOOD, 300, 60)
    with pytest.raises(ValueError, match="a read of 10 bases with 9 " + what):
        call(GOOD, short, W_GOOD, 300, 300)
    # the length is checked before any vote of the chunk is counted: it comes before the N of the same chunk
    with pytest.raises(ValueError, match="a chunk of 5 bases with 4 " + what):
        call(WITH_N, short, W_GOOD, 300, 60)
    with pytest.raises(KeyError):
        call(WITH_N, W_GOOD, W_GOOD, 300, 60)
    # an N in an earlier chunk than the short array is met first
    with pytest.raises(KeyError):
        call([["A N G T A"], ["G T A C C"]], short, W_GOOD, 300, 60)


@pytest.mark.parametrize("kw", [dict(), dict(weights=1), dict(weights=1, mod_weights=1), dict(positions=1),
                                dict(weights=1, mod_weights=1, positions=1)], ids=["plain", "q", "m", "p", "qmp"])
def test_defer_errors_yields_none_for_exactly_the_failing_read(monkeypatch, kw):
    """The device is stood in for by one that assembles nothing, so every read takes the per-read fallback."""
    reads = [GOOD, WITH_N, GOOD]
    kw = {k: [W_GOOD] * 3 for k in kw}
    calls = []

    def nothing(bases, chunk_off, read_off, device, qw=None, mw=None, bp=None):
        R = len(read_off) - 1
        calls.append((qw is not None, mw is not None, bp is not None))
        return frontend.AssemblyOutput(np.zeros(bases.size, np.uint8), np.full(R, -1, np.int32),
                                       np.full(R, frontend.ASM_STATUS_CHAR, np.int32),
                                       None if qw is None else np.zeros(bases.size, np.uint8),
                                       None if mw is None else np.zeros(bases.size, np.uint8),
                                       None if bp is None else np.zeros(bases.size, np.uint32))
    monkeypatch.setattr(frontend, "_assemble_device", nothing)
    stats = {}
    got = frontend.assemble_reads(reads, 300, 60, device=0, stats=stats, defer_errors=True, **kw)
    want = frontend.assemble_reads([GOOD], 300, 60, **{k: v[:1] for k, v in kw.items()})[0]
    assert got[1] is None and stats == {"reads": 3, "fallback": 3}
    for g in (got[0], got[2]):
        assert type(g) is type(want) and len(g) == len(want)
        assert g == want if isinstance(g, str) else all(np.array_equal(a, b) for a, b in zip(g, want))
    # one call per form; positions beside weights are a second call, on the same packing
    q, m, p = "weights" in kw, "mod_weights" in kw, "positions" in kw
    assert calls == ([(q, m, False)] if q or not p else []) + ([(False, False, True)] if p else [])
    with pytest.raises(KeyError):
        frontend.assemble_reads(reads, 300, 60, device=0, **kw)


def test_pack_assembly_input_with_all_three(group):
    reads, ws, ms, ps = group
    reads = reads + [[["A ç"], ["C"]]]  # kept on the host: packed with no chunks
    ws, ms, ps = ws + [[[1, 2], [3]]], ms + [[[1, 2], [3]]], ps + [[[1, 2], [3]]]
    every = frontend.pack_assembly_input(reads, ws, ms, ps, src_seq_stride=60)
    by_w = frontend.pack_assembly_input(reads, ws, ms)
    by_p = frontend.pack_assembly_input(reads, positions=ps, src_seq_stride=60)
    assert every.host == by_w.host == by_p.host == [6] and by_w.bp is None and by_p.qw is None and by_p.mw is None
    for k in ("bases", "chunk_off", "read_off", "qw", "mw"):
        a, b = getattr(every, k), getattr(by_w, k)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    assert every.qw.tobytes() == frontend.pack_assembly_input(reads, ws).qw.tobytes()
    assert every.bp.dtype == by_p.bp.dtype == np.uint32 and every.bp.tobytes() == by_p.bp.tobytes()
    assert every.bp.size == every.qw.size == every.mw.size == every.bases.size > 200
    with pytest.raises(ValueError):
        frontend.pack_assembly_input(reads, ws, ms, ps)  # no stride
    with pytest.raises(ValueError):
        frontend.pack_assembly_input(reads, None, ms, ps, src_seq_stride=60)
