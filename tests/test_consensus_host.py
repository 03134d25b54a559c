"""Consensus accuracy on the host (CPU only): accuracy.fit_pos_host against a cell-by-cell table with the rule's
traceback, a pile and its call worked by hand, the ties and thresholds of the call, variants planted in a genome
and recovered from reads of both strands, translate.py -truth_ref -consensus end to end with the stand-in engine,
and the argument errors of nd_align_fit_pos, nd_pileup_add and nd_pileup_call."""
import ctypes

import numpy as np
import pytest
import torch

from nanodecoder_amd import accuracy, cli, opts
from tests.test_accuracy_host import _Eng, fasta_sequence, make_reads, mutate, random_seq
from tests.test_mapping_host import FIT_FIXED, fit_pairs

A = accuracy
NONE = A.CONS_NONE


# ---------------------------------------------------------------- positions
def plain_fit_pos(a, b, w0):
    """counts, span, ops and rpos from a full D table, the directions decided cell by cell as the rule words them."""
    a, b = a.encode(), b.encode()
    n, m = len(a), len(b)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        D[i][0] = i
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    jstar = min(range(m + 1), key=lambda j: (D[n][j], j))
    ops, rpos = [0] * n, [None] * n
    i, j = n, jstar
    match = sub = ins = dele = 0
    while i > 0:
        if j >= 1 and D[i - 1][j - 1] + (a[i - 1] != b[j - 1]) == D[i][j]:
            ops[i - 1] = int(a[i - 1] != b[j - 1])
            sub += ops[i - 1]
            match += 1 - ops[i - 1]
            rpos[i - 1] = w0 + j - 1  # the reference base it is matched or mismatched to
            i, j = i - 1, j - 1
        elif j == 0 or D[i - 1][j] + 1 == D[i][j]:
            ops[i - 1] = 2
            ins += 1
            rpos[i - 1] = w0 + j - 1  # the reference base to its left; w0 - 1 on the column-0 border
            i -= 1
        else:
            dele += 1
            j -= 1
    return [D[n][jstar], match, sub, ins, dele], (j, jstar), ops, rpos


@pytest.mark.parametrize("k", range(len(FIT_FIXED) + 12))
def test_fit_pos_host_equals_fit_host_and_the_plain_table(k):
    call, window = fit_pairs()[k]
    w0 = 7 * k
    counts, span, ops, rpos = A.fit_pos_host(call, window, w0)
    c0, s0, o0 = A.fit_host(call, window)
    assert counts.tobytes() == c0.tobytes() and span == s0 and ops.tobytes() == o0.tobytes()
    assert rpos.dtype == np.int32 and rpos.shape == (len(call),)
    assert (counts.tolist(), tuple(span), ops.tolist(), rpos.tolist()) == plain_fit_pos(call, window, w0)
    # the diagonal bases climb one reference base or more at a time, inside the span; an inserted base sits on the
    # diagonal base before it
    diag = rpos[ops <= 1]
    assert (np.diff(diag) >= 1).all() and counts[4] == (np.diff(diag) - 1).sum()
    if diag.size:
        assert diag[0] == w0 + span[0] and diag[-1] == w0 + span[1] - 1
    assert (np.diff(rpos) >= 0).all() and rpos.min(initial=w0) >= w0 - 1


# ---------------------------------------------------------------- a case worked by hand
#            0         1         2
#            012345678901234567890123
HAND_WIN = "GATCTACGGTCAAGCTTGCATCCG"
# the call: a leading T; window base 5 (A) called G; window bases 10, 11 (CA) missing; CCC inserted after base 16;
# a trailing T
HAND_CALL = "T" + "GATCT" + "G" + "CGGT" + "AGCTT" + "CCC" + "GCATCCG" + "T"
HAND_W0 = 100
HAND_OPS = [2] + [0] * 5 + [1] + [0] * 4 + [0] * 5 + [2] * 3 + [0] * 7 + [2]
HAND_RPOS = [99] + [100, 101, 102, 103, 104] + [105] + [106, 107, 108, 109] + [112, 113, 114, 115, 116] + [116] * 3 + \
    [117, 118, 119, 120, 121, 122, 123] + [123]
HAND_PILE = {0: [101, 112, 119],                      # A (not 105: that base was called G)
             1: [103, 106, 114, 118, 121, 122],       # C
             2: [100, 105, 107, 108, 113, 117, 123],  # G
             3: [102, 104, 109, 115, 116, 120],       # T
             4: [110, 111],                           # the two deleted bases
             6: [116]}                                # iC after base 116; the leading and the trailing T: nowhere


def hand_reference():
    rng = np.random.default_rng(5)
    return A.Reference(["hand"], [random_seq(rng, HAND_W0) + HAND_WIN + random_seq(rng, 6)])


def test_pile_and_call_by_hand():
    counts, span, ops, rpos = A.fit_pos_host(HAND_CALL, HAND_WIN, HAND_W0)
    assert counts.tolist() == [8, 21, 1, 5, 2] and span == (0, 24)
    assert ops.tolist() == HAND_OPS and rpos.tolist() == HAND_RPOS
    ref = hand_reference()
    pile = np.zeros((9, ref.total), np.uint32)
    A.pile_add_host(pile, HAND_CALL, ops, rpos)
    for plane in range(9):
        assert np.flatnonzero(pile[plane]).tolist() == HAND_PILE.get(plane, []), plane
    assert pile.max() == 1 and pile.sum() == 22 + 2 + 1
    cons, ins, cov, rec = A.consensus_host(pile, ref, 1)
    assert cons.dtype == ins.dtype == np.uint8 and cov.dtype == np.int32 and rec.dtype == np.int64
    want = np.full(ref.total, NONE, np.uint8)
    for plane, where in HAND_PILE.items():
        if plane < 5:
            want[where] = plane
    assert cons.tolist() == want.tolist()
    assert np.flatnonzero(ins != NONE).tolist() == [116] and ins[116] == 1
    assert np.flatnonzero(cov).tolist() == list(range(100, 124)) and cov.max() == 1
    assert rec.tolist() == [[24, 21, 1, 2, 1, 24]]  # called, match, sub, del, ins, cov_sum
    assert A.consensus_host(pile, ref, 2)[3].tolist() == [[0] * 6]
    # the texts
    fa = A.consensus_fasta(ref, cons, ins)
    # the stated limit: the inserted CCC is named by its first base only
    text = "GATCT" + "G" + "CGGT" + "AGCTT" + "C" + "GCATCCG"
    assert fa == ">hand called=24 identity=%.6f\n%s\n" % (21 / 25, "N" * 100 + text + "N" * 6)
    assert A.variant_lines(ref, cons, ins, cov, pile) == ["hand\t106\tA\tG\t1\t1\n", "hand\t111\tC\t-\t1\t1\n",
                                                          "hand\t112\tA\t-\t1\t1\n", "hand\t117\t-\tC\t1\t1\n"]
    assert A.coverage_lines(ref, rec) == ["hand\t130\t24\t1.00\t21\t1\t2\t1\t0.840000\n",
                                          "total\t130\t24\t1.00\t21\t1\t2\t1\t0.840000\n"]
    # a second, identical read doubles every count; a pair that is not aligned (rpos -1 throughout) adds nothing
    A.pile_add_host(pile, HAND_CALL, ops, rpos)
    A.pile_add_host(pile, HAND_CALL, np.zeros(len(HAND_CALL), np.uint8), np.full(len(HAND_CALL), -1, np.int32))
    assert pile.max() == 2 and pile.sum() == 50


def test_positions_outside_the_reference_are_skipped():
    """rpos is not trusted: whatever lies outside [0, total) adds nothing, and what lies inside still does."""
    call = "ACGTAC"
    ops = np.asarray([0, 0, 2, 0, 0, 0], np.uint8)
    pile = np.zeros((9, 10), np.uint32)
    A.pile_add_host(pile, call, ops, np.asarray([-3, -1, -1, 2, 8, 12], np.int32))
    assert np.argwhere(pile).tolist() == [[0, 8], [3, 2], [4, 0], [4, 1], [4, 3], [4, 4], [4, 5], [4, 6], [4, 7], [4, 9]]
    pile[:] = 0  # the insertion's anchor inside: piled; a descending pair deletes nothing
    A.pile_add_host(pile, call, ops, np.asarray([5, 4, 4, 6, 2, 2 ** 31 - 1], np.int32))
    assert np.argwhere(pile).tolist() == [[0, 2], [0, 5], [1, 4], [3, 6], [4, 3], [4, 4], [4, 5], [4, 6], [4, 7],
                                          [4, 8], [4, 9], [7, 4]]


# ---------------------------------------------------------------- ties and thresholds
def threshold_case():
    """(reference of two records, pile, rows): rows[r] = (cons, ins) expected at min_cov 5 for the planted columns
    of the issue; every other column is empty.  Shared with the device tests."""
    ref = A.Reference(["t0", "t1"], ["ACGTNACGTACG", "TTTTACGT"])
    pile = np.zeros((9, ref.total), np.uint32)
    rows = {}

    def plant(r, col, want):
        pile[:, r] = col
        rows[r] = want
    plant(0, [3, 3, 0, 0, 0, 0, 0, 0, 0], (0, NONE))    # a two-way tie: the lower index
    plant(1, [0, 2, 0, 2, 2, 0, 0, 0, 0], (1, NONE))    # a three-way tie with D
    plant(2, [0, 0, 2, 0, 2, 0, 0, 0, 0], (NONE, NONE))  # cov 4 = min_cov - 1: uncalled
    plant(3, [0, 0, 0, 5, 0, 0, 0, 0, 0], (3, NONE))    # cov 5 = min_cov: called
    plant(4, [0, 0, 6, 0, 0, 0, 0, 0, 0], (2, NONE))    # a reference N: a substitution
    plant(5, [6, 0, 0, 0, 0, 1, 1, 1, 0], (0, NONE))    # 2 ins = cov: no insertion
    plant(6, [0, 7, 0, 0, 0, 0, 2, 2, 0], (1, 1))       # 2 ins = cov + 1: an insertion, its tie the lower index
    plant(7, [0, 0, 0, 0, 9, 0, 0, 0, 5], (4, 3))       # a deleted base with an insertion after it
    plant(8, [1, 0, 0, 1, 0, 9, 0, 0, 0], (NONE, NONE))  # insertions on an uncalled position: none
    plant(12, [0, 0, 0, 8, 0, 0, 0, 0, 0], (3, NONE))   # the second record's first base: a match
    plant(19, [0, 0, 0, 2, 6, 0, 0, 0, 0], (4, NONE))   # its last: deleted
    return ref, pile, rows


def test_ties_and_thresholds():
    ref, pile, rows = threshold_case()
    cons, ins, cov, rec = A.consensus_host(pile, ref, 5)
    for r in range(ref.total):
        assert (int(cons[r]), int(ins[r])) == rows.get(r, (NONE, NONE)), r
    assert cov.tolist() == pile[:5].astype(np.int64).sum(axis=0).tolist()
    # t0: called 0, 1, 3, 4, 5, 6, 7 (ref A C T N A C G): match at 0, 1, 3, 5, 6; sub at 4 (the N); del at 7
    assert rec.tolist() == [[7, 5, 1, 1, 2, 6 + 6 + 5 + 6 + 6 + 7 + 9], [2, 1, 0, 1, 0, 16]]
    cons1, ins1, _, rec1 = A.consensus_host(pile, ref, 1)
    assert (int(cons1[2]), int(cons1[8]), int(ins1[8])) == (2, 0, 0) and rec1[0, 0] == 9
    with pytest.raises(ValueError):
        A.consensus_host(pile, ref, 0)
    lines = A.variant_lines(ref, cons, ins, cov, pile)
    assert lines == ["t0\t5\tN\tG\t6\t6\n", "t0\t7\t-\tC\t7\t2\n", "t0\t8\tG\t-\t9\t9\n", "t0\t8\t-\tT\t9\t5\n",
                     "t1\t8\tT\t-\t8\t6\n"]
    assert A.consensus_fasta(ref, cons, ins) == (">t0 called=7 identity=%.6f\nACNTGACCTNNNN\n>t1 called=2 identity=%.6f\n"
                                                 "TNNNNNN\n" % (5 / 9, 1 / 2))


# ---------------------------------------------------------------- planted variants
def planted_variants(seed, step, rate, length=4000, n_var=12, read_len=400):
    """(reference, mutated genome, reads): a seeded genome with n_var variants (substitutions, 1-base deletions,
    1-base insertions in turn) at least 200 bases from its ends and 50 apart, and reads of the mutated genome
    every ``step`` bases with ``rate`` errors, alternately reverse-complemented.  Shared with the device tests."""
    rng = np.random.default_rng(seed)
    genome = random_seq(rng, length)
    where = np.sort(rng.choice(np.arange(200, length - 200, 50), n_var, replace=False))
    parts, prev = [], 0
    for k, p in enumerate(where.tolist()):
        parts.append(genome[prev:p])
        if k % 3 == 0:
            parts.append("ACGT"[("ACGT".index(genome[p]) + 1 + k % 3) % 4])
        elif k % 3 == 2:
            parts.append(genome[p] + "ACGT"[int(rng.integers(0, 4))])
        prev = p + 1
    mutated = "".join(parts) + genome[prev:]
    reads = []
    for k, lo in enumerate(range(0, len(mutated) - read_len + 1, step)):
        r = mutated[lo: lo + read_len]
        r = mutate(rng, r, rate) if rate else r
        reads.append(A.reverse_complement(r).tobytes().decode() if k % 2 else r)
    return A.Reference(["genome"], [genome]), mutated, reads


def check_planted(ref, mutated, stats, counts, cons, ins, min_cov):
    """The issue's condition; returns (the consensus over the called interval, its counts against the mutated
    genome)."""
    assert stats["unmapped"] == 0 and stats["reads"] == stats["segments"]
    called = np.flatnonzero(cons != NONE)
    lo, hi = int(called[0]), int(called[-1]) + 1
    assert hi - lo > 3000 and (cons[lo:hi] != NONE).all()  # no N inside the called interval
    text = fasta_sequence_of(A.consensus_fasta(ref, cons, ins)).strip("N")
    assert "N" not in text
    c, span, _ = A.fit_host(text, mutated)
    assert c.tolist() == [0, len(text), 0, 0, 0], (c.tolist(), span)  # the mutated genome, exactly
    return text, c


def fasta_sequence_of(text):
    return text.split("\n")[1]


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_planted_variants_from_error_free_reads(seed):
    ref, mutated, reads = planted_variants(seed, step=40, rate=0.0)
    pile, stats = A.Pileup(ref), {}
    counts, recs, _ = pile.add(reads, stats=stats)
    cons, ins, cov, rec = pile.call(3)
    check_planted(ref, mutated, stats, counts, cons, ins, 3)
    lines = A.variant_lines(ref, cons, ins, cov, pile.counts())
    assert len(lines) == 12 and rec[0, 2] == 4 and rec[0, 3] == 4 and rec[0, 4] == 4
    assert A.identity(counts.sum(axis=0)) > 0.99  # the reads against the unmutated reference: the variants only


@pytest.mark.parametrize("seed", (1, 2))
def test_planted_variants_from_reads_with_errors(seed):
    ref, mutated, reads = planted_variants(seed, step=20, rate=0.10)
    pile, stats = A.Pileup(ref), {}
    counts, recs, _ = pile.add(reads, stats=stats)
    cons, ins, cov, rec = pile.call(5)
    text, c = check_planted(ref, mutated, stats, counts, cons, ins, 5)
    pooled = A.identity(counts.sum(axis=0))
    assert 0.85 < pooled < 0.93 and A.identity(c) > pooled
    assert len(A.variant_lines(ref, cons, ins, cov, pile.counts())) == 12


def test_pileup_add_returns_what_map_reads_returns():
    ref, mutated, reads = planted_variants(4, step=400, rate=0.10)
    reads = reads[:4] + ["ACGT"]
    hs, ps = {}, {}
    want = A.map_reads(reads, ref, want_ops=True, stats=hs)
    pile = A.Pileup(ref)
    got = pile.add(reads, want_ops=True, stats=ps)
    assert hs == ps and got[0].tobytes() == want[0].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[2], want[2]))
    assert [[r[:7] for r in rr] for rr in got[1]] == [[r[:7] for r in rr] for rr in want[1]]
    assert pile.add(reads[:1])[2] is None
    t = pile.counts()
    assert t.shape == (9, ref.total) and t.dtype == np.uint32 and t[:4].sum() == sum(
        int(c[1] + c[2]) for c in want[0]) + int(want[0][0][1] + want[0][0][2])
    t[:] = 0
    assert pile.counts().any()  # a copy


# ---------------------------------------------------------------- translate.py -truth_ref -consensus
def test_cli_consensus_end_to_end(tmp_path, monkeypatch):
    import nanodecoder_amd.translator as T
    monkeypatch.setattr(T, "Engine", _Eng)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    from nanodecoder_amd import frontend

    def fake(preds):  # as test_cli_truth_ref_end_to_end: a seeded sequence per read, told apart by its chunks
        r = np.random.default_rng(len(preds))
        n = 150 + 20 * len(preds)
        return random_seq(r, n), "".join(chr(33 + int(v)) for v in r.integers(0, 41, n))
    monkeypatch.setattr(frontend, "assemble_read", lambda preds, *a, **k: fake(preds)[0])
    monkeypatch.setattr(frontend, "assemble_read_q", lambda preds, w, *a, **k: fake(preds))
    monkeypatch.setattr(frontend, "assemble_reads",
                        lambda reads, *a, **k: [fake(p) if k.get("weights") else fake(p)[0] for p in reads])
    ck, src = make_reads(tmp_path)
    argv = lambda out: ["-model", str(ck), "-src_dir", str(src), "-save_data", str(out), "-gpu", "0",  # noqa: E731
                        "-beam_size", "1", "-batch_size", "2", "-thread", "2", "-max_length", "10", "-pack_reads",
                        "2", "-src_seq_length", "300", "-src_seq_stride", "100"]
    plain = tmp_path / "plain"
    assert cli.main(opts.parse_translate_opts(argv(plain))) == 3
    called = {f"read{i}": A.normalise(fasta_sequence(plain / "result" / f"read{i}.fasta")) for i in range(3)}
    # the reference: read0's call with one base changed and one left out, forward, in one record; read1's reverse
    # complement in another; a third record nothing maps to; read2 is nowhere
    rng = np.random.default_rng(4321)
    r0 = called["read0"]
    r0 = r0[:60] + "ACGT"[("ACGT".index(r0[60]) + 1) % 4] + r0[61:100] + r0[101:]
    rc1 = A.reverse_complement(called["read1"]).tobytes().decode()
    ref_file = tmp_path / "ref.fasta"
    ref_file.write_text(">ctgA x\n" + random_seq(rng, 700) + r0 + random_seq(rng, 300) + "\n>ctgB\n"
                        + random_seq(rng, 900) + "\n" + rc1 + random_seq(rng, 50) + "\n>ctgC\n" + random_seq(rng, 80)
                        + "\n")
    ref = A.read_reference(str(ref_file))
    without, log0 = tmp_path / "without", tmp_path / "log0.txt"
    base = ["-truth_ref", str(ref_file), "-truth_align", "cpu", "-fastq"]
    assert cli.main(opts.parse_translate_opts(argv(without) + base + ["-log_file", str(log0)])) == 3
    for f in ("consensus.fasta", "variants.tsv", "coverage.tsv"):
        assert not (without / f).exists()
    assert "-consensus" not in log0.read_text()
    out, log = tmp_path / "with", tmp_path / "log.txt"
    o = opts.parse_translate_opts(argv(out) + base + ["-consensus", "-consensus_min_cov", "1", "-log_file", str(log)])
    assert o.consensus and o.consensus_min_cov == 1
    assert opts.parse_translate_opts(argv(out) + base + ["-consensus"]).consensus_min_cov == 5
    assert cli.main(o) == 3
    # nothing that existed changes
    for f in ("accuracy.tsv", "mapping.paf", "quality_calibration.tsv"):
        assert (out / f).read_bytes() == (without / f).read_bytes(), f
    for d in ("result", "segment"):
        for f in (plain / d).iterdir():
            assert (out / d / f.name).read_bytes() == f.read_bytes(), f
    # the three files, against the host rule on the written reads
    pile = A.Pileup(ref)
    pile.add(list(called.values()))
    cons, ins, cov, rec = pile.call(1)
    variants = A.variant_lines(ref, cons, ins, cov, pile.counts())
    assert (out / "consensus.fasta").read_text() == A.consensus_fasta(ref, cons, ins)
    assert (out / "variants.tsv").read_text() == "".join(variants)
    assert (out / "coverage.tsv").read_text() == "".join(A.coverage_lines(ref, rec))
    n0, n1 = len(called["read0"]), len(called["read1"])
    assert rec.tolist() == [[n0 - 1, n0 - 2, 1, 0, 1, n0 - 1], [n1, n1, 0, 0, 0, n1], [0] * 6]
    assert len(variants) == 2 and variants[0] == "ctgA\t761\t%s\t%s\t1\t1\n" % (r0[60], called["read0"][60])
    name, pos, was, alt, c, n = variants[1].rstrip("\n").split("\t")  # the left-out base: an insertion in the call,
    assert (name, was, c, n) == ("ctgA", "-", "1", "1")               # placed up to its homopolymer
    assert abs(int(pos) - 800) <= 3 and alt == called["read0"][int(pos) - 700]
    fa = (out / "consensus.fasta").read_text().split("\n")
    assert fa[0] == ">ctgA called=%d identity=%.6f" % (n0 - 1, (n0 - 2) / n0) and fa[2].startswith(">ctgB called=")
    assert len(fa) == 5 and fa[1].strip("N") == called["read0"] and fa[3].strip("N") == rc1
    assert len(fa[1]) == 1000 + len(r0) + 1 and len(fa[3]) == 950 + n1
    cov_lines = (out / "coverage.tsv").read_text().splitlines()
    assert [ln.split("\t")[0] for ln in cov_lines] == ["ctgA", "ctgB", "ctgC", "total"]
    assert cov_lines[2] == "ctgC\t80\t0\t0.00\t0\t0\t0\t0\t0.000000"
    want_log = A.consensus_summary(ref, rec, 1, 2)
    assert want_log in log.read_text() and "%d of %d reference bases called at coverage >= 1" % (
        n0 - 1 + n1, ref.total) in want_log and "2 variant lines" in want_log
    # a resumed run translates nothing and piles nothing: the reads already done are not in the pile
    assert cli.main(o) == 0
    assert (out / "consensus.fasta").read_text() == "" and (out / "variants.tsv").read_text() == ""
    assert (out / "accuracy.tsv").read_bytes() == (without / "accuracy.tsv").read_bytes()


def test_cli_consensus_flag_errors(tmp_path):
    base = ["-model", "m.pt", "-src_dir", str(tmp_path), "-save_data", str(tmp_path / "o"), "-gpu", "0"]
    for extra in (["-consensus"], ["-consensus", "-truth", str(tmp_path / "t.fasta")],
                  ["-consensus", "-truth_ref", str(tmp_path / "r.fasta"), "-consensus_min_cov", "0"]):
        with pytest.raises(ValueError):
            cli.main(opts.parse_translate_opts(base + extra))
        assert not (tmp_path / "o").exists()
    o = opts.parse_translate_opts(base)
    assert o.consensus is False and o.consensus_min_cov == 5


# ---------------------------------------------------------------- argument errors, no device
def test_consensus_argument_errors_without_gpu():
    from nanodecoder_amd import _lib, build
    build.build()
    L = _lib.lib()
    ERR = _lib.ND_ERR_ARG
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before any HIP call
    need = L.nd_align_fit_pos_work_bytes(3, 1000)
    assert need == L.nd_align_fit_work_bytes(3, 1000) and L.nd_align_fit_pos_work_bytes(-1, 1) < 0
    fit = [p, p, p, 100, p, 3, 1000, p, p, None, p, p, p, need, None]
    for k in (0, 1, 2, 4, 7, 8, 10, 11, 12):  # 9 is d_ops: nullable; 10 is d_rpos: required
        args = list(fit)
        args[k] = None
        assert L.nd_align_fit_pos(*args) == ERR, k
        assert b"null" in L.nd_last_error()
    for k, v in ((3, -1), (5, -1), (6, -1), (13, need - 1)):
        args = list(fit)
        args[k] = v
        assert L.nd_align_fit_pos(*args) == ERR and b"align_fit_pos" in L.nd_last_error()
    assert L.nd_align_fit_pos(ctypes.c_void_p(4100), p, p, 100, p, 3, 1000, p, p, None, p, p, ctypes.c_void_p(4100),
                              need, None) == ERR and b"aligned" in L.nd_last_error()
    assert L.nd_align_fit_pos(None, None, None, 0, None, 0, 0, None, None, None, None, None, None, 0, None) == 0
    add = [p, p, p, p, p, 3, p, 100, None]
    for k in (0, 1, 2, 3, 4, 6):
        args = list(add)
        args[k] = None
        assert L.nd_pileup_add(*args) == ERR, k
        assert b"null" in L.nd_last_error()
    for k in (5, 7):
        args = list(add)
        args[k] = -1
        assert L.nd_pileup_add(*args) == ERR and b"pileup_add" in L.nd_last_error()
    assert L.nd_pileup_add(None, None, None, None, None, 0, None, 100, None) == 0
    assert L.nd_pileup_add(None, None, None, None, None, 3, None, 0, None) == 0
    call = [p, p, 100, p, 2, 5, p, p, p, p, None]
    for k in (0, 1, 3, 6, 7, 8, 9):
        args = list(call)
        args[k] = None
        assert L.nd_pileup_call(*args) == ERR, k
        assert b"null" in L.nd_last_error()
    for k, v in ((2, -1), (4, -1), (5, 0), (5, -3)):
        args = list(call)
        args[k] = v
        assert L.nd_pileup_call(*args) == ERR and b"pileup_call" in L.nd_last_error()
    assert L.nd_pileup_call(None, None, 0, None, 2, 5, None, None, None, None, None) == 0
    assert L.nd_pileup_call(None, None, 100, None, 0, 5, None, None, None, None, None) == 0
    assert L.nd_pileup_call(None, None, 0, None, 0, 0, None, None, None, None, None) == ERR  # min_cov first
