"""Read mapping on the host (CPU only): accuracy.fit_host against a cell-by-cell table with the rule's traceback,
the k-mer index and locate_host against a plain dictionary restatement, the segmentation, reads planted in a
reference, translate.py -truth_ref end to end with the stand-in engine, and the argument errors of nd_locate_segs
and nd_align_fit."""
import ctypes

import numpy as np
import pytest
import torch

from nanodecoder_amd import accuracy, cli, opts
from tests.test_accuracy_host import (_Eng, fasta_sequence, host_pairs, make_reads, mutate, plain_align,
                                      random_seq)

A = accuracy


# ---------------------------------------------------------------- the rules, restated as plainly as possible
def plain_fit(a, b):
    a, b = a.encode(), b.encode()
    n, m = len(a), len(b)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        D[i][0] = i
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    jstar = min(range(m + 1), key=lambda j: (D[n][j], j))
    ops = [0] * n
    i, j = n, jstar
    match = sub = ins = dele = 0
    while i > 0:
        if j >= 1 and D[i - 1][j - 1] + (a[i - 1] != b[j - 1]) == D[i][j]:
            if a[i - 1] != b[j - 1]:
                ops[i - 1] = 1
                sub += 1
            else:
                match += 1
            i, j = i - 1, j - 1
        elif j == 0 or D[i - 1][j] + 1 == D[i][j]:
            ops[i - 1] = 2
            ins += 1
            i -= 1
        else:
            dele += 1
            j -= 1
    assert D[n][jstar] == sub + ins + dele
    return [D[n][jstar], match, sub, ins, dele], (j, jstar), ops


def plain_index(names_seqs):
    """{k-mer text: [positions in the concatenation]} without the k-mers occurring more than MAP_OCC_MAX times."""
    out, base = {}, 0
    for s in names_seqs:
        for p in range(len(s) - A.MAP_K + 1):
            k = s[p: p + A.MAP_K]
            if set(k) <= set("ACGT"):
                out.setdefault(k, []).append(base + p)
        base += len(s)
    return {k: v for k, v in out.items() if len(v) <= A.MAP_OCC_MAX}


def plain_locate(q, seqs):
    idx, total = plain_index(seqs), sum(len(s) for s in seqs)
    n = len(q)
    if n < A.MAP_K:
        return False, 0, 0, 0, 0
    best = (0, 0, 0)
    for strand in (0, 1):
        qs = q if strand == 0 else A.reverse_complement(q).tobytes().decode()
        votes = {}
        for x in range(n - A.MAP_K + 1):
            for y in idx.get(qs[x: x + A.MAP_K], ()):
                b = (y - x + A.MAP_SEG) >> A.MAP_BIN_SHIFT
                votes[b] = votes.get(b, 0) + 1
        for b in sorted(set(votes) | {v - 1 for v in votes if v > 0}):
            sc = votes.get(b, 0) + votes.get(b + 1, 0)
            if sc > best[0]:
                best = (sc, strand, b)
    sc, strand, b = best
    if sc < A.MAP_MIN_VOTES:
        return False, strand, 0, 0, sc
    lo = (b << 9) - A.MAP_SEG
    c = min(max(lo + 512 + n // 2, 0), total - 1)
    start = 0
    for s in seqs:
        if start <= c < start + len(s):
            break
        start += len(s)
    return True, strand, max(start, lo - A.MAP_PAD), min(start + len(s), lo + 1024 + n + A.MAP_PAD), sc


def code_of(kmer):
    v = 0
    for ch in kmer:
        v = v * 4 + "ACGT".index(ch)
    return v


FIT_FIXED = [("A", "AAAA"),          # ties in the last row: j* = 1
             ("ACGT", "TTTT"),       # one base matches somewhere
             ("GGGG", "ACAC"),       # nothing matches: D[n][j] = n everywhere, j* = 0
             ("ACGT", "ACGT"),       # j* = m
             ("ACGT", "TTACGT"),     # j* = m, t_start = 2
             ("ACGT", "ACGTTT"),     # t_end = 4 < m
             ("", "ACGT"), ("ACGT", ""), ("", ""),
             ("TTTTACGTACGT", "ACGTACGTCC"),  # the path reaches column 0 with i > 0
             ("AAAA", "AA"), ("ACAC", "CACA")]


def fit_pairs(seed=3):
    rng = np.random.default_rng(seed)
    pairs = list(FIT_FIXED)
    for n in (1, 2, 7, 31, 64, 65):
        w = random_seq(rng, 3 * n + 5)
        pairs.append((mutate(rng, w[n: 2 * n], 0.15), w))
        pairs.append((random_seq(rng, n, "AC"), random_seq(rng, n + 3, "AC")))
    return pairs


@pytest.mark.parametrize("k", range(len(FIT_FIXED) + 12))
def test_fit_host_equals_the_plain_table(k):
    call, window = fit_pairs()[k]
    want = plain_fit(call, window)
    counts, span, ops = A.fit_host(call, window)
    assert counts.dtype == np.int32 and ops.dtype == np.uint8
    assert (counts.tolist(), tuple(span), ops.tolist()) == want
    c = counts.tolist()
    assert c[1] + c[2] + c[3] == len(call) and c[1] + c[2] + c[4] == span[1] - span[0] and c[0] == c[2] + c[3] + c[4]


def test_fit_by_hand():
    c, span, o = A.fit_host("A", "AAAA")
    assert c.tolist() == [0, 1, 0, 0, 0] and span == (0, 1) and o.tolist() == [0]
    c, span, o = A.fit_host("ACGT", "ACGT")
    assert span == (0, 4) and c.tolist() == [0, 4, 0, 0, 0]
    c, span, o = A.fit_host("", "ACGT")
    assert c.tolist() == [0] * 5 and span == (0, 0) and o.size == 0
    c, span, o = A.fit_host("ACGT", "")
    assert c.tolist() == [4, 0, 0, 4, 0] and span == (0, 0) and o.tolist() == [2] * 4
    c, span, o = A.fit_host("G", "AC")  # D[1] = 1, 1, 1: j* = 0, one insertion
    assert c.tolist() == [1, 0, 0, 1, 0] and span == (0, 0) and o.tolist() == [2]
    c, span, o = A.fit_host("TTTTACGTACGT", "ACGTACGTCC")
    assert span == (0, 8) and c.tolist() == [4, 8, 0, 4, 0] and o.tolist() == [2] * 4 + [0] * 8


# ---------------------------------------------------------------- the index
def test_index_against_the_plain_dictionary():
    rng = np.random.default_rng(7)
    k8, k9 = "ACGTTGCAAGCTTAC", "GGATCCTTAGACCAT"
    spacer = lambda: random_seq(rng, 40)  # noqa: E731
    rec0 = "".join(spacer() + k8 for _ in range(8)) + "".join(spacer() + k9 for _ in range(9)) + spacer()
    rec1 = random_seq(rng, 100) + "N" + random_seq(rng, 60) + "nn".upper() + random_seq(rng, 20)
    rec2 = random_seq(rng, 14)  # too short for a k-mer
    seqs = [rec0, rec1, "", rec2, random_seq(rng, 15)]
    ref = A.Reference(["r%d" % i for i in range(len(seqs))], seqs)
    assert ref.rec_off.tolist() == np.cumsum([0] + [len(s) for s in seqs]).tolist()
    code, pos = ref.index
    assert code.dtype == pos.dtype == np.uint32
    want = sorted((code_of(k), p) for k, v in plain_index(seqs).items() for p in v)
    assert list(zip(code.tolist(), pos.tolist())) == want
    assert int((code == code_of(k8)).sum()) == 8 and int((code == code_of(k9)).sum()) == 0
    # no k-mer across a record boundary or over the N
    b01 = len(rec0)
    assert not any(b01 - 14 <= p < b01 for p in pos.tolist())
    assert not any(b01 + 100 - 14 <= p <= b01 + 100 for p in pos.tolist())
    assert ref.record_of(b01 - 1) == 0 and ref.record_of(b01) == 1 and ref.record_of(len(rec0) + len(rec1)) == 3


def test_read_reference(tmp_path):
    f = tmp_path / "ref.fasta"
    f.write_text("junk\n>chr1 first\nacgt\nACMm\n>chr2\nGGNN\n\nTT\n>chr1\nAC\n")
    ref = A.read_reference(str(f))
    assert ref.names == ["chr1", "chr2", "chr1"] and ref.seq.tobytes() == b"ACGTACCCGGNNTTAC"
    assert ref.rec_off.tolist() == [0, 8, 14, 16] and ref.rec_off.dtype == np.int32
    with pytest.raises(ValueError):
        A.Reference(["big"], [np.zeros(A.MAP_REF_MAX + 1, np.uint8)])


# ---------------------------------------------------------------- locate
def locate_cases(seed=11):
    """(name, query, the reference's records): the cases of the issue; shared with the device tests."""
    rng = np.random.default_rng(seed)
    cases = []
    half = random_seq(rng, 100)
    pal = half + A.reverse_complement(half).tobytes().decode()
    cases.append(("palindrome", pal, [random_seq(rng, 1500) + pal + random_seq(rng, 1500)]))
    s = random_seq(rng, 300)
    cases.append(("bin tie", s, [random_seq(rng, 1000) + s + random_seq(rng, 2000) + s + random_seq(rng, 700)]))
    cases.append(("bin edge", s, [random_seq(rng, 1024) + s + random_seq(rng, 900)]))
    one = random_seq(rng, 3000)
    cases.append(("n 14", one[100:114], [one]))
    cases.append(("n 15", one[100:115], [one]))
    cases.append(("votes 7", one[500:521], [one]))
    cases.append(("votes 8", one[500:522], [one]))
    two = [random_seq(rng, 3000), random_seq(rng, 3000)]
    cases.append(("record start", two[0][:500], two))
    cases.append(("record end", two[1][-500:], two))
    cases.append(("before a boundary", two[0][-400:], two))
    cases.append(("after a boundary", mutate(rng, two[1][200:800], 0.1), two))
    cases.append(("reverse strand", A.reverse_complement(mutate(rng, two[1][1000:2000], 0.1)).tobytes().decode(), two))
    cases.append(("an N inside", one[700:800] + "N" + one[801:900], [one]))
    cases.append(("unrelated", random_seq(rng, 400), two))
    return cases


@pytest.mark.parametrize("k", range(14))
def test_locate_host_equals_the_plain_rule(k):
    name, q, seqs = locate_cases()[k]
    ref = A.Reference(["r%d" % i for i in range(len(seqs))], seqs)
    got = A.locate_host(q, ref)
    assert tuple(got) == plain_locate(q, seqs), name
    mapped, strand, w0, w1, votes = got
    total = ref.total
    if name == "palindrome":
        assert mapped and strand == 0 and votes == 200 - 14
    if name == "bin tie":  # both copies and both bins of each score 286: the lowest bin of the first copy
        assert votes == 286 and w0 == max(0, ((((1000 + 4096) >> 9) - 1) << 9) - 4096 - 1024)
    if name == "bin edge":  # the diagonal 1024 is the first of bin 10: bins 9 and 10 tie, 9 wins
        assert votes == 286 and (w0, w1) == (0, min(total, (9 << 9) - 4096 + 1024 + 300 + 1024))
    if name in ("n 14", "n 15", "votes 7", "unrelated"):
        assert not mapped and (w0, w1) == (0, 0) and votes == {"n 14": 0, "n 15": 1, "votes 7": 7}.get(name, votes)
    if name == "votes 8":
        assert mapped and votes == 8
    if name == "record start":
        assert mapped and w0 == 0 and w1 < 3000
    if name == "record end":
        assert mapped and w1 == 6000 and w0 > 3000
    if name == "before a boundary":
        assert mapped and w1 == 3000 and w0 < 2600
    if name == "after a boundary":
        assert mapped and w0 == 3000 and w1 > 3600
    if name == "reverse strand":
        assert mapped and strand == 1 and w0 <= 4000 and w1 >= 5000
    if mapped:
        assert 0 <= w0 < w1 <= total and w1 - w0 <= len(q) + 3072


def test_segments():
    assert A.segments(0) == [(0, 0)] and A.segments(4096) == [(0, 4096)]
    assert A.segments(4097) == [(0, 2048), (2048, 4097)]
    assert A.segments(12289) == [(0, 3072), (3072, 6144), (6144, 9216), (9216, 12289)]
    for n in (1, 4095, 8192, 8193, 100000):
        sg = A.segments(n)
        assert len(sg) == -(-n // 4096) and sg[0][0] == 0 and sg[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(sg, sg[1:])) and all(0 < e - s <= 4096 for s, e in sg)


# ---------------------------------------------------------------- planted reads
RATE = 0.10


def planted_reads(seed=23, lengths=(500, 1000, 2500, 4096, 5000, 700, 1500, 3000)):
    """(reference, [(call, strand, start, end) in the concatenation's coordinates])."""
    rng = np.random.default_rng(seed)
    seqs = [random_seq(rng, 35000), random_seq(rng, 25000)]
    ref = A.Reference(["chrA", "chrB"], seqs)
    cat = "".join(seqs)
    reads = []
    for k, n in enumerate(lengths):
        r = k % 2
        lo = int(ref.rec_off[r]) + int(rng.integers(0, len(seqs[r]) - n))
        call = mutate(rng, cat[lo: lo + n], RATE)
        strand = int(rng.integers(0, 2)) if k >= 2 else k
        reads.append((A.reverse_complement(call).tobytes().decode() if strand else call, strand, lo, lo + n))
    return ref, reads


@pytest.fixture(scope="module")
def planted():
    ref, reads = planted_reads()
    return ref, reads, [A.map_host(r[0], ref) for r in reads]


def test_planted_reads_map_where_they_came_from(planted):
    ref, reads, res = planted
    assert {r[1] for r in reads} == {0, 1}
    for (call, strand, lo, hi), (counts, recs, ops) in zip(reads, res):
        sg = A.segments(len(call))
        assert [(r[0], r[1]) for r in recs] == sg                      # every segment mapped
        assert all(r[2] == strand for r in recs)
        assert all(r[3] == ref.record_of(lo) for r in recs)
        assert abs(min(r[4] for r in recs) - lo) <= 8 and abs(max(r[5] for r in recs) - hi) <= 8
        assert abs(A.identity(counts) - (1 - RATE)) <= 0.03
        assert counts.tolist() == np.sum([r[7] for r in recs], axis=0).tolist()
        assert ops.size == len(call) and (ops <= 2).all()
        assert int((ops == 0).sum()) == counts[1] and int((ops == 2).sum()) == counts[3]
        for r in recs:  # consecutive segments tile the reference, in the strand's direction
            assert r[7][1] + r[7][2] + r[7][3] == r[1] - r[0] and r[7][1] + r[7][2] + r[7][4] == r[5] - r[4]


def test_map_reads_host_path(planted):
    ref, reads, res = planted
    stats = {}
    calls = [r[0] for r in reads[:3]] + ["ACGT", random_seq(np.random.default_rng(1), 300)]
    counts, recs, ops = A.map_reads(calls, ref, want_ops=True, stats=stats)
    assert counts.shape == (5, 5) and counts.dtype == np.int32
    for k in range(3):
        assert counts[k].tolist() == res[k][0].tolist() and ops[k].tobytes() == res[k][2].tobytes()
        assert [r[:7] for r in recs[k]] == [r[:7] for r in res[k][1]]
    assert recs[3] == [] and recs[4] == [] and (ops[3] == 255).all() and (ops[4] == 255).all()
    assert counts[3].tolist() == [0] * 5
    assert stats == {"reads": 5, "segments": 5, "unmapped": 2}
    assert A.map_reads(calls[:1], ref)[2] is None
    line = A.paf_line("rd", len(calls[1]), recs[1][0], ref).rstrip("\n").split("\t")
    r = recs[1][0]
    assert len(line) == 13 and line[0] == "rd" and line[4] == "-" and line[5] == "chrB" and line[11] == "255"
    assert [int(v) for v in line[1:4]] == [len(calls[1]), 0, len(calls[1])] and int(line[6]) == 25000
    assert [int(line[7]), int(line[8])] == [r[4] - 35000, r[5] - 35000]
    assert int(line[9]) == r[7][1] and int(line[10]) == int(r[7][1:].sum()) and line[12] == "vt:i:%d" % r[6]


def test_map_host_is_map_reads_of_one_call_and_records_have_names():
    rng = np.random.default_rng(41)
    seqs = [random_seq(rng, 2500), random_seq(rng, 1500)]
    ref = A.Reference(["a", "b"], seqs)
    calls = [mutate(rng, seqs[0][700:1100], 0.1),
             A.reverse_complement(mutate(rng, seqs[1][300:800], 0.1)).tobytes().decode(),
             random_seq(rng, 300), "ACGT", ""]
    n_records = 0
    for c in calls:
        counts, recs, ops = A.map_host(c, ref)
        rc, rr, ro = A.map_reads([c], ref, want_ops=True)
        assert counts.dtype == np.int32 and counts.tolist() == rc[0].tolist() and len(rc) == len(rr) == len(ro) == 1
        assert ops.dtype == np.uint8 and ops.tobytes() == ro[0].tobytes() and ops.size == len(c)
        assert [(r[:7], r[7].tolist()) for r in recs] == [(r[:7], r[7].tolist()) for r in rr[0]]
        for r in recs:
            n_records += 1
            assert isinstance(r, tuple) and len(r) == 8 and A.Segment._fields == (
                "seg_start", "seg_end", "strand", "rec", "ref_start", "ref_end", "votes", "counts")
            assert (r.seg_start, r.seg_end, r.strand, r.rec, r.ref_start, r.ref_end, r.votes) == r[:7]
            assert r.counts is r[7] and r.counts.dtype == np.int32
    assert n_records == 2 and [bool(A.map_host(c, ref)[1]) for c in calls] == [True, True, False, False, False]


# ---------------------------------------------------------------- one DP for the global and the fit form
def dp_pairs(seed=17):
    """host_pairs(), FIT_FIXED and 200 seeded pairs of a two-letter alphabet (ties everywhere), lengths 0..40."""
    rng = np.random.default_rng(seed)
    pairs = host_pairs() + FIT_FIXED
    for _ in range(200):
        n, m = (int(v) for v in rng.integers(0, 41, 2))
        pairs.append((random_seq(rng, n, "AC"), random_seq(rng, m, "AC")))
    return pairs


def test_one_dp_equals_both_plain_tables():
    pairs = dp_pairs()
    assert any(not a and b for a, b in pairs) and any(a and not b for a, b in pairs)
    assert sum(len(a) > len(b) for a, b in pairs[-200:]) > 50 and ("", "") in pairs
    for call, truth in pairs:
        counts, ops = A.align_host(call, truth)
        assert counts.dtype == np.int32 and ops.dtype == np.uint8
        assert [counts.tolist(), ops.tolist()] == list(plain_align(call, truth)), (call, truth)
        counts, span, ops = A.fit_host(call, truth)
        assert counts.dtype == np.int32 and ops.dtype == np.uint8
        assert (counts.tolist(), tuple(span), ops.tolist()) == plain_fit(call, truth), (call, truth)
        pc, ps, po, rpos = A.fit_pos_host(call, truth, 100)
        assert (pc.tolist(), tuple(ps), po.tolist()) == (counts.tolist(), tuple(span), ops.tolist())
        assert rpos.dtype == np.int32 and rpos.size == len(call)
        # the positions: from the span's start to its end, a diagonal base past the one before, an inserted one not
        last = 100 + span[0] - 1
        for o, r in zip(po.tolist(), rpos.tolist()):
            assert r >= last if o == 2 else r > last
            last = r
        assert last == 100 + span[1] - 1 or not len(call)


# ---------------------------------------------------------------- translate.py -truth_ref
def test_cli_truth_ref_end_to_end(tmp_path, monkeypatch):
    import nanodecoder_amd.translator as T
    monkeypatch.setattr(T, "Engine", _Eng)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    # the stand-in engine calls three bases per read: the assembly is stood in for too, with a seeded sequence
    # (and qualities) per read, told apart by its number of chunks
    from nanodecoder_amd import frontend

    def fake(preds):
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
    for f in ("accuracy.tsv", "mapping.paf", "quality_calibration.tsv"):
        assert not (plain / f).exists()
    called = {f"read{i}": A.normalise(fasta_sequence(plain / "result" / f"read{i}.fasta")) for i in range(3)}
    # the reference: read0's call forward in one record, read1's reverse complement in another; read2 is nowhere
    rng = np.random.default_rng(1234)
    rc1 = A.reverse_complement(called["read1"]).tobytes().decode()
    ref_file = tmp_path / "ref.fasta"
    ref_file.write_text(">ctgA x\n" + random_seq(rng, 700) + called["read0"].lower() + random_seq(rng, 300) + "\n>ctgB\n"
                        + random_seq(rng, 900) + "\n" + rc1 + random_seq(rng, 50) + "\n")
    ref = A.read_reference(str(ref_file))
    want = {n: A.map_host(c, ref) for n, c in called.items()}
    mapped = sorted(n for n, w in want.items() if w[1])
    assert len(set(called.values())) == 3 and mapped == ["read0", "read1"]
    out, log = tmp_path / "mapped", tmp_path / "log.txt"
    o = opts.parse_translate_opts(argv(out) + ["-truth_ref", str(ref_file), "-truth_align", "cpu", "-fastq",
                                               "-log_file", str(log)])
    assert o.truth_ref == str(ref_file)
    assert cli.main(o) == 3
    for d in ("result", "segment"):
        for f in (plain / d).iterdir():
            assert (out / d / f.name).read_bytes() == f.read_bytes(), f
    lines = {ln.split("\t")[0]: ln for ln in (out / "accuracy.tsv").read_text().splitlines(True)}
    assert sorted(lines) == mapped
    paf = (out / "mapping.paf").read_text().splitlines(True)
    assert sorted(paf) == sorted(A.paf_line(n, len(called[n]), r, ref) for n in mapped for r in want[n][1])
    b, e = np.zeros(41, np.int64), np.zeros(41, np.int64)
    for n in mapped:
        counts, recs, ops = want[n]
        assert lines[n] == A.accuracy_line(n, len(called[n]), sum(r[5] - r[4] for r in recs), counts)
        qual = (out / "result" / (n + ".fastq")).read_text().split("\n")[3]
        keep = ops != 255
        tb, te = A.quality_table(np.frombuffer(qual.encode(), np.uint8)[keep].tobytes(), ops[keep])
        b += tb
        e += te
    assert (out / "quality_calibration.tsv").read_text() == "".join(A.calibration_lines(b, e))
    if "read1" in mapped:
        assert lines["read1"].split("\t")[7] == "1.000000\n" and "\t-\tctgB\t" in "".join(paf)
    nseg = sum(len(A.segments(len(c))) for c in called.values())
    nmap = sum(len(w[1]) for w in want.values())
    assert "-truth_ref: %d reads evaluated, %d reads unmapped, %d segments mapped, %d unmapped; pooled identity" \
        % (len(mapped), 3 - len(mapped), nmap, nseg - nmap) in log.read_text()
    before = (out / "accuracy.tsv").read_bytes(), (out / "mapping.paf").read_bytes()
    assert cli.main(o) == 0 and ((out / "accuracy.tsv").read_bytes(), (out / "mapping.paf").read_bytes()) == before


def test_cli_truth_ref_exclusions(tmp_path):
    base = ["-model", "m.pt", "-src_dir", str(tmp_path), "-save_data", str(tmp_path / "o"), "-gpu", "0",
            "-truth_ref", str(tmp_path / "r.fasta")]
    for extra in (["-attn_debug"], ["-truth", str(tmp_path / "t.fasta")]):
        with pytest.raises(ValueError):
            cli.main(opts.parse_translate_opts(base + extra))
        assert not (tmp_path / "o").exists()
    assert opts.parse_translate_opts(["-model", "m.pt", "-src_dir", "x", "-save_data", "y"]).truth_ref == ""


# ---------------------------------------------------------------- argument errors, no device
def test_mapping_argument_errors_without_gpu():
    from nanodecoder_amd import _lib, build
    build.build()
    L = _lib.lib()
    ERR = _lib.ND_ERR_ARG
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before any HIP call
    q = ctypes.c_void_p(8192)
    loc = [p, p, 3, p, p, 10, p, 1, p, p, q, None]
    for k in (0, 1, 3, 4, 6, 8, 9, 10):
        args = list(loc)
        args[k] = None
        assert L.nd_locate_segs(*args) == ERR, k
        assert b"null" in L.nd_last_error()
    for k, v in ((2, -1), (5, -1), (7, -1)):
        args = list(loc)
        args[k] = v
        assert L.nd_locate_segs(*args) == ERR and b"locate_segs" in L.nd_last_error()
    assert L.nd_locate_segs(p, p, 3, p, p, 10, p, 1, p, p, p, None) == ERR  # in place
    assert L.nd_locate_segs(None, None, 0, None, None, 0, None, 0, None, None, None, None) == 0
    need = L.nd_align_fit_work_bytes(3, 1000)
    assert need == L.nd_align_seqs_work_bytes(3, 1000) and L.nd_align_fit_work_bytes(-1, 1) < 0
    fit = [p, p, p, 100, p, 3, 1000, p, p, None, p, p, need, None]
    for k in (0, 1, 2, 4, 7, 8, 10, 11):  # 9 is d_ops: nullable
        args = list(fit)
        args[k] = None
        assert L.nd_align_fit(*args) == ERR, k
        assert b"null" in L.nd_last_error()
    for k, v in ((3, -1), (5, -1), (6, -1), (12, need - 1)):
        args = list(fit)
        args[k] = v
        assert L.nd_align_fit(*args) == ERR and b"align_fit" in L.nd_last_error()
    assert L.nd_align_fit(None, None, None, 0, None, 0, 0, None, None, None, None, None, 0, None) == 0
