"""Read accuracy on the host (CPU only): accuracy.align_host against a plain triple-loop DP with the rule's
traceback, read_truth, quality_table and the empirical_Q formula, translate.py -truth end to end with the
stand-in engine, and nd_align_seqs' argument errors."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from nanodecoder_amd import accuracy, checkpoint, cli, opts, synth
from tests.test_quality_host import QualityEngine


# ---------------------------------------------------------------- the rule, restated as plainly as possible
def plain_align(a, b):
    """(counts, ops) by the full (n + 1) x (m + 1) table, cell by cell, and the traceback of the rule."""
    a, b = a.encode(), b.encode()
    n, m = len(a), len(b)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        D[i][0] = i
    for j in range(m + 1):
        D[0][j] = j
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    ops = [0] * n
    i, j = n, m
    match = sub = ins = dele = 0
    while i > 0 or j > 0:
        if i >= 1 and j >= 1 and D[i - 1][j - 1] + (a[i - 1] != b[j - 1]) == D[i][j]:
            if a[i - 1] != b[j - 1]:
                ops[i - 1] = 1
                sub += 1
            else:
                match += 1
            i, j = i - 1, j - 1
        elif i >= 1 and (j == 0 or D[i - 1][j] + 1 == D[i][j]):
            ops[i - 1] = 2
            ins += 1
            i -= 1
        else:
            dele += 1
            j -= 1
    assert D[n][m] == sub + ins + dele
    return [D[n][m], match, sub, ins, dele], ops


def mutate(rng, truth, rate, alphabet="ACGT"):
    """``truth`` with about ``rate`` errors: equal parts substitution, insertion and deletion."""
    out = []
    for ch in truth:
        x = rng.random()
        if x < rate / 3:
            out.append(rng.choice([c for c in alphabet if c != ch]))
        elif x < 2 * rate / 3:
            out.append(ch)
            out.append(rng.choice(list(alphabet)))
        elif x < rate:
            continue
        else:
            out.append(ch)
    return "".join(out)


def random_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n))


FIXED = [("", ""), ("ACGT", ""), ("", "ACGT"), ("AAAA", "AA"), ("AA", "AAAAA"), ("ACAC", "CACA")]
SIZES = (1, 2, 7, 63, 64, 65, 130)


def seeded_pairs(seed=5):
    """Per n in SIZES: a 15 % mutated copy of a random ACGT string against it, and a two-letter random pair of
    unequal lengths (ties everywhere)."""
    rng = np.random.default_rng(seed)
    pairs = []
    for n in SIZES:
        truth = random_seq(rng, n)
        pairs.append((mutate(rng, truth, 0.15), truth))
        pairs.append((random_seq(rng, n, "AC"), random_seq(rng, n + 1 + int(rng.integers(0, 5)), "AC")))
    return pairs


def host_pairs():
    return FIXED + seeded_pairs()


def check_invariants(counts, n, m):
    dist, match, sub, ins, dele = (int(v) for v in counts)
    assert match + sub + ins == n and match + sub + dele == m and dist == sub + ins + dele


@pytest.mark.parametrize("k", range(len(FIXED) + 2 * len(SIZES)))
def test_align_host_equals_the_plain_dp(k):
    call, truth = host_pairs()[k]
    want_counts, want_ops = plain_align(call, truth)
    counts, ops = accuracy.align_host(call, truth)
    assert counts.dtype == np.int32 and ops.dtype == np.uint8
    assert counts.tolist() == want_counts and ops.tolist() == want_ops
    check_invariants(counts, len(call), len(truth))


def test_fixed_pairs_by_hand():
    # the tie rule: diagonal first, then up (an insertion), then left
    assert accuracy.align_host("", "")[0].tolist() == [0, 0, 0, 0, 0]
    c, o = accuracy.align_host("ACGT", "")
    assert c.tolist() == [4, 0, 0, 4, 0] and o.tolist() == [2, 2, 2, 2]
    assert accuracy.align_host("", "ACGT")[0].tolist() == [4, 0, 0, 0, 4]
    c, o = accuracy.align_host("AAAA", "AA")  # the diagonal is taken while it can be: the first two bases are left over
    assert c.tolist() == [2, 2, 0, 2, 0] and o.tolist() == [2, 2, 0, 0]
    c, o = accuracy.align_host("AA", "AAAAA")
    assert c.tolist() == [3, 2, 0, 0, 3] and o.tolist() == [0, 0]
    assert accuracy.identity(c) == 2 / 5
    assert accuracy.identity([0, 0, 0, 0, 0]) == 0.0
    assert accuracy.identity(np.asarray([[3, 2, 0, 0, 3], [0, 0, 0, 0, 0]])).tolist() == [0.4, 0.0]


def test_align_reads_host_path():
    pairs = host_pairs()
    stats = {}
    counts, ops = accuracy.align_reads([p[0] for p in pairs], [p[1] for p in pairs], want_ops=True, stats=stats)
    assert counts.shape == (len(pairs), 5) and counts.dtype == np.int32
    for k, (call, truth) in enumerate(pairs):
        c, o = accuracy.align_host(call, truth)
        assert counts[k].tolist() == c.tolist() and ops[k].tolist() == o.tolist()
    assert accuracy.align_reads(["A"], ["A"])[1] is None
    with pytest.raises(ValueError):
        accuracy.align_reads(["A"], [])


def test_read_truth(tmp_path):
    f = tmp_path / "truth.fasta"
    f.write_text("; a comment before the first record\n>read1 some description\nacgt\nACMm\n\nTT\n>read2\n"
                 "GGCC\n>empty\n>read3\tx\nnnA\n")
    got = accuracy.read_truth(str(f))
    assert got == {"read1": "ACGTACCCTT", "read2": "GGCC", "empty": "", "read3": "NNA"}
    assert accuracy.normalise("acMmT") == "ACCCT"


def test_fasta_records(tmp_path):
    f = tmp_path / "records.fasta"
    f.write_text("; a comment before the first record\n>read1 some description\nacgt\nACMm\n\nTT\n>read2\n"
                 "GGCC\n>empty\n>read3\tx\nnnA\n>\nac\n>read2 again\n\ntt\nM\n")
    records = [("read1", "ACGTACCCTT"), ("read2", "GGCC"), ("empty", ""), ("read3", "NNA"), ("", "AC"),
               ("read2", "TTC")]
    assert list(accuracy.fasta_records(str(f))) == records
    # a repeated name: the last record for read_truth, a record of its own for read_reference
    assert accuracy.read_truth(str(f)) == {"read1": "ACGTACCCTT", "read2": "TTC", "empty": "", "read3": "NNA",
                                           "": "AC"}
    ref = accuracy.read_reference(str(f))
    assert ref.names == [n for n, _ in records] and ref.seq.tobytes() == "".join(s for _, s in records).encode()
    assert ref.rec_off.tolist() == [0, 10, 14, 14, 17, 19, 22]
    f.write_text("junk\n>chr1 first\nacgt\nACMm\n>chr2\nGGNN\n\nTT\n>chr1\nAC\n")  # test_read_reference's file
    assert list(accuracy.fasta_records(str(f))) == [("chr1", "ACGTACCC"), ("chr2", "GGNNTT"), ("chr1", "AC")]
    f.write_text("no header at all\nACGT\n")
    assert list(accuracy.fasta_records(str(f))) == [] and accuracy.read_truth(str(f)) == {}
    assert accuracy.read_reference(str(f)).names == [] and accuracy.read_reference(str(f)).total == 0


def test_quality_table_and_empirical_q():
    #        Q: 0    1    1    40   40   40
    quals = "!" + '"' + '"' + "III"
    ops = [1, 0, 2, 0, 0, 1]
    bases, errors = accuracy.quality_table(quals, ops)
    assert bases.shape == errors.shape == (41,)
    assert bases.tolist() == [1, 2] + [0] * 38 + [3]
    assert errors.tolist() == [1, 1] + [0] * 38 + [1]
    assert accuracy.empirical_q(1, 3) == -10.0 * math.log10(2 / 5)
    assert accuracy.empirical_q(0, 98) == 20.0
    assert accuracy.calibration_lines(bases, errors) == ["0\t1\t1\t%.2f\n" % (-10 * math.log10(2 / 3)),
                                                         "1\t2\t1\t%.2f\n" % (-10 * math.log10(2 / 4)),
                                                         "40\t3\t1\t%.2f\n" % (-10 * math.log10(2 / 5))]
    with pytest.raises(ValueError):
        accuracy.quality_table("II", [0])
    with pytest.raises(ValueError):
        accuracy.quality_table("J", [0])  # Q 41


# ---------------------------------------------------------------- translate.py -truth
class _Eng(QualityEngine):
    def __init__(self, cfg, W, device=0, max_batch=8, max_src_len=512, max_steps=100, max_beam=1):
        super().__init__(max_batch=max_batch, max_src_len=max_src_len)


def make_reads(tmp_path, sizes=(1300, 700, 400)):
    cfg = synth.ModelConfig()
    ck = tmp_path / "m.pt"
    checkpoint.save_synthetic(str(ck), cfg, synth.make_weights(cfg, seed=1))
    src = tmp_path / "reads"
    src.mkdir()
    for i, n in enumerate(sizes):
        raw = synth.synth_raw_read(i, n)
        (src / f"read{i}.signal").write_text(" ".join(str(int(v)) for v in raw))
    return ck, src


def fasta_sequence(path):
    text = path.read_text()
    return text.split("\n", 1)[1] if "\n" in text else ""


def check_accuracy_files(out, truths):
    """accuracy.tsv of a finished run against align_host on the written .fasta files; returns the evaluated
    reads' names."""
    lines = (out / "accuracy.tsv").read_text().splitlines()
    names = [ln.split("\t")[0] for ln in lines]
    assert sorted(names) == sorted(n for n in truths if (out / "result" / (n + ".fasta")).exists())
    for ln in lines:
        f = ln.split("\t")
        assert len(f) == 8
        called = accuracy.normalise(fasta_sequence(out / "result" / (f[0] + ".fasta")))
        counts, _ = accuracy.align_host(called, truths[f[0]])
        assert [int(v) for v in f[1:7]] == [len(called), len(truths[f[0]])] + counts[1:].tolist()
        assert f[7] == "%.6f" % accuracy.identity(counts)
    return names


def test_cli_truth_end_to_end(tmp_path, monkeypatch):
    import nanodecoder_amd.translator as T
    monkeypatch.setattr(T, "Engine", _Eng)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    ck, src = make_reads(tmp_path)
    argv = lambda out: ["-model", str(ck), "-src_dir", str(src), "-save_data", str(out), "-gpu", "0",  # noqa: E731
                        "-beam_size", "1", "-batch_size", "2", "-thread", "2", "-max_length", "10", "-pack_reads",
                        "2", "-src_seq_length", "300", "-src_seq_stride", "100"]
    plain = tmp_path / "plain"
    assert cli.main(opts.parse_translate_opts(argv(plain))) == 3
    assert not (plain / "accuracy.tsv").exists() and not (plain / "quality_calibration.tsv").exists()
    called = {f"read{i}": fasta_sequence(plain / "result" / f"read{i}.fasta") for i in range(3)}
    assert any(called.values())
    # read0's truth is its own call with a few edits, read1's an unrelated string over lines; read2 has none
    seq0 = accuracy.normalise(called["read0"])
    truth_file = tmp_path / "truth.fasta"
    truth_file.write_text(">read0 edited\n" + ("G" + seq0[:3] + seq0[4:] + "t").lower() + "\n>read1\nACGTM\nACGTAC\n"
                          ">stranger\nACGT\n")
    truths = accuracy.read_truth(str(truth_file))
    out = tmp_path / "truth"
    log = tmp_path / "log.txt"
    o = opts.parse_translate_opts(argv(out) + ["-truth", str(truth_file), "-truth_align", "cpu", "-fastq", "-log_file",
                                               str(log)])
    assert o.truth == str(truth_file) and o.truth_align == "cpu"
    assert cli.main(o) == 3
    # the outputs that were there before are the same bytes
    for d in ("result", "segment"):
        for f in os.listdir(plain / d):
            assert (out / d / f).read_bytes() == (plain / d / f).read_bytes(), f
    names = check_accuracy_files(out, truths)
    assert sorted(names) == ["read0", "read1"]
    text = log.read_text()
    assert "-truth: 2 reads evaluated, 1 without a truth, 0 host fallbacks" in text and "pooled identity" in text
    # the calibration table: one line per Q that has bases, summing to the evaluated reads' called bases
    rows = [ln.split("\t") for ln in (out / "quality_calibration.tsv").read_text().splitlines()]
    assert all(len(r) == 4 for r in rows) and [int(r[0]) for r in rows] == sorted({int(r[0]) for r in rows})
    assert sum(int(r[1]) for r in rows) == len(called["read0"]) + len(called["read1"])
    want_b, want_e = np.zeros(41, np.int64), np.zeros(41, np.int64)
    for n in names:
        qual = (out / "result" / (n + ".fastq")).read_text().split("\n")[3]
        b, e = accuracy.quality_table(qual, accuracy.align_host(accuracy.normalise(called[n]), truths[n])[1])
        want_b += b
        want_e += e
    assert "".join("\t".join(r) + "\n" for r in rows) == "".join(accuracy.calibration_lines(want_b, want_e))
    for r in rows:
        assert int(r[1]) > 0 and r[3] == "%.2f" % (-10 * math.log10((int(r[2]) + 1) / (int(r[1]) + 2)))
    # resume: nothing left to do, nothing appended
    before = (out / "accuracy.tsv").read_bytes()
    assert cli.main(o) == 0 and (out / "accuracy.tsv").read_bytes() == before
    # without -fastq there is no calibration table
    out2 = tmp_path / "truth_nofastq"
    assert cli.main(opts.parse_translate_opts(argv(out2) + ["-truth", str(truth_file), "-truth_align", "cpu"])) == 3
    assert (out2 / "accuracy.tsv").read_bytes() == before and not (out2 / "quality_calibration.tsv").exists()


def test_cli_truth_refuses_attn_debug(tmp_path):
    o = opts.parse_translate_opts(["-model", "m.pt", "-src_dir", str(tmp_path), "-save_data", str(tmp_path / "o"),
                                   "-gpu", "0", "-truth", str(tmp_path / "t.fasta"), "-attn_debug"])
    with pytest.raises(ValueError):
        cli.main(o)
    assert not (tmp_path / "o").exists()
    d = opts.parse_translate_opts(["-model", "m.pt", "-src_dir", "x", "-save_data", "y"])
    assert d.truth == "" and d.truth_align == "gpu"


# ---------------------------------------------------------------- argument errors, no device
def test_align_seqs_argument_errors_without_gpu():
    from nanodecoder_amd import _lib, build
    build.build()
    L = _lib.lib()
    ERR = _lib.ND_ERR_ARG
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before any HIP call
    need = L.nd_align_seqs_work_bytes(3, 1000)
    assert 0 < need <= 1000 // 4 + 16 * 3 + 64
    assert L.nd_align_seqs_work_bytes(-1, 10) < 0 and L.nd_align_seqs_work_bytes(1, -10) < 0
    a = lambda *x: L.nd_align_seqs(*x)  # noqa: E731
    for k in (0, 1, 2, 3, 6, 8, 9):  # every required buffer in turn (7 is d_ops: nullable)
        args = [p, p, p, p, 3, 1000, p, None, p, p, need, None]
        args[k] = None
        assert a(*args) == ERR, k
        assert b"null" in L.nd_last_error()
    assert a(p, p, p, p, -1, 1000, p, None, p, p, need, None) == ERR
    assert a(p, p, p, p, 3, -1, p, None, p, p, need, None) == ERR
    assert a(p, p, p, p, 3, 1000, p, None, p, p, need - 1, None) == ERR
    assert b"work_bytes" in L.nd_last_error()
    assert a(p, p, p, p, 3, 1000, p, None, p, p, -5, None) == ERR
    assert a(None, None, None, None, 0, 0, None, None, None, None, 0, None) == 0  # P == 0: at once
