"""translate.py -truth / -truth_ref on the host (CPU only), the paths beside the plain run: the evaluation raises for
a group, and a read whose files cannot be written.  cli.main is driven as a black box with the stand-in engine and
assembly of test_cli_truth_ref_end_to_end; every test asserts on the files, the printed lines and the log's counts."""
import numpy as np
import pytest
import torch

from nanodecoder_amd import accuracy, cli, opts
from tests.test_accuracy_host import _Eng, fasta_sequence, make_reads, random_seq

A = accuracy


def fake(preds):
    """A seeded sequence (and qualities) per read, told apart by its number of chunks."""
    r = np.random.default_rng(len(preds))
    n = 150 + 20 * len(preds)
    return random_seq(r, n), "".join(chr(33 + int(v)) for v in r.integers(0, 41, n))


@pytest.fixture
def run(tmp_path, monkeypatch):
    """(argv(out) of a three-read run, the reads' normalised calls, a reference file: read0 forward in one record,
    read1's reverse complement in another, read2 nowhere)."""
    import nanodecoder_amd.translator as T
    from nanodecoder_amd import frontend
    monkeypatch.setattr(T, "Engine", _Eng)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(frontend, "assemble_read", lambda preds, *a, **k: fake(preds)[0])
    monkeypatch.setattr(frontend, "assemble_read_q", lambda preds, w, *a, **k: fake(preds))
    monkeypatch.setattr(frontend, "assemble_reads",
                        lambda reads, *a, **k: [fake(p) if k.get("weights") else fake(p)[0] for p in reads])
    ck, src = make_reads(tmp_path)
    argv = lambda out: ["-model", str(ck), "-src_dir", str(src), "-save_data", str(out), "-gpu", "0",  # noqa: E731
                        "-beam_size", "1", "-batch_size", "2", "-thread", "2", "-max_length", "10", "-pack_reads",
                        "2", "-src_seq_length", "300", "-src_seq_stride", "100", "-truth_align", "cpu"]
    plain = tmp_path / "plain"
    assert cli.main(opts.parse_translate_opts(argv(plain))) == 3
    called = {f"read{i}": A.normalise(fasta_sequence(plain / "result" / f"read{i}.fasta")) for i in range(3)}
    assert len(set(called.values())) == 3
    rng = np.random.default_rng(1234)
    rc1 = A.reverse_complement(called["read1"]).tobytes().decode()
    ref_file = tmp_path / "ref.fasta"
    ref_file.write_text(">ctgA x\n" + random_seq(rng, 700) + called["read0"].lower() + random_seq(rng, 300) + "\n>ctgB\n"
                        + random_seq(rng, 900) + "\n" + rc1 + random_seq(rng, 50) + "\n")
    return argv, called, ref_file


def boom(*a, **k):
    raise RuntimeError("boom")


def error_lines(text):
    return sorted(ln for ln in text.splitlines() if ln.startswith("!!!error!!!"))


def test_cli_truth_ref_when_the_mapping_raises(tmp_path, monkeypatch, capsys, run):
    argv, called, ref_file = run
    monkeypatch.setattr(accuracy, "map_reads", boom)
    out, log = tmp_path / "out", tmp_path / "log.txt"
    capsys.readouterr()
    assert cli.main(opts.parse_translate_opts(argv(out) + ["-truth_ref", str(ref_file), "-fastq", "-log_file",
                                                           str(log)])) == 3
    assert error_lines(capsys.readouterr().out) == ["!!!error!!!accuracy: read%d (RuntimeError('boom'))" % i
                                                    for i in range(3)]
    for n, c in called.items():  # the reads are written all the same
        assert A.normalise(fasta_sequence(out / "result" / (n + ".fasta"))) == c
        assert (out / "result" / (n + ".fastq")).exists() and (out / "segment" / (n + ".txt")).exists()
    assert not (out / "accuracy.tsv").exists() and not (out / "mapping.paf").exists()
    assert (out / "quality_calibration.tsv").read_text() == ""
    assert ("-truth_ref: 0 reads evaluated, 0 reads unmapped, 0 segments mapped, 0 unmapped; pooled identity 0.000000 "
            "(0 matches over 0 alignment columns)") in log.read_text()


def test_cli_truth_when_the_alignment_raises(tmp_path, monkeypatch, capsys, run):
    argv, called, _ = run
    truth_file = tmp_path / "truth.fasta"
    truth_file.write_text(">read0\n" + called["read0"] + "\n>read1\n" + called["read1"][5:] + "\n")
    monkeypatch.setattr(accuracy, "align_reads", boom)
    out, log = tmp_path / "out", tmp_path / "log.txt"
    capsys.readouterr()
    assert cli.main(opts.parse_translate_opts(argv(out) + ["-truth", str(truth_file), "-fastq", "-log_file",
                                                           str(log)])) == 3
    # read2 has no truth: it was not to be evaluated, and is counted as such once written
    assert error_lines(capsys.readouterr().out) == ["!!!error!!!accuracy: read%d (RuntimeError('boom'))" % i
                                                    for i in range(2)]
    for n, c in called.items():
        assert A.normalise(fasta_sequence(out / "result" / (n + ".fasta"))) == c
        assert (out / "result" / (n + ".fastq")).exists() and (out / "segment" / (n + ".txt")).exists()
    assert not (out / "accuracy.tsv").exists()
    assert (out / "quality_calibration.tsv").read_text() == ""
    assert ("-truth: 0 reads evaluated, 1 without a truth, 0 host fallbacks (a read or a truth above 8192 bases); "
            "pooled identity 0.000000 (0 matches over 0 alignment columns)") in log.read_text()


def test_cli_truth_ref_read_that_cannot_be_written(tmp_path, capsys, run):
    argv, called, ref_file = run
    ref = A.read_reference(str(ref_file))
    want = {n: A.map_host(c, ref) for n, c in called.items()}
    assert [bool(want["read%d" % i][1]) for i in range(3)] == [True, True, False]
    out, log = tmp_path / "out", tmp_path / "log.txt"
    (out / "segment" / "read0.txt").mkdir(parents=True)  # a directory where read0's segment file goes
    capsys.readouterr()
    assert cli.main(opts.parse_translate_opts(argv(out) + ["-truth_ref", str(ref_file), "-fastq", "-log_file",
                                                           str(log)])) == 3
    assert error_lines(capsys.readouterr().out) == ["!!!error!!!data src: read0"]
    # read0 is in neither the sums nor the calibration table; read1 (mapped) and read2 (unmapped) are in both
    counts, recs, ops = want["read1"]
    c = [int(v) for v in counts]
    assert len(recs) == 1 and len(A.segments(len(called["read2"]))) == 1
    assert ("-truth_ref: 1 reads evaluated, 1 reads unmapped, 1 segments mapped, 1 unmapped; pooled identity %.6f "
            "(%d matches over %d alignment columns)" % (c[1] / sum(c[1:]), c[1], sum(c[1:]))) in log.read_text()
    qual = (out / "result" / "read1.fastq").read_text().split("\n")[3]
    keep = ops != A.OP_UNMAPPED
    b, e = A.quality_table(np.frombuffer(qual.encode(), np.uint8)[keep].tobytes(), ops[keep])
    assert int(b.sum()) == len(called["read1"])
    assert (out / "quality_calibration.tsv").read_text() == "".join(A.calibration_lines(b, e))
    # its lines were appended before the file that failed, as write_output orders its files
    lines = (out / "accuracy.tsv").read_text().splitlines(True)
    assert sorted(ln.split("\t")[0] for ln in lines) == ["read0", "read1"]
    assert len((out / "mapping.paf").read_text().splitlines()) == 2
    assert not (out / "speed.txt").read_text().startswith("read0\t") and "\nread0\t" not in (out / "speed.txt").read_text()
