"""Read accuracy on the device: nd_align_seqs against the host rule accuracy.align_host.  Integer min-plus, so
every comparison is exact equality: counts, ops and status."""
import os

import numpy as np
import pytest
import torch

from nanodecoder_amd import accuracy
from tests.test_accuracy_host import host_pairs, mutate, random_seq

pytestmark = pytest.mark.gpu
MAX = accuracy.ALIGN_MAX_LEN


def device_raw(pairs, want_ops=True, cells=None):
    """(counts [P, 5], status [P], ops per pair or None) straight from one nd_align_seqs call."""
    call, call_off, truth, truth_off, true_cells = accuracy.pack_align_input([p[0] for p in pairs],
                                                                             [p[1] for p in pairs])
    counts, status, flat = accuracy._align_device(call, call_off, truth, truth_off,
                                                  true_cells if cells is None else cells, 0, want_ops)
    ops = [flat[call_off[k]: call_off[k + 1]] for k in range(len(pairs))] if want_ops else None
    return counts, status, ops


def boundary_pairs(seed=21):
    """The issue's shapes, and one pair each side of every boundary csrc/align.hip has:
       - a direction word is 16 columns (m = 15, 16, 17, 31, 32, 33), and the last m mod 16 columns of a thread's
         four rows are packed into m mod 16 bytes (every m mod 16 against every n mod 4 in the sweep);
       - a thread owns 4 rows (n = 3, 4, 5), a strip is 1024 rows (n = 1023, 1024, 1025, and 2049: three strips);
       - the strips are chained max(blocks, 256) steps apart: 255, 256 and 257 blocks (m = 4080, 4096, 4112)
         under two strips;
       - the traceback window is 64 rows by 64 columns (the 63 / 64 / 65 pairs of the host file, 255 / 256 / 257)."""
    rng = np.random.default_rng(seed)
    pairs = []

    def related(n, m, rate=0.1, alphabet="ACGT"):
        truth = random_seq(rng, m, alphabet)
        call = mutate(rng, truth, rate, alphabet)
        call = (call + random_seq(rng, max(0, n - len(call)), alphabet))[:n]
        pairs.append((call, truth))
    for n in (255, 256, 257):
        for m in (255, 256, 257):
            related(n, m)
    related(300, 700)
    related(700, 300)
    related(1000, 1000, 0.10)
    pairs.append((random_seq(rng, 500), random_seq(rng, 500)))  # unrelated
    for m in (15, 16, 17, 31, 32, 33):
        related(40, m, 0.2)
    for n in (3, 4, 5):
        related(n, 50, 0.2)
    for m in range(1, 34):  # the packed remainder: every m mod 16, n mod 4 cycling, two-letter ties
        related(5 + m % 4, m, 0.3, "AC")
    for n in (1023, 1024, 1025, 2049):
        related(n, 200 + n % 7)
    for m in (4080, 4096, 4112):
        related(1030, m)
    return pairs


@pytest.fixture(scope="module")
def main_case():
    pairs = host_pairs() + boundary_pairs()
    want = [accuracy.align_host(c, t) for c, t in pairs]
    return pairs, want


def check(pairs, want, counts, status, ops, idx=None):
    for k in (range(len(pairs)) if idx is None else idx):
        assert status[k] == 0, (k, len(pairs[k][0]), len(pairs[k][1]))
        assert counts[k].tolist() == want[k][0].tolist(), (k, len(pairs[k][0]), len(pairs[k][1]))
        if ops is not None:
            assert ops[k].tobytes() == want[k][1].tobytes(), (k, len(pairs[k][0]), len(pairs[k][1]))


def test_one_call_equals_the_host_rule(main_case):
    pairs, want = main_case
    counts, status, ops = device_raw(pairs)
    assert counts.dtype == np.int32 and counts.shape == (len(pairs), 5)
    check(pairs, want, counts, status, ops)
    # the public function: the same, with nothing redone on the host
    stats = {}
    c2, o2 = accuracy.align_reads([p[0] for p in pairs], [p[1] for p in pairs], device=0, want_ops=True, stats=stats)
    assert stats == {"reads": len(pairs), "fallback": 0}
    assert c2.tobytes() == counts.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(o2, ops))


def test_null_ops_order_and_stream(main_case):
    pairs, want = main_case
    counts, status, ops = device_raw(pairs)
    c0, s0, none = device_raw(pairs, want_ops=False)  # d_ops null: the same counts
    assert none is None and c0.tobytes() == counts.tobytes() and s0.tobytes() == status.tobytes()
    rc, rs, ro = device_raw(pairs[::-1])  # pair order reversed: the same per-pair results
    assert rc[::-1].tobytes() == counts.tobytes() and rs[::-1].tobytes() == status.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ro[::-1], ops))
    side = torch.cuda.Stream(device=0)  # a repeat on another stream: identical bytes
    with torch.cuda.stream(side):
        c1, s1, o1 = device_raw(pairs)
    side.synchronize()
    assert c1.tobytes() == counts.tobytes() and s1.tobytes() == status.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(o1, ops))


def test_cap_edges():
    rng = np.random.default_rng(33)
    t_long, t_short = random_seq(rng, MAX), random_seq(rng, 64)
    pairs = [(random_seq(rng, 20), random_seq(rng, 23)),
             (mutate(rng, t_long, 0.02)[:MAX].ljust(MAX, "A"), t_short),   # 8192 x 64
             (random_seq(rng, MAX + 1), random_seq(rng, 10)),              # 8193 x 10: status bit 0
             (random_seq(rng, 31), random_seq(rng, 29)),
             (random_seq(rng, 10), random_seq(rng, MAX + 1)),              # 10 x 8193: status bit 0
             (t_short, mutate(rng, t_long, 0.02)[:MAX].ljust(MAX, "C")),   # 64 x 8192
             (random_seq(rng, 17), random_seq(rng, 16))]
    assert [len(p[0]) for p in pairs[1:3]] == [MAX, MAX + 1] and len(pairs[5][1]) == MAX
    counts, status, ops = device_raw(pairs)
    assert status.tolist() == [0, 0, 1, 0, 1, 0, 0]
    good = [0, 1, 3, 5, 6]
    want = {k: accuracy.align_host(*pairs[k]) for k in good}
    check(pairs, want, counts, status, ops, good)
    for k in (2, 4):
        assert counts[k].tolist() == [-1] * 5 and not ops[k].any() and ops[k].size == len(pairs[k][0])
    # the public function repairs the two on the host
    stats = {}
    c2, o2 = accuracy.align_reads([p[0] for p in pairs], [p[1] for p in pairs], device=0, want_ops=True, stats=stats)
    assert stats == {"reads": 7, "fallback": 2}
    for k in (2, 4):
        w = accuracy.align_host(*pairs[k])
        assert c2[k].tolist() == w[0].tolist() and o2[k].tobytes() == w[1].tobytes()
    for k in good:
        assert c2[k].tolist() == want[k][0].tolist() and o2[k].tobytes() == want[k][1].tobytes()


def test_work_offsets_past_2_31():
    """36 pairs of 8192 x 8192 (call == truth: distance 0, all matches, known without a DP) put the directions
    of the pairs behind them past byte 2^29 and their cells past 2^31; three small pairs follow."""
    rng = np.random.default_rng(44)
    filler = random_seq(rng, MAX)
    small = [(mutate(rng, t, 0.15), t) for t in (random_seq(rng, 90), random_seq(rng, 33), random_seq(rng, 150))]
    pairs = [(filler, filler)] * 36 + small
    assert accuracy.pack_align_input([p[0] for p in pairs], [p[1] for p in pairs])[4] > 2 ** 31
    counts, status, ops = device_raw(pairs)
    assert not status.any()
    assert (counts[:36] == np.asarray([0, MAX, 0, 0, 0], np.int32)).all()
    assert not any(o.any() for o in ops[:36])
    want = [accuracy.align_host(c, t) for c, t in small]
    check(small, want, counts[36:], status[36:], ops[36:])


def test_cells_understated(monkeypatch):
    rng = np.random.default_rng(55)
    pairs = [(mutate(rng, t, 0.1), t) for t in (random_seq(rng, 100 + 10 * k) for k in range(8))]
    true_cells = sum(len(c) * len(t) for c, t in pairs)
    want = [accuracy.align_host(c, t) for c, t in pairs]
    for cells in (0, true_cells // 2):
        counts, status, ops = device_raw(pairs, cells=cells)
        assert set(status.tolist()) <= {0, 2} and (status == 2).any()
        if cells:
            assert (status == 0).any()
        for k in range(len(pairs)):
            if status[k]:
                assert counts[k].tolist() == [-1] * 5 and not ops[k].any()
        check(pairs, want, counts, status, ops, [k for k in range(len(pairs)) if status[k] == 0])
    # align_reads repairs them on the host and counts them
    real = accuracy.pack_align_input
    monkeypatch.setattr(accuracy, "pack_align_input", lambda c, t: real(c, t)[:4] + (true_cells // 2,))
    stats = {}
    c2, o2 = accuracy.align_reads([p[0] for p in pairs], [p[1] for p in pairs], device=0, want_ops=True, stats=stats)
    assert stats["reads"] == len(pairs) and stats["fallback"] == int((status == 2).sum()) > 0
    for k in range(len(pairs)):
        assert c2[k].tolist() == want[k][0].tolist() and o2[k].tobytes() == want[k][1].tobytes()


def test_cli_truth_align_gpu_matches_cpu(tmp_path):
    """translate.py -truth with -truth_align gpu against -truth_align cpu: the same accuracy.tsv and
    quality_calibration.tsv bytes."""
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
    # truths from a fixed seed (the model is synthetic: its calls are related to nothing); read2 has none
    rng = np.random.default_rng(66)
    truth_file = tmp_path / "truth.fasta"
    truth_file.write_text(">read0\n%s\n>read1 x\n%s\n%s\n" % (random_seq(rng, 90), random_seq(rng, 60),
                                                            random_seq(rng, 45).lower()))
    files = {}
    try:
        T.Translator.__init__ = spy
        for mode in ("cpu", "gpu"):
            out = tmp_path / ("out_" + mode)
            o = opts.parse_translate_opts(["-model", str(ck), "-src_dir", str(src), "-save_data", str(out), "-gpu",
                                           "0", "-beam_size", "1", "-batch_size", "4", "-thread", "2", "-max_length",
                                           "30", "-min_length", "4", "-engine_max_batch", "8", "-engine_lanes", "1",
                                           "-src_seq_length", "300", "-src_seq_stride", "60", "-assembly", "gpu",
                                           "-fastq", "-truth", str(truth_file), "-truth_align", mode])
            assert cli.main(o) == len(sizes)
            files[mode] = {f: (out / f).read_bytes() for f in ("accuracy.tsv", "quality_calibration.tsv")}
            files[mode].update({f: (out / "result" / f).read_bytes() for f in sorted(os.listdir(out / "result"))})
    finally:
        T.Translator.__init__ = orig
    for e in built:
        e.close()
    assert files["gpu"] == files["cpu"]
    lines = files["gpu"]["accuracy.tsv"].decode().splitlines()
    assert sorted(ln.split("\t")[0] for ln in lines) == ["read0", "read1"]
    truths = accuracy.read_truth(str(truth_file))
    for ln in lines:
        f = ln.split("\t")
        called = accuracy.normalise(files["gpu"][f[0] + ".fasta"].decode().split("\n", 1)[1])
        counts, _ = accuracy.align_host(called, truths[f[0]])
        assert len(called) > 0 and [int(v) for v in f[3:7]] == counts[1:].tolist()
