"""Read assembly on the device (assembly.hip, nd_assemble_reads, frontend.assemble_reads, -assembly gpu)
against the host path: the expected value is always frontend.assemble_read, and correctness is string
identity."""
import random

import numpy as np
import pytest
import torch

from nanodecoder_amd import frontend

pytestmark = pytest.mark.gpu
LEN, STRIDE = 300, 60


def host(reads):
    return [frontend.assemble_read(p, LEN, STRIDE) for p in reads]


def device_raw(reads):
    """(strings or None where status != 0, status) straight from one nd_assemble_reads call."""
    bases, chunk_off, read_off, kept = frontend.pack_assembly_input(reads)[:4]
    assert kept == []
    seq, seq_len, status = frontend._assemble_device(bases, chunk_off, read_off, 0)[:3]
    start = chunk_off[read_off[:-1]]
    out = []
    for r in range(len(reads)):
        assert (seq_len[r] == -1) == (status[r] != 0)
        out.append(None if status[r] else seq[start[r]: start[r] + seq_len[r]].tobytes().decode())
    return out, status, seq


def spaced(s):
    return " ".join(s)


def test_golden_cases_as_one_group():
    from tests import golden_util as gu
    z, meta = gu.load_frontend()
    n = len(meta["assembly"])
    assert n == 6
    reads = [[[str(p)] for p in z[f"asm_preds{j}"]] for j in range(n)]
    stats = {}
    got = frontend.assemble_reads(reads, LEN, STRIDE, device=0, stats=stats)
    assert got == [str(z[f"asm_seq{j}"]) for j in range(n)]
    assert stats == {"reads": n, "fallback": 0}


HAND = [
    ("no shared char", [["A A A"], ["C C"]], "AAA"),
    ("nested second chunk", [["A C G T A C"], ["G T"]], "ACGT"),
    # b's block starts at 3 and a's at 0: position -3, the first three chars of b are clipped
    ("negative position", [["A C G G"], ["T T T A C G G C"]], "ACGGC"),
    ("homopolymer tie", [["A A A A"], ["A A A"]], "AAA"),
    # blocks of 2: "AC" (a 0, b 3) and "GT" (a 3, b 0): the earliest in a wins although the other is earliest in b
    ("earliest in a before earliest in b", [["A C T G T"], ["G T C A C"]], None),
    # the same block twice in b: the earliest in b
    ("earliest in b", [["T A C"], ["A C G A C"]], None),
    ("lower case matches case-sensitively", [["a c g t"], ["A C G T"], ["c g t t"]], None),
    ("lower case votes as upper", [["A c G"], ["c G t"]], "ACGT"),
    ("an M base", [["A C M T"], ["C M T T"]], "ACMTT"),
    ("single chunk", [["A C G T"]], ""),
    ("only empty chunks", [[""], [""], [""]], ""),
    ("zero chunks", [], ""),
    ("empty chunks between", [[""], ["A C G T"], [""], [""], ["G T A A"], [""]], "ACGTAA"),
    ("three chunks drifting left", [["G G A C"], ["T T G G A"], ["C C T T G"]], None),
]


def test_hand_made_reads_in_one_group():
    reads = [h[1] for h in HAND]
    exp = host(reads)
    for (name, _, want), e in zip(HAND, exp):
        assert want is None or e == want, name  # the cases are what their names say, on the host path
    got, status, _ = device_raw(reads)
    assert not status.any()
    for (name, _, _), g, e in zip(HAND, got, exp):
        assert g == e, name
    assert frontend.assemble_reads(reads, LEN, STRIDE, device=0) == exp


def random_group(seed=7):
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
            st = max(0, min(len(truth) - n, st + rng.randint(-40, 60)))  # positions go both ways
            w = [rng.choice(alpha) if rng.random() < 0.07 else ch for ch in truth[st: st + n]]
            preds.append([spaced(w), spaced("ACGT")])  # n-best: the second is never used
        reads.append(preds)
    return reads


def test_random_group_matches_host():
    reads = random_group()
    exp = host(reads)  # raises for none of them
    assert sum(1 for e in exp if e) > 25 and max(len(e) for e in exp) > 300
    got, status, _ = device_raw(reads)
    assert not status.any()
    bad = [r for r in range(len(reads)) if got[r] != exp[r]]
    assert not bad, bad
    stats = {}
    assert frontend.assemble_reads(reads, LEN, STRIDE, device=0, stats=stats) == exp
    assert stats == {"reads": 60, "fallback": 0}


def test_read_of_5000_short_chunks():
    """More chunks than one workgroup scans at once: the blocked scan's carry."""
    rng = random.Random(3)
    truth = "".join(rng.choice("ACGT") for _ in range(5000 * 3 + 12))
    preds = [[spaced(truth[3 * i: 3 * i + 12])] if i % 97 else [""] for i in range(5000)]
    reads = [preds, [["A C G T"], ["G T A"]]]
    exp = host(reads)
    assert len(exp[0]) > 14000 and exp[1] == "ACGTA"
    assert frontend.assemble_reads(reads, LEN, STRIDE, device=0) == exp


def test_fallback_is_per_read_counted_and_exact():
    rng = random.Random(5)
    t = "".join(rng.choice("ACGT") for _ in range(400))
    long_read = [[spaced(t[0:150])], [spaced(t[100:300])], [spaced(t[250:400])]]      # one 200-char chunk
    edge_read = [[spaced(t[0:199])], [spaced(t[60:259])], [spaced(t[120:319])]]       # 199: on the device
    unk_read = [["A C G T"], ["C G <unk> T"]]
    plain = [["A C G T A"], ["G T A C C"]]
    reads = [plain, long_read, edge_read, unk_read, plain]
    got, status, _ = device_raw(reads)
    assert list(status) == [0, frontend.ASM_STATUS_LONG, 0, frontend.ASM_STATUS_CHAR, 0]
    assert got[0] == got[4] == frontend.assemble_read(plain, LEN, STRIDE) == "ACGTACC"
    assert got[2] == frontend.assemble_read(edge_read, LEN, STRIDE) and len(got[2]) == 319
    with pytest.raises(KeyError) as host_err:
        frontend.assemble_read(unk_read, LEN, STRIDE)
    stats = {}
    with pytest.raises(KeyError) as dev_err:
        frontend.assemble_reads(reads, LEN, STRIDE, device=0, stats=stats)
    assert dev_err.value.args == host_err.value.args
    assert stats == {"reads": 5, "fallback": 2}
    # deferred: the failing read is left to the caller, the others are whole
    stats = {}
    out = frontend.assemble_reads(reads, LEN, STRIDE, device=0, stats=stats, defer_errors=True)
    assert out[3] is None and stats == {"reads": 5, "fallback": 2}
    assert [out[i] for i in (0, 1, 2, 4)] == host([reads[i] for i in (0, 1, 2, 4)])


def test_repeatable_and_stream_independent():
    from nanodecoder_amd import synth
    from nanodecoder_amd.engine import Engine
    reads = random_group(seed=11)[:30]
    a = device_raw(reads)
    b = device_raw(reads)
    # the non-default stream is an engine context's own (the stream a translate call of that lane runs on),
    # as everywhere in this suite.  Not torch.cuda.Stream(): torch's stream pool, once made, stays for the
    # process, and with it made here test_pool_scores_match_single_engine_bitwise later returned zero scores
    cfg = synth.ModelConfig()
    eng = Engine(cfg, synth.make_weights(cfg, seed=1), device=0, max_batch=4, max_steps=8)
    try:
        assert eng.stream != torch.cuda.default_stream(0)
        with torch.cuda.stream(eng.stream):
            c = device_raw(reads)
        eng.stream.synchronize()
    finally:
        eng.close()
    for other in (b, c):
        assert other[0] == a[0]
        assert (other[1] == a[1]).all() and other[2].tobytes() == a[2].tobytes()
    assert a[0] == host(reads)


def test_cli_gpu_assembly_matches_host(tmp_path, capfd):
    """translate.py end to end with overlapping windows, -assembly cpu against -assembly gpu: the same
    result/*.fasta and segment/* bytes.  A synthetic model's neighbouring hypotheses are nearly unrelated:
    short matches and frequent ties, the hard case for the tie-break."""
    import os

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
    sizes = (400, 3000, 700, 1300, 2049)
    for i, n in enumerate(sizes):
        raw = synth.synth_raw_read(i, n)
        (src / f"read{i}.signal").write_text(" ".join(str(int(v)) for v in raw))
    files = {}
    try:
        T.Translator.__init__ = spy
        for m in ("cpu", "gpu"):
            out = tmp_path / ("out_" + m)
            o = opts.parse_translate_opts(["-model", str(ck), "-src_dir", str(src), "-save_data", str(out), "-gpu",
                                           "0", "-beam_size", "1", "-batch_size", "4", "-thread", "2", "-max_length",
                                           "30", "-min_length", "4", "-engine_max_batch", "8", "-engine_lanes", "1",
                                           "-src_seq_length", "300", "-src_seq_stride", "60", "-assembly", m])
            assert cli.main(o) == len(sizes)
            files[m] = {os.path.join(d, f): (out / d / f).read_bytes() for d in ("result", "segment")
                        for f in sorted(os.listdir(out / d))}
    finally:
        T.Translator.__init__ = orig
    for e in built:
        e.close()
    assert len(files["cpu"]) == 2 * len(sizes) and set(files["cpu"]) == set(files["gpu"])
    for name in files["cpu"]:
        assert files["cpu"][name] == files["gpu"][name], name
    fasta = [v for k, v in files["gpu"].items() if k.startswith("result")]
    assert any(v.split(b"\n", 1)[1] for v in fasta)  # not a comparison of empty reads
    assert "reads were assembled on the host" in capfd.readouterr().err


def test_every_annotation_in_one_call_with_a_fallback():
    """weights, mod_weights and positions together: one packing, two device calls (_m, then _p) and one host
    fallback, equal to the host path."""
    from tests.test_assembly_forms_host import make_group
    reads, ws, ms, ps = (list(v) for v in make_group())
    rng = random.Random(9)
    t = "".join(rng.choice("ACGTM") for _ in range(230))
    reads[5] = [[spaced(t[:200])], [spaced(t[190:230])]]  # a chunk of 200 chars: assembled on the host
    ws[5] = ms[5] = ps[5] = [list(range(200)), list(range(40))]
    stats = {}
    got = frontend.assemble_reads(reads, LEN, STRIDE, device=0, stats=stats, weights=ws, mod_weights=ms, positions=ps)
    exp = frontend.assemble_reads(reads, LEN, STRIDE, device=None, weights=ws, mod_weights=ms, positions=ps)
    assert stats == {"reads": 6, "fallback": 1}
    assert sum(len(e[0]) for e in exp) > 300 and len(exp[5][0]) > 200
    for r, (g, e) in enumerate(zip(got, exp)):
        assert len(g) == len(e) == 4 and g[:2] == e[:2], r
        assert g[2].dtype == e[2].dtype == np.uint8 and g[2].tolist() == e[2].tolist(), r
        assert g[3].dtype == e[3].dtype == np.uint32 and g[3].tolist() == e[3].tolist(), r
