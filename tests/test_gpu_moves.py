"""Per-base signal positions on the device (assembly.hip: nd_token_positions, nd_assemble_reads_p) against the
host restatement in frontend.py, through the Translator on the golden models, and through translate.py -moves.
Every comparison is exact equality."""
import ctypes
import os
import random
import types

import numpy as np
import pytest
import torch

from nanodecoder_amd import _lib, frontend
from tests import golden_util as gu
from tests.test_moves_host import scripted_rows, softmax_rows

pytestmark = pytest.mark.gpu
LEN, STRIDE = 300, 60


# ---------------------------------------------------------------- nd_token_positions
def device_positions(attn, spans, S, T, ld_chunk):
    """One nd_token_positions call on the current stream: pos [B, S] int32 on the host."""
    a = torch.from_numpy(np.ascontiguousarray(attn, np.float32)).cuda()
    sp = torch.from_numpy(np.asarray(spans, np.int32)).cuda()
    B = sp.numel()
    pos = torch.full((B, S), -7, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().nd_token_positions(p(a), ld_chunk, p(sp), B, S, T, p(pos), stream), "nd_token_positions")
    return pos.cpu().numpy()


@pytest.mark.parametrize("T", [64, 100])
def test_token_positions_scripted_rows(T):
    spans = [T, 37, 1]
    attn = np.stack([scripted_rows(T, s) for s in spans])  # B = 3, S = 9
    got = device_positions(attn, spans, 9, T, 9 * T)
    want = frontend.token_positions(attn, np.asarray(spans))
    assert got.dtype == np.int32 and got.tolist() == want.tolist()
    assert want[0].max() == T - 1 and want[1].max() == 36 and want[2].max() == 0


def test_token_positions_softmax_rows():
    B, S, T = 8, 16, 512
    attn = softmax_rows(B, S, T, seed=3)
    spans = np.asarray([512, 511, 300, 65, 64, 63, 2, 1], np.int32)
    attn[2, 5] = 0.0  # a zero row keeps the position before it
    got = device_positions(attn, spans, S, T, S * T)
    want = frontend.token_positions(attn, spans)
    assert got.tolist() == want.tolist()
    assert (np.diff(got, axis=1) >= 0).all() and (got < spans[:, None]).all() and got.max() > 100


def test_token_positions_beam_stride_reads_hypothesis_0():
    B, S, T, n_best = 4, 9, 100, 2
    spans = np.asarray([100, 37, 64, 1], np.int32)
    attn = np.zeros((B, n_best, S, T), np.float32)
    attn[:, 0] = softmax_rows(B, S, T, seed=5)
    attn[:, 0, 6:] = 0.0  # rows past hypothesis 0's length are zero rows
    attn[:, 1] = softmax_rows(B, S, T, seed=6)[:, ::-1]
    attn[:, 1, :, 90:] = np.nan
    got = device_positions(attn, spans, S, T, n_best * S * T)
    want = frontend.token_positions(attn[:, 0], spans)
    assert got.tolist() == want.tolist()
    assert (got[:, 6:] == got[:, 5:6]).all()
    other = frontend.token_positions(np.nan_to_num(attn[:, 1]), spans)
    assert got.tolist() != other.tolist()


def test_token_positions_more_steps_than_one_scan_block():
    # S crosses the kernel's block of 256 steps: the carry holds the running maximum across blocks
    B, S, T = 2, 600, 64
    attn = softmax_rows(B, S, T, seed=9)
    spans = np.asarray([64, 50], np.int32)
    got = device_positions(attn, spans, S, T, S * T)
    assert got.tolist() == frontend.token_positions(attn, spans).tolist()


def test_token_positions_argument_refusals():
    L = _lib.lib()
    ERR = _lib.ND_ERR_ARG
    a = torch.zeros(3, 9, 64, device="cuda")
    sp = torch.ones(3, dtype=torch.int32, device="cuda")
    pos = torch.zeros(3, 9, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert L.nd_token_positions(None, 9 * 64, p(sp), 3, 9, 64, p(pos), None) == ERR
    assert L.nd_token_positions(p(a), 9 * 64, None, 3, 9, 64, p(pos), None) == ERR
    assert L.nd_token_positions(p(a), 9 * 64, p(sp), 3, 9, 64, None, None) == ERR
    assert L.nd_token_positions(p(a), 9 * 64, p(sp), -3, 9, 64, p(pos), None) == ERR
    assert L.nd_token_positions(p(a), 9 * 64, p(sp), 3, -9, 64, p(pos), None) == ERR
    assert L.nd_token_positions(p(a), 9 * 64, p(sp), 3, 9, 0, p(pos), None) == ERR
    assert L.nd_token_positions(p(a), 9 * 64 - 1, p(sp), 3, 9, 64, p(pos), None) == ERR
    assert L.nd_token_positions(p(a), 2 ** 40, p(sp), 70000, 70000, 64, p(pos), None) == ERR
    torch.cuda.synchronize()
    assert (pos == 0).all()


# ---------------------------------------------------------------- nd_assemble_reads_p
def seeded_group(seed=11):
    """Reads of 1, 2, 7 and 40 chunks of 20 to 60 bases cut from a truth with errors, empty chunks between,
    one read of some 60 chunks (about 1500 columns) and one with a 200-base chunk; with chunk-relative
    positions as a decoder gives them (non-decreasing inside a chunk, below LEN)."""
    rng = random.Random(seed)
    reads, pos = [], []
    for n_chunks in (1, 2, 7, 40, 2, 7, 40, 0, 60, 3):
        truth = "".join(rng.choice("ACGT") for _ in range(4000))
        st = rng.randrange(0, 50)
        preds = []
        for k in range(n_chunks):
            if rng.random() < 0.12 and n_chunks != 60:
                preds.append([""])
                continue
            n = rng.randrange(50, 61) if n_chunks == 60 else rng.randrange(20, 61)
            s = [c if rng.random() > 0.04 else rng.choice("ACGTM") for c in truth[st: st + n]]
            preds.append([" ".join(s)])
            st += rng.randrange(22, 32) if n_chunks == 60 else rng.randrange(5, 25)
        reads.append(preds)
    reads[-1][1] = [" ".join(rng.choice("ACGT") for _ in range(200))]  # status bit 0: the host assembles it
    for preds in reads:
        pos.append([sorted(rng.randrange(LEN) for _ in p[0].replace(" ", "")) for p in preds])
    return reads, pos


@pytest.fixture(scope="module")
def group():
    reads, pos = seeded_group()
    host = [frontend.assemble_read_p(p, q, LEN, STRIDE) for p, q in zip(reads, pos)]
    return reads, pos, host


def test_assemble_p_raw_outputs_equal_the_plain_call(group):
    reads, pos, host = group
    packed = frontend.pack_assembly_input(reads, positions=pos, src_seq_stride=STRIDE)
    (bases, chunk_off, read_off, kept), bp = packed[:4], packed.bp
    assert kept == [] and bp.size == bases.size
    seq0, len0, st0 = frontend._assemble_device(bases, chunk_off, read_off, 0)[:3]
    dev = frontend._assemble_device(bases, chunk_off, read_off, 0, bp=bp)
    (seq, seq_len, status), rpos = dev[:3], dev.rpos
    assert dev.qual is None and dev.ml is None
    assert seq.tobytes() == seq0.tobytes() and seq_len.tolist() == len0.tolist() and status.tolist() == st0.tolist()
    assert rpos.dtype == np.uint32 and rpos.size == bases.size
    start = chunk_off[read_off[:-1]]
    end = chunk_off[read_off[1:]]
    assert status.tolist() == [0] * (len(reads) - 1) + [frontend.ASM_STATUS_LONG]
    longest = 0
    for r in range(len(reads)):
        n = max(int(seq_len[r]), 0)
        assert (rpos[start[r] + n: end[r]] == 0).all()  # 0 past a read's length
        if status[r] == 0:
            assert seq[start[r]: start[r] + n].tobytes().decode() == host[r][0]
            assert rpos[start[r]: start[r] + n].tolist() == host[r][1].tolist(), r
            longest = max(longest, n)
    assert longest > 1100  # the read that crosses several 256-column scan blocks
    # the same bytes again, and on another stream
    again = frontend._assemble_device(bases, chunk_off, read_off, 0, bp=bp)
    with torch.cuda.stream(torch.cuda.Stream()):
        other = frontend._assemble_device(bases, chunk_off, read_off, 0, bp=bp)
    for o in (again, other):
        assert o.rpos.tobytes() == rpos.tobytes() and o.seq.tobytes() == seq.tobytes()


def test_assemble_p_group_with_fallback_equals_host(group):
    reads, pos, host = group
    stats = {}
    got = frontend.assemble_reads(reads, LEN, STRIDE, device=0, stats=stats, positions=pos)
    assert stats == {"reads": len(reads), "fallback": 1}
    for g, h in zip(got, host):
        assert g[0] == h[0] and g[1].dtype == np.uint32 and g[1].tolist() == h[1].tolist()
    assert sum(len(h[0]) for h in host) > 2500 and len(host[0][0]) == 0  # one valid chunk: ""
    # beside weights: the quality call, then a second call for the positions; reads counted once
    rng = random.Random(2)
    ws = [[[rng.randrange(65536) for _ in p[0].replace(" ", "")] for p in preds] for preds in reads]
    stats = {}
    both = frontend.assemble_reads(reads, LEN, STRIDE, device=0, stats=stats, weights=ws, positions=pos)
    assert stats == {"reads": len(reads), "fallback": 1}
    for b, h, preds, w in zip(both, host, reads, ws):
        assert b[:2] == frontend.assemble_read_q(preds, w, LEN, STRIDE) and b[2].tolist() == h[1].tolist()


def test_assemble_p_empty_groups():
    for reads in ([], [[]], [[[""]], [[""], [""]]]):
        pos = [[[] for _ in preds] for preds in reads]
        got = frontend.assemble_reads(reads, LEN, STRIDE, device=0, positions=pos)
        assert [(g[0], g[1].tolist()) for g in got] == [("", [])] * len(reads)
    L = _lib.lib()
    need = L.nd_assemble_reads_p_work_bytes(3, 100)
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = ctypes.c_void_p(t.data_ptr())
    assert L.nd_assemble_reads_p(p, None, p, p, 2, 3, 100, p, p, p, p, p, need, None) == _lib.ND_ERR_ARG
    assert L.nd_assemble_reads_p(p, p, p, p, 2, 3, 100, p, p, p, p, p, need - 1, None) == _lib.ND_ERR_ARG


# ---------------------------------------------------------------- the Translator on the golden models
def _translator(cfg, eng, **kw):
    from nanodecoder_amd.translator import Translator
    opt = dict(gpu=0, n_best=1, max_length=100, min_length=0, beam_size=1, fast=False, alpha=0.0, beta=0.0,
               batch_size=8)
    opt.update(kw)
    return Translator(cfg, None, types.SimpleNamespace(**opt), engine=eng)


def _record(eng, calls):
    """Keep the arguments of every translate call of ``eng`` (copies of its tensors)."""
    keep = lambda v: v.clone() if isinstance(v, torch.Tensor) else v  # noqa: E731
    for name in ("translate_greedy", "translate_beam", "translate_beam_classic"):
        def wrap(*a, _f=getattr(eng, name), _n=name, **kw):
            calls.append((_n, tuple(keep(v) for v in a), {k: keep(v) for k, v in kw.items()}))
            return _f(*a, **kw)
        setattr(eng, name, wrap)


def _check_moves(name, mode, pool=False):
    from nanodecoder_amd.engine import Engine, EnginePool
    z, meta = gu.load(name)
    cfg, W = gu.model_for(meta)
    kw = dict(meta[{"greedy": "greedy", "fast": "beam", "classic": "classic"}[mode]])
    chunks = gu.chunks_of(z)
    assert len(chunks) <= 8
    beam = kw.get("beam_size", 1)
    ekw = dict(device=0, max_batch=len(chunks), max_steps=kw["max_length"], max_beam=beam)
    eng = EnginePool(cfg, W, lanes=2, **ekw) if pool else Engine(cfg, W, **ekw)
    try:
        tr = _translator(cfg, eng, max_length=kw["max_length"], min_length=kw.get("min_length", 0), beam_size=beam,
                         n_best=kw.get("n_best", 1), fast=mode == "fast", alpha=kw.get("alpha", 0.0),
                         length_penalty=kw.get("length_penalty", "none"))
        reads = [chunks, chunks[::-1]] if pool else [chunks]  # a pool: one call per lane
        calls = []
        _record(eng, calls)
        got = tr.translate_reads(reads, batch_size=len(chunks), moves=True)
        n_moves = len(calls)
        plain = tr.translate_reads(reads, batch_size=len(chunks))
        assert [g[:2] for g in got] == plain and all(len(g) == 3 for g in got)  # the same scores and strings
        assert n_moves == len(reads) and all(c[2]["return_attn"] is True for c in calls[:n_moves])
        assert all(c[2]["return_attn"] is False for c in calls[n_moves:])
        if pool:
            assert n_moves == 2
        n_checked = 0
        for (cname, a, k), g, read in zip(calls[:n_moves], got, reads):
            # the same call again, on its own: its attention through the host rule
            r = getattr(eng, cname)(*a, **k)
            if "event" in r:
                r["event"].synchronize()
            torch.cuda.synchronize()
            n = len(read)
            at = r["attn"].cpu().numpy()[:n]
            spans = a[2].cpu().numpy()[:n]
            tok = r["tokens"].cpu().numpy()
            m = frontend.token_positions(at[:, 0] if mode != "greedy" else at, spans)
            for i in range(n):
                toks = tok[i].tolist() if mode == "greedy" else tok[i, 0, : int(r["lens"][i, 0])].tolist()
                want = tr._char_weights(toks, m[i], np.int32)
                s = g[1][i][0].replace(" ", "")
                assert g[2][i].dtype == np.int32 and len(g[2][i]) == len(s)
                assert g[2][i].tolist() == want.tolist(), (name, mode, i)
                assert (np.diff(g[2][i]) >= 0).all() and (g[2][i] < spans[i]).all() and (g[2][i] >= 0).all()
                n_checked += len(s)
        print(name, mode, "pool" if pool else "single", "bases checked:", n_checked)
        assert n_checked > 0
    finally:
        eng.close()


@pytest.mark.parametrize("name,mode", [("transformer_greedy", "greedy"), ("transformer_beam", "fast"),
                                       ("transformer_classic_beam", "classic"), ("transformer_aan", "greedy"),
                                       ("transformer_aan", "fast")])
def test_translator_moves_on_golden_models(name, mode):
    _check_moves(name, mode)


def test_translator_moves_on_a_pool_of_two_lanes():
    _check_moves("transformer_greedy", "greedy", pool=True)


def test_engine_token_positions_method():
    from nanodecoder_amd import synth
    from nanodecoder_amd.engine import Engine
    cfg = synth.ModelConfig()
    eng = Engine(cfg, synth.make_weights(cfg, seed=1), device=0, max_batch=4, max_steps=8)
    try:
        attn = softmax_rows(3, 8, 128, seed=4)
        spans = np.asarray([128, 100, 5], np.int32)
        got = eng.token_positions(torch.from_numpy(attn), spans)
        assert got.dtype == torch.int32 and got.is_cuda
        assert got.cpu().numpy().tolist() == frontend.token_positions(attn, spans).tolist()
        four = np.stack([attn, attn[:, ::-1]], axis=1)
        got = eng.token_positions(torch.from_numpy(np.ascontiguousarray(four)), spans)  # hyp0 by the axes
        assert got.cpu().numpy().tolist() == frontend.token_positions(attn, spans).tolist()
        with pytest.raises(ValueError):
            eng.token_positions(torch.from_numpy(attn), spans[:2])
    finally:
        eng.close()


def test_raw_reads_arrays_carry_the_token_positions():
    """stream_raw_reads(arrays=True, moves=True): the last array holds every token's position, and spread over
    the characters it is what translate_raw_reads(moves=True) returns per chunk."""
    from nanodecoder_amd import synth
    from nanodecoder_amd.engine import Engine
    cfg = synth.ModelConfig()
    eng = Engine(cfg, synth.make_weights(cfg, seed=11, eos_bias=-1.0), device=0, max_batch=8, max_steps=30)
    try:
        tr = _translator(cfg, eng, max_length=30, min_length=4, batch_size=4)
        raws = [synth.synth_raw_read(i, n).astype(np.float64) for i, n in enumerate((700, 1300))]
        kw = dict(batch_size=4, normalization="median", src_seq_length=300, src_seq_stride=60)
        per_chunk = tr.translate_raw_reads(raws, moves=True, **kw)
        plain = tr.translate_raw_reads(raws, **kw)
        assert [p[:2] for p in per_chunk] == plain
        n_checked = 0
        for out in tr.stream_raw_reads(raws, arrays=True, moves=True, **kw):
            ri, tok, sc, ps = out
            assert ps.dtype == np.int32 and ps.shape == tok.shape and (np.diff(ps, axis=1) >= 0).all()
            for ci in range(tok.shape[0]):
                want = tr._char_weights(tok[ci].tolist(), ps[ci], np.int32)
                assert per_chunk[ri][2][ci].tolist() == want.tolist()
                n_checked += len(want)
        assert n_checked > 0
    finally:
        eng.close()


# ---------------------------------------------------------------- translate.py -moves
def test_cli_moves_gpu_assembly_matches_host(tmp_path):
    """-moves with -assembly cpu against -assembly gpu (and the device front end) on a few short reads with
    overlapping windows: the same result/*.moves bytes, and every other file as without -moves."""
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
    files = {}
    try:
        T.Translator.__init__ = spy
        for m, asm, fe, mv in (("plain", "cpu", "cpu", []), ("cpu", "cpu", "cpu", ["-moves"]),
                               ("gpu", "gpu", "gpu", ["-moves"])):
            out = tmp_path / ("out_" + m)
            o = opts.parse_translate_opts(["-model", str(ck), "-src_dir", str(src), "-save_data", str(out), "-gpu",
                                           "0", "-beam_size", "1", "-batch_size", "4", "-thread", "2", "-max_length",
                                           "30", "-min_length", "4", "-engine_max_batch", "8", "-engine_lanes", "1",
                                           "-src_seq_length", "300", "-src_seq_stride", "60", "-assembly", asm,
                                           "-frontend", fe, "-fastq"] + mv)
            assert cli.main(o) == len(sizes)
            files[m] = {os.path.join(d, f): (out / d / f).read_bytes() for d in ("result", "segment")
                        for f in sorted(os.listdir(out / d))}
    finally:
        T.Translator.__init__ = orig
    for e in built:
        e.close()
    moves = sorted(k for k in files["cpu"] if k.endswith(".moves"))
    assert moves == [os.path.join("result", f"read{i}.moves") for i in range(len(sizes))]
    assert not any(k.endswith(".moves") for k in files["plain"])
    for m in ("cpu", "gpu"):
        assert {k: v for k, v in files[m].items() if not k.endswith(".moves")} == files["plain"], m
        assert {k: files[m][k] for k in moves} == {k: files["cpu"][k] for k in moves}, m
    some = 0
    for i, n in enumerate(sizes):
        head, seq, pos = files["gpu"][os.path.join("result", f"read{i}.moves")].decode().split("\n")[:3]
        assert head == f">read{i}" and files["plain"][os.path.join("result", f"read{i}.fasta")].decode() == \
            f">read{i}\n{seq}"
        vals = [int(v) for v in pos.split(",")] if pos else []
        assert len(vals) == len(seq) and vals == sorted(vals) and all(0 <= v < n for v in vals)
        some += len(vals)
    assert some > 0  # not only empty reads
