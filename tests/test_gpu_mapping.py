"""Read mapping on the device: nd_locate_segs and nd_align_fit against the host rules accuracy.locate_host and
accuracy.fit_host, and accuracy.map_reads on the device against the host.  Integer rules, so every comparison is
exact equality: hits, oriented bytes, counts, spans, ops and status."""
import ctypes

import numpy as np
import pytest
import torch

from nanodecoder_amd import _lib, accuracy
from tests.test_accuracy_host import mutate, random_seq
from tests.test_mapping_host import FIT_FIXED, locate_cases, planted_reads

pytestmark = pytest.mark.gpu
A = accuracy
MAX = A.ALIGN_MAX_LEN
DEV = "cuda:0"


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _offsets(parts):
    off = np.zeros(len(parts) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in parts])
    return off


def fit_raw(pairs, skip=(), cells=None, want_ops=True, windows=None):
    """One nd_align_fit call: pair k is (call, window); the windows are laid one after another (a spacer base
    between them) as the reference.  Pairs in ``skip`` come in with status 1.  Returns (counts, span in window
    coordinates, ops per pair, status).  ``windows`` {k: (w0, w1)} replaces pair k's window by one given in the
    reference's own coordinates."""
    P = len(pairs)
    calls = [A._bytes(c) for c, _ in pairs]
    ref = "X".join(w for _, w in pairs) + "X"
    w0 = np.cumsum([0] + [len(w) + 1 for _, w in pairs])[:-1]
    hit = np.zeros((P, 4), np.int32)
    hit[:, 1] = w0
    hit[:, 2] = w0 + np.asarray([len(w) for _, w in pairs])
    for k, (a, b) in (windows or {}).items():
        hit[k, 1:3] = a, b
    off = _offsets(calls)
    nbytes = int(off[-1])
    true_cells = sum(len(c) * len(w) for k, (c, w) in enumerate(pairs) if k not in skip and len(c) <= MAX and len(w) <= MAX)
    cells = true_cells if cells is None else cells
    L = _lib.lib()
    work_bytes = int(L.nd_align_fit_work_bytes(P, cells))
    call_d = torch.zeros(nbytes + 1, dtype=torch.uint8, device=DEV)
    if nbytes:
        call_d[:nbytes] = torch.from_numpy(np.concatenate(calls)).to(DEV)
    ref_d = torch.from_numpy(np.frombuffer(ref.encode(), np.uint8).copy()).to(DEV)
    off_d, hit_d = torch.from_numpy(off).to(DEV), torch.from_numpy(hit).to(DEV)
    status = np.zeros(P, np.int32)
    status[list(skip)] = 1
    status_d = torch.from_numpy(status).to(DEV)
    counts_d = torch.full((P, 5), 77, dtype=torch.int32, device=DEV)
    span_d = torch.full((P, 2), 77, dtype=torch.int32, device=DEV)
    ops_d = torch.full((nbytes + 1,), 9, dtype=torch.uint8, device=DEV) if want_ops else None
    work_d = torch.zeros(work_bytes, dtype=torch.uint8, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    _lib.check(L.nd_align_fit(_ptr(call_d), _ptr(off_d), _ptr(ref_d), len(ref), _ptr(hit_d), P, cells, _ptr(counts_d),
                              _ptr(span_d), _ptr(ops_d) if want_ops else None, _ptr(status_d), _ptr(work_d), work_bytes,
                              stream), "nd_align_fit")
    torch.cuda.synchronize()
    counts, span, st = counts_d.cpu().numpy(), span_d.cpu().numpy(), status_d.cpu().numpy()
    ops = None
    if want_ops:
        flat = ops_d.cpu().numpy()
        assert flat[nbytes] == 9  # nothing past the last base
        ops = [flat[off[k]: off[k + 1]] for k in range(P)]
    span = np.where(span >= 0, span - w0[:, None], span)
    return counts, span, ops, st


def fit_boundary_pairs(seed=31):
    """One pair each side of every boundary the fit form has: 16-column direction words and the packed remainder
    (m = 15, 16, 17), 4 rows per thread and 1024 per strip (n = 1, 3, 4, 5, 1023, 1024, 1025, 2049), row n owned by
    the first (n <= 4, 1025, 2049), a middle (n = 513, 1023 - 500) and the last thread (n = 1023, 1024), 255 / 256 /
    257 blocks (m = 4080, 4096, 4112), j* in the last partial block (the call is the window's end), j* = 0 (nothing
    matches), and paths longer than the 64-row, 64-column traceback window."""
    rng = np.random.default_rng(seed)
    pairs = list(FIT_FIXED)

    def inside(n, m, rate=0.1, at=None, alphabet="ACGT"):
        w = random_seq(rng, m, alphabet)
        lo = int(rng.integers(0, max(1, m - n))) if at is None else at
        call = mutate(rng, w[lo: lo + n], rate, alphabet)
        call = (call + random_seq(rng, max(0, n - len(call)), alphabet))[:n]
        pairs.append((call, w))
    for m in (15, 16, 17, 31, 33):
        for n in (1, 3, 4, 5, 9):
            inside(n, m, 0.2)
    for m in range(1, 20):
        inside(5 + m % 4, m, 0.3, alphabet="AC")  # ties everywhere
    for n in (513, 523, 1023, 1024, 1025, 2049):
        inside(n, n + 300 + n % 13)
    for n in (1023, 1025):
        inside(n, 1500 + n % 16, at=1500 + n % 16 - n)  # the call is the window's end: j* in the last partial block
        inside(n, 1500, at=0)                            # its beginning: t_start = 0
    for m in (4080, 4096, 4112):
        inside(1030, m)
    inside(300, 3367, at=3067)
    pairs.append(("G" * 70, "AC" * 100))  # nothing matches: D[n][j] = n everywhere, j* = 0
    pairs.append((random_seq(rng, 200), random_seq(rng, 150)))  # unrelated
    pairs.append(("T" * 40 + pairs[-1][1][:100], pairs[-1][1]))  # the path reaches column 0 with i > 0
    return pairs


@pytest.fixture(scope="module")
def fit_case():
    pairs = fit_boundary_pairs()
    return pairs, [A.fit_host(c, w) for c, w in pairs]


def check_fit(pairs, want, counts, span, ops, status, idx=None):
    for k in (range(len(pairs)) if idx is None else idx):
        tag = (k, len(pairs[k][0]), len(pairs[k][1]))
        assert status[k] == 0, tag
        assert counts[k].tolist() == want[k][0].tolist(), tag
        assert tuple(span[k].tolist()) == tuple(want[k][1]), tag
        if ops is not None:
            assert ops[k].tobytes() == want[k][2].tobytes(), tag


def test_fit_equals_the_host_rule(fit_case):
    pairs, want = fit_case
    counts, span, ops, status = fit_raw(pairs)
    check_fit(pairs, want, counts, span, ops, status)
    # the cases of the issue are among them
    by = {p: w for p, w in zip(pairs, want)}
    assert by[("A", "AAAA")][1] == (0, 1) and by[("G" * 70, "AC" * 100)][1] == (0, 0)
    assert any(w[1][1] == len(p[1]) and len(p[1]) % 16 for p, w in zip(pairs, want) if len(p[0]) > 1000)
    c0, s0, none, st0 = fit_raw(pairs, want_ops=False)  # d_ops null: the same
    assert none is None and c0.tobytes() == counts.tobytes() and s0.tobytes() == span.tobytes()
    rc, rs, ro, rst = fit_raw(pairs[::-1])  # pair order reversed: the same per-pair results
    assert rc[::-1].tobytes() == counts.tobytes() and rs[::-1].tobytes() == span.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ro[::-1], ops))


def test_fit_skipped_understated_and_too_long(fit_case):
    pairs, want = fit_case
    # two skipped pairs between three live ones: a short one, one of two strips by 255 blocks, one of three strips
    pick = [next(k for k, p in enumerate(pairs) if cond(p, want[k])) for cond in (
        lambda p, w: len(p[0]) == 5 and len(p[1]) == 16,
        lambda p, w: len(p[0]) == 1023,
        lambda p, w: len(p[0]) == 1030 and len(p[1]) == 4080,
        lambda p, w: len(p[0]) == 300,
        lambda p, w: len(p[0]) == 2049)]
    assert len(set(pick)) == 5
    sub, wsub = [pairs[k] for k in pick], [want[k] for k in pick]
    counts, span, ops, status = fit_raw(sub, skip=(1, 3))
    assert status.tolist() == [0, 1, 0, 1, 0]
    check_fit(sub, wsub, counts, span, ops, status, (0, 2, 4))
    for k in (1, 3):
        assert counts[k].tolist() == [-1] * 5 and span[k].tolist() == [-1, -1] and not ops[k].any()
    # cells understated: bit 1 for the pairs that did not fit, the others exact
    rng = np.random.default_rng(55)
    many = []
    for k in range(8):
        w = random_seq(rng, 300 + 10 * k)
        many.append((mutate(rng, w[100:200], 0.1), w))
    wmany = [A.fit_host(c, w) for c, w in many]
    true_cells = sum(len(c) * len(w) for c, w in many)
    for cells in (0, true_cells // 2):
        counts, span, ops, status = fit_raw(many, cells=cells)
        assert set(status.tolist()) <= {0, 2} and (status == 2).any()
        if cells:
            assert (status == 0).any()
        for k in range(len(many)):
            if status[k]:
                assert counts[k].tolist() == [-1] * 5 and span[k].tolist() == [-1, -1] and not ops[k].any()
        check_fit(many, wmany, counts, span, ops, status, [k for k in range(len(many)) if status[k] == 0])
    # a side above 8192: bit 2; its neighbours exact
    long_ = [many[0], (random_seq(rng, 20), random_seq(rng, MAX + 1)), many[1], (random_seq(rng, MAX + 1), "ACGT"),
             (random_seq(rng, 64), random_seq(rng, MAX))]
    counts, span, ops, status = fit_raw(long_)
    assert status.tolist() == [0, 4, 0, 4, 0]
    check_fit(long_, [wmany[0], None, wmany[1], None, A.fit_host(*long_[4])], counts, span, ops, status, (0, 2, 4))
    for k in (1, 3):
        assert counts[k].tolist() == [-1] * 5 and span[k].tolist() == [-1, -1] and not ops[k].any()
    # a window that is not inside the reference: bit 2, nothing read there; its neighbours exact
    five = many[:5]
    total = sum(len(w) + 1 for _, w in five)  # fit_raw's reference
    counts, span, ops, status = fit_raw(five, windows={1: (total - 50, total + 1), 3: (-1, 120)})
    assert status.tolist() == [0, 4, 0, 4, 0]
    check_fit(five, wmany[:5], counts, span, ops, status, (0, 2, 4))
    for k in (1, 3):
        assert counts[k].tolist() == [-1] * 5 and span[k].tolist() == [-1, -1] and not ops[k].any()
    # the reference's last byte is a legal end
    total = len(five[0][1]) + 1  # one pair: its window and the spacer
    c1, s1, o1, st1 = fit_raw(five[:1], windows={0: (total - 40, total)})
    assert st1.tolist() == [0] and c1[0, 1] + c1[0, 2] + c1[0, 3] == len(five[0][0])


# ---------------------------------------------------------------- the index
def test_index_built_with_the_device_sort_equals_the_host_build():
    rng = np.random.default_rng(99)
    unit = random_seq(rng, 40)
    seqs = [random_seq(rng, 70000), unit * 12 + "N" + random_seq(rng, 500), "", random_seq(rng, 14)]  # repeats: > 8
    ref = A.Reference(["a", "b", "c", "d"], seqs)
    host = A.build_index(ref.seq, ref.rec_off)
    dev = A.build_index(ref.seq, ref.rec_off, device=0)
    assert all(a.dtype == b.dtype == np.uint32 and a.tobytes() == b.tobytes() for a, b in zip(host, dev))
    assert host[0].size > 70000 and (np.diff(host[0].astype(np.int64)) >= 0).all()
    # a Reference whose index was not built yet builds it on the device
    fresh = A.Reference(["a", "b", "c", "d"], seqs)
    code_d, pos_d = fresh.on_device(torch.device(DEV))[2:]
    assert code_d.cpu().numpy().view(np.uint32).tobytes() == host[0].tobytes()
    assert pos_d.cpu().numpy().view(np.uint32).tobytes() == host[1].tobytes()
    assert fresh.index[0].tobytes() == host[0].tobytes()


# ---------------------------------------------------------------- locate
def locate_raw(queries, ref):
    """One nd_locate_segs call: (hit [P, 4], status [P], the oriented segments)."""
    P = len(queries)
    qs = [A._bytes(q) for q in queries]
    off = _offsets(qs)
    nbytes = int(off[-1])
    dev = torch.device(DEV)
    seq_d, rec_d, code_d, pos_d = ref.on_device(dev)
    call_d = torch.zeros(nbytes + 1, dtype=torch.uint8, device=DEV)
    call_d[:nbytes] = torch.from_numpy(np.concatenate(qs)).to(DEV)
    off_d = torch.from_numpy(off).to(DEV)
    hit_d = torch.full((P, 4), 77, dtype=torch.int32, device=DEV)
    status_d = torch.full((P,), 77, dtype=torch.int32, device=DEV)
    or_d = torch.full((nbytes + 1,), 9, dtype=torch.uint8, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L = _lib.lib()
    _lib.check(L.nd_locate_segs(_ptr(call_d), _ptr(off_d), P, _ptr(code_d), _ptr(pos_d), int(code_d.numel()),
                                _ptr(rec_d), int(rec_d.numel()) - 1, _ptr(hit_d), _ptr(status_d), _ptr(or_d), stream),
               "nd_locate_segs")
    torch.cuda.synchronize()
    flat = or_d.cpu().numpy()
    assert flat[nbytes] == 9
    return hit_d.cpu().numpy(), status_d.cpu().numpy(), [flat[off[k]: off[k + 1]] for k in range(P)]


def check_locate(queries, ref, hit, status, oriented):
    for k, q in enumerate(queries):
        mapped, strand, w0, w1, votes = A.locate_host(q, ref)
        assert hit[k].tolist() == [strand, w0, w1, votes], (k, len(q))
        assert status[k] == (0 if mapped else 1), (k, len(q))
        want = A.reverse_complement(q) if strand else A._bytes(q)
        assert oriented[k].tobytes() == want.tobytes(), (k, len(q))


def test_locate_cases_of_the_host_file():
    cases = locate_cases()
    strands = set()
    for name, q, seqs in cases:
        ref = A.Reference(["r%d" % i for i in range(len(seqs))], seqs)
        hit, status, oriented = locate_raw([q], ref)
        check_locate([q], ref, hit, status, oriented)
        strands.add(int(hit[0, 0]))
    assert strands == {0, 1}


def test_locate_300_segments_in_one_call():
    rng = np.random.default_rng(77)
    seqs = [random_seq(rng, 40000), random_seq(rng, 30000)]  # positions above 2^16
    ref = A.Reference(["a", "b"], seqs)
    cat = "".join(seqs)
    queries = []
    for k in range(300):
        n = int(rng.integers(10, 400)) if k % 7 else int(rng.integers(3000, 4097))
        lo = int(rng.integers(0, len(cat) - n))
        q = mutate(rng, cat[lo: lo + n], 0.1)[:4096] if k % 11 else random_seq(rng, n)
        if k % 13 == 0:
            q = q[: len(q) // 2] + "N" + q[len(q) // 2 + 1:]
        queries.append(A.reverse_complement(q).tobytes().decode() if k % 2 else q)
    hit, status, oriented = locate_raw(queries, ref)
    check_locate(queries, ref, hit, status, oriented)
    assert (status == 0).sum() > 100 and (status == 1).sum() > 10 and (hit[:, 1] > 2 ** 16).any()
    assert {0, 1} <= set(hit[status == 0, 0].tolist())


def test_locate_the_last_bin_of_the_largest_reference():
    """A reference of 2^23 bases, invalid bytes but for three planted stretches (so its index is small): one ends
    with the reference, and its query votes in the last bin there is."""
    rng = np.random.default_rng(88)
    total = A.MAP_REF_MAX
    seq = np.full(total, ord("N"), np.uint8)
    spots = [(100000, 900), (5000000, 2000), (total - 700, 700)]
    for lo, n in spots:
        seq[lo: lo + n] = A._bytes(random_seq(rng, n))
    ref = A.Reference(["big"], [seq])
    text = lambda lo, n: seq[lo: lo + n].tobytes().decode()  # noqa: E731
    queries = [text(total - 600, 600), A.reverse_complement(text(total - 700, 650)).tobytes().decode(),
               mutate(rng, text(5000300, 1500), 0.1), text(100000, 900), text(total - 15, 15) + "ACGT" * 5]
    hit, status, oriented = locate_raw(queries, ref)
    check_locate(queries, ref, hit, status, oriented)
    assert status[:4].tolist() == [0, 0, 0, 0] and hit[0, 2] == total and hit[1, 2] == total and hit[1, 0] == 1
    assert hit[0, 3] == 600 - 14


# ---------------------------------------------------------------- the public function
def test_map_reads_device_equals_host():
    lengths = (500, 1000, 2500, 4096, 4097, 9000, 12289, 700) + tuple(300 + 37 * k for k in range(16))
    ref, reads = planted_reads(seed=29, lengths=lengths)
    assert len(reads) == 24  # planted; then two that map nowhere
    calls = [r[0] for r in reads] + ["ACGT", random_seq(np.random.default_rng(2), 500)]
    hs, ds = {}, {}
    hc, hr, ho = A.map_reads(calls, ref, want_ops=True, stats=hs)
    dc, dr, do = A.map_reads(calls, ref, device=0, want_ops=True, stats=ds)
    assert hs == ds and hs["unmapped"] == 2 and hs["segments"] > 24
    assert dc.dtype == np.int32 and dc.tobytes() == hc.tobytes()
    for k in range(len(calls)):
        assert [r[:7] for r in dr[k]] == [r[:7] for r in hr[k]], k
        assert all(a[7].tolist() == b[7].tolist() for a, b in zip(dr[k], hr[k])), k
        assert do[k].tobytes() == ho[k].tobytes(), k
    assert A.map_reads(calls[:2], ref, device=0)[2] is None
    assert A.map_reads([], ref, device=0)[0].shape == (0, 5)
