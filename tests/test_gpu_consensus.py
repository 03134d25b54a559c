"""Consensus accuracy on the device: nd_align_fit_pos against nd_align_fit and accuracy.fit_pos_host, nd_pileup_add
against accuracy.pile_add_host, nd_pileup_call against accuracy.consensus_host, and accuracy.Pileup on the device
against the host.  Integer rules, so every comparison is exact equality."""
import ctypes

import numpy as np
import pytest
import torch

from nanodecoder_amd import _lib, accuracy
from tests.test_accuracy_host import mutate, random_seq
from tests.test_consensus_host import (HAND_CALL, HAND_W0, HAND_WIN, hand_reference, planted_variants,
                                       threshold_case)
from tests.test_mapping_host import FIT_FIXED

pytestmark = pytest.mark.gpu
A = accuracy
MAX = A.ALIGN_MAX_LEN
DEV = "cuda:0"
NONE = A.CONS_NONE


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------- nd_align_fit_pos
def fit_both(pairs, skip=(), cells=None):
    """nd_align_fit and nd_align_fit_pos on the same inputs: pair k is (call, window), the windows laid one after
    another with one spacer base between them, so that the first starts at reference position 0 and the last ends
    at ref_len.  Returns (w0 per pair, off, (counts, span, ops, status) of nd_align_fit, the same and rpos of
    nd_align_fit_pos), spans and rpos in the reference's coordinates."""
    P = len(pairs)
    calls = [A._bytes(c) for c, _ in pairs]
    ref = "X".join(w for _, w in pairs)
    w0 = np.cumsum([0] + [len(w) + 1 for _, w in pairs])[:-1]
    hit = np.zeros((P, 4), np.int32)
    hit[:, 1] = w0
    hit[:, 2] = w0 + np.asarray([len(w) for _, w in pairs])
    assert hit[0, 1] == 0 and hit[-1, 2] == len(ref)
    off = np.zeros(P + 1, np.int32)
    off[1:] = np.cumsum([c.size for c in calls])
    nbytes = int(off[-1])
    true_cells = sum(len(c) * len(w) for k, (c, w) in enumerate(pairs)
                     if k not in skip and len(c) <= MAX and len(w) <= MAX)
    cells = true_cells if cells is None else cells
    L = _lib.lib()
    work_bytes = int(L.nd_align_fit_pos_work_bytes(P, cells))
    assert work_bytes == int(L.nd_align_fit_work_bytes(P, cells))
    call_d = torch.zeros(nbytes + 1, dtype=torch.uint8, device=DEV)
    call_d[:nbytes] = _dev(np.concatenate(calls))
    ref_d = _dev(np.frombuffer((ref + "X").encode(), np.uint8).copy())  # one byte more than ref_len: an address
    off_d, hit_d = _dev(off), _dev(hit)
    status = np.zeros(P, np.int32)
    status[list(skip)] = 1
    out = []
    for pos in (False, True):
        status_d = _dev(status)
        counts_d = torch.full((P, 5), 77, dtype=torch.int32, device=DEV)
        span_d = torch.full((P, 2), 77, dtype=torch.int32, device=DEV)
        ops_d = torch.full((nbytes + 1,), 9, dtype=torch.uint8, device=DEV)
        rpos_d = torch.full((nbytes + 1,), 77, dtype=torch.int32, device=DEV)
        work_d = torch.zeros(work_bytes, dtype=torch.uint8, device=DEV)
        if pos:
            _lib.check(L.nd_align_fit_pos(_ptr(call_d), _ptr(off_d), _ptr(ref_d), len(ref), _ptr(hit_d), P, cells,
                                          _ptr(counts_d), _ptr(span_d), _ptr(ops_d), _ptr(rpos_d), _ptr(status_d),
                                          _ptr(work_d), work_bytes, _stream()), "nd_align_fit_pos")
        else:
            _lib.check(L.nd_align_fit(_ptr(call_d), _ptr(off_d), _ptr(ref_d), len(ref), _ptr(hit_d), P, cells,
                                      _ptr(counts_d), _ptr(span_d), _ptr(ops_d), _ptr(status_d), _ptr(work_d),
                                      work_bytes, _stream()), "nd_align_fit")
        torch.cuda.synchronize()
        ops, rpos = ops_d.cpu().numpy(), rpos_d.cpu().numpy()
        assert ops[nbytes] == 9 and rpos[nbytes] == 77  # nothing past the last base
        out.append((counts_d.cpu().numpy(), span_d.cpu().numpy(), ops[:nbytes], status_d.cpu().numpy(),
                    rpos[:nbytes]))
    assert (out[0][4] == 77).all()  # nd_align_fit was given no rpos
    return w0, off, out[0][:4], out[1]


def pos_boundary_pairs(seed=41):
    """n and m around 1, 15 / 16 / 17 (the 16-column direction words) and 63 / 64 / 65 (the 64-row, 64-column
    traceback window), paths longer than that window, n = 1030 across the 1024-row strip, an empty call, and the
    fixed cases of the host file (j* = 0, a path that reaches column 0 with i > 0, an empty window)."""
    rng = np.random.default_rng(seed)
    sizes = (1, 2, 15, 16, 17, 63, 64, 65)
    pairs = []
    for n in sizes:
        for m in sizes:
            w = random_seq(rng, m)
            lo = int(rng.integers(0, max(1, m - n + 1)))
            call = mutate(rng, w[lo: lo + n], 0.15)
            pairs.append(((call + random_seq(rng, n))[:n], w))
    for n in (63, 64, 65, 130):
        for m in (100, 129, 200):
            w = random_seq(rng, m)
            call = mutate(rng, (w + w)[m // 5: m // 5 + n], 0.15)
            pairs.append(((call + random_seq(rng, n))[:n], w))
        pairs.append((random_seq(rng, n, "AC"), random_seq(rng, n + 3, "AC")))  # ties everywhere
    w = random_seq(rng, 1400)
    pairs.append((mutate(rng, w[150: 1300], 0.1)[:1030], w))
    # the first pair, its window at reference position 0: the column-0 border with 70 rows left, rpos = -1
    pairs.insert(0, ("T" * 70 + w[:100], w[:300]))
    pairs.append(("", "ACGT"))
    pairs += [p for p in FIT_FIXED if p[0]]
    pairs.append((w[1200:1260], w[1000:1260]))  # the last pair: its window ends with the reference
    return pairs


@pytest.fixture(scope="module")
def pos_case():
    pairs = pos_boundary_pairs()
    return pairs, [A.fit_pos_host(c, w) for c, w in pairs]


def test_fit_pos_equals_fit_and_the_host_positions(pos_case):
    pairs, want = pos_case
    assert any(len(c) == 1 for c, _ in pairs) and any(len(c) == 1030 for c, _ in pairs) and any(len(c) == 0 for c, _ in pairs)
    w0, off, fit, pos = fit_both(pairs)
    for name, a, b in zip(("counts", "span", "ops", "status"), fit, pos):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name  # bit for bit nd_align_fit's
    counts, span, ops, status, rpos = pos
    assert not status.any()
    for k, (c, w) in enumerate(pairs):
        tag = (k, len(c), len(w))
        wc, wspan, wops, wrpos = want[k]
        assert counts[k].tolist() == wc.tolist(), tag
        assert (span[k] - w0[k]).tolist() == list(wspan), tag
        assert ops[off[k]: off[k + 1]].tobytes() == wops.tobytes(), tag
        assert (rpos[off[k]: off[k + 1]] - w0[k]).tolist() == wrpos.tolist(), tag
    # the ends of the reference and the border are among them
    assert rpos.min() == -1 and rpos.max() == len("X".join(w for _, w in pairs)) - 1
    assert pairs[0][0].startswith("T" * 70) and (rpos[:70] == -1).all() and rpos[70] == 0


def test_fit_pos_of_pairs_that_are_not_aligned(pos_case):
    pairs, want = pos_case
    rng = np.random.default_rng(43)
    pick = [next(k for k, p in enumerate(pairs) if len(p[0]) == n) for n in (17, 1030, 64)]
    sub = [pairs[pick[0]], pairs[pick[1]], pairs[pick[2]], (random_seq(rng, 20), random_seq(rng, MAX + 1)),
           pairs[pick[0]]]
    w0, off, fit, pos = fit_both(sub, skip=(1,))
    counts, span, ops, status, rpos = pos
    assert status.tolist() == [0, 1, 0, 4, 0] and fit[3].tolist() == status.tolist()
    for a, b in zip(fit, pos):
        assert a.tobytes() == b.tobytes()
    for k in (1, 3):  # skipped (status bit 0 on entry), too long
        assert counts[k].tolist() == [-1] * 5 and (rpos[off[k]: off[k + 1]] == -1).all()
        assert off[k + 1] > off[k] and not ops[off[k]: off[k + 1]].any()
    for k, j in ((0, pick[0]), (2, pick[2]), (4, pick[0])):
        assert (rpos[off[k]: off[k + 1]] - w0[k]).tolist() == want[j][3].tolist()
    # cells understated: the pairs that did not fit have rpos -1, the others the host's
    many = []
    for k in range(8):
        w = random_seq(rng, 300 + 10 * k)
        many.append((mutate(rng, w[100:200], 0.1), w))
    w0, off, fit, pos = fit_both(many, cells=sum(len(c) * len(w) for c, w in many) // 2)
    counts, span, ops, status, rpos = pos
    assert set(status.tolist()) == {0, 2}
    for a, b in zip(fit, pos):
        assert a.tobytes() == b.tobytes()
    for k, (c, w) in enumerate(many):
        got = rpos[off[k]: off[k + 1]]
        if status[k]:
            assert (got == -1).all() and got.size
        else:
            assert (got - w0[k]).tolist() == A.fit_pos_host(c, w)[3].tolist()


# ---------------------------------------------------------------- nd_pileup_add
def pile_raw(batches, ref_len):
    """nd_pileup_add per batch into one table: a batch is a list of (oriented call, ops, rpos, status).  Returns
    the table [9, ref_len] uint32."""
    L = _lib.lib()
    pile_d = torch.zeros(9 * ref_len + 1, dtype=torch.int32, device=DEV)
    for batch in batches:
        calls = [A._bytes(b[0]) for b in batch]
        off = np.zeros(len(batch) + 1, np.int32)
        off[1:] = np.cumsum([c.size for c in calls])
        n = int(off[-1])
        pad = lambda parts, dt: np.concatenate([np.asarray(x, dt).reshape(-1) for x in parts]  # noqa: E731
                                               + [np.zeros(1, dt)])
        call_d, ops_d = _dev(pad(calls, np.uint8)), _dev(pad([b[1] for b in batch], np.uint8))
        rpos_d = _dev(pad([b[2] for b in batch], np.int32))
        assert call_d.numel() == ops_d.numel() == rpos_d.numel() == n + 1
        off_d, status_d = _dev(off), _dev(np.asarray([b[3] for b in batch], np.int32))
        _lib.check(L.nd_pileup_add(_ptr(call_d), _ptr(off_d), _ptr(ops_d), _ptr(rpos_d), _ptr(status_d), len(batch),
                                   _ptr(pile_d), ref_len, _stream()), "nd_pileup_add")
        torch.cuda.synchronize()
    flat = pile_d.cpu().numpy()
    assert flat[-1] == 0
    return flat[:-1].view(np.uint32).reshape(9, ref_len)


def pile_host(batches, ref_len):
    pile = np.zeros((9, ref_len), np.uint32)
    for batch in batches:
        for call, ops, rpos, status in batch:
            if status == 0:
                A.pile_add_host(pile, call, ops, rpos)
    return pile


def fitted(call, window, w0, status=0):
    _, _, ops, rpos = A.fit_pos_host(call, window, w0)
    return (call, ops, rpos, status)


def test_pileup_add_the_hand_case_and_contention():
    ref = hand_reference()
    one = fitted(HAND_CALL, HAND_WIN, HAND_W0)
    got = pile_raw([[one]], ref.total)
    assert got.tobytes() == pile_host([[one]], ref.total).tobytes() and got.sum() == 25 and got[6, 116] == 1
    # 64 identical reads on one window: every add of a wave's lane meets 63 others on its address
    got = pile_raw([[one] * 64], ref.total)
    assert got.tobytes() == pile_host([[one] * 64], ref.total).tobytes()
    assert got.max() == 64 and got.sum() == 64 * 25 and got[4, 110] == 64


def test_pileup_add_edges_statuses_and_accumulation():
    rng = np.random.default_rng(47)
    total = 700
    genome = random_seq(rng, total)
    batch = []
    for k, (lo, hi) in enumerate(((0, 300), (420, 700), (100, 500), (250, 650), (0, 700))):
        call = mutate(rng, genome[lo:hi], 0.12)
        w0, w1 = max(0, lo - 40), min(total, hi + 40)
        batch.append(fitted(call, genome[w0:w1], w0))
    exact = fitted(genome[:120], genome[:120], 0)           # position 0 as a diagonal base
    tail = fitted(genome[600:], genome[560:], 560)          # position ref_len - 1
    odd = genome[300:330] + "N" + genome[331:350] + "NN" + genome[350:380]   # non-ACGT bytes: matched, inserted
    odd = fitted(odd, genome[280:400], 280)
    assert (odd[1][[30]] == 1).all() and 2 in odd[1].tolist()
    dead = fitted(genome[50:250], genome[:300], 0, status=1)     # a pair with status 1 keeps its rpos here: no add
    wrong = (genome[:50], np.zeros(50, np.uint8), np.full(50, -1, np.int32), 2)
    first = batch[:3] + [dead] + [exact, odd] + [wrong] + batch[3:] + [tail]
    second = [batch[1], ("", np.zeros(0, np.uint8), np.zeros(0, np.int32), 0), batch[4], exact]
    want1 = pile_host([first], total)
    got1 = pile_raw([first], total)
    assert got1.tobytes() == want1.tobytes()
    assert got1[:4, 0].sum() >= 1 and got1[:4, total - 1].sum() >= 1 and got1[4].any() and got1[5:].any()
    assert pile_raw([first[::-1]], total).tobytes() == want1.tobytes()  # the order of the pairs: the same sums
    # two calls into one table
    got2 = pile_raw([first, second], total)
    assert got2.tobytes() == pile_host([first, second], total).tobytes() and got2.sum() > got1.sum()
    # the status decides, not the rpos: the dead pair alone adds nothing
    assert not pile_raw([[dead, wrong]], total).any()


# ---------------------------------------------------------------- nd_pileup_call
def call_raw(pile, ref, min_cov):
    L = _lib.lib()
    total, R = ref.total, len(ref.names)
    pile_d = _dev(np.concatenate([pile.reshape(-1).view(np.int32), np.zeros(1, np.int32)]))
    seq_d = _dev(np.concatenate([ref.seq, np.zeros(1, np.uint8)]))
    off_d = _dev(ref.rec_off)
    cons_d = torch.full((total + 1,), 9, dtype=torch.uint8, device=DEV)
    ins_d = torch.full((total + 1,), 9, dtype=torch.uint8, device=DEV)
    cov_d = torch.full((total + 1,), 77, dtype=torch.int32, device=DEV)
    rec_d = torch.full((R * 6 + 1,), 77, dtype=torch.int64, device=DEV)  # comes in non-zero
    _lib.check(L.nd_pileup_call(_ptr(pile_d), _ptr(seq_d), total, _ptr(off_d), R, min_cov, _ptr(cons_d), _ptr(ins_d),
                                _ptr(cov_d), _ptr(rec_d), _stream()), "nd_pileup_call")
    torch.cuda.synchronize()
    cons, ins, cov, rec = (t.cpu().numpy() for t in (cons_d, ins_d, cov_d, rec_d))
    assert cons[total] == 9 and ins[total] == 9 and cov[total] == 77 and rec[R * 6] == 77
    return cons[:total], ins[:total], cov[:total], rec[: R * 6].reshape(R, 6)


def check_call(pile, ref, min_cov):
    want = A.consensus_host(pile, ref, min_cov)
    got = call_raw(pile, ref, min_cov)
    for name, g, w in zip(("cons", "ins", "cov", "rec"), got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, min_cov)
    return want


def random_pile(rng, total, empty_from=None):
    pile = rng.integers(0, 4, (9, total)).astype(np.uint32)
    pile[:5] *= rng.integers(0, 4, (1, total)).astype(np.uint32)     # columns of coverage 0 .. 45
    pile[5:] *= (rng.integers(0, 3, (1, total)) == 0).astype(np.uint32) * 3
    if empty_from is not None:
        pile[:, empty_from:] = 0
    return pile


@pytest.mark.parametrize("min_cov", (1, 5))
def test_pileup_call_equals_the_host_rule(min_cov):
    rng = np.random.default_rng(53)
    total = 1000 + 37
    text = random_seq(rng, total, "ACGTN")
    # a record shorter than a workgroup's stretch, one that straddles two workgroups, one with no coverage
    ref = A.Reference(["short", "long", "bare"], [text[:30], text[30:1030], text[1030:]])
    pile = random_pile(rng, total, empty_from=1030)
    cons, ins, cov, rec = check_call(pile, ref, min_cov)
    assert rec[0, 0] > 0 and rec[1, 0] > 500 and rec[2].tolist() == [0] * 6 and rec[:2, 1:5].all()
    assert (cons == NONE).any() and (ins != NONE).any()
    # more records in a stretch than are summed at a time, empty ones among them
    cuts = np.unique(np.r_[0, rng.integers(0, total, 150), total])
    parts = [text[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    parts.insert(40, "")
    many = A.Reference(["r%d" % k for k in range(len(parts))], parts)
    assert len(parts) > 100
    check_call(random_pile(rng, total), many, min_cov)


def test_pileup_call_ties_and_thresholds():
    ref, pile, rows = threshold_case()
    cons, ins, cov, rec = check_call(pile, ref, 5)
    for r in range(ref.total):
        assert (int(cons[r]), int(ins[r])) == rows.get(r, (NONE, NONE)), r
    check_call(pile, ref, 1)
    big = pile.copy()   # counts above 2^31: unsigned, and a 64-bit coverage
    big[:, 3] = [2 ** 31 + 5, 2 ** 31 + 5, 7, 0, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 0]
    cons, ins, cov, rec = check_call(big, ref, 5)
    assert cons[3] == 4 and ins[3] == 0


# ---------------------------------------------------------------- the public class
@pytest.fixture(scope="module")
def planted_b():
    ref, mutated, reads = planted_variants(1, step=20, rate=0.10)
    pile, stats = A.Pileup(ref), {}
    res = pile.add(reads, want_ops=True, stats=stats)
    return ref, reads, pile, res, stats


def test_pileup_device_equals_host_on_planted_variants(planted_b):
    ref, reads, host, hres, hstats = planted_b
    dev, dstats = A.Pileup(ref, device=0), {}
    half = len(reads) // 2
    dres = dev.add(reads[:half], want_ops=True, stats=dstats)  # two adds into one table
    dres2 = dev.add(reads[half:], want_ops=True, stats=dstats)
    assert dstats == hstats
    assert np.concatenate([dres[0], dres2[0]]).tobytes() == hres[0].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(dres[2] + dres2[2], hres[2]))
    t = dev.counts()
    assert t.dtype == np.uint32 and t.shape == (9, ref.total) and t.tobytes() == host.counts().tobytes()
    for min_cov in (5, 1):
        h, d = host.call(min_cov), dev.call(min_cov)
        for name, a, b in zip(("cons", "ins", "cov", "rec"), d, h):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, min_cov)
    cons, ins, cov, rec = d = dev.call(5)
    h = host.call(5)
    assert A.consensus_fasta(ref, cons, ins) == A.consensus_fasta(ref, h[0], h[1])
    assert A.variant_lines(ref, cons, ins, cov, t) == A.variant_lines(ref, h[0], h[1], h[2], host.counts())
    assert len(A.variant_lines(ref, cons, ins, cov, t)) == 12
    assert A.coverage_lines(ref, rec) == A.coverage_lines(ref, h[3])
    with pytest.raises(ValueError):
        dev.call(0)


def test_pileup_device_both_strands_and_record_ends():
    """Three records; reads of both strands, one ending on a record's last base, one starting on the next record's
    first, one from position 0 and one to the reference's last base.  The reads are of 1100 bases or more: the
    locate rule takes the record from the middle of its window, and a shorter read at a record's first bases can
    be given the record before."""
    rng = np.random.default_rng(59)
    seqs = [random_seq(rng, 1500), random_seq(rng, 1300), random_seq(rng, 1400)]
    ref = A.Reference(["a", "b", "c"], seqs)
    rc = lambda s: A.reverse_complement(s).tobytes().decode()  # noqa: E731
    reads = [seqs[0][:1100], rc(seqs[0][400:]), seqs[1][:1100], rc(seqs[1][200:]), seqs[2][:1100], rc(seqs[2][300:]),
             seqs[2][250:], mutate(rng, seqs[0][300:1400], 0.1), rc(mutate(rng, seqs[1][100:1250], 0.1)),
             mutate(rng, seqs[2][50:1200], 0.1), "ACGT" * 10]
    host, dev = A.Pileup(ref), A.Pileup(ref, device=0)
    hres, dres = host.add(reads), dev.add(reads)
    assert [[r[:7] for r in rr] for rr in dres[1]] == [[r[:7] for r in rr] for rr in hres[1]]
    assert {r[2] for rr in hres[1] for r in rr} == {0, 1} and sum(1 for rr in hres[1] if not rr) == 1
    t = dev.counts()
    assert t.tobytes() == host.counts().tobytes()
    cov = t[:5].sum(axis=0)
    assert [r[3] for rr in hres[1] for r in rr] == [0, 0, 1, 1, 2, 2, 2, 0, 1, 2]
    assert cov[[0, 1499, 1500, 2799, 2800, -1]].tolist() == [1, 1, 1, 1, 1, 2]
    for a, b in zip(dev.call(1), host.call(1)):
        assert a.tobytes() == b.tobytes()
