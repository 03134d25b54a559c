"""Read accuracy against known sequences: the global alignment of a called read to its truth under a fixed tie
rule, identity, and the table that sets the predicted qualities against the observed errors.

The reference measures accuracy outside its own code: pipeline.evaluate.sh maps the reads with minimap2 and
scripts/read_length_identity.py:58 reads identity as matches over alignment length.  Here the alignment is the
edit-distance DP below, on the host (align_host) or for a whole list of pairs in one device call
(nd_align_seqs, csrc/align.hip), with the same integers either way.

The rule.  Call a[0..n), truth b[0..m), bytes compared for equality; the caller normalises them (normalise:
upper case, M written as C on both sides; methylation accuracy is out of scope).
  borders    : D[i][0] = i, D[0][j] = j
  recurrence : D[i][j] = min(D[i-1][j-1] + (a[i-1] != b[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)
  direction at (i, j), taken in this order:
    diagonal if i, j >= 1 and D[i-1][j-1] + (a[i-1] != b[j-1]) == D[i][j];
    else up  if i >= 1 and (j == 0 or D[i-1][j] + 1 == D[i][j]): consumes a[i-1] only, an inserted base in the call;
    else left: consumes b[j-1] only, a base missing from the call
  alignment  : the path those directions give from (n, m) back to (0, 0)
  per call base, op[i]: 0 = match, 1 = mismatch, 2 = insertion
  per pair, counts = {dist, n_match, n_sub, n_ins, n_del} (int32): n_match + n_sub + n_ins == n,
    n_match + n_sub + n_del == m, dist == n_sub + n_ins + n_del
  identity   : n_match / (n_match + n_sub + n_ins + n_del) in double, 0.0 when that sum is 0 (PAF column 10 over
    column 11)
"""
from __future__ import annotations

import math

import numpy as np

ALIGN_MAX_LEN = 8192      # include/nanodec.h nd_align_seqs: a longer side is aligned on the host
ALIGN_STATUS_LONG = 1     # status bit 0: n or m above ALIGN_MAX_LEN
ALIGN_STATUS_WORK = 2     # status bit 1: the pair's directions did not fit (cells understated)
OP_MATCH, OP_SUB, OP_INS = 0, 1, 2
Q_LEVELS = 41             # FASTQ qualities 0..40 (frontend.quality_string)


def normalise(seq: str) -> str:
    """Upper case, and M (a methylated C) written as C."""
    return seq.upper().replace("M", "C")


def _bytes(seq) -> np.ndarray:
    if isinstance(seq, np.ndarray):
        return np.ascontiguousarray(seq, np.uint8).reshape(-1)
    if isinstance(seq, str):
        seq = seq.encode("utf-8")
    return np.frombuffer(bytes(seq), np.uint8)


def align_host(call, truth):
    """(counts int32 [5], ops uint8 [n]) of one pair by the rule above: numpy over the anti-diagonals i + j = d
    (three of them live at a time), one direction byte per cell, then the traceback.  The host path, the
    fallback of align_reads and the tests' oracle."""
    a, b = _bytes(call), _bytes(truth)
    n, m = int(a.size), int(b.size)
    ops = np.zeros(n, np.uint8)
    dirs = np.zeros(n * m, np.uint8)  # cell (i, j) at (i - 1) * m + (j - 1): 0 diagonal, 1 up, 2 left
    if n and m:
        # diagonal d as an array over i: X[i] = D[i][d - i]
        prev2 = np.zeros(n + 1, np.int32)  # d - 2
        prev = np.zeros(n + 1, np.int32)   # d - 1
        prev[0] = 1                        # D[0][1]
        prev[1] = 1                        # D[1][0]
        rb = b[::-1]
        for d in range(2, n + m + 1):
            cur = np.zeros(n + 1, np.int32)
            if d <= m:
                cur[0] = d
            if d <= n:
                cur[d] = d
            lo, hi = max(1, d - m), min(n, d - 1)  # the inner cells' rows
            # j = d - i runs from d - lo down to d - hi: b[j - 1] read backwards
            cost = (a[lo - 1: hi] != rb[m - (d - lo): m - (d - hi) + 1]).astype(np.int32)
            diag = prev2[lo - 1: hi] + cost
            up = prev[lo - 1: hi] + 1
            left = prev[lo: hi + 1] + 1
            best = np.minimum(diag, np.minimum(up, left))
            cur[lo: hi + 1] = best
            i = np.arange(lo, hi + 1, dtype=np.int64)
            dirs[(i - 1) * m + (d - i - 1)] = np.where(diag == best, 0, np.where(up == best, 1, 2)).astype(np.uint8)
            prev2, prev = prev, cur
    i, j = n, m
    n_match = n_sub = n_ins = n_del = 0
    while i > 0 or j > 0:
        if j == 0:
            ops[:i] = OP_INS
            n_ins += i
            break
        if i == 0:
            n_del += j
            break
        d = dirs[(i - 1) * m + (j - 1)]
        if d == 0:
            if a[i - 1] != b[j - 1]:
                ops[i - 1] = OP_SUB
                n_sub += 1
            else:
                n_match += 1
            i -= 1
            j -= 1
        elif d == 1:
            ops[i - 1] = OP_INS
            n_ins += 1
            i -= 1
        else:
            n_del += 1
            j -= 1
    return np.asarray([n_sub + n_ins + n_del, n_match, n_sub, n_ins, n_del], np.int32), ops


def pack_align_input(calls, truths):
    """The input of nd_align_seqs, packed as frontend.pack_assembly_input packs its own: (call uint8 [bytes],
    call_off int32 [P + 1], truth uint8 [bytes], truth_off int32 [P + 1], cells), cells the sum of n * m over the
    pairs with both sides within ALIGN_MAX_LEN."""
    if len(calls) != len(truths):
        raise ValueError("one truth per call")
    ca, tb = [_bytes(s) for s in calls], [_bytes(s) for s in truths]
    call_off = np.zeros(len(ca) + 1, np.int64)
    truth_off = np.zeros(len(tb) + 1, np.int64)
    call_off[1:] = np.cumsum([x.size for x in ca], dtype=np.int64)
    truth_off[1:] = np.cumsum([x.size for x in tb], dtype=np.int64)
    if call_off[-1] >= 2 ** 31 or truth_off[-1] >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 bases in one alignment call")
    cells = sum(int(x.size) * int(y.size) for x, y in zip(ca, tb)
                if x.size <= ALIGN_MAX_LEN and y.size <= ALIGN_MAX_LEN)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint8)  # noqa: E731
    return cat(ca), call_off.astype(np.int32), cat(tb), truth_off.astype(np.int32), cells


def _align_device(call, call_off, truth, truth_off, cells, device, want_ops=True):
    """One nd_align_seqs call on the CURRENT stream of ``device``: (counts int32 [P, 5], status int32 [P], ops
    uint8 [bytes] or None) on the host."""
    import ctypes

    import torch

    from . import _lib
    from .frontend import _pinned
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    P = len(call_off) - 1
    L = _lib.lib()
    work_bytes = int(L.nd_align_seqs_work_bytes(P, int(cells)))
    if work_bytes < 0:
        raise ValueError("nd_align_seqs_work_bytes refused P = %d, cells = %d" % (P, cells))
    with torch.cuda.device(dev):
        off_d = _pinned(np.concatenate([call_off, truth_off])).to(dev, non_blocking=True)
        # one byte more than the bases: an empty side still has an address
        call_d = torch.zeros(call.size + 1, dtype=torch.uint8, device=dev)
        truth_d = torch.zeros(truth.size + 1, dtype=torch.uint8, device=dev)
        if call.size:
            call_d[: call.size].copy_(_pinned(call), non_blocking=True)
        if truth.size:
            truth_d[: truth.size].copy_(_pinned(truth), non_blocking=True)
        out_d = torch.empty(P * 6, dtype=torch.int32, device=dev)  # counts [P, 5], status [P]
        ops_d = torch.empty(call.size + 1, dtype=torch.uint8, device=dev) if want_ops else None
        work_d = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        _lib.check(L.nd_align_seqs(p(call_d), p(off_d), p(truth_d), p(off_d[P + 1:]), P, int(cells), p(out_d),
                                   p(ops_d) if want_ops else None, p(out_d[5 * P:]), p(work_d), work_bytes, stream),
                   "nd_align_seqs")
        out = out_d.cpu().numpy()  # synchronises the stream: the device tensors above are done with
        ops = ops_d.cpu().numpy()[: call.size] if want_ops else None
    return out[: 5 * P].reshape(P, 5).copy(), out[5 * P:].copy(), ops


def align_reads(calls, truths, device=None, want_ops=False, stats=None):
    """The rule for a list of pairs: (counts int32 [P, 5], ops) with ops a list of uint8 arrays, one per call
    base, or None without ``want_ops``.  ``device=None`` is align_host pair by pair.  Otherwise the whole list is
    one nd_align_seqs call on the current torch stream of ``device``; a pair the device reports a nonzero status
    for (a side above ALIGN_MAX_LEN bases) is redone by align_host.  ``stats`` (a dict) gets its "reads" entry
    increased by the pairs of this call and "fallback" by those aligned on the host after a device status."""
    calls, truths = list(calls), list(truths)
    if len(calls) != len(truths):
        raise ValueError("one truth per call")
    P = len(calls)
    if device is None:
        res = [align_host(c, t) for c, t in zip(calls, truths)]
        counts = np.asarray([r[0] for r in res], np.int32).reshape(P, 5)
        return counts, ([r[1] for r in res] if want_ops else None)
    counts = np.zeros((P, 5), np.int32)
    ops = [None] * P
    redo = []
    if P:
        call, call_off, truth, truth_off, cells = pack_align_input(calls, truths)
        counts, status, flat = _align_device(call, call_off, truth, truth_off, cells, device, want_ops)
        for r in range(P):
            if status[r] != 0:
                redo.append(r)
            elif want_ops:
                ops[r] = flat[call_off[r]: call_off[r + 1]].copy()
    if stats is not None:
        stats["reads"] = stats.get("reads", 0) + P
        stats["fallback"] = stats.get("fallback", 0) + len(redo)
    for r in redo:
        counts[r], o = align_host(calls[r], truths[r])
        if want_ops:
            ops[r] = o
    return counts, (ops if want_ops else None)


def identity(counts):
    """n_match / (n_match + n_sub + n_ins + n_del) in double, 0.0 when the denominator is 0: a float for one
    pair's five counts, a float64 array for [P, 5]."""
    c = np.asarray(counts, np.int64)
    den = c[..., 1] + c[..., 2] + c[..., 3] + c[..., 4]
    out = np.where(den > 0, c[..., 1].astype(np.float64) / np.maximum(den, 1).astype(np.float64), 0.0)
    return float(out) if out.ndim == 0 else out


def read_truth(path):
    """{read name: sequence} of a FASTA file: records may span lines, the first word of the header is the read
    name, and the sequence is normalised (upper case, M written as C).  Text before the first header is
    ignored; a repeated name keeps its last record."""
    out, name, parts = {}, None, []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                if name is not None:
                    out[name] = normalise("".join(parts))
                words = line[1:].split()
                name, parts = (words[0] if words else ""), []
            elif name is not None and line:
                parts.append(line)
    if name is not None:
        out[name] = normalise("".join(parts))
    return out


def quality_table(quals, ops):
    """(bases int64 [41], errors int64 [41]) of one read: ``quals`` its FASTQ quality characters (Q + 33, Q in
    0..40), ``ops`` its per-base verdicts; bases[Q] counts the called bases written with quality Q, errors[Q]
    those of them with op != 0 (a mismatch or an insertion).  A deletion is a base of the truth that the call
    lacks: it belongs to no called base, carries no quality, and is left out of both columns."""
    q = np.frombuffer(quals.encode("ascii") if isinstance(quals, str) else bytes(quals), np.uint8).astype(np.int64) - 33
    ops = np.asarray(ops).reshape(-1)
    if q.size != ops.size:
        raise ValueError("a read of %d qualities with %d ops" % (q.size, ops.size))
    if q.size and (q.min() < 0 or q.max() >= Q_LEVELS):
        raise ValueError("a quality outside 0..40")
    bases = np.bincount(q, minlength=Q_LEVELS).astype(np.int64)
    errors = np.bincount(q[ops != 0], minlength=Q_LEVELS).astype(np.int64)
    return bases, errors


def empirical_q(errors: int, bases: int) -> float:
    """-10 log10((errors + 1) / (bases + 2)): the observed error rate of a quality level, with one error and one
    correct base added so that a level without errors stays finite."""
    return -10.0 * math.log10((int(errors) + 1) / (int(bases) + 2))


def calibration_lines(bases, errors):
    """The lines of quality_calibration.tsv: ``Q, bases, errors, empirical_Q`` for every Q that has bases."""
    return ["%d\t%d\t%d\t%.2f\n" % (q, bases[q], errors[q], empirical_q(errors[q], bases[q]))
            for q in range(Q_LEVELS) if bases[q] > 0]


def accuracy_line(name, n_called, n_truth, counts):
    """One line of accuracy.tsv: name, called, truth, match, sub, ins, del, identity (%.6f)."""
    c = [int(v) for v in counts]
    return "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f\n" % (name, n_called, n_truth, c[1], c[2], c[3], c[4], identity(c))
