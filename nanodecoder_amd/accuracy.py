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

Against a shared reference (a genome, a control sequence) a read is a fragment from either strand: the second half
of this file maps it (read_reference, locate_host, fit_host, map_reads; nd_locate_segs and nd_align_fit on the
device) and states those rules there.
"""
from __future__ import annotations

import ctypes
import math
import os
from dataclasses import dataclass, field
from typing import NamedTuple

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


class _Device:
    """What every device call below needs of torch: ``dev`` (``device`` an index, a string or a torch.device),
    the current stream and a tensor's address as the C entries take them, and the upload of byte arrays."""

    def __init__(self, device):
        import torch
        self.dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)

    def stream(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    @staticmethod
    def ptr(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def upload(self, *arrays):
        """Per uint8 array a zeroed tensor one byte longer (an empty one still has an address) with the bytes
        copied in from pinned memory on the current stream: all tensors first, then the copies."""
        import torch

        from .frontend import _pinned
        out = [torch.zeros(a.size + 1, dtype=torch.uint8, device=self.dev) for a in arrays]
        for t, a in zip(out, arrays):
            if a.size:
                t[: a.size].copy_(_pinned(a), non_blocking=True)
        return out


def _dp(call, truth, free, w0=0):
    """(counts int32 [5], (t_start, t_end), ops uint8 [n], rpos int32 [n]) of one pair: the recurrence and the
    direction order of the rule above, global (``free`` False) or with free ends on the truth side (the fit rule
    below, ``truth`` a window that starts at ``w0`` of the reference).  numpy over the rows (D[i][j] = j + the
    running minimum of min(diagonal, up)[k] - k), one direction byte per cell, then the traceback.  The two forms
    differ in row 0 (D[0][j] = j, or 0), in where the path starts ((n, m), or (n, j*)) and in what is left when i
    reaches 0 at column j (j deletions, or nothing)."""
    a, b = _bytes(call), _bytes(truth)
    n, m = int(a.size), int(b.size)
    ops = np.zeros(n, np.uint8)
    rpos = np.full(n, int(w0) - 1, np.int32)
    dirs = np.zeros((n, m), np.uint8)  # cell (i, j) at [i - 1, j - 1]: 0 diagonal, 1 up, 2 left
    ramp = np.arange(m + 1, dtype=np.int32)
    prev = np.zeros(m + 1, np.int32) if free else ramp  # D[0][j]
    for i in range(1, n + 1):
        t = np.empty(m + 1, np.int32)
        t[0] = i
        diag = prev[:-1] + (b != a[i - 1])
        up = prev[1:] + 1
        np.minimum(diag, up, out=t[1:])
        cur = np.minimum.accumulate(t - ramp) + ramp
        dirs[i - 1] = np.where(diag == cur[1:], 0, np.where(up == cur[1:], 1, 2))
        prev = cur
    t_end = int(np.argmin(prev)) if free else m  # argmin: the smallest j of the minimum; row 0 of zeros gives 0
    i, j = n, t_end
    n_match = n_sub = n_ins = n_del = 0
    while i > 0:
        if j == 0:
            ops[:i] = OP_INS
            n_ins += i
            break
        d = dirs[i - 1, j - 1]
        if d != 2:
            rpos[i - 1] = w0 + j - 1
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
    if not free:  # row 0 at column j: the rest of the truth is missing from the call
        n_del, j = n_del + j, 0
    return np.asarray([n_sub + n_ins + n_del, n_match, n_sub, n_ins, n_del], np.int32), (j, t_end), ops, rpos


def align_host(call, truth):
    """(counts int32 [5], ops uint8 [n]) of one pair by the rule above.  The host path, the fallback of
    align_reads and the tests' oracle."""
    counts, _, ops, _ = _dp(call, truth, False)
    return counts, ops


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
    import torch

    from . import _lib
    from .frontend import _pinned
    d = _Device(device)
    dev, p = d.dev, d.ptr
    P = len(call_off) - 1
    L = _lib.lib()
    work_bytes = int(L.nd_align_seqs_work_bytes(P, int(cells)))
    if work_bytes < 0:
        raise ValueError("nd_align_seqs_work_bytes refused P = %d, cells = %d" % (P, cells))
    with torch.cuda.device(dev):
        off_d = _pinned(np.concatenate([call_off, truth_off])).to(dev, non_blocking=True)
        call_d, truth_d = d.upload(call, truth)
        out_d = torch.empty(P * 6, dtype=torch.int32, device=dev)  # counts [P, 5], status [P]
        ops_d = torch.empty(call.size + 1, dtype=torch.uint8, device=dev) if want_ops else None
        work_d = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
        _lib.check(L.nd_align_seqs(p(call_d), p(off_d), p(truth_d), p(off_d[P + 1:]), P, int(cells), p(out_d),
                                   p(ops_d), p(out_d[5 * P:]), p(work_d), work_bytes, d.stream()), "nd_align_seqs")
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


def fasta_records(path):
    """(name, sequence) of every record of a FASTA file, in the file's order: records may span lines, the first
    word of the header is the name ("" for a header without one), and the sequence is normalised (upper case, M
    written as C).  Text before the first header is ignored, and so are blank lines."""
    name, parts = None, []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                if name is not None:
                    yield name, normalise("".join(parts))
                words = line[1:].split()
                name, parts = (words[0] if words else ""), []
            elif name is not None and line:
                parts.append(line)
    if name is not None:
        yield name, normalise("".join(parts))


def read_truth(path):
    """{read name: sequence} of a FASTA file (fasta_records); a repeated name keeps its last record."""
    return dict(fasta_records(path))


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


# ---------------------------------------------------------------------------------------------------------------
# Read accuracy against a shared reference (-truth_ref): where a piece of a read lies in a genome or a control
# sequence, on which strand, and its alignment there with free ends on the reference side.  Integer rules, on the
# host (locate_host, fit_host) or for all segments of a list of reads in two device calls (nd_locate_segs,
# csrc/locate.hip; nd_align_fit, csrc/align.hip) with the same integers.
#
# Reference : the FASTA's records, normalised, concatenated with no separator; rec_off[R + 1] their starts.
# k-mer     : MAP_K consecutive valid bases (A, C, G, T = 0..3) inside one record; code = the 30-bit number with the
#             first base in the highest bits.
# index     : (code, pos) of every k-mer of the forward reference, sorted by code, then pos, without the codes that
#             occur more than MAP_OCC_MAX times; two uint32 arrays.
# segments  : a call of n bases is cut into nseg = max(1, ceil(n / MAP_SEG)) segments, segment s = [s n div nseg,
#             (s + 1) n div nseg); each is mapped on its own, a read's counts are the sums over its mapped segments.
# locate    : for strand 0 (the segment q) and strand 1 (its reverse complement, invalid bytes as they are): every
#             k-mer of the query at offset x and every index entry (code, y) with its code votes for bin
#             (y - x + MAP_SEG) >> MAP_BIN_SHIFT; score[b] = votes[b] + votes[b + 1]; the hit is the (strand, b) of
#             the largest score, strand 0 before strand 1, then the lowest b; votes = that score; below
#             MAP_MIN_VOTES, or n < MAP_K (or n > MAP_SEG): unmapped, window (0, 0).
# window    : lo = (b << 9) - MAP_SEG; the record containing clamp(lo + 512 + n div 2, 0, total - 1); w0 =
#             max(record start, lo - MAP_PAD), w1 = min(record end, lo + 1024 + n + MAP_PAD): w1 - w0 <= n + 3072.
# fit       : call a[0..n) against the window b[0..m): D[0][j] = 0, D[i][0] = i, recurrence and direction order of
#             the rule at the top; j* the smallest j with D[n][j] minimal; the path runs from (n, j*) until i == 0,
#             nothing consumed on row 0, and at j == 0 with i > 0 the rest is insertions.  counts = {D[n][j*],
#             n_match, n_sub, n_ins, n_del}, span (t_start, t_end = j*) in window coordinates:
#             n_match + n_sub + n_ins == n, n_match + n_sub + n_del == t_end - t_start.
MAP_K = 15
MAP_OCC_MAX = 8
MAP_SEG = 4096
MAP_BIN_SHIFT = 9
MAP_PAD = 1024
MAP_MIN_VOTES = 8
MAP_REF_MAX = 1 << 23
MAP_STATUS_UNMAPPED = 1   # status bit 0 of nd_locate_segs (kept by nd_align_fit)
OP_UNMAPPED = 255         # map_reads: the op of a base in an unmapped segment

_CODE = np.full(256, 255, np.uint8)
_CODE[[ord(c) for c in "ACGT"]] = [0, 1, 2, 3]
_COMPLEMENT = np.arange(256, dtype=np.uint8)
_COMPLEMENT[[ord(c) for c in "ACGT"]] = [ord(c) for c in "TGCA"]


def reverse_complement(seq) -> np.ndarray:
    """The bytes of ``seq`` reversed, A <-> T and C <-> G; any other byte stays as it is."""
    return _COMPLEMENT[_bytes(seq)[::-1]]


def _kmers(seq):
    """(code uint32 [L], valid bool [L]), L = max(0, size - MAP_K + 1): the k-mer starting at every position."""
    c = _CODE[_bytes(seq)]
    L = max(0, int(c.size) - MAP_K + 1)
    code = np.zeros(L, np.uint32)
    bad = np.zeros(L, np.int32)
    for k in range(MAP_K if L else 0):
        part = c[k: k + L]
        code = (code << np.uint32(2)) | (part & 3).astype(np.uint32)
        bad += part > 3
    return code, bad == 0


def build_index(seq, rec_off, device=None):
    """(code uint32 [L], pos uint32 [L]): the index of the rule above.  The k-mers and the occurrence filter are
    numpy; the sort of the 64-bit key (code << 32 | pos) is numpy's, or torch.sort on ``device``."""
    rec_off = np.asarray(rec_off, np.int64)
    code, valid = _kmers(seq)
    pos = np.arange(code.size, dtype=np.int64)
    # inside one record: the k-mer's first and last base in the same one
    rec = np.searchsorted(rec_off[:-1], pos, side="right")
    valid &= pos + MAP_K <= rec_off[rec]
    key = (code[valid].astype(np.int64) << 32) | pos[valid]
    if device is None:
        key = np.sort(key)
    else:
        import torch
        key = torch.sort(torch.from_numpy(key).to(_Device(device).dev))[0].cpu().numpy()
    code = (key >> 32).astype(np.uint32)
    first = np.flatnonzero(np.r_[True, code[1:] != code[:-1]]) if code.size else np.zeros(0, np.int64)
    runs = np.diff(np.r_[first, code.size])
    keep = np.repeat(runs <= MAP_OCC_MAX, runs)
    return np.ascontiguousarray(code[keep]), (key[keep] & 0xFFFFFFFF).astype(np.uint32)


class Reference:
    """A shared reference: ``names`` of its R records, ``seq`` (uint8, the records concatenated), ``rec_off``
    (int32 [R + 1]) and ``index`` (build_index, built on first use)."""

    def __init__(self, names, seqs):
        parts = [_bytes(s) for s in seqs]
        total = sum(int(x.size) for x in parts)
        if total > MAP_REF_MAX:
            raise ValueError("a reference of %d bases: more than MAP_REF_MAX = %d" % (total, MAP_REF_MAX))
        self.names = list(names)
        self.seq = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        self.rec_off = np.zeros(len(parts) + 1, np.int32)
        self.rec_off[1:] = np.cumsum([x.size for x in parts], dtype=np.int64)
        self._index = None
        self._device = {}

    @property
    def total(self):
        return int(self.rec_off[-1])

    @property
    def index(self):
        if self._index is None:
            self._index = build_index(self.seq, self.rec_off)
        return self._index

    def record_of(self, pos):
        """The record that holds base ``pos`` of the concatenation (0 <= pos < total)."""
        return int(np.searchsorted(self.rec_off[:-1], pos, side="right")) - 1

    def on_device(self, dev):
        """(seq uint8 [total + 1], rec_off int32 [R + 1], idx_code, idx_pos int32 bit patterns [L]) as tensors on
        ``dev``, uploaded once per device.  An index not built yet is built here with the device's sort (the same
        arrays as the host build's)."""
        import torch
        key = str(dev)
        if key not in self._device:
            if self._index is None:
                self._index = build_index(self.seq, self.rec_off, device=dev)
            code, pos = self.index
            seq = np.concatenate([self.seq, np.zeros(1, np.uint8)])
            self._device[key] = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in
                                      (seq, self.rec_off, code.view(np.int32), pos.view(np.int32)))
        return self._device[key]


def read_reference(path):
    """The Reference of a FASTA file: every record in the file's order (a repeated name stays a record of its
    own), as fasta_records gives them.  More than MAP_REF_MAX bases in total is a ValueError."""
    records = list(fasta_records(path))
    return Reference([name for name, _ in records], [seq for _, seq in records])


def segments(n):
    """[(start, end)] of a call of n bases: max(1, ceil(n / MAP_SEG)) segments of nearly equal length."""
    nseg = max(1, -(-int(n) // MAP_SEG))
    return [(s * n // nseg, (s + 1) * n // nseg) for s in range(nseg)]


def locate_host(seg, ref):
    """(mapped, strand, w0, w1, votes) of one segment by the rule above."""
    q = _bytes(seg)
    n, total = int(q.size), ref.total
    icode, ipos = ref.index
    if n < MAP_K or n > MAP_SEG or total < MAP_K or icode.size == 0:
        return False, 0, 0, 0, 0
    nbins = ((total + MAP_SEG) >> MAP_BIN_SHIFT) + 1
    best = (0, 0, 0)  # score, strand, b
    for strand in (0, 1):
        code, valid = _kmers(q if strand == 0 else reverse_complement(q))
        xs = np.flatnonzero(valid)
        lo = np.searchsorted(icode, code[xs], side="left")
        cnt = np.searchsorted(icode, code[xs], side="right") - lo
        x = np.repeat(xs, cnt)
        entry = np.repeat(lo, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        votes = np.bincount((ipos[entry].astype(np.int64) - x + MAP_SEG) >> MAP_BIN_SHIFT, minlength=nbins + 1)
        score = votes[:nbins] + votes[1: nbins + 1]
        b = int(np.argmax(score))  # the lowest b of the largest score
        if int(score[b]) > best[0]:
            best = (int(score[b]), strand, b)
    votes, strand, b = best
    if votes < MAP_MIN_VOTES:
        return False, strand, 0, 0, votes
    lo = (b << MAP_BIN_SHIFT) - MAP_SEG
    r = ref.record_of(min(max(lo + (1 << MAP_BIN_SHIFT) + n // 2, 0), total - 1))
    w0 = max(int(ref.rec_off[r]), lo - MAP_PAD)
    w1 = min(int(ref.rec_off[r + 1]), lo + (2 << MAP_BIN_SHIFT) + n + MAP_PAD)
    return True, strand, w0, w1, votes


def fit_host(call, window):
    """(counts int32 [5], (t_start, t_end), ops uint8 [n]) of a call against a window by the fit rule."""
    return _dp(call, window, True)[:3]


def fit_pos_host(call, window, w0=0):
    """fit_host plus rpos int32 [n], the reference position of every call base for a window that starts at ``w0``
    of the reference: a diagonal step at cell (i + 1, j) gives w0 + j - 1 (the base matched or mismatched to), an
    up step at column j the same (the base to the left of the inserted one; w0 - 1 on the column-0 border).  The
    rule of nd_align_fit_pos."""
    return _dp(call, window, True, w0)


class Segment(NamedTuple):
    """A mapped segment of a call: [seg_start, seg_end) of the call as written, its strand, the reference record
    and the aligned reference interval in the concatenation's coordinates, the locate votes and the fit's counts."""
    seg_start: int
    seg_end: int
    strand: int
    rec: int
    ref_start: int
    ref_end: int
    votes: int
    counts: np.ndarray


def map_host(call, ref, pile=None):
    """(counts int32 [5], segment records, ops uint8 [n]) of one call: its segments located and fitted on the
    host.  Only mapped segments have a record (Segment).  ops is per base of the call as written (a strand-1
    segment's reversed back), OP_UNMAPPED in an unmapped segment.  ``pile`` (a [9, total] uint32 table, Pileup)
    takes every mapped segment by pile_add_host."""
    counts, recs, ops = map_reads([call], ref, want_ops=True, pile=pile)
    return counts[0], recs[0], ops[0]


def _map_segments_host(call, seg_off, ref, pile=None):
    """What _map_device returns, by the host rule: segment k is call[seg_off[k] .. seg_off[k + 1])."""
    P = len(seg_off) - 1
    hit, status = np.zeros((P, 4), np.int32), np.zeros(P, np.int32)
    counts, span = np.zeros((P, 5), np.int32), np.zeros((P, 2), np.int32)
    ops = np.zeros(call.size, np.uint8)
    for k in range(P):
        q = call[seg_off[k]: seg_off[k + 1]]
        mapped, strand, w0, w1, votes = locate_host(q, ref)
        hit[k] = strand, w0, w1, votes
        if not mapped:
            status[k] = MAP_STATUS_UNMAPPED
            continue
        oriented = q if strand == 0 else reverse_complement(q)
        counts[k], (t0, t1), o, rpos = _dp(oriented, ref.seq[w0:w1], True, w0)
        span[k] = w0 + t0, w0 + t1
        ops[seg_off[k]: seg_off[k + 1]] = o
        if pile is not None:
            pile_add_host(pile, oriented, o, rpos)
    return hit, status, counts, span, ops


def _map_device(call, seg_off, ref, device, want_ops, pile=None):
    """nd_locate_segs, then nd_align_fit, on the CURRENT stream of ``device`` with no host round trip in between:
    (hit int32 [P, 4], status int32 [P], counts int32 [P, 5], span int32 [P, 2], oriented ops uint8 [bytes] or
    None) on the host.  With ``pile`` (a Pileup's table on that device) the fit is nd_align_fit_pos and
    nd_pileup_add follows it on the same stream."""
    import torch

    from . import _lib
    from .frontend import _pinned
    d = _Device(device)
    dev, p = d.dev, d.ptr
    P = len(seg_off) - 1
    n = np.diff(seg_off).astype(np.int64)
    cells = int((n * (n + 2 * MAP_PAD + (2 << MAP_BIN_SHIFT))).sum())
    L = _lib.lib()
    work_bytes = int(L.nd_align_fit_work_bytes(P, cells))
    if work_bytes < 0:
        raise ValueError("nd_align_fit_work_bytes refused P = %d, cells = %d" % (P, cells))
    with torch.cuda.device(dev):
        seq_d, rec_d, code_d, pos_d = ref.on_device(dev)
        off_d = _pinned(seg_off).to(dev, non_blocking=True)
        call_d, = d.upload(call)
        or_d = torch.zeros(call.size + 1, dtype=torch.uint8, device=dev)
        out_d = torch.zeros(P * 12, dtype=torch.int32, device=dev)  # hit [P, 4], status [P], counts [P, 5], span [P, 2]
        ops_d = (torch.zeros(call.size + 1, dtype=torch.uint8, device=dev)
                 if want_ops or pile is not None else None)
        work_d = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
        stream = d.stream()
        hit_d, status_d, counts_d, span_d = out_d, out_d[4 * P:], out_d[5 * P:], out_d[10 * P:]
        _lib.check(L.nd_locate_segs(p(call_d), p(off_d), P, p(code_d), p(pos_d), int(code_d.numel()), p(rec_d),
                                    int(rec_d.numel()) - 1, p(hit_d), p(status_d), p(or_d), stream), "nd_locate_segs")
        if pile is None:
            _lib.check(L.nd_align_fit(p(or_d), p(off_d), p(seq_d), ref.total, p(hit_d), P, cells, p(counts_d),
                                      p(span_d), p(ops_d), p(status_d), p(work_d), work_bytes, stream), "nd_align_fit")
        else:
            rpos_d = torch.empty(call.size + 1, dtype=torch.int32, device=dev)
            _lib.check(L.nd_align_fit_pos(p(or_d), p(off_d), p(seq_d), ref.total, p(hit_d), P, cells, p(counts_d),
                                          p(span_d), p(ops_d), p(rpos_d), p(status_d), p(work_d), work_bytes, stream),
                       "nd_align_fit_pos")
            _lib.check(L.nd_pileup_add(p(or_d), p(off_d), p(ops_d), p(rpos_d), p(status_d), P, p(pile), ref.total,
                                       stream), "nd_pileup_add")
        out = out_d.cpu().numpy()  # synchronises the stream: the device tensors above are done with
        ops = ops_d.cpu().numpy()[: call.size] if want_ops else None
    return (out[: 4 * P].reshape(P, 4).copy(), out[4 * P: 5 * P].copy(), out[5 * P: 10 * P].reshape(P, 5).copy(),
            out[10 * P:].reshape(P, 2).copy(), ops)


def map_reads(calls, ref, device=None, want_ops=False, stats=None, pile=None):
    """The rule for a list of calls: (counts int32 [reads, 5], per read its list of segment records, per read its
    ops or None without ``want_ops``), each as map_host gives them.  ``device=None`` is the host rule segment by
    segment.  Otherwise all segments of all reads are one nd_locate_segs call and one nd_align_fit call on the
    current torch stream of ``device``: a read of any length runs there.  ``stats`` (a dict) gets "reads",
    "segments" and "unmapped" (segments) increased.  ``pile``, a Pileup's table (on the host or on ``device``),
    takes every mapped segment."""
    calls = [_bytes(c) for c in calls]
    segs = [segments(c.size) for c in calls]
    base = np.zeros(len(calls) + 1, np.int64)
    base[1:] = np.cumsum([c.size for c in calls], dtype=np.int64)
    seg_off = np.asarray([0] + [base[r] + s1 for r, sg in enumerate(segs) for _, s1 in sg], np.int64)
    flat = np.concatenate(calls) if base[-1] else np.zeros(0, np.uint8)
    if device is None or not calls:
        hit, status, counts, span, ops_or = _map_segments_host(flat, seg_off, ref, pile)
    else:
        if base[-1] >= 2 ** 31:
            raise ValueError("more than 2^31 - 1 bases in one mapping call")
        hit, status, counts, span, ops_or = _map_device(flat, seg_off.astype(np.int32), ref, device, want_ops, pile)
        if (status & ~MAP_STATUS_UNMAPPED).any():
            raise RuntimeError("nd_align_fit status %s" % sorted(set(status.tolist())))
    res, k = [], 0
    for c, sg in zip(calls, segs):
        total, recs, ops = np.zeros(5, np.int32), [], np.full(c.size, OP_UNMAPPED, np.uint8)
        for s0, s1 in sg:
            if status[k] == 0:
                strand, w0 = int(hit[k, 0]), int(hit[k, 1])
                total += counts[k]
                recs.append(Segment(s0, s1, strand, ref.record_of(w0), int(span[k, 0]), int(span[k, 1]),
                                    int(hit[k, 3]), counts[k].copy()))
                if ops_or is not None:
                    o = ops_or[seg_off[k]: seg_off[k + 1]]
                    ops[s0:s1] = o if strand == 0 else o[::-1]
            k += 1
        res.append((total, recs, ops))
    if stats is not None:
        stats["reads"] = stats.get("reads", 0) + len(calls)
        stats["segments"] = stats.get("segments", 0) + k
        stats["unmapped"] = stats.get("unmapped", 0) + k - sum(len(r[1]) for r in res)
    counts = np.asarray([r[0] for r in res], np.int32).reshape(len(calls), 5)
    return counts, [r[1] for r in res], ([r[2] for r in res] if want_ops else None)


def paf_line(name, n_called, rec, ref):
    """One line of mapping.paf for a segment record: the 12 PAF columns (query coordinates on the read as written,
    target coordinates inside the record, matches, block length = match + sub + ins + del, mapq 255) and vt:i: =
    the locate votes."""
    rec = Segment(*rec)
    c = [int(v) for v in rec.counts]
    base = int(ref.rec_off[rec.rec])
    return "%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\tvt:i:%d\n" % (
        name, n_called, rec.seg_start, rec.seg_end, "-" if rec.strand else "+", ref.names[rec.rec],
        int(ref.rec_off[rec.rec + 1]) - base, rec.ref_start - base, rec.ref_end - base, c[1],
        c[1] + c[2] + c[3] + c[4], rec.votes)


# ---------------------------------------------------------------------------------------------------------------
# Consensus accuracy (-consensus under -truth_ref): the mapped reads of the whole run piled up on the reference,
# a consensus base called per position, and what differs from the reference.  Integer rules, on the host
# (fit_pos_host, pile_add_host, consensus_host) or on the device (nd_align_fit_pos, csrc/align.hip; nd_pileup_add,
# nd_pileup_call, csrc/pileup.hip) with the same integers.
#
# positions : rpos[i] of every oriented call base of a fitted pair (fit_pos_host): the reference base a diagonal
#             step matches or mismatches it to; for an inserted base the reference base to its left.
# pile      : [9, total] uint32, planes A, C, G, T, D, iA, iC, iG, iT.  Per mapped segment: a diagonal base (op 0
#             or 1) +1 in the plane of its code at its rpos (a byte other than A, C, G, T adds nothing); +1 in D at
#             every position strictly between the rpos of two consecutive diagonal bases; for an insertion run
#             between two diagonal bases +1 in the i plane of the run's first base at the rpos of the diagonal base
#             before it.  Leading and trailing insertions are not piled; a longer insertion is named by its first
#             base only; a position outside [0, total) is skipped wherever it would add.
# call      : cov = A + C + G + T + D; below min_cov: cons = ins = 255 (uncalled); else cons = the index 0..4 (4 =
#             deleted) of the largest of the five, the lowest on a tie, and ins = the index of the largest of the
#             four i counts (the lowest on a tie) when 2 (iA + iC + iG + iT) > cov, else 255.
# records   : {called, match, sub, del, ins, cov_sum} int64 per reference record: match = cons is the reference
#             base's code, sub = cons < 4 and is not (a reference byte other than A, C, G, T counts here), del =
#             cons == 4, ins = the called insertions, cov_sum = cov over the called positions.
# identity  : match / (match + sub + del + ins), per record and pooled (identity above, with dist unused).
PILE_PLANES = 9
PILE_DEL = 4
PILE_INS = 5
CONS_NONE = 255
_LETTERS = np.frombuffer(b"ACGT", np.uint8)


def pile_add_host(pile, call, ops, rpos):
    """One fitted pair (status 0) added to ``pile`` ([9, total] uint32, in place) by the rule above: ``call`` the
    oriented bytes, ``ops`` and ``rpos`` as fit_pos_host gives them.  The rule of nd_pileup_add."""
    a = _bytes(call)
    ops = np.asarray(ops, np.uint8).reshape(-1)
    rpos = np.asarray(rpos, np.int64).reshape(-1)
    total = pile.shape[1]
    diag = np.flatnonzero(ops <= OP_SUB)
    if diag.size == 0:
        return
    r = rpos[diag]
    inside = (r >= 0) & (r < total)
    code = _CODE[a[diag]]
    ok = inside & (code < 4)
    np.add.at(pile, (code[ok], r[ok]), 1)
    # consecutive diagonal bases k < i with nothing but insertions in between
    k, i = diag[:-1], diag[1:]
    n_ins = np.concatenate([[0], np.cumsum(ops == OP_INS)])
    pair = n_ins[i] - n_ins[k + 1] == i - k - 1
    k, i, rk, ri, rk_inside = k[pair], i[pair], r[:-1][pair], r[1:][pair], inside[:-1][pair]
    lo = np.clip(rk + 1, 0, total)
    hi = np.maximum(np.clip(ri, 0, total), lo)
    step = np.zeros(total + 1, np.int64)
    np.add.at(step, lo, 1)
    np.add.at(step, hi, -1)
    pile[PILE_DEL] += np.cumsum(step[:-1]).astype(np.uint32)
    run = i - k > 1
    first = _CODE[a[np.minimum(k + 1, a.size - 1)]]
    ok = run & rk_inside & (first < 4)
    np.add.at(pile, (PILE_INS + first[ok].astype(np.int64), rk[ok]), 1)


def _record_sums(ref, cons, ins, cov):
    """rec int64 [R, 6] = {called, match, sub, del, ins, cov_sum} of the rule above."""
    called = cons != CONS_NONE
    match = called & (cons == _CODE[ref.seq])
    dele = cons == PILE_DEL
    cols = [called, match, called & ~match & ~dele, dele, ins != CONS_NONE]
    sums = [np.concatenate([[0], np.cumsum(c, dtype=np.int64)]) for c in cols]
    sums.append(np.concatenate([[0], np.cumsum(np.where(called, cov, 0), dtype=np.int64)]))
    off = ref.rec_off.astype(np.int64)
    return np.stack([c[off[1:]] - c[off[:-1]] for c in sums], axis=1).reshape(len(off) - 1, 6)


def consensus_host(pile, ref, min_cov):
    """(cons uint8 [total], ins uint8 [total], cov int32 [total], rec int64 [R, 6]) of a pile by the rule above.
    The rule of nd_pileup_call."""
    if min_cov < 1:
        raise ValueError("min_cov must be at least 1")
    t = np.asarray(pile).astype(np.int64)
    cov = t[:PILE_INS].sum(axis=0)
    called = cov >= min_cov
    cons = np.where(called, np.argmax(t[:PILE_INS], axis=0), CONS_NONE).astype(np.uint8)  # argmax: the lowest index
    has = called & (2 * t[PILE_INS:].sum(axis=0) > cov)
    ins = np.where(has, np.argmax(t[PILE_INS:], axis=0), CONS_NONE).astype(np.uint8)
    return cons, ins, cov.astype(np.int32), _record_sums(ref, cons, ins, cov)  # cov_sum from the 64-bit cov


class Pileup:
    """The pile of a whole run on ``ref``.  ``device=None`` keeps the table on the host and uses the host rule;
    otherwise the table is a tensor on ``device`` for the life of the object and every add is nd_locate_segs,
    nd_align_fit_pos and nd_pileup_add on the current torch stream, with no host round trip beyond map_reads' own."""

    def __init__(self, ref, device=None):
        self.ref, self.device = ref, device
        if device is None:
            self._pile = np.zeros((PILE_PLANES, ref.total), np.uint32)
        else:
            import torch
            self._d = _Device(device)
            self._pile = torch.zeros(PILE_PLANES * ref.total + 1, dtype=torch.int32, device=self._d.dev)

    def add(self, calls, want_ops=False, stats=None):
        """map_reads(calls, ref, device, want_ops, stats), its results, with every mapped segment piled."""
        return map_reads(calls, self.ref, self.device, want_ops, stats, self._pile)

    def counts(self):
        """The table as a [9, total] uint32 numpy array (a copy)."""
        if self.device is None:
            return self._pile.copy()
        return self._pile[:-1].cpu().numpy().view(np.uint32).reshape(PILE_PLANES, self.ref.total)

    def call(self, min_cov):
        """(cons, ins, cov, rec) as consensus_host gives them: on a device by nd_pileup_call."""
        if min_cov < 1:
            raise ValueError("min_cov must be at least 1")
        if self.device is None:
            return consensus_host(self._pile, self.ref, min_cov)
        import torch

        from . import _lib
        total, R = self.ref.total, len(self.ref.names)
        dev, p = self._d.dev, self._d.ptr
        with torch.cuda.device(dev):
            seq_d, rec_off_d = self.ref.on_device(dev)[:2]
            cc_d = torch.full((2 * total + 1,), CONS_NONE, dtype=torch.uint8, device=dev)  # cons, ins
            cov_d = torch.zeros(total + 1, dtype=torch.int32, device=dev)
            rec_d = torch.zeros(R * 6 + 1, dtype=torch.int64, device=dev)
            _lib.check(_lib.lib().nd_pileup_call(p(self._pile), p(seq_d), total, p(rec_off_d), R, int(min_cov),
                                                 p(cc_d), p(cc_d[total:]), p(cov_d), p(rec_d), self._d.stream()),
                       "nd_pileup_call")
            cc, cov, rec = cc_d.cpu().numpy(), cov_d.cpu().numpy(), rec_d.cpu().numpy()
        return cc[:total].copy(), cc[total: 2 * total].copy(), cov[:total].copy(), rec[: R * 6].reshape(R, 6).copy()


def consensus_fasta(ref, cons, ins):
    """The text of consensus.fasta: one record per reference record that has a called position, ``>NAME called=N
    identity=F``; the sequence covers the whole record, N where uncalled, deleted positions left out, a called
    insertion after its position."""
    rec = _record_sums(ref, cons, ins, np.zeros(cons.size, np.int32))
    base = np.zeros(256, np.uint8)
    base[:4], base[CONS_NONE] = _LETTERS, ord("N")
    after = np.zeros(256, np.uint8)
    after[:4] = _LETTERS
    both = np.stack([base[cons], after[ins]], axis=1)
    out = []
    for r, name in enumerate(ref.names):
        if rec[r, 0] == 0:
            continue
        part = both[int(ref.rec_off[r]): int(ref.rec_off[r + 1])].reshape(-1)
        out.append(">%s called=%d identity=%.6f\n%s\n" % (name, rec[r, 0], identity(rec[r, :5]),
                                                         part[part != 0].tobytes().decode("ascii")))
    return "".join(out)


def variant_lines(ref, cons, ins, cov, pile):
    """The lines of variants.tsv, in reference order: ``record, pos (1-based), ref, alt, cov, count`` for every
    called position whose consensus differs from the reference (a substitution ``A G``, a deletion ``A -``) and,
    after the position's own line, for a called insertion after it (``- G``).  count is the winning count of
    ``pile`` (Pileup.counts)."""
    differs = (cons != CONS_NONE) & ((cons != _CODE[ref.seq]) | (ins != CONS_NONE))
    out = []
    for r in np.flatnonzero(differs):
        k = ref.record_of(r)
        name, pos = ref.names[k], int(r) - int(ref.rec_off[k]) + 1
        c = int(cons[r])
        if c != _CODE[ref.seq[r]]:
            out.append("%s\t%d\t%s\t%s\t%d\t%d\n" % (name, pos, chr(ref.seq[r]), "ACGT-"[c], cov[r], pile[c, r]))
        if ins[r] != CONS_NONE:
            out.append("%s\t%d\t-\t%s\t%d\t%d\n" % (name, pos, "ACGT"[int(ins[r])], cov[r],
                                                      pile[PILE_INS + int(ins[r]), r]))
    return out


def coverage_lines(ref, rec):
    """The lines of coverage.tsv: ``record, length, called, mean_cov (cov_sum / called, %.2f), match, sub, del,
    ins, identity (%.6f)`` per reference record, and a last line ``total``."""
    def line(name, length, v):
        v = [int(x) for x in v]
        return "%s\t%d\t%d\t%.2f\t%d\t%d\t%d\t%d\t%.6f\n" % (name, length, v[0], v[5] / v[0] if v[0] else 0.0,
                                                               v[1], v[2], v[3], v[4], identity(v[:5]))
    out = [line(name, int(ref.rec_off[r + 1]) - int(ref.rec_off[r]), rec[r]) for r, name in enumerate(ref.names)]
    out.append(line("total", ref.total, np.asarray(rec, np.int64).reshape(-1, 6).sum(axis=0)))
    return out


def consensus_summary(ref, rec, min_cov, n_variants):
    """The log's line of -consensus: the reference bases called, the mean coverage, the pooled consensus identity
    with its four counts, and the number of variant lines."""
    v = [int(x) for x in np.asarray(rec, np.int64).reshape(-1, 6).sum(axis=0)]
    return ("-consensus: %d of %d reference bases called at coverage >= %d, mean coverage %.2f; consensus identity "
            "%.6f (%d matches, %d substitutions, %d deletions, %d insertions); %d variant lines"
            % (v[0], ref.total, min_cov, v[5] / v[0] if v[0] else 0.0, identity(v[:5]), v[1], v[2], v[3], v[4],
               n_variants))


# ---------------------------------------------------------------------------------------------------------------
# The evaluation of a run (translate.py -truth, -truth_ref, -consensus): what a read's evaluation leaves for its
# writer, and the object that holds the run's truth, device choice, pile and sums.
@dataclass
class ReadEntry:
    """One assembled read's evaluation.  ``line`` is its line of accuracy.tsv, None for a read without a known
    sequence (-truth) or without a mapped segment (-truth_ref); ``quality`` and ``ops`` are there under -fastq;
    ``paf_lines``, ``segments`` and ``mapped`` (of those segments) belong to -truth_ref."""
    line: str | None = None
    counts: np.ndarray | None = None
    quality: str | None = None
    ops: np.ndarray | None = None
    paf_lines: list = field(default_factory=list)
    segments: int = 0
    mapped: int = 0


class Evaluation:
    """-truth or -truth_ref for one run: ``opt`` gives the file, where to align (-truth_align, -gpu) and
    -consensus.  evaluate() aligns or maps a translated group, account() takes a read's entry into the run's sums
    once the read is written, finish() writes the end-of-run files and log lines."""

    def __init__(self, opt):
        self.seqs = read_truth(opt.truth) if opt.truth else None
        self.ref = read_reference(opt.truth_ref) if opt.truth_ref else None
        self.device = None if opt.truth_align == "cpu" else max(0, opt.gpu)
        self.pile = Pileup(self.ref, device=self.device) if opt.consensus else None
        self.min_cov = opt.consensus_min_cov
        self.align_stats = {"reads": 0, "fallback": 0}  # -truth: reads aligned / of them on the host after a status
        # the written reads: those with a line and those without one; under -truth_ref their segments and the
        # unmapped ones; the sums of matches and alignment columns; the called bases and errors per quality
        self.evaluated = self.missing = self.segments = self.unmapped = self.match = self.length = 0
        self.bases, self.errors = np.zeros(Q_LEVELS, np.int64), np.zeros(Q_LEVELS, np.int64)

    def evaluate(self, names, seqs, fastq):
        """Per read of a group None (not evaluated: no assembled sequence, or the evaluation raised) or its
        ReadEntry.  ``seqs`` are the reads as frontend.assemble_reads gives them (None: not assembled), with the
        quality string second under ``fastq``.  -truth: every read with a known sequence is aligned to it, one
        device call for the group or the host rule.  -truth_ref: every read is mapped to the reference, all
        segments of the group in one locate call and one fit call or by the host rule, and piled under
        -consensus as it is mapped."""
        res = [None] * len(names)
        todo = []
        for k, name in enumerate(names):
            if seqs[k] is None:
                continue
            if self.ref is None and name not in self.seqs:
                res[k] = ReadEntry()  # written, without a truth
            else:
                todo.append(k)
        if not todo:
            return res
        called = [normalise(seqs[k] if isinstance(seqs[k], str) else seqs[k][0]) for k in todo]
        try:
            if self.ref is None:
                truths = [self.seqs[names[k]] for k in todo]
                counts, ops = align_reads(called, truths, device=self.device, want_ops=fastq, stats=self.align_stats)
                recs = [None] * len(todo)
            elif self.pile is not None:
                counts, recs, ops = self.pile.add(called, want_ops=fastq)
            else:
                counts, recs, ops = map_reads(called, self.ref, device=self.device, want_ops=fastq)
        except Exception as e:
            for k in todo:
                print("!!!error!!!accuracy: " + names[k] + " (%r)" % (e,))
            return res
        for x, k in enumerate(todo):
            name, n = names[k], len(called[x])
            entry = ReadEntry(counts=counts[x])
            if self.ref is None:
                entry.line = accuracy_line(name, n, len(truths[x]), counts[x])
            else:
                entry.segments, entry.mapped = len(segments(n)), len(recs[x])
                if recs[x]:
                    entry.line = accuracy_line(name, n, sum(r.ref_end - r.ref_start for r in recs[x]), counts[x])
                    entry.paf_lines = [paf_line(name, n, r, self.ref) for r in recs[x]]
            if fastq and entry.line is not None:
                entry.quality, entry.ops = seqs[k][1], ops[x]
            res[k] = entry
        return res

    def account(self, entry):
        """A written read's entry into the run's sums."""
        if entry is None:
            return
        self.segments += entry.segments
        self.unmapped += entry.segments - entry.mapped
        if entry.line is None:
            self.missing += 1
            return
        self.evaluated += 1
        self.match += int(entry.counts[1])
        self.length += int(entry.counts[1:5].sum())
        if entry.quality is not None:
            quality, ops = entry.quality, entry.ops
            if self.ref is not None:  # the bases of the mapped segments only
                keep = ops != OP_UNMAPPED
                quality, ops = np.frombuffer(quality.encode("ascii"), np.uint8)[keep].tobytes(), ops[keep]
            b, e = quality_table(quality, ops)
            self.bases += b
            self.errors += e

    def finish(self, save_data, fastq, logger):
        """The end of the run: quality_calibration.tsv under ``fastq``, the mode's line of the log and, under
        -consensus, the pile called into consensus.fasta, variants.tsv and coverage.tsv with their line."""
        if fastq:
            with open(os.path.join(save_data, "quality_calibration.tsv"), "w") as f:
                f.writelines(calibration_lines(self.bases, self.errors))
        pooled = "pooled identity %.6f (%d matches over %d alignment columns)" % (
            self.match / self.length if self.length else 0.0, self.match, self.length)
        if self.ref is None:
            logger.info("-truth: %d reads evaluated, %d without a truth, %d host fallbacks (a read or a truth above "
                        "%d bases); %s" % (self.evaluated, self.missing, self.align_stats["fallback"], ALIGN_MAX_LEN,
                                           pooled))
        else:
            logger.info("-truth_ref: %d reads evaluated, %d reads unmapped, %d segments mapped, %d unmapped; %s"
                        % (self.evaluated, self.missing, self.segments - self.unmapped, self.unmapped, pooled))
        if self.pile is not None:
            cons, ins, cov, rec = self.pile.call(self.min_cov)
            variants = variant_lines(self.ref, cons, ins, cov, self.pile.counts())
            with open(os.path.join(save_data, "consensus.fasta"), "w") as f:
                f.write(consensus_fasta(self.ref, cons, ins))
            with open(os.path.join(save_data, "variants.tsv"), "w") as f:
                f.writelines(variants)
            with open(os.path.join(save_data, "coverage.tsv"), "w") as f:
                f.writelines(coverage_lines(self.ref, rec))
            logger.info(consensus_summary(self.ref, rec, self.min_cov, len(variants)))
