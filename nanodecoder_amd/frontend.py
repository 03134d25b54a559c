"""Signal front end and output assembly around the translate path.

Host-side restatement of utils/labelop.py: the
median/MAD normalisation + windowing that produces 512-sample chunks
(extract_fast5_raw, :194-243) and the overlap consensus that joins per-chunk
base strings back into a read (simple_assembly / index2base, :295-352).
Chunks stay float32 arrays end to end — the reference's float -> str -> float
round trip (:231, inputters/nano_dataset.py:52-58) is value-preserving, so it
is skipped.
"""
from __future__ import annotations

import collections
import difflib
import math
from typing import List

import numpy as np

from .synth import MAD_SCALE

BASE_KEYS = ["A", "C", "G", "T", "M"]                       # utils/labelop.py:17
BASE_DICT = {"A": 0, "C": 1, "G": 2, "T": 3, "M": 4}        # utils/labelop.py:18


def read_raw(path: str, suffix: str) -> np.ndarray:
    if suffix == "fast5":
        try:
            import h5py  # noqa: F401
        except ImportError as e:  # pragma: no cover - h5py absent in this image
            raise IOError("fast5 input needs h5py, which is not installed; convert reads to .signal text") from e
        import h5py
        with h5py.File(path, "r") as f:
            raw = list(f["/Raw/Reads/"].values())[0]["Signal"][()]
        return np.asarray(raw, dtype=np.float64)
    with open(path) as f:
        return np.asarray(f.read().strip().split(), dtype=np.float64)


def normalize(raw: np.ndarray, normalization: str) -> np.ndarray:
    """utils/labelop.py:220-223 ('mean' divides by std but still centres on
    the median, exactly as the reference does)."""
    raw = np.asarray(raw, dtype=np.float64)
    if normalization == "mean":
        return (raw - np.median(raw)) / float(np.std(raw))
    if normalization == "median":
        med = np.median(raw)
        return (raw - med) / float(np.median(np.abs(raw - med) / MAD_SCALE))
    return raw


def window(sig: np.ndarray, max_length: int, stride: int) -> List[np.ndarray]:
    """utils/labelop.py:225-233."""
    out = []
    for i in range(0, math.ceil(sig.size / stride)):
        s = i * stride
        e = min(s + max_length, len(sig))
        out.append(np.asarray(sig[s:e], dtype=np.float32))
        if e >= len(sig):
            break
    return out


def extract_raw(input_file_path: str, output_prefix: str, normalization: str, max_length: int,
                signal_stride: int, suffix: str):
    """extract_fast5_raw (utils/labelop.py:194-243): [prefix, chunk, ...]."""
    try:
        raw = read_raw(input_file_path, suffix)
        return [output_prefix] + window(normalize(raw, normalization), max_length, signal_stride)
    except Exception as e:
        raise RuntimeError("Raw data is not stored in Raw/Reads/Read_[read#] so new segments cannot be "
                           "identified.") from e


NORM_METHOD = {"none": 0, "None": 0, "median": 1, "mean": 2}


def windows(n: int, max_length: int, stride: int):
    """(start, length) of each chunk window() cuts from an n-sample read
    (utils/labelop.py:225-233)."""
    out = []
    for i in range(0, math.ceil(n / stride)):
        st = i * stride
        e = min(st + max_length, n)
        out.append((st, e - st))
        if e >= n:
            break
    return out


def _pinned(a: np.ndarray):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory()


def device_batch(raws, rd, start, length, normalization: str, B: int, T: int, device):
    """The device front end for one engine batch (nd_normalize_reads +
    nd_window_reads, frontend.hip) on the CURRENT stream: the reads ``raws``
    (float64 arrays) are copied to the device once (pinned, asynchronous),
    normalised in fp64 (median/MAD, median/std or none as
    utils/labelop.py:220-223) and cut into chunk rows c = samples
    [start[c], start[c] + length[c]) of read rd[c] (index into ``raws``), zero
    padded, in a [B, T] float32 batch (rows >= len(rd) zero).  Returns
    (signal [B, T], the device tensors to keep alive until the stream has
    used them)."""
    import ctypes

    import torch

    from . import _lib
    method = NORM_METHOD.get(normalization, 0)  # anything else: the raw read, as labelop.py:220-223
    lens = np.fromiter((r.size for r in raws), np.int64, len(raws))
    if (lens < 1).any():
        raise ValueError("empty read")
    off = np.zeros(len(raws) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    C = len(rd)
    if C > B or (C and int(np.max(length)) > T):
        raise ValueError("chunk descriptors exceed the batch")
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    idx = np.zeros((len(off) * 2 + 3 * C + 1) // 2 * 2, np.int32)  # one pinned block of every index array
    idx.view(np.int64)[: len(off)] = off
    idx[2 * len(off): 2 * len(off) + 3 * C] = np.concatenate([np.asarray(rd, np.int32), np.asarray(start, np.int32),
                                         np.asarray(length, np.int32)])
    raw_d = _pinned(np.concatenate(raws) if len(raws) > 1 else raws[0]).to(dev, non_blocking=True)
    idx_d = _pinned(idx).to(dev, non_blocking=True)
    off_d = idx_d[: 2 * len(off)].view(torch.int64)
    rd_d = idx_d[2 * len(off): 2 * len(off) + C]
    st_d = idx_d[2 * len(off) + C: 2 * len(off) + 2 * C]
    ln_d = idx_d[2 * len(off) + 2 * C: 2 * len(off) + 3 * C]
    norm_d = torch.empty(int(off[-1]), dtype=torch.float32, device=dev)
    sig = torch.zeros(B, T, dtype=torch.float32, device=dev)
    L = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(L.nd_normalize_reads(p(raw_d), p(off_d), len(raws), method, p(norm_d), stream), "nd_normalize_reads")
    _lib.check(L.nd_window_reads(p(norm_d), p(off_d), p(rd_d), p(st_d), p(ln_d), C, T, p(sig), stream),
               "nd_window_reads")
    return sig, (raw_d, idx_d, norm_d)


def normalize_window_gpu(raws, normalization: str, max_length: int, stride: int, device=0, T: int = None):
    """extract_fast5_raw's normalisation and windowing for many reads on the
    GPU (device_batch over every window of every read).  Returns (signal
    [C, T] device tensor, chunk lengths [C] int32, chunk -> read index [C]
    int32)."""
    raws = [np.asarray(r, dtype=np.float64).reshape(-1) for r in raws]
    rd, st, ln = [], [], []
    for r, x in enumerate(raws):
        for a, b in windows(int(x.size), max_length, stride):
            rd.append(r)
            st.append(a)
            ln.append(b)
    sig, _ = device_batch(raws, rd, st, ln, normalization, len(rd), T or max_length, device)
    return sig, np.array(ln, np.int32), np.array(rd, np.int32)


def index2base(read) -> str:
    """utils/labelop.py:295-307."""
    return "".join(BASE_KEYS[x] for x in read)


def _add_count(consensus, start, segment):
    """utils/labelop.py:310-317."""
    if start < 0:
        segment = segment[-start:]
        start = 0
    for i, base in enumerate(segment):
        consensus[BASE_DICT[base.upper()]][start + i] += 1


def simple_assembly(bpreads, flag_intersection: bool = True):
    """utils/labelop.py:320-352.  ``bpreads`` = all_predictions (lists of
    n_best space-separated strings); with flag_intersection the consecutive
    chunks are aligned by their longest difflib matching block and voted."""
    valid = [x[0].replace(" ", "") for x in bpreads if x[0] != ""]
    if not flag_intersection:
        return "".join(valid)
    consensus = np.zeros([len(BASE_KEYS), 1000])
    pos = 0
    length = 0
    census_len = 1000
    for indx, bpread in enumerate(valid):
        if indx == 0:
            _add_count(consensus, 0, bpread)
            continue
        d = difflib.SequenceMatcher(None, valid[indx - 1], bpread)
        match_block = max(d.get_matching_blocks(), key=lambda x: x[2])
        disp = match_block[0] - match_block[1]
        if disp + pos + len(valid[indx]) > census_len:
            consensus = np.pad(consensus, ((0, 0), (0, 1000)), mode="constant", constant_values=0)
            census_len += 1000
        _add_count(consensus, pos + disp, valid[indx])
        pos += disp
        length = max(length, pos + len(valid[indx]))
    return consensus[:, :length]


def assemble_read(all_predictions, src_seq_length: int, src_seq_stride: int) -> str:
    """translate.py:84-87."""
    if src_seq_stride < src_seq_length:
        return index2base(np.argmax(simple_assembly(all_predictions), axis=0))
    return simple_assembly(all_predictions, flag_intersection=False)


# ---------------------------------------------------------------- per-base qualities (FASTQ)
# The reference writes no qualities.  A token's weight is its model probability in 16 bits,
# w = min(65535, floor(65535 * exp((double)lp) + 0.5)) (nd_token_weights; 0 for a non-finite lp or the beam's -1
# padding); every char of a token's word carries the token's weight.  A column of a read's vote with n votes, of
# which those for the winning class weigh S together, gets the largest Q in 0..40 with
# float(65535 n - S) * PHRED_RATIO[Q] <= float(65535 n), and Q = 0 when n = 0: one fp64 product and one compare
# per level, on exact integers, so the device (assembly.hip, nd_assemble_reads_q) gives the same bytes.
PHRED_RATIO = (  # the doubles 10.0 ** (k / 10.0), k = 0..40, printed with 17 significant digits
    1.0, 1.2589254117941673, 1.5848931924611136, 1.9952623149688795, 2.5118864315095801, 3.1622776601683795,
    3.9810717055349722, 5.011872336272722, 6.3095734448019334, 7.9432823472428158, 10.0, 12.589254117941675,
    15.848931924611133, 19.952623149688797, 25.118864315095795, 31.622776601683793, 39.810717055349734,
    50.118723362727224, 63.095734448019329, 79.43282347242814, 100.0, 125.89254117941675, 158.48931924611142,
    199.52623149688787, 251.18864315095797, 316.22776601683796, 398.10717055349733, 501.18723362727246,
    630.957344480193, 794.32823472428129, 1000.0, 1258.9254117941675, 1584.893192461114, 1995.2623149688789,
    2511.8864315095798, 3162.2776601683795, 3981.0717055349733, 5011.8723362727251, 6309.5734448019302,
    7943.2823472428136, 10000.0)
WEIGHT_ONE = 65535  # the weight of probability 1


def token_weight(lp) -> int:
    """The uint16 weight of a token of log-probability ``lp`` (float32)."""
    lp = float(np.float32(lp))
    if not math.isfinite(lp):
        return 0
    try:
        return int(min(float(WEIGHT_ONE), math.floor(WEIGHT_ONE * math.exp(lp) + 0.5)))
    except OverflowError:
        return WEIGHT_ONE


def column_quality(n, S):
    """Q of columns with ``n`` votes whose winning class weighs ``S`` (ints or integer arrays): int or uint8
    array."""
    n64, s64 = np.asarray(n, np.int64), np.asarray(S, np.int64)
    full = WEIGHT_ONE * n64
    e, f = (full - s64).astype(np.float64), full.astype(np.float64)
    ok = e[..., None] * np.asarray(PHRED_RATIO, np.float64) <= f[..., None]  # true up to Q: the ratios increase
    q = np.where(n64 > 0, ok.sum(-1) - 1, 0).astype(np.uint8)
    return int(q) if q.ndim == 0 else q


def quality_string(q) -> str:
    """FASTQ text of the qualities ``q``: chr(33 + Q) per base."""
    return (np.asarray(q, np.uint8) + np.uint8(33)).tobytes().decode("ascii")


# ---------------------------------------------------------------- per-base methylation probabilities (MM / ML)
# CpG models have a ninth token M, a methylated C.  A C or M token's modification weight is the model's
# P(methylated | the base is a C) at its step in 16 bits: with d = (double)lp[C] - (double)lp[M],
# mw = min(65535, floor(65535 / (1 + exp(d)) + 0.5)), every operation rounded once (nd_token_mod_weights); 0 for
# every other token; a NaN d gives the hard call.  Every char of a token's word carries the token's mw.  A column
# of a read's vote called C or M is a site: with n_cm its C plus M votes and W the sum of their mw,
# ML = min(255, (256 W) // (65535 n_cm)), SAM's ML scale; every other column gets 0.  Integers throughout, so the
# device (assembly.hip, nd_assemble_reads_m) gives the same bytes.  The call itself is never changed.
def token_mod_weight(lp_c, lp_m, is_mod) -> int:
    """The uint16 modification weight of a C (``is_mod`` false) or M (true) token whose step gave the
    log-probabilities ``lp_c`` and ``lp_m`` (float32) to the tokens C and M."""
    d = float(np.float32(lp_c)) - float(np.float32(lp_m))
    if math.isnan(d):
        return WEIGHT_ONE if is_mod else 0
    try:
        e = math.exp(d)
    except OverflowError:
        e = math.inf
    p = 1.0 / (1.0 + e)
    return int(min(float(WEIGHT_ONE), math.floor(WEIGHT_ONE * p + 0.5)))


def column_ml(n_cm, W):
    """ML of sites with ``n_cm`` votes of class C or M whose modification weights sum to ``W`` (ints or integer
    arrays): int or uint8 array; 0 where n_cm is 0."""
    n64, w64 = np.asarray(n_cm, np.int64), np.asarray(W, np.int64)
    ml = np.where(n64 > 0, np.minimum(255, (256 * w64) // np.maximum(WEIGHT_ONE * n64, 1)), 0).astype(np.uint8)
    return int(ml) if ml.ndim == 0 else ml


def mod_fastq_record(name: str, sequence: str, quality: str, ml) -> str:
    """The four lines of result/<read>.mod.fastq: the read with every M written as C (the canonical sequence the
    SAM tags refer to), its qualities, and in the header, when the read has a site, the tags MM:Z:C+m. (every C
    of the canonical sequence is listed: all skip counts 0, the '.' mode) and ML:B:C (the sites' ML in sequence
    order)."""
    ml = np.asarray(ml, np.uint8).reshape(-1)
    if ml.size != len(sequence) or len(quality) != len(sequence):
        raise ValueError("a read of %d bases with %d qualities and %d ML values" % (len(sequence), len(quality),
                                                                                   ml.size))
    sites = [int(v) for b, v in zip(sequence, ml) if _is_cm(b)]
    head = "@" + name
    if sites:
        head += "\tMM:Z:C+m." + ",0" * len(sites) + ";\tML:B:C" + "".join(",%d" % v for v in sites)
    return "%s\n%s\n+\n%s\n" % (head, sequence.replace("M", "C").replace("m", "c"), quality)


# ---------------------------------------------------------------- per-base signal positions (-moves)
# Where in the signal each base was called, from the last decoder layer's head-0 context attention (DESIGN.md
# §1.6).  A token's position is the centroid of its attention row in 24-bit fixed point, rounded half up, made
# monotone over the chunk's steps (nd_token_positions); every char of a token's word carries it; a char of chunk
# ci of a read sits at ci * src_seq_stride + m.  A column of the vote gets the mean (integer division) of its
# votes' positions, and the read the running maximum of its columns.  Integers throughout, so the device
# (assembly.hip, nd_assemble_reads_p) gives the same values.  The call itself is never changed.
POS_ONE = 1 << 24  # the fixed-point weight of probability 1


def token_positions(attn_rows, span) -> np.ndarray:
    """The positions m [..., S] (int32) of the attention rows ``attn_rows`` [..., S, T] (float32 probabilities,
    as a translate call returns them with return_attn) of chunks with ``span`` (an int, or an array over the
    leading axes): per row, with q_t = 0 unless a[t] > 0, 2^24 when a[t] >= 1, else
    floor(float64(a[t]) * 2^24 + 0.5) over t < min(span, T), Q = sum q_t and M = sum q_t t, the centroid
    c = (2 M + Q) // (2 Q) (0 when Q is 0); then the running maximum of c over the steps."""
    a = np.asarray(attn_rows, np.float32)
    if a.ndim < 2:
        raise ValueError("attention rows must be [..., S, T]")
    T = a.shape[-1]
    t = np.arange(T, dtype=np.uint64)
    n = np.minimum(np.maximum(np.asarray(span, np.int64), 0), T)
    inside = np.arange(T) < n[..., None, None]
    with np.errstate(invalid="ignore"):
        live = inside & (a > 0)  # False for NaN, negatives and -0
        one = live & (a >= 1)
    v = np.where(live & ~one, a, np.float32(0)).astype(np.float64)
    q = np.where(one, np.uint64(POS_ONE), np.floor(v * 16777216.0 + 0.5).astype(np.uint64))
    Q = q.sum(-1, dtype=np.uint64)
    M = (q * t).sum(-1, dtype=np.uint64)
    c = np.where(Q > 0, (np.uint64(2) * M + Q) // np.maximum(np.uint64(2) * Q, np.uint64(1)), np.uint64(0))
    return np.maximum.accumulate(c.astype(np.int64), axis=-1).astype(np.int32)


def candidate_posterior(scores, cand_len):
    """The posterior over each chunk's candidate targets (Engine.score_candidates; nd_cand_posterior is the same
    rule in fp32): ``scores`` [..., K] the candidates' summed log-probabilities, ``cand_len`` [..., K] their
    lengths, <= 0 for an empty slot.  Returns (post [..., K] float64, best [...] int64): post = score -
    logsumexp over the non-empty slots, taken about their maximum, -inf in an empty slot; best = the non-empty
    slot of the largest score, the lowest on a tie, -1 when every slot is empty.  A NaN score is never best and
    makes its chunk's post values NaN."""
    s = np.asarray(scores, np.float64)
    live = np.asarray(cand_len) > 0
    if s.ndim < 1 or live.shape != s.shape:
        raise ValueError("scores and cand_len must both be [..., K]")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ranked = np.where(live & ~np.isnan(s), s, -np.inf)
        m = ranked.max(-1, keepdims=True)
        hit = live & (s == m)  # never a NaN
        best = np.where(hit.any(-1), hit.argmax(-1), -1).astype(np.int64)
        lse = np.log(np.where(live, np.exp(s - m), 0.0).sum(-1, keepdims=True))
        post = np.where(live, (s - m) - lse, -np.inf)
    return post, best


def column_position(n, P):
    """The position of columns with ``n`` votes whose absolute positions sum to ``P`` (ints or integer arrays):
    P // n, and 0 where n is 0; int or int64 array."""
    n64, p64 = np.asarray(n, np.int64), np.asarray(P, np.int64)
    col = np.where(n64 > 0, p64 // np.maximum(n64, 1), 0).astype(np.int64)
    return int(col) if col.ndim == 0 else col


def moves_record(name: str, sequence: str, rpos) -> str:
    """The three lines of result/<read>.moves: the header, the sequence (the .fasta's) and the read positions
    as comma-separated decimals, one per base (an empty line for an empty read)."""
    rpos = np.asarray(rpos).reshape(-1)
    if rpos.size != len(sequence):
        raise ValueError("a read of %d bases with %d positions" % (len(sequence), rpos.size))
    return ">%s\n%s\n%s\n" % (name, sequence, ",".join("%d" % int(v) for v in rpos))


# ---------------------------------------------------------------- the annotated vote (-fastq, -mod_probs, -moves)
# One restatement of simple_assembly carries every per-base value through the vote: beside a column's counts,
# the int64 sums of its votes' weights per class (wsum), of its C and M votes' modification weights (msum) and
# of its votes' absolute positions (psum), each only when asked for.  column_quality, column_ml and
# column_position turn a column's counts and sums into its values.
Annotated = collections.namedtuple("Annotated", "sequence quality ml rpos")


def _is_cm(base: str) -> bool:
    return base.upper() in ("C", "M")


def _valid_arrays(bpreads, arrays, what: str, stride: int = 0):
    """The per-char values of simple_assembly's ``valid`` chunks, one int64 array per chunk; chunk ci of
    ``bpreads`` (empty ones counted) adds ci * stride to its ``arrays[ci]``.  None for no ``arrays``."""
    if arrays is None:
        return None
    if len(arrays) != len(bpreads):
        raise ValueError("one %s array per chunk" % what)
    return [np.asarray(a, np.int64).reshape(-1) + ci * stride
            for ci, (x, a) in enumerate(zip(bpreads, arrays)) if x[0] != ""]


def simple_assembly_annotated(bpreads, weights=None, mod_weights=None, positions=None, src_seq_stride=0):
    """simple_assembly with flag_intersection, line for line, with the sums of the votes' values beside the
    counts: (consensus, wsum, msum, psum), None for what was not given.  ``weights``: wsum [5, length], each
    vote's weight added at its class and column (where _add_count counts it).  ``mod_weights``: msum [length], the
    modification weights of the C and M votes.  ``positions`` with ``src_seq_stride``: psum [length], the votes'
    absolute positions, chunk ci's at ci * src_seq_stride, ci counting the empty chunks.  All sums int64.  A
    chunk whose array has another length than the chunk raises ValueError before any of its votes is counted."""
    valid = [x[0].replace(" ", "") for x in bpreads if x[0] != ""]
    vw = _valid_arrays(bpreads, weights, "weight")
    vm = _valid_arrays(bpreads, mod_weights, "weight")
    vp = _valid_arrays(bpreads, positions, "position", int(src_seq_stride))
    consensus = np.zeros([len(BASE_KEYS), 1000])
    wsum = None if vw is None else np.zeros([len(BASE_KEYS), 1000], np.int64)
    msum = None if vm is None else np.zeros(1000, np.int64)
    psum = None if vp is None else np.zeros(1000, np.int64)
    pos = 0
    length = 0
    census_len = 1000
    for indx, bpread in enumerate(valid):
        if indx > 0:
            d = difflib.SequenceMatcher(None, valid[indx - 1], bpread)
            match_block = max(d.get_matching_blocks(), key=lambda x: x[2])
            disp = match_block[0] - match_block[1]
            if disp + pos + len(bpread) > census_len:
                consensus, wsum, msum, psum = (
                    a if a is None else np.pad(a, [(0, 0)] * (a.ndim - 1) + [(0, 1000)], mode="constant",
                                               constant_values=0) for a in (consensus, wsum, msum, psum))
                census_len += 1000
            pos += disp
            length = max(length, pos + len(bpread))
        for v, what in ((vm, "modification weights"), (vw, "weights"), (vp, "positions")):
            if v is not None and len(v[indx]) != len(bpread):
                raise ValueError("a chunk of %d bases with %d %s" % (len(bpread), len(v[indx]), what))
        _add_count(consensus, pos, bpread)
        # the same votes' values: the chars left of column 0 are dropped, the others land on distinct columns
        lo = max(-pos, 0)
        cols = np.arange(pos + lo, pos + len(bpread))
        if wsum is not None or msum is not None:
            k = np.array([BASE_DICT[base.upper()] for base in bpread[lo:]], np.int64)
        if wsum is not None:
            wsum[k, cols] += vw[indx][lo:]
        if msum is not None:
            msum[cols] += np.where((k == BASE_DICT["C"]) | (k == BASE_DICT["M"]), vm[indx][lo:], 0)
        if psum is not None:
            psum[cols] += vp[indx][lo:]
    return tuple(a if a is None else a[..., :length] for a in (consensus, wsum, msum, psum))


def assemble_read_annotated(all_predictions, src_seq_length: int, src_seq_stride: int, weights=None,
                            mod_weights=None, positions=None) -> Annotated:
    """assemble_read with a read's per-base values: Annotated(sequence, quality, ml, rpos), None for what was
    not asked for.  The three arguments are laid out alike: per chunk, one value for every char of its x[0] with
    the spaces removed.  ``weights`` (uint16 token weights): ``quality``, the FASTQ string of the columns' Q.
    ``mod_weights`` (uint16 modification weights, only beside ``weights``): ``ml`` uint8 [len(sequence)], 0
    wherever the sequence is neither C nor M.  ``positions`` (chunk-relative signal positions,
    Translator.translate_reads(..., moves=True); chunk ci's offset ci * src_seq_stride is added here, ci counting
    the empty chunks too): ``rpos`` uint32 [len(sequence)], the running maximum of the columns' positions.  The
    sequence is assemble_read's, and what assemble_read raises is raised here."""
    if mod_weights is not None and weights is None:
        raise ValueError("mod_weights need weights")
    if weights is None and positions is None:
        return Annotated(assemble_read(all_predictions, src_seq_length, src_seq_stride), None, None, None)
    if src_seq_stride < src_seq_length:
        consensus, S, W, P = simple_assembly_annotated(all_predictions, weights, mod_weights, positions,
                                                       src_seq_stride)
        win = np.argmax(consensus, axis=0)
        seq = index2base(win)
        n = consensus.sum(axis=0).astype(np.int64)
        n_cm = (consensus[BASE_DICT["C"]] + consensus[BASE_DICT["M"]]).astype(np.int64)
        if S is not None:
            S = S[win, np.arange(win.size)]  # the winning class's weights
    else:
        # the concatenation branch: every base is its own column, with one vote and its own value as each sum
        seq = simple_assembly(all_predictions, flag_intersection=False)
        n = n_cm = np.ones(len(seq), np.int64)

        def own(arrays, what, many, stride=0):
            v = _valid_arrays(all_predictions, arrays, what, stride)
            if v is not None:
                v = np.concatenate(v) if v else np.zeros(0, np.int64)
                if v.size != len(seq):
                    raise ValueError("a read of %d bases with %d %s" % (len(seq), v.size, many))
            return v
        S = own(weights, "weight", "weights")
        W = own(mod_weights, "weight", "modification weights")
        P = own(positions, "position", "positions", int(src_seq_stride))
    quality = ml = rpos = None
    if S is not None:
        quality = quality_string(column_quality(n, S))
    if W is not None:
        site = np.fromiter((_is_cm(b) for b in seq), bool, len(seq))
        ml = np.where(site, column_ml(n_cm, W), 0).astype(np.uint8)
    if P is not None:
        rpos = np.maximum.accumulate(column_position(n, P)).astype(np.uint32)
    return Annotated(seq, quality, ml, rpos)


def assemble_read_q(all_predictions, weights, src_seq_length: int, src_seq_stride: int):
    """assemble_read with per-base qualities: (sequence, quality string); see assemble_read_annotated."""
    a = assemble_read_annotated(all_predictions, src_seq_length, src_seq_stride, weights=weights)
    return a.sequence, a.quality


def assemble_read_m(all_predictions, weights, mod_weights, src_seq_length: int, src_seq_stride: int):
    """assemble_read_q with per-base methylation values: (sequence, quality string, ml uint8 [len(sequence)])."""
    a = assemble_read_annotated(all_predictions, src_seq_length, src_seq_stride, weights=weights,
                                mod_weights=mod_weights)
    return a.sequence, a.quality, a.ml


def assemble_read_p(all_predictions, positions, src_seq_length: int, src_seq_stride: int):
    """assemble_read with per-base signal positions: (sequence, read positions uint32 [len(sequence)])."""
    a = assemble_read_annotated(all_predictions, src_seq_length, src_seq_stride, positions=positions)
    return a.sequence, a.rpos


# ---------------------------------------------------------------- assembly on the device (-assembly gpu)
ASM_STATUS_LONG = 1   # include/nanodec.h nd_assemble_reads: a chunk of 200 or more chars (difflib autojunk)
ASM_STATUS_CHAR = 2   # a char whose upper case is not in BASE_KEYS
AssemblyInput = collections.namedtuple("AssemblyInput", "bases chunk_off read_off host qw mw bp")
AssemblyOutput = collections.namedtuple("AssemblyOutput", "seq seq_len status qual ml rpos")


def pack_assembly_input(reads, weights=None, mod_weights=None, positions=None, src_seq_stride=None):
    """The input of nd_assemble_reads for a group of reads (each the
    all_predictions assemble_read takes): every chunk's x[0] with the spaces
    removed, as ASCII bytes, concatenated.  Returns AssemblyInput(bases uint8 [total],
    chunk_off int32 [C + 1], read_off int32 [R + 1], host, qw, mw, bp): read r owns chunks
    read_off[r] .. read_off[r+1], one per prediction, empty ones included.
    ``host`` lists the reads kept back for assemble_read: text that is not
    ASCII, and a hypothesis of nothing but spaces (simple_assembly drops ""
    before it removes the spaces, so that one stays in its chunk list as an
    empty string).  Such a read is packed with no chunks.
    The last three are None unless asked for.  ``weights`` (per read, per chunk, the uint16 weight of every char
    of that string): qw uint16 [total], the weight of each byte of ``bases`` (nd_assemble_reads_q).
    ``mod_weights`` (laid out like ``weights``, which it needs): mw uint16 [total], each byte's modification
    weight (nd_assemble_reads_m).  ``positions`` (per read, per chunk, the chunk-relative position of every char)
    with ``src_seq_stride``: bp uint32 [total], each byte's absolute position, chunk ci of its read at
    ci * src_seq_stride (nd_assemble_reads_p)."""
    if positions is not None and (src_seq_stride is None or len(positions) != len(reads)):
        raise ValueError("one list of positions per read, with src_seq_stride")
    if weights is not None and len(weights) != len(reads):
        raise ValueError("one list of weights per read")
    if mod_weights is not None and (weights is None or len(mod_weights) != len(reads)):
        raise ValueError("one list of modification weights per read, beside the weights")
    # what was given: its name in the messages (one, many), the per-read lists, the dtype, and the chunks' arrays
    kinds = [k + ([],) for k in (("weight", "weights", weights, np.uint16),
                                 ("modification weight", "modification weights", mod_weights, np.uint16),
                                 ("position", "positions", positions, None)) if k[2] is not None]
    lens, parts, host, pci = [], [], [], []
    read_off = np.zeros(len(reads) + 1, np.int64)
    for r, preds in enumerate(reads):
        strs = [x[0].replace(" ", "") for x in preds]
        try:
            if any(s == "" and x[0] != "" for s, x in zip(strs, preds)):
                raise ValueError("a hypothesis of spaces")
            raw = "".join(strs).encode("ascii")
        except ValueError:  # UnicodeEncodeError is one
            host.append(r)
            read_off[r + 1] = read_off[r]
            continue
        for one, many, given, dtype, packed in kinds:
            if len(given[r]) != len(strs):
                raise ValueError("one %s array per chunk" % one)
            for st, w in zip(strs, given[r]):
                w = np.asarray(w, dtype).reshape(-1)
                if w.size != len(st):
                    raise ValueError("a chunk of %d bases with %d %s" % (len(st), w.size, many))
                packed.append(w)
        parts.append(raw)
        lens.extend(len(s) for s in strs)
        if positions is not None:
            pci.extend(range(len(strs)))
        read_off[r + 1] = read_off[r] + len(strs)
    chunk_off = np.zeros(len(lens) + 1, np.int64)
    chunk_off[1:] = np.cumsum(np.asarray(lens, np.int64))
    if chunk_off[-1] >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 bases in one assembly group")
    bases = np.frombuffer(bytearray(b"").join(parts), np.uint8)  # a bytearray: writable, as torch.from_numpy wants
    flat = {many: np.concatenate(packed) if packed else np.zeros(0, dtype) for one, many, given, dtype, packed in kinds}
    bp = flat.get("positions")
    if bp is not None:
        # the chunks' offsets in one pass: ci * stride repeated over each chunk's chars
        off = np.repeat(np.asarray(pci, np.int64) * int(src_seq_stride), lens)
        bp = (bp.astype(np.int64) + off).astype(np.uint32)
    return AssemblyInput(bases, chunk_off.astype(np.int32), read_off.astype(np.int32), host, flat.get("weights"),
                         flat.get("modification weights"), bp)


# which optional inputs (qw, mw, bp) a call carries -> its entry point; <entry>_work_bytes sizes its work buffer.
# Every entry takes bases, the optional inputs it has, chunk_off, read_off, R, C, total, seq, one output per optional
# input (qual, ml, rpos), seq_len, status, work, work_bytes, stream.
_ASSEMBLE_ENTRY = {(False, False, False): "nd_assemble_reads", (True, False, False): "nd_assemble_reads_q",
                   (True, True, False): "nd_assemble_reads_m", (False, False, True): "nd_assemble_reads_p"}


def _assemble_device(bases, chunk_off, read_off, device, qw=None, mw=None, bp=None):
    """One nd_assemble_reads call on the CURRENT stream of ``device``: AssemblyOutput(seq uint8 [total],
    seq_len int32 [R], status int32 [R], qual, ml, rpos) on the host, the last three None unless computed.  With
    ``qw`` (uint16 [total], each base's weight) the call is nd_assemble_reads_q and qual is uint8 [total]; with
    ``mw`` too (uint16 [total], each base's modification weight) it is nd_assemble_reads_m and ml is uint8
    [total].  With ``bp`` instead (uint32 [total], each base's absolute position) it is nd_assemble_reads_p and
    rpos is uint32 [total]."""
    import ctypes

    import torch

    from . import _lib
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    R, C, total = len(read_off) - 1, len(chunk_off) - 1, int(bases.size)
    L = _lib.lib()
    if mw is not None and qw is None:
        raise ValueError("mw needs qw")
    if bp is not None and qw is not None:
        raise ValueError("bp goes with the plain call only")
    for name, a, dtype in (("qw", qw, np.uint16), ("mw", mw, np.uint16), ("bp", bp, np.uint32)):
        if a is not None and (a.dtype != dtype or a.size != total):
            raise ValueError("%s must hold one %s per base" % (name, np.dtype(dtype).name))
    entry = _ASSEMBLE_ENTRY[(qw is not None, mw is not None, bp is not None)]
    work_bytes = int(getattr(L, entry + "_work_bytes")(C, total))
    with torch.cuda.device(dev):
        off_d = _pinned(np.concatenate([chunk_off, read_off])).to(dev, non_blocking=True)
        bases_d = _pinned(bases).to(dev, non_blocking=True)
        seq_d = torch.empty(total, dtype=torch.uint8, device=dev)
        out_d = torch.empty(2, R, dtype=torch.int32, device=dev)  # seq_len, status
        work_d = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
        # the optional inputs go over as their bits (torch copies no unsigned 16- or 32-bit type)
        in_d = [_pinned(a.view("i%d" % a.itemsize)).to(dev, non_blocking=True) for a in (qw, mw, bp) if a is not None]
        opt_d = [None if a is None else torch.empty(total, dtype=t, device=dev)
                 for a, t in ((qw, torch.uint8), (mw, torch.uint8), (bp, torch.int32))]  # qual, ml, rpos
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        _lib.check(getattr(L, entry)(p(bases_d), *map(p, in_d), p(off_d), p(off_d[C + 1:]), R, C, total, p(seq_d),
                                     *(p(t) for t in opt_d if t is not None), p(out_d[0]), p(out_d[1]), p(work_d),
                                     work_bytes, stream), entry)
        out = out_d.cpu().numpy()  # synchronises the stream: the device tensors above are done with
        seq = seq_d.cpu().numpy()
        qual, ml, rpos = (None if t is None else t.cpu().numpy() for t in opt_d)
    return AssemblyOutput(seq, out[0], out[1], qual, ml, None if rpos is None else rpos.view(np.uint32))


def assemble_reads(reads, src_seq_length: int, src_seq_stride: int, device=None, stats=None,
                   defer_errors: bool = False, weights=None, mod_weights=None, positions=None):
    """assemble_read for a group of reads: one string per read.

    ``device=None``, or ``src_seq_stride >= src_seq_length`` (translate.py's
    concatenation branch: nothing to align), is exactly
    ``[assemble_read(p, ...) for p in reads]``.  Otherwise the whole group is
    assembled by one nd_assemble_reads call (assembly.hip) on the current
    torch stream of ``device``, and every read the device does not assemble
    (a chunk of 200 or more chars, a char outside BASE_KEYS, text
    pack_assembly_input kept back) goes through assemble_read on the host,
    which raises for it whatever it raises.  That fallback is per read and
    counted: ``stats`` (a dict) gets its "reads" and "fallback" entries
    increased by the reads of this call and by those assembled on the host.
    ``defer_errors``: a read whose host assembly raises yields None instead
    (the caller assembles it again where it handles that read's errors).
    With ``weights``, ``mod_weights`` (beside ``weights``) or ``positions`` (each per read what
    assemble_read_annotated takes) the host path and the fallback are assemble_read_annotated and every read
    yields a tuple: (sequence, quality string) with ``weights``, the device call being nd_assemble_reads_q;
    (sequence, quality string, ml uint8 array) with ``mod_weights``, by nd_assemble_reads_m; and with
    ``positions`` the read positions (uint32 array) come last, by nd_assemble_reads_p: that call alone, or beside
    ``weights`` a second call on the same packed group (the forms are not multiplied)."""
    reads = list(reads)
    if mod_weights is not None and weights is None:
        raise ValueError("mod_weights need weights")
    given = []
    for many, arrays in (("weights", weights), ("modification weights", mod_weights), ("positions", positions)):
        given.append(None if arrays is None else list(arrays))
        if arrays is not None and len(given[-1]) != len(reads):
            raise ValueError("one list of %s per read" % many)
    weights, mod_weights, positions = given

    plain = weights is None and positions is None

    def shape(a):  # a read as the caller gets it: the string, or a tuple with what was asked for
        return a[0] if plain else tuple(v for v in a if v is not None)

    def one(r):
        return shape(assemble_read_annotated(reads[r], src_seq_length, src_seq_stride,
                                             *(None if v is None else v[r] for v in given)))
    R = len(reads)
    if device is None or src_seq_stride >= src_seq_length:
        return [one(r) for r in range(R)]
    packed = pack_assembly_input(reads, weights, mod_weights, positions, src_seq_stride)
    bases, chunk_off, read_off = packed[:3]
    # no bases at all: every device read is empty
    out = [shape(("", None if weights is None else "", None if mod_weights is None else np.zeros(0, np.uint8),
                  None if positions is None else np.zeros(0, np.uint32)))] * R
    todo = set(packed.host)
    if bases.size:
        d = None
        if weights is not None or positions is None:
            d = _assemble_device(bases, chunk_off, read_off, device, packed.qw, packed.mw)
        if positions is not None:  # a call of its own on the same packing; the same bases give the same status
            p = _assemble_device(bases, chunk_off, read_off, device, bp=packed.bp)
            d = p if d is None else d._replace(status=d.status | p.status, rpos=p.rpos)
        raw, seq_len, status = d.seq.tobytes(), d.seq_len, d.status
        extras = [(v, f) for v, f in ((d.qual, quality_string), (d.ml, np.copy), (d.rpos, np.copy)) if v is not None]
        start = chunk_off[read_off[:-1]]
        for r in range(R):
            if status[r] != 0:
                todo.add(r)
            elif seq_len[r] > 0:
                s = slice(start[r], start[r] + seq_len[r])
                seq = raw[s].decode("ascii")
                out[r] = seq if plain else (seq,) + tuple(f(v[s]) for v, f in extras)
    if stats is not None:
        stats["reads"] = stats.get("reads", 0) + R
        stats["fallback"] = stats.get("fallback", 0) + len(todo)
    for r in sorted(todo):
        try:
            out[r] = one(r)
        except Exception:
            if not defer_errors:
                raise
            out[r] = None
    return out
