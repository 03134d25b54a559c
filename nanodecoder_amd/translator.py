"""Drop-in for translate/translator.py on MI355X.

``build_translator(opt, report_score, logger, out_file)`` and
``Translator.translate(src, tgt, src_dir, batch_size, attn_debug)`` keep the
reference's names, arguments, return values and error behaviour
(translate/translator.py:65-90,181-369), so translate.py's call
(translate.py:76,113-120) works unchanged.  The model runs in
libnanodec_hip.so (``Engine``); there is no CPU path — ``-gpu -1`` raises.

Reference semantics reproduced:
* batches are ``batch_size`` consecutive chunks of ONE read, each zero padded
  to its own longest chunk (inputters/inputter.py:86-95); that padded length is
  passed to the engine as the chunk's ``span`` so results are identical to the
  reference however the engine packs chunks;
* greedy (beam_size == 1) runs all max_length steps and scores with the last
  step's top log-prob (:396-503); --fast beam for beam_size > 1 (:619-825);
* predictions are cut at the first EOS and joined with spaces
  (translate/translation.py:31-47, translate/translator.py:271-273).

Additions: chunks may be given as float32 arrays instead of strings, and
``translate_reads`` packs chunks of many reads into full engine batches (same
per-chunk results, far higher throughput than one read at a time).
"""
from __future__ import annotations

import collections
import contextlib
import json
import os
from typing import Iterable, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import checkpoint
from .engine import Engine
from .engine import Engine as _HipEngine  # the real engine class (tests substitute Engine)
from .engine import EnginePool

_REAL_ENGINES = (_HipEngine, EnginePool)


class GNMTGlobalScorer:
    """onmt/translate/beam.py:181-199: alpha/beta, and the length / coverage
    penalty kinds (onmt/translate/penalties.py) the classic Beam applies."""

    def __init__(self, opt):
        self.alpha = float(getattr(opt, "alpha", 0.0))
        self.beta = float(getattr(opt, "beta", 0.0))
        self.length_penalty = str(getattr(opt, "length_penalty", "none") or "none")
        self.coverage_penalty = str(getattr(opt, "coverage_penalty", "none") or "none")


class Request(NamedTuple):
    """What one public call was asked to return beside each chunk's scores and tokens: the attention rows
    (``attn_debug``), the token weights of the best hypothesis (``qualities``), their modification weights
    (``mods``) and the tokens' signal positions (``moves``).  Translator._request builds it, every job carries
    it.  ``join`` and ``split`` are the one place that knows the layout of a result, per chunk and per read
    alike: (scores, predictions), then of weights, modification weights and positions, in this order, those
    that were asked."""
    attn: bool = False
    weights: bool = False
    mods: bool = False
    positions: bool = False

    def asked(self, weights, mod_weights, positions) -> tuple:
        """Of one value per optional output, those of the outputs that were asked, in the layout's order."""
        return tuple(v for v, on in zip((weights, mod_weights, positions), self[1:]) if on)

    def join(self, scores, predictions, weights, mod_weights, positions):
        return (scores, predictions) + self.asked(weights, mod_weights, positions)

    def split(self, result):
        """(scores, predictions, weights, mod_weights, positions) of a result, None for what was not asked."""
        rest = iter(result[2:])
        return (result[0], result[1]) + tuple(next(rest) if on else None for on in self[1:])


def _asked(**flags):
    """The keywords of ``flags`` that are set, each as True.  Optional outputs cross to the engine object only
    this way: a call that was not asked for one passes exactly the keywords it always has (the stand-in
    engines of the host tests take no others)."""
    return {k: True for k, on in flags.items() if on}


def _lane(r):
    """The ``lane=`` keyword of token_weights / token_mod_weights / token_positions for the result ``r`` of an
    EnginePool call, so they follow that call on its lane's stream; nothing for a single Engine."""
    return {"lane": r["lane"]} if "lane" in r else {}


def _flagged(overflow) -> bool:
    """Is a call's overflow word (nd_take_overflow; None where the engine has none) set?"""
    return overflow is not None and int(overflow.reshape(-1)[0]) != 0


def parse_chunk(c) -> np.ndarray:
    """NanoDataset.extract_features (inputters/nano_dataset.py:43-83) for
    corpus_type 'translate': a chunk is a whitespace-separated string of
    floats, or the path of a file holding one; returns float32."""
    if isinstance(c, np.ndarray):
        return np.ascontiguousarray(c, dtype=np.float32)
    if isinstance(c, torch.Tensor):
        return c.detach().to(torch.float32).cpu().numpy().reshape(-1)
    if isinstance(c, (list, tuple)):
        return np.asarray(c, dtype=np.float64).astype(np.float32)
    if isinstance(c, str) and os.path.exists(c):
        with open(c) as f:
            c = f.read()
    return np.asarray(str(c).split(), dtype=np.float64).astype(np.float32)


def _bucket(n: int, cap: int) -> int:
    b = 8
    while b < n:
        b *= 2
    return min(max(b, n), cap)


def build_translator(opt, report_score=False, logger=None, out_file=None):
    """translate/translator.py:65-90."""
    models = getattr(opt, "models", None) or []
    if len(models) != 1:
        raise NotImplementedError("exactly one -model is supported (ensembles are not on the MI355X path)")
    if logger:
        logger.info("Loading model...")
    cfg, W = checkpoint.load(models[0])
    scorer = GNMTGlobalScorer(opt)
    return Translator(cfg, W, opt, global_scorer=scorer, report_score=report_score, logger=logger)


class Translator(object):
    """translate/translator.py:93-173, engine-backed."""

    def __init__(self, cfg, weights, opt, global_scorer=None, report_score=False, logger=None, engine=None):
        self.cfg = cfg
        self.opt = opt
        self.gpu = getattr(opt, "gpu", -1)
        if self.gpu < 0 and engine is None:
            raise RuntimeError("nanodecoder_amd runs on MI355X only: pass -gpu N (there is no CPU path)")
        self.n_best = int(getattr(opt, "n_best", 1))
        self.max_length = int(getattr(opt, "max_length", 100))
        self.min_length = int(getattr(opt, "min_length", 0))
        self.beam_size = int(getattr(opt, "beam_size", 5))
        self.random_sampling_temp = float(getattr(opt, "random_sampling_temp", 1.0))
        self.sample_from_topk = int(getattr(opt, "random_sampling_topk", 1))
        self.block_ngram_repeat = int(getattr(opt, "block_ngram_repeat", 0))
        self.ignore_when_blocking = set(getattr(opt, "ignore_when_blocking", None) or [])
        self.dump_beam = getattr(opt, "dump_beam", "")
        # translator.py:166-173: the beam trace accumulator -dump_beam writes
        self.beam_trace = self.dump_beam != ""
        self.beam_accum = ({"predicted_ids": [], "beam_parent_ids": [], "scores": [], "log_probs": []}
                           if self.beam_trace else None)
        self.replace_unk = bool(getattr(opt, "replace_unk", False))
        self.verbose = bool(getattr(opt, "verbose", False))
        self.fast = bool(getattr(opt, "fast", False))
        self.stepwise_penalty = bool(getattr(opt, "stepwise_penalty", False))
        # random sampling draws: keyed by -seed when given (>= 0), else by fresh entropy;
        # successive calls advance like a generator
        seed = getattr(opt, "seed", -1)
        self._seed = int(seed) if seed is not None and int(seed) >= 0 else int.from_bytes(os.urandom(8), "little")
        self._draws = 0
        self.global_scorer = global_scorer or GNMTGlobalScorer(opt)
        self.report_score = report_score
        self.logger = logger
        self.out_file_attn = None
        self._check_supported()
        batch_cap = max(1, int(getattr(opt, "batch_size", 100)))
        self.max_batch = int(getattr(opt, "engine_max_batch", 0) or 0) or max(batch_cap, 256)
        if engine is None:
            dev = torch.cuda.current_device()  # the reference moves tensors to the default "cuda" device
            kw = dict(device=dev, max_batch=self.max_batch, max_steps=self.max_length,
                      max_src_len=min(512, int(getattr(opt, "src_seq_length", 512))),
                      max_beam=max(1, self.beam_size))
            # -engine_lanes: that many calls in flight on the GPU (EnginePool),
            # stream_reads keeping every lane busy.  Default 3 for greedy /
            # sampling; 1 for beam search, whose calls poll the host between
            # graph segments (stream_reads' one host thread would serialise
            # them) and whose lanes each hold the context K/V (~2.4 GB at
            # B = 1024, beam 5)
            lanes = int(getattr(opt, "engine_lanes", 0) or 0) or (3 if self.beam_size == 1 else 1)
            if lanes > 1 and Engine is _HipEngine:
                engine = EnginePool(cfg, weights, lanes=lanes, **kw)
            else:
                engine = Engine(cfg, weights, **kw)
        self.engine = engine
        self._pinned, self._pin_i = None, 0
        self.last_gold_scores = None  # per-chunk gold scores of the last translate(src, tgt=...)

    def _check_supported(self, qualities: bool = False, mods: bool = False):
        if mods and not ("C" in self.cfg.itos and "M" in self.cfg.itos):
            raise ValueError("methylation probabilities need a vocabulary with the tokens C and M (a -cpg model)")
        if qualities and self.beam_size > 1 and self.cfg.self_attn_type == "average":
            # the beam's qualities come from the scoring pass, which refuses such decoders
            raise NotImplementedError("qualities with beam search are not supported for average-attention decoders")
        if self.beam_size == 1:
            # translator.py:371-394: keep_topk == 1 (or temp == 0) is argmax, anything else samples
            if self.sample_from_topk > self.cfg.vocab:
                raise ValueError("random_sampling_topk larger than the vocabulary")
            if self.block_ngram_repeat != 0:
                raise AssertionError("block_ngram_repeat is not supported (translator.py:430)")
        elif not self.fast:
            # the classic onmt Beam (translator.py:827-926, onmt/translate/beam.py): length and
            # coverage penalties (stepwise or at scoring time), n-gram blocking, -dump_beam
            if self.global_scorer.length_penalty not in ("none", "wu", "avg"):
                raise ValueError(f"unknown length_penalty {self.global_scorer.length_penalty!r}")
            if self.global_scorer.coverage_penalty not in ("none", "wu", "summary"):
                raise ValueError(f"unknown coverage_penalty {self.global_scorer.coverage_penalty!r}")
            if self.block_ngram_repeat < 0 or self.block_ngram_repeat > self.max_length:
                raise ValueError("block_ngram_repeat must be in [0, max_length]")
            if self.n_best > self.beam_size:
                raise ValueError("n_best must be <= beam_size")
        else:
            if self.dump_beam:
                raise AssertionError("dump_beam is not supported with --fast (translator.py:631)")
            if self.block_ngram_repeat != 0:
                raise AssertionError("block_ngram_repeat is not supported with --fast (translator.py:633)")
            if self.global_scorer.beta != 0:
                raise AssertionError("beta must be 0 with --fast (translator.py:634)")
            if self.n_best > self.beam_size:
                raise ValueError("n_best must be <= beam_size")
        # -replace_unk is accepted: TranslationBuilder only replaces when the
        # batch carries text src (translation.py:42-47), which nano data never
        # does (src is None, :73-81), so predictions are unchanged

    def _request(self, attn_debug: bool = False, qualities: bool = False, mods: bool = False,
                 moves: bool = False) -> Request:
        """The Request of one public call, after the refusals: qualities or positions together with
        attn_debug, ``mods`` without C and M in the vocabulary, beam qualities on an average-attention
        decoder.  ``mods`` implies ``qualities`` here, and nowhere else."""
        qualities = bool(qualities or mods)  # the methylation values travel beside the qualities
        if qualities:
            if attn_debug:
                raise ValueError("qualities are not available together with attn_debug")
            self._check_supported(qualities=True, mods=bool(mods))
        if moves and attn_debug:
            raise ValueError("signal positions are not available together with attn_debug")
        return Request(bool(attn_debug), qualities, bool(mods), bool(moves))

    def split_result(self, result, qualities: bool = False, mods: bool = False, moves: bool = False):
        """(scores, predictions, weights, mod_weights, positions) of one read's result from translate_reads /
        translate_raw_reads (or of one chunk's from stream_reads) called with the same ``qualities``, ``mods``
        and ``moves``; None for what was not asked."""
        return self._request(qualities=qualities, mods=mods, moves=moves).split(result)

    def setAttnFile(self, out_file_attn):
        self.out_file_attn = out_file_attn

    # ------------------------------------------------------------------ core
    def _stage(self, B: int, T: int):
        """Host staging of one engine batch: views into a ring of pinned
        buffers (real engine; the host-to-device copies then run async, so the
        next batch is packed while the device works on this one), or plain
        numpy arrays (stand-in engines)."""
        if not self._real_engine():
            return np.zeros((B, T), np.float32), np.ones(B, np.int32), np.ones(B, np.int32), None
        if self._pinned is None:
            # one buffer per call in flight, one being packed, one spare
            cap, tl = self.engine.max_batch, self.engine.max_src_len
            self._pinned = [(torch.empty(cap * tl, dtype=torch.float32).pin_memory(),
                             torch.empty(2 * cap, dtype=torch.int32).pin_memory()) for _ in range(self._depth() + 2)]
        fbuf, ibuf = self._pinned[self._pin_i % len(self._pinned)]
        self._pin_i += 1
        sig_t = fbuf[: B * T].view(B, T)
        sig_t.zero_()
        L_t, S_t = ibuf[:B], ibuf[B: 2 * B]
        L_t.fill_(1)
        S_t.fill_(1)
        return sig_t.numpy(), L_t.numpy(), S_t.numpy(), (sig_t, L_t, S_t)

    def _real_engine(self) -> bool:
        return isinstance(self.engine, _REAL_ENGINES)

    def _depth(self) -> int:
        """Engine calls kept in flight by stream_reads: one per EnginePool lane."""
        return max(1, int(getattr(self.engine, "lanes", 1)))

    def _batch_dims(self, n: int, spans, cap: Optional[int] = None):
        """(B, T, spans as int32) of an engine batch of n chunks: T the longest span rounded up to 64 samples,
        B the bucket of n under ``cap`` (max_batch when not given)."""
        spans = np.asarray(spans, np.int32)
        if spans.max() > self.engine.max_src_len:
            raise ValueError(f"chunk longer than {self.engine.max_src_len} samples (src_seq_length) is not supported")
        T = min(self.engine.max_src_len, ((int(spans.max()) + 63) // 64) * 64)
        return _bucket(n, cap or self.engine.max_batch), T, spans

    def _pack(self, chunks: List[np.ndarray], spans: Sequence[int], cap: Optional[int] = None):
        """Stage one engine batch (_stage): the chunks with their reference spans in its first rows.  Returns
        what the engine gets, signal [B, T], chunk lengths [B] and spans [B] (pinned tensors for a real
        engine), then B and the chunk lengths as numpy."""
        n = len(chunks)
        lens = np.array([len(c) for c in chunks], np.int32)
        if (lens < 1).any():
            raise ValueError("empty signal chunk")
        B, T, spans = self._batch_dims(n, spans, cap)
        sig, L, S, dev_in = self._stage(B, T)
        for i, c in enumerate(chunks):
            sig[i, : len(c)] = c
        L[:n], S[:n] = lens, spans
        if dev_in is not None:
            sig, L, S = dev_in
        return sig, L, S, B, lens

    def _submit(self, chunks: List[np.ndarray], spans: Sequence[int], groups: Optional[Sequence[int]] = None,
                req: Request = Request()):
        """Stage up to max_batch chunks with their reference spans (and, for
        the classic Beam, their reference batch ids) and enqueue the engine
        call.  Greedy and sampling calls return before the device finishes;
        ``_finish`` collects the results, those ``req`` asks for among them
        (see stream_reads)."""
        sig, L, S, B, lens = self._pack(chunks, spans)
        job = self._enqueue(sig, L, S, B, len(chunks), lens, groups, req, (sig, L, S))
        job["again"] = lambda: self._submit(chunks, spans, groups, req)
        return job

    def _enqueue(self, sig, L, S, B: int, n: int, lens: np.ndarray, groups, req: Request, inputs):
        """The engine call for one staged batch (signal [B, T], chunk lengths
        and spans [B]; the first n rows are chunks), its results copied to
        pinned host buffers on the call's own stream.  ``req.weights``: a
        greedy or sampling call also returns its log-probs and the chosen
        tokens' weights (nd_token_weights) follow it on its stream; a beam
        call's inputs are kept for the scoring pass of ``_beam_weights``.
        ``req.mods``: the tokens' modification weights (nd_token_mod_weights)
        follow the weights, from the same log-probs.  ``req.positions``: the
        call also returns its attention, the tokens' positions
        (nd_token_positions, of hypothesis 0 for a beam call) follow it on its
        stream, and only those [B, S] positions are copied out, not the
        attention."""
        job = dict(n=n, lens=lens, req=req, B=B, inputs=inputs)
        attn = req.attn or req.positions  # the engine call's return_attn
        if self.beam_size == 1:
            want = _asked(return_logp=req.weights)
            if not (self.random_sampling_temp == 0.0 or self.sample_from_topk == 1):
                # sample_with_temperature's random branch (translator.py:376-393)
                self._draws += 1
                seed = (self._seed * 0x9E3779B97F4A7C15 + self._draws) & (2 ** 64 - 1)
                r = self.engine.translate_sample(sig, L, S, temp=self.random_sampling_temp,
                                                 keep_topk=self.sample_from_topk, seed=seed, max_len=self.max_length,
                                                 min_len=self.min_length, return_attn=attn, **want)
            else:
                r = self.engine.translate_greedy(sig, L, S, max_len=self.max_length, min_len=self.min_length,
                                                 return_attn=attn, **want)
            if req.weights:
                r["weights"] = self.engine.token_weights(r["tokens"], logp=r["logp"], **_lane(r))
            if req.mods:
                r["mod_weights"] = self.engine.token_mod_weights(r["tokens"], r["logp"], *self._cm_ids(), **_lane(r))
            if req.positions:
                self._positions(r, S)
            job.update(kind="greedy", r=r)
        else:
            # reference batches: the chunks of one group, sorted by length
            # descending (stable) as the reference's batch rows are
            grp = np.zeros(n, np.int64) if groups is None else np.asarray(groups)
            members = {}
            for i in range(n):
                members.setdefault(int(grp[i]), []).append(i)
            sorted_rows = {gid: sorted(m, key=lambda i: -int(lens[i])) for gid, m in members.items()}
            beam = self.beam_size
            cut = None
            if self.fast:
                r = self.engine.translate_beam(sig, L, S, beam=beam, n_best=self.n_best,
                                               alpha=self.global_scorer.alpha, max_len=self.max_length,
                                               min_len=self.min_length, return_attn=attn)
            else:
                # dense reference-batch ids; the engine's padding rows are batches of their own
                g = np.zeros(B, np.int32)
                g[:n] = np.unique(grp, return_inverse=True)[1]
                base = int(g[:n].max()) + 1
                g[n:] = np.arange(base, base + B - n)
                # beam j of a batch reads memory_lengths[j] of the beam-tiled lengths
                # (translator.py:902-907): the length of the batch's row j // beam
                cut = np.ones(B, np.int32)
                for rows in sorted_rows.values():
                    for pos, i in enumerate(rows):
                        cut[i] = lens[rows[pos // beam]]
                gs = self.global_scorer
                exclusion = [self.cfg.itos.index(t) if t in self.cfg.itos else 0 for t in self.ignore_when_blocking]
                r = self.engine.translate_beam_classic(
                    sig, L, S, groups=g, beam=beam, n_best=self.n_best, length_penalty=gs.length_penalty,
                    alpha=gs.alpha, max_len=self.max_length, min_len=self.min_length,
                    coverage_penalty=gs.coverage_penalty, beta=gs.beta, stepwise_penalty=self.stepwise_penalty,
                    block_ngram_repeat=self.block_ngram_repeat, ignore_ids=exclusion, cut=cut, return_attn=attn)
            if req.positions:
                self._positions(r, S, hyp0=True)
            job.update(kind="beam", r=r, grp=grp, sorted_rows=sorted_rows, cut=cut)
            if req.weights:
                job["eng_in"] = (sig, L, S)
        if self._real_engine():
            self._copy_out(job)
        return job

    _HOST_KEYS = ("tokens", "scores", "lens", "attn", "done_step", "overflow", "weights", "mod_weights", "positions")

    def _positions(self, r, spans, hyp0: bool = False):
        """The token positions [B, S] of a call's result ``r`` (Engine.token_positions on the call's stream, its
        EnginePool lane), in r["positions"]; the attention they came from is dropped from the result, so it is
        not copied to the host."""
        r["positions"] = self.engine.token_positions(r["attn"], spans, hyp0=hyp0, **_lane(r))
        r["attn"] = None

    def _cm_ids(self):
        """(id of "C", id of "M") in the target vocabulary."""
        return self.cfg.itos.index("C"), self.cfg.itos.index("M")

    def _copy_out(self, job):
        """Enqueue the call's device-to-host copies (into pinned buffers) on
        the stream the call ran on (its EnginePool lane, or the current
        stream the single Engine joined), then an event: ``_host`` waits on
        that event alone, never on calls submitted after this one."""
        r = job["r"]
        st = self.engine.stream_of(r)
        host = {}
        with torch.cuda.stream(st):
            for k in self._HOST_KEYS:
                t = r.get(k)
                if isinstance(t, torch.Tensor):
                    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                    h.copy_(t, non_blocking=True)
                    host[k] = h
            ev = torch.cuda.Event()
            ev.record(st)
        job["host"], job["event"] = host, ev

    def _host(self, job, *names):
        """Results of a submitted call on the host (numpy; None where the
        call has no such output)."""
        if "host" in job:
            job["event"].synchronize()
            h = job["host"]
            return [h[k].numpy() if k in h else None for k in names]
        r = job["r"]  # stand-in engines: host tensors
        return [None if r.get(k) is None else r[k].cpu().numpy() for k in names]

    @contextlib.contextmanager
    def _exact_fp32(self):
        """Split-fp16 range guard (nd_take_overflow): a call in which some
        split activation reached |x| >= 65504 (fp16's range; the reference's
        fp32 is still finite there) runs again inside this block, with every
        product in exact fp32, and its results replace the flagged ones.  The
        mode is switched off again however the block ends."""
        self.engine.set_exact_fp32(True)
        try:
            yield
        finally:
            self.engine.set_exact_fp32(False)

    def _run_guarded(self, call, exact: bool = False):
        """The result of the engine call ``call()`` once the device has finished it, under the range guard
        (_exact_fp32): a flagged call runs once more in exact fp32, unless ``exact`` says that the mode is on
        already."""
        def run():
            r = call()
            if "event" in r:  # an EnginePool call returns before its outputs exist
                r["event"].synchronize()
            return r
        r = run()
        if _flagged(r.get("overflow")) and not exact:
            with self._exact_fp32():
                r = run()
        return r

    def _finish(self, job, arrays: bool = False):
        """Per chunk (scores[n_best], token lists[n_best]), then what the call's Request asked for: the best
        hypothesis' weights, modification weights and positions, each spread over the characters of its string
        (_char_weights), or with ``attn`` the attention rows of each hypothesis ([steps, cut] arrays, cut as
        the reference's results["attention"] has it).  ``arrays`` (greedy / sampling): the columns themselves
        instead, (tokens [n, S], scores [n]) numpy, then one [n, S] array per token for each output asked:
        weights and modification weights uint16, positions int32."""
        n, req, beam = job["n"], job["req"], job["kind"] == "beam"
        tok, sc, ln, at, done, ov = self._host(job, "tokens", "scores", "lens", "attn", "done_step", "overflow")
        if _flagged(ov) and not job.get("exact"):
            # range guard: the whole call again, and all that follows from it (a rerun never reruns again)
            with self._exact_fp32():
                again = job["again"]()
                again["exact"] = True
                return self._finish(again, arrays)
        w = mw = ps = None
        if req.weights:
            w, mw = self._beam_weights(job, tok, ln) if beam else self._host(job, "weights", "mod_weights")
            w, mw = w.view(np.uint16), mw.view(np.uint16) if req.mods else None
        if req.positions:
            ps = self._host(job, "positions")[0]
        cols = req.asked((w, np.uint16), (mw, np.uint16), (ps, np.int32))
        if arrays:
            return (tok[:n], sc[:n]) + tuple(a[:n] for a, _ in cols)
        out = []
        for i in range(n):
            if beam:
                o = ([float(sc[i, k]) for k in range(self.n_best)],
                     [tok[i, k, : ln[i, k]].tolist() for k in range(self.n_best)])
            else:
                o = ([float(sc[i])], [tok[i].tolist()])
            if cols:
                o += tuple(self._char_weights(o[1][0], a[i], dtype) for a, dtype in cols)
            if req.attn:
                o += (self._attn_rows(job, i, at, ln, done),)
            out.append(o)
        return out

    def _attn_rows(self, job, i: int, at, ln, done):
        """The attention rows of chunk i's hypotheses, each cut at memory_lengths as the reference cuts it."""
        lens = job["lens"]
        if job["kind"] == "greedy":  # results["attention"]: rows cut at the chunk's length (translator.py:491-501)
            return [at[i, :, : lens[i]]]
        grp, sorted_rows, cut, beam = job["grp"], job["sorted_rows"], job["cut"], self.beam_size
        atts = []
        for k in range(self.n_best):
            if self.fast:
                # translator.py:780-790: attention[:, i, j, :memory_lengths[i]] with i the
                # chunk's index among the batches alive at the hypothesis' last step
                step = int(ln[i, k]) - 1
                alive = [q for q in sorted_rows[int(grp[i])] if done[q] == 0 or done[q] > step]
                c = int(lens[alive[alive.index(i) // beam]])
            else:
                c = int(cut[i])
            atts.append(at[i, k, : ln[i, k], :c])
        return atts

    def _beam_weights(self, job, tok, ln):
        """The token weights [B, L] of a finished beam call's best hypotheses: the existing
        teacher-forced scoring pass (score_targets) over the call's own inputs, each gold row the hypothesis'
        tokens as returned (EOS included when it finished) and gold_len its length, then nd_token_weights of
        the pass's per-token log-probs.  The encoder runs a second time for this.  A call submitted with
        ``mods`` asks the same pass for its full log-probs too; returns (weights, modification weights), the
        latter nd_token_mod_weights of those log-probs, or None without ``mods``.  The pass has a range guard
        of its own: when it alone is flagged, it alone runs again."""
        sig, ln_in, sp = job["eng_in"]
        B, mods = job["B"], job["req"].mods
        n_tok = np.clip(ln[:B, 0].astype(np.int32), 1, min(tok.shape[2], self.engine.max_steps))
        L = min(self.engine.max_steps, (int(n_tok.max()) + 7) // 8 * 8)  # one captured graph per (B, T, L)
        gold = np.full((B, L), self.cfg.pad_idx, np.int32)
        for i in range(B):
            gold[i, : n_tok[i]] = tok[i, 0, : n_tok[i]]
        gold[gold < 0] = self.cfg.eos_idx  # a row without a hypothesis (engine padding) scores a lone EOS
        gold_t, len_t = torch.from_numpy(gold), torch.from_numpy(n_tok)
        r = self._run_guarded(lambda: self.engine.score_targets(sig, ln_in, sp, gold=gold_t, gold_len=len_t,
                                                                return_tok_logp=True, **_asked(return_logp=mods)),
                              exact=job.get("exact", False))
        w = self.engine.token_weights(gold_t, tok_logp=r["tok_logp"], **_lane(r))
        # positions past a hypothesis' length hold pad_idx, which is neither C nor M: their weight is 0
        mw = self.engine.token_mod_weights(gold_t, r["logp"], *self._cm_ids(), **_lane(r)) if mods else None
        if "lane" in r:
            self.engine.stream_of(r).synchronize()
        return w.cpu().numpy(), mw.cpu().numpy() if mods else None

    def _char_weights(self, toks, w, dtype=np.uint16) -> np.ndarray:
        """The weight of every character of a hypothesis' string with the spaces removed (uint16): the
        tokens up to the first EOS as _tokens_to_sent cuts them, each character of a token's word carrying
        the token's weight.  The tokens' positions (int32) are spread the same way."""
        out = []
        for t, wt in zip(toks, w):
            word = self.cfg.itos[t]
            if t == self.cfg.eos_idx:
                break
            out.extend([int(wt)] * len(word.replace(" ", "")))
        return np.asarray(out, dtype)

    def _run(self, chunks: List[np.ndarray], spans: Sequence[int], groups: Optional[Sequence[int]] = None,
             attn: bool = False):
        """One engine batch, synchronously (see _submit / _finish)."""
        return self._finish(self._submit(chunks, spans, groups, Request(attn=attn)))

    def _tokens_to_sent(self, toks) -> List[str]:
        """translate/translation.py:31-47."""
        words = []
        for t in toks:
            w = self.cfg.itos[t]
            if t == self.cfg.eos_idx:
                break
            words.append(w)
        return words

    # --------------------------------------------------------------- gold scoring
    def _gold_ids(self, target) -> List[int]:
        """One target as token ids without EOS: a token string ("A C G T"; words outside the vocabulary
        become <unk>, as torchtext maps them) or a sequence of ids.  ValueError for an id outside the
        vocabulary, for pad / BOS / EOS inside the sequence, and for more tokens than max_steps - 1."""
        cfg = self.cfg
        if isinstance(target, str):
            ids = [cfg.itos.index(w) if w in cfg.itos else cfg.unk_idx for w in target.split()]
        else:
            ids = [int(t) for t in np.asarray(target).reshape(-1).tolist()]
        for t in ids:
            if t < 0 or t >= cfg.vocab:
                raise ValueError(f"target token id {t} outside the vocabulary [0, {cfg.vocab})")
            if t in (cfg.pad_idx, cfg.bos_idx, cfg.eos_idx):
                raise ValueError(f"target holds the special token {cfg.itos[t]!r}: pass the bases only "
                                 "(BOS and EOS are added here)")
        if len(ids) > self.engine.max_steps - 1:
            raise ValueError(f"target of {len(ids)} tokens is longer than max_steps - 1 = "
                             f"{self.engine.max_steps - 1}")
        return ids

    @staticmethod
    def _reference_spans(chunks, batch_size: int) -> List[int]:
        """Per chunk the span of its reference batch: the longest of its ``batch_size`` consecutive chunks."""
        spans = []
        for b0 in range(0, len(chunks), batch_size):
            part = chunks[b0: b0 + batch_size]
            spans += [max(len(c) for c in part)] * len(part)
        return spans

    def score(self, chunks, targets, batch_size, moves: bool = False):
        """Teacher-forced scores of given target sequences (Translator._score_target,
        translate/translator.py:928-941): per chunk (score, tok_logp list), score = the sum of the target's
        token log-probabilities, EOS (appended here) included, tok_logp = the summands.  ``targets``: one
        token string or id sequence per chunk (see _gold_ids).  Each chunk keeps the span of its reference
        batch (consecutive ``batch_size`` chunks), exactly as stream_reads assigns it.  With ``moves`` (forced
        alignment) each chunk's result is (score, tok_logp, positions): the signal sample of every target
        token, EOS included, chunk-relative and non-decreasing: nd_token_positions of the scoring pass's own
        context attention, the rule -moves applies to decoded tokens (DESIGN.md sections 1.6, 1.7)."""
        if batch_size is None:
            raise ValueError("batch_size must be set")
        chunks = [parse_chunk(c) for c in chunks]
        if len(chunks) != len(targets):
            raise ValueError("one target per chunk")
        ids = [self._gold_ids(t) for t in targets]
        if self.cfg.self_attn_type == "average":
            raise NotImplementedError("scoring targets is not supported for average-attention decoders")
        spans = self._reference_spans(chunks, batch_size)
        out, cap = [], self.engine.max_batch
        for b0 in range(0, len(chunks), cap):
            out += self._score_batch(chunks[b0: b0 + cap], spans[b0: b0 + cap], ids[b0: b0 + cap], moves)
        return out

    def _score_batch(self, chunks, spans, ids, moves: bool = False):
        """One engine batch of score(): stage, call (under the range guard), collect on the host.  With
        ``moves`` the call returns its attention too, token_positions reduces it on the call's stream (its
        EnginePool lane), and only the [B, L] positions come to the host."""
        n = len(chunks)
        sig, ln, sp, B, _ = self._pack(chunks, spans)
        # target rows padded to a multiple of 8 positions (one captured graph per (B, T, L); the padding
        # positions add exactly 0)
        L = min(self.engine.max_steps, (max(len(t) for t in ids) + 1 + 7) // 8 * 8)
        gold = np.full((B, L), self.cfg.pad_idx, np.int32)
        gold_len = np.ones(B, np.int32)
        gold[:, 0] = self.cfg.eos_idx  # the engine's padding rows score a lone EOS
        for i, t in enumerate(ids):
            gold[i, : len(t)] = t
            gold[i, len(t)] = self.cfg.eos_idx
            gold_len[i] = len(t) + 1
        gold_t, len_t = torch.from_numpy(gold), torch.from_numpy(gold_len)
        r = self._run_guarded(lambda: self.engine.score_targets(sig, ln, sp, gold=gold_t, gold_len=len_t,
                                                                return_tok_logp=True, **_asked(return_attn=moves)))
        if moves:
            self._positions(r, sp)
            if "lane" in r:
                self.engine.stream_of(r).synchronize()
        sc, tl = r["scores"].cpu().numpy(), r["tok_logp"].cpu().numpy()
        if moves:
            ps = r["positions"].cpu().numpy()
            return [(float(sc[i]), tl[i, : gold_len[i]].tolist(), ps[i, : gold_len[i]].tolist()) for i in range(n)]
        return [(float(sc[i]), tl[i, : gold_len[i]].tolist()) for i in range(n)]

    def score_candidates(self, chunks, candidates, batch_size):
        """Which of its candidate targets does each chunk's signal support?
        ``candidates[i]``: a non-empty list of targets for chunk i, each a token string or an id sequence (see
        _gold_ids).  Returns per chunk (scores, log_posteriors, best): the teacher-forced score of every
        candidate (what score() gives for it, EOS included), their log-posterior over the chunk's own
        candidates, and the index of the best one (the first on a tie); the lists are as long as the chunk's
        candidate list.  Each chunk keeps the span score() gives it.  A chunk's candidates share its encoder
        pass: consecutive chunks go into one engine call while chunks * K <= max_batch, K = the call's
        largest candidate count rounded up to a power of two (few captured graphs); the slots a chunk does
        not fill stay empty and take no part in its posterior."""
        if batch_size is None:
            raise ValueError("batch_size must be set")
        chunks = [parse_chunk(c) for c in chunks]
        if len(chunks) != len(candidates):
            raise ValueError("one candidate list per chunk")
        cap = self.engine.max_batch
        ids = []
        for i, cl in enumerate(candidates):
            cl = [cl] if isinstance(cl, str) else list(cl)
            if not cl:
                raise ValueError(f"chunk {i} has no candidates")
            if len(cl) > cap:
                raise ValueError(f"chunk {i} has {len(cl)} candidates, more than max_batch = {cap}")
            ids.append([self._gold_ids(t) for t in cl])
        if self.cfg.self_attn_type == "average":
            raise NotImplementedError("scoring targets is not supported for average-attention decoders")
        spans = self._reference_spans(chunks, batch_size)

        def slots(n):  # a power of two while one chunk of it fits a call
            k = 1
            while k < n:
                k *= 2
            return k if k <= cap else n

        out, b0, K = [], 0, 1  # the open call: chunks b0 .. i - 1 at K slots each
        for i in range(len(chunks)):
            k = slots(max(K, len(ids[i])))
            if i > b0 and (i - b0 + 1) * k > cap:
                out += self._score_cand_batch(chunks[b0:i], spans[b0:i], ids[b0:i], K)
                b0, k = i, slots(len(ids[i]))
            K = k
        if chunks:
            out += self._score_cand_batch(chunks[b0:], spans[b0:], ids[b0:], K)
        return out

    def _score_cand_batch(self, chunks, spans, ids, K: int):
        """One engine call of score_candidates(): n chunks of at most K candidates each, n * K <= max_batch."""
        sig, ln, sp, B, _ = self._pack(chunks, spans, cap=self.engine.max_batch // K)
        # as _score_batch: rows padded to a multiple of 8 positions (one captured graph per (B, T, K, L))
        L = min(self.engine.max_steps, (max(len(t) for cl in ids for t in cl) + 1 + 7) // 8 * 8)
        # padding chunks and the slots a chunk does not fill are empty slots (cand_len 0)
        cand = np.full((B, K, L), self.cfg.pad_idx, np.int32)
        cand_len = np.zeros((B, K), np.int32)
        for i, cl in enumerate(ids):
            for k, t in enumerate(cl):
                cand[i, k, : len(t)] = t
                cand[i, k, len(t)] = self.cfg.eos_idx
                cand_len[i, k] = len(t) + 1
        cand_t, len_t = torch.from_numpy(cand), torch.from_numpy(cand_len)
        r = self._run_guarded(lambda: self.engine.score_candidates(sig, ln, sp, cand=cand_t, cand_len=len_t))
        sc, post, best = r["scores"].cpu().numpy(), r["post"].cpu().numpy(), r["best"].cpu().numpy()
        return [(sc[i, : len(cl)].tolist(), post[i, : len(cl)].tolist(), int(best[i])) for i, cl in enumerate(ids)]

    def translate(self, src, tgt=None, src_dir=None, batch_size=None, attn_debug=False):
        """translate/translator.py:181-369.  Returns (all_scores,
        all_predictions): per chunk, n_best scores and n_best strings.  With ``tgt`` (one target per chunk,
        see score) the gold scores are computed too (Translator._score_target): kept per chunk on
        ``last_gold_scores`` and, with -verbose, logged as GOLD / GOLD SCORE after PRED SCORE
        (translate/translation.py:147-150)."""
        assert src is not None
        if batch_size is None:
            raise ValueError("batch_size must be set")
        chunks = [parse_chunk(c) for c in src]
        if tgt is None:
            return self.translate_reads([chunks], batch_size=batch_size, attn_debug=attn_debug)[0]
        tgt = list(tgt)
        gold = self.score(chunks, tgt, batch_size)
        self.last_gold_scores = [g[0] for g in gold]
        sents = [t if isinstance(t, str) else " ".join(self.cfg.itos[i] for i in self._gold_ids(t)) for t in tgt]
        req = self._request(attn_debug)
        results = [res for _, res in self._stream_reads([chunks], batch_size, req)]
        return self._report(results, req, gold=list(zip(sents, self.last_gold_scores)))[0]

    def _write_attn(self, chunk: np.ndarray, sent: List[str], attn: np.ndarray):
        """translate/translator.py:285-336: the source samples and the
        prediction (+ </s>) as headers, then one row of attention weights per
        decoder step, into the file set by setAttnFile."""
        preds = list(sent) + ["</s>"]
        srcs = [str(x) for x in np.asarray(chunk, np.float32).reshape(-1)]
        header_format = "{:>8.7} " + "{:>8.7} " * len(srcs)
        row_format = "{:>8.5f} " * len(srcs)
        output = header_format.format(">", *srcs)
        header_format = "{:>8.7} " + "{:>8.7} " * len(preds)
        output += header_format.format("|", *preds) + "\n"
        for row in attn.tolist():
            output += row_format.format(*row) + "\n"
        self.out_file_attn.write(output)

    # ------------------------------------------------------------- many reads
    def _stream(self, reads: Iterable, batch_size: int, describe, submit, store):
        """The loop of stream_reads and stream_raw_reads.  ``describe(read)`` gives the read's result holder
        and one (what, length) per chunk; chunk descriptors (read, chunk, what, length, span, reference
        batch) fill a pending list, span the longest of the chunk's reference batch (``batch_size``
        consecutive chunks of its read).  At max_batch descriptors ``submit(items)`` enqueues an engine call
        and returns its job; ``store(job, items, results)`` waits for a job and puts each chunk's result into
        results[read][chunk].  A call is collected only when more than one call per lane is in flight after a
        submit, so those stay on the device while the next batch is packed, and (read index, holder) is
        yielded once a read's last chunk is stored, a read without chunks at once."""
        cap, depth = self.engine.max_batch, self._depth()
        pending, inflight = [], collections.deque()
        results, remaining = {}, {}
        nb = 0

        def collect():
            job, items = inflight.popleft()
            store(job, items, results)
            for it in items:
                remaining[it[0]] -= 1
                if remaining[it[0]] == 0:
                    yield it[0], results.pop(it[0])

        for ri, read in enumerate(reads):
            holder, parts = describe(read)
            if not parts:
                yield ri, holder
                continue
            results[ri], remaining[ri] = holder, len(parts)
            for b0 in range(0, len(parts), batch_size):
                part = parts[b0: b0 + batch_size]
                span = max(n for _, n in part)
                for k, (what, n) in enumerate(part):
                    pending.append((ri, b0 + k, what, n, span, nb))
                    if len(pending) == cap:
                        inflight.append((submit(pending), pending))
                        pending = []
                        while len(inflight) > depth:
                            yield from collect()
                nb += 1
        if pending:
            inflight.append((submit(pending), pending))
        while inflight:
            yield from collect()

    def stream_reads(self, reads: Iterable[Sequence], batch_size: int, attn_debug: bool = False,
                     qualities: bool = False, mods: bool = False, moves: bool = False):
        """Generator over many reads (any iterable of chunk lists): chunks are
        packed across reads into engine batches of max_batch, one batch (one
        per EnginePool lane) stays in flight on the device while the next is
        packed on the host, and
        (read index, per-chunk results) is yielded as each read completes.
        Each chunk keeps the span of the reference batch it would belong to
        (consecutive ``batch_size`` chunks of its own read), so results equal
        per-read translate().  ``qualities``: each chunk's result also carries,
        as its third entry, the uint16 weights of its best hypothesis, one per
        character of its string with the spaces removed (frontend.assemble_read_q
        turns them into a read's quality string).  Greedy and sampling take them
        from the call's own log-probs; beam search scores the best hypothesis in
        a second, teacher-forced pass (_beam_weights).  ``mods`` (a vocabulary
        with C and M; implies ``qualities``): a fourth entry follows, the uint16
        modification weights of the same characters (frontend.assemble_read_m
        turns them into a read's ML values), from the same log-probs.  ``moves``:
        one more trailing entry, the chunk-relative signal position (int32) of
        the same characters (frontend.assemble_read_p turns them into a read's
        positions): the call returns its head-0 context attention and
        nd_token_positions reduces it on the call's stream, in every search
        mode (a beam call's hypothesis 0; no scoring pass)."""
        yield from self._stream_reads(reads, batch_size, self._request(attn_debug, qualities, mods, moves))

    def _stream_reads(self, reads, batch_size: int, req: Request):
        def describe(read):
            chunks = [parse_chunk(c) for c in read]
            return [None] * len(chunks), [(c, len(c)) for c in chunks]

        def submit(items):
            return self._submit([it[2] for it in items], [it[4] for it in items], [it[5] for it in items], req)

        def store(job, items, results):
            for it, o in zip(items, self._finish(job)):
                results[it[0]][it[1]] = o + (it[2],) if req.attn else o  # -attn_debug dumps the chunk too

        return self._stream(reads, batch_size, describe, submit, store)

    def translate_reads(self, reads: Sequence[Sequence], batch_size: int, attn_debug: bool = False,
                        qualities: bool = False, mods: bool = False, moves: bool = False):
        """Translate many reads (stream_reads); returns per read
        (all_scores, all_predictions) as translate() does; with ``qualities``
        (all_scores, all_predictions, all_weights), all_weights per chunk the
        uint16 weights of its best hypothesis (see stream_reads); with ``mods``
        (which implies ``qualities``) also all_mod_weights, laid out like all_weights; with ``moves`` a last
        entry all_positions, per chunk the int32 chunk-relative signal positions of the same characters
        (split_result takes such a result apart)."""
        req = self._request(attn_debug, qualities, mods, moves)
        results = [None] * len(reads)
        for ri, res in self._stream_reads(reads, batch_size, req):
            results[ri] = res
        return self._report(results, req)

    def translate_raw_reads(self, raws: Sequence[np.ndarray], batch_size: int, normalization: str = "median",
                            src_seq_length: int = 512, src_seq_stride: int = 512, qualities: bool = False,
                            mods: bool = False, moves: bool = False):
        """translate_reads on raw reads with the signal front end on the
        device (stream_raw_reads); returns per read (all_scores,
        all_predictions), with ``qualities`` also all_weights, with ``mods`` also all_mod_weights, with ``moves``
        a last entry all_positions."""
        req = self._request(False, qualities, mods, moves)
        results = [None] * len(raws)
        for ri, res in self._stream_raw_reads(raws, batch_size, normalization, src_seq_length, src_seq_stride,
                                              False, req):
            results[ri] = res
        return self._report(results, req)

    def _report(self, results, req: Request, gold=None):
        """Per read (all_scores, all_predictions), then what ``req`` asked for, from per-chunk results, with
        the reference's verbose / -dump_beam / report_score side outputs
        (translate/translator.py:255-369).  gold (translate with tgt): per chunk
        in order (gold sentence, gold score), logged after PRED SCORE."""
        ret = []
        counter = 0
        pred_score_total, pred_words_total = 0.0, 0
        for r in results:
            per_read = [[] for _ in range(5)]  # scores, predictions, weights, modification weights, positions
            for res in r:
                scores, toks, *optional = req.split(res)
                sents = [self._tokens_to_sent(t) for t in toks]
                if req.attn:
                    self._write_attn(res[3], sents[0], res[2][0])
                for column, v in zip(per_read, [scores[: self.n_best], [" ".join(s) for s in sents[: self.n_best]]]
                                     + optional):
                    column.append(v)
                pred_score_total += scores[0]
                pred_words_total += len(sents[0])
                if self.verbose:
                    counter += 1
                    msg = "\nSENT {}: {}\n".format(counter, None) + \
                          "PRED {}: {}\n".format(counter, " ".join(sents[0])) + \
                          "PRED SCORE: {:.4f}\n".format(scores[0])
                    if gold is not None:  # translation.py:147-150
                        msg += "GOLD {}: {}\n".format(counter, gold[counter - 1][0]) + \
                               "GOLD SCORE: {:.4f}\n".format(gold[counter - 1][1])
                    if len(sents) > 1:
                        msg += "\nBEST HYP:\n" + "".join("[{:.4f}] {}\n".format(sc, s)
                                                         for sc, s in zip(scores, sents))
                    if self.logger:
                        self.logger.info(msg)
                    else:
                        os.write(1, msg.encode("utf-8"))
            ret.append(req.join(*per_read))
        if self.dump_beam:
            # translator.py:365-368 dumps the beam trace accumulator.  (The
            # reference reads it through a `self.translator` attribute the
            # Translator does not have, and nothing in it appends to the
            # lists: the intended file is these four empty lists.)
            with open(self.dump_beam, "w", encoding="utf-8") as f:
                json.dump(self.beam_accum, f)
        if self.report_score and pred_words_total:
            msg = "PRED AVG SCORE: %.4f, PRED PPL: %.4f" % (pred_score_total / pred_words_total,
                                                           np.exp(-pred_score_total / pred_words_total))
            (self.logger.info if self.logger else print)(msg)
        return ret

    # ------------------------------------------------------ device front end
    def _submit_raw(self, items, normalization: str, req: Request):
        """One engine batch from raw reads: chunk descriptors ``items`` =
        (read, chunk, (the read's float64 samples, start), length, span,
        reference batch).  The front end (frontend.device_batch) runs on the
        call's own stream, so the normalised chunks go from HBM to the engine
        with no host pass."""
        from . import frontend
        n = len(items)
        reads = {}  # the reads this batch cuts, in order of appearance
        for it in items:
            reads.setdefault(it[0], it[2][0])
        local = {ri: j for j, ri in enumerate(reads)}
        lens = np.fromiter((it[3] for it in items), np.int32, n)
        B, T, spans = self._batch_dims(n, np.fromiter((it[4] for it in items), np.int32, n))
        ls = np.ones(2 * B, np.int32)
        ls[:n], ls[B: B + n] = lens, spans
        with torch.cuda.stream(self.engine.next_stream()):
            sig, keep = frontend.device_batch(list(reads.values()),
                                              np.fromiter((local[it[0]] for it in items), np.int32, n),
                                              np.fromiter((it[2][1] for it in items), np.int32, n), lens,
                                              normalization, B, T, self.engine.device)
            ls_d = torch.from_numpy(ls).pin_memory().to(self.engine.device, non_blocking=True)
            job = self._enqueue(sig, ls_d[:B], ls_d[B:], B, n, lens, [it[5] for it in items], req,
                                (sig, ls_d, keep))
        job["again"] = lambda: self._submit_raw(items, normalization, req)
        return job

    def stream_raw_reads(self, raws: Iterable, batch_size: int, normalization: str = "median",
                         src_seq_length: int = 512, src_seq_stride: int = 512, arrays: bool = False,
                         qualities: bool = False, mods: bool = False, moves: bool = False):
        """stream_reads on RAW reads (float64 sample arrays, as
        frontend.read_raw returns them) with extract_fast5_raw's
        normalisation and windowing (utils/labelop.py:194-243) on the device:
        the reads of each engine batch go to HBM once and are cut into its
        [B, T] signal batch there (nd_normalize_reads / nd_window_reads),
        bit-identical to the host front end.  Chunks keep the span of their
        reference batch (``batch_size`` consecutive chunks of one read), so
        results equal per-read translate() on the host front end's chunks.
        Yields (read index, per-chunk results) as stream_reads does; with
        ``arrays`` (greedy and sampling only) (read index, tokens [n_chunks,
        max_length] int32, scores [n_chunks] float32) instead.  ``qualities``
        as in stream_reads; with ``arrays`` a fourth array follows, the
        tokens' weights [n_chunks, max_length] uint16 (one per token, EOS and
        what follows it included).  ``mods`` as in stream_reads; with
        ``arrays`` a fifth array, the tokens' modification weights, laid out
        like the fourth.  ``moves`` as in stream_reads; with ``arrays`` a last
        array follows, the tokens' positions [n_chunks, max_length] int32."""
        if arrays and self.beam_size != 1:
            raise ValueError("arrays=True is for greedy / sampling decoding")
        req = self._request(False, qualities, mods, moves)
        for ri, res in self._stream_raw_reads(raws, batch_size, normalization, src_seq_length, src_seq_stride,
                                              arrays, req):
            yield (ri,) + res if arrays else (ri, res)

    def _stream_raw_reads(self, raws, batch_size: int, normalization: str, src_seq_length: int, src_seq_stride: int,
                          arrays: bool, req: Request):
        from . import frontend
        S = self.max_length
        per_token = req.asked((np.uint16, (S,)), (np.uint16, (S,)), (np.int32, (S,)))
        columns = ((np.int32, (S,)), (np.float32, ())) + per_token  # tokens and scores first

        def holder(n):  # a read's n chunk results: a list, or with ``arrays`` one [n, ...] array per column
            return tuple(np.empty((n,) + shape, dtype) for dtype, shape in columns) if arrays else [None] * n

        def describe(raw):
            raw = np.asarray(raw, dtype=np.float64).reshape(-1)
            wins = frontend.windows(int(raw.size), src_seq_length, src_seq_stride) if raw.size else []
            return holder(len(wins)), [((raw, st), ln) for st, ln in wins]

        def submit(items):
            return self._submit_raw(items, normalization, req)

        def store(job, items, results):
            if not arrays:
                for it, o in zip(items, self._finish(job)):
                    results[it[0]][it[1]] = o
                return
            cols = self._finish(job, arrays=True)
            for i, it in enumerate(items):
                for dst, a in zip(results[it[0]], cols):
                    dst[it[1]] = a[i]

        return self._stream(raws, batch_size, describe, submit, store)

    def translate_batch(self, batch, data=None, attn_debug=False, fast=False):
        """translate/translator.py:505-540 on a batch object with
        src [T, B, 1], src_lengths [B] (reference batch layout).  Returns the
        reference's results dict; predictions are token-id tensors (greedy:
        all max_length tokens; beam: through EOS), scores floats."""
        src = batch.src[0] if isinstance(batch.src, tuple) else batch.src
        src = src.detach().to(torch.float32).cpu()
        T, B = src.shape[0], src.shape[1]
        lens = batch.src_lengths.detach().cpu().numpy().astype(np.int32)
        chunks = [src[: lens[i], i, 0].numpy() for i in range(B)]
        saved, self.fast = self.fast, bool(fast)  # translator.py:523-540 dispatches on the argument
        try:
            if self.beam_size > 1:
                self._check_supported()
            # return_attention (:521-529); the classic Beam always keeps its attention (:902-924)
            want = bool(attn_debug or self.replace_unk) or (self.beam_size > 1 and not self.fast)
            outs = self._run(chunks, [T] * B, attn=want)
        finally:
            self.fast = saved
        att = [[torch.from_numpy(np.ascontiguousarray(a)) for a in o[2]] if want else [[]] * len(o[0])
               for o in outs]
        return {"predictions": [[torch.tensor(t, dtype=torch.long) for t in o[1]] for o in outs],
                "scores": [list(o[0]) for o in outs], "attention": att,
                "gold_score": [0] * B, "batch": batch}
