"""Shared by the op-level search tests (test_search_scheme.py on the CPU, test_gpu_search_ops.py on the GPU):
a scripted model that replaces the decoder by a table, the fp64 references of the output head, and the Python
restatement of the sampling draw.  No GPU code here.

The scripted model.  The decoder's output rows of step s for a row of chunk c whose last token is t (BOS at
step 0) are X[c][s][t], a fixed 256-vector, so a search step's input depends on (chunk, step, last token) only.
The device side gathers those rows and calls the step entry; the reference side runs oracle/ref_cpu.py's
searches, unchanged, on `Stub`, whose decode_step returns LP[c][s][t] (and ATT[c][s][t] as the attention).  LP
is the device head's own fp32 log-probs of the X rows (one greedy-head launch with the dump), so both sides
start from bit-identical numbers; on the CPU (seed selection, the scheme tests) LP is the fp64 head rounded to
fp32.

Ties.  torch.topk leaves the order among equal values unspecified; the kernels' documented rule is the lower
flat index.  `pinned_topk` replaces Tensor.topk during a reference run by a stable descending sort (identical
wherever the values differ) and records, for every selection, the gaps between consecutive values down to the
first one not selected: each must be exactly 0 (a tie, built on purpose) or above the margin, else the run
raises: no case is exempt.
"""
import contextlib
import math

import numpy as np
import torch

from oracle import ref_cpu

D = 256
LN_EPS = 1e-6
TIE_MARGIN = 1e-4   # the suite's constant (test_gpu_parity.py)
SEED_MARGIN = 1e-3  # seeds are picked on the CPU with this gap, so the GPU head's rounding cannot close it


# ------------------------------------------------------------------ the head
def head_fp64(x, ln_g, ln_b, gw, gb):
    """LayerNorm (eps 1e-6) -> generator -> log_softmax in float64: [R, V]."""
    f = lambda a: np.asarray(a, np.float64)
    x, ln_g, ln_b, gw, gb = map(f, (x, ln_g, ln_b, gw, gb))
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    z = ((x - mu) / np.sqrt(var + LN_EPS) * ln_g + ln_b) @ gw.T + gb
    m = z.max(-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(-1, keepdims=True))


def head_fp32(x, ln_g, ln_b, gw, gb):
    """The same operation materialised in fp32 by torch on the CPU (the reference model's own arithmetic)."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    x, ln_g, ln_b, gw, gb = map(t, (x, ln_g, ln_b, gw, gb))
    y = torch.nn.functional.layer_norm(x, (D,), ln_g, ln_b, LN_EPS)
    return torch.log_softmax(torch.nn.functional.linear(y, gw, gb), -1).numpy()


def sinusoid_pe(S, d=D):
    """embeddings.py:36-43"""
    pe = np.zeros((S, d))
    pos = np.arange(S)[:, None]
    div = np.exp(np.arange(0, d, 2) * -(math.log(10000.0) / d))
    pe[:, 0::2], pe[:, 1::2] = np.sin(pos * div), np.cos(pos * div)
    return pe.astype(np.float32)


def embed_ref(emb, pe, tok, step_next):
    """fp32 emb[tok] * 16 + pe[step_next] (one rounding: the product is exact), or emb[tok] without pe."""
    e = np.asarray(emb, np.float32)[tok]
    return e if pe is None else (e * np.float32(16.0) + np.asarray(pe, np.float32)[step_next]).astype(np.float32)


def row_stats(e, dtype):
    """{mean, M2} of rows by the two-pass formula in `dtype`."""
    e = np.asarray(e, dtype)
    mu = e.sum(-1, dtype=dtype) / dtype(D)
    d = e - mu[..., None]
    return mu, (d * d).sum(-1, dtype=dtype)


# ------------------------------------------------------------------ sampling
M64 = (1 << 64) - 1


def draw_uniform(seed, row, step):
    """head.hpp draw_uniform in Python integers: the splitmix64 finaliser of seed + golden * ((row << 32) + step
    + 1), its top 24 bits as a float in [0, 1)."""
    ctr = ((row << 32) + (step & 0xFFFFFFFF) + 1) & M64
    z = (seed + 0x9E3779B97F4A7C15 * ctr) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z >> 40) / 16777216.0


def draw_uniform_rows(seed, R, step):
    """draw_uniform for rows 0..R-1, vectorised (uint64 arithmetic wraps like the device's)."""
    with np.errstate(over="ignore"):
        ctr = (np.arange(R, dtype=np.uint64) << np.uint64(32)) + np.uint64((step & 0xFFFFFFFF) + 1)
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * ctr
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(40)).astype(np.float64) / 16777216.0


def sample_ref(lp, temp, topk, u, eos=None):
    """The inverse-CDF pick in float64 for one row of fp32 log-probs lp (EOS masked to -1e20 when eos is given)
    and draws u [R]: l = fp32(lp) / fp32(temp) (the returned score, bitwise); with topk > 0 the tokens below the
    k-th largest l drop out (ties at it are kept); pick = the first k with u * sum < cdf[k].  Returns (pick [R],
    l [V] fp32, kept [V] bool, margin [R]: each draw's distance to the nearest CDF boundary over the sum)."""
    lp = np.asarray(lp, np.float32).copy()
    if eos is not None:
        lp[eos] = np.float32(-1e20)
    l = (lp / np.float32(temp)).astype(np.float32)
    kept = np.ones(l.size, bool)
    if topk > 0:
        kept = l >= np.sort(l)[::-1][topk - 1]
    p = np.where(kept, np.exp(l.astype(np.float64) - float(l.max())), 0.0)
    cdf = np.cumsum(p)
    target = np.asarray(u, np.float64) * cdf[-1]
    pick = np.minimum((target[:, None] >= cdf[None, :]).sum(1), l.size - 1)
    inner = np.unique(cdf[:-1])
    margin = np.abs(target[:, None] - inner[None, :]).min(1) / cdf[-1] if inner.size else np.ones(target.size)
    return pick.astype(np.int32), l, kept, margin


# ------------------------------------------------------------------ the scripted model
class Script:
    """Tables and head weights of one scripted run (numpy, fp32).

    C chunks, S steps, V tokens; X [C, S, V, 256]; ATT [C, S, V, T] (rows of probabilities) when T > 0.
    dup: pairs (a, b) of tokens made indistinguishable: generator row and bias of b copied from a (bit-equal
    logits), X and ATT rows of last token b copied from a's (two beams ending in a and b get equal rows).
    eos_bias / boost: generator bias of EOS, and of the listed tokens.  spread scales the logits."""

    def __init__(self, C, S, V, seed, T=0, eos=3, bos=2, dup=(), eos_bias=0.0, boost=(), spread=0.3, pe=True):
        rng = np.random.default_rng(seed)
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        self.C, self.S, self.V, self.T, self.eos, self.bos, self.seed = C, S, V, T, eos, bos, seed
        self.ln_g = f(1.0 + 0.1 * rng.standard_normal(D))
        self.ln_b = f(0.1 * rng.standard_normal(D))
        self.gw = f(rng.standard_normal((V, D)) * spread)
        self.gb = f(rng.standard_normal(V) * 0.1)
        if V > eos:
            self.gb[eos] += np.float32(eos_bias)
        for t, b in boost:
            self.gb[t] += np.float32(b)
        self.emb = f(rng.standard_normal((V, D)) * 0.5)
        self.pe = sinusoid_pe(S + 1) if pe else None
        self.X = f(rng.standard_normal((C, S, V, D)))
        att = rng.standard_normal((C, S, V, max(T, 1))) * 1.5
        att[..., 0] += 4.0  # key 0 draws about half of every row: its coverage passes 1 after a few steps
        att = np.exp(att - att.max(-1, keepdims=True))
        self.ATT = f(att / att.sum(-1, keepdims=True))
        for a, b in dup:
            self.gw[b], self.gb[b] = self.gw[a], self.gb[a]
            self.X[:, :, b], self.ATT[:, :, b] = self.X[:, :, a], self.ATT[:, :, a]
        self.LP = None

    def head(self):
        return dict(ln_g=self.ln_g, ln_b=self.ln_b, gw=self.gw, gb=self.gb)

    def cpu_lp(self):
        """LP from the fp64 head, rounded to fp32: [C, S, V, V]"""
        C, S, V = self.C, self.S, self.V
        return head_fp64(self.X.reshape(-1, D), **self.head()).astype(np.float32).reshape(C, S, V, V)


class Stub:
    """What ref_cpu's searches ask of a model, answered from a Script's tables.  `src` carries the chunk ids
    ([B, 1] float), which travel through tile and reorder with their rows.  Records, per decode_step, the
    chunk of every row, and per reorder the selected parent rows."""

    def __init__(self, script, lp):
        self.s = script
        self.cfg = type("Cfg", (), dict(vocab=script.V, bos_idx=script.bos, eos_idx=script.eos, pad_idx=0,
                                        encoder_type="stub"))()
        self.lp = torch.as_tensor(np.asarray(lp, np.float32))
        self.att = torch.as_tensor(script.ATT)
        self.steps = []     # per decode_step: chunk id of each row
        self.toks = []      # per decode_step: input token of each row
        self.selects = []   # per reorder: (chunk of each row before, idx)

    def encode(self, src, lengths):
        return src[:, :1].clone()

    def decoder_state(self, memory, src, n_rows_per_chunk=1, max_len=100):
        return {"chunk": memory.reshape(-1).long()}

    def decode_step(self, st, tok, step):
        c = st["chunk"]
        self.steps.append(c.numpy().copy())
        self.toks.append(tok.numpy().copy())
        st["attn"] = self.att[c, step, tok].clone()
        return self.lp[c, step, tok].clone()

    def reorder(self, st, idx):
        self.selects.append((st["chunk"].numpy().copy(), idx.numpy().copy()))
        st["chunk"] = st["chunk"].index_select(0, idx)


def chunk_src(chunks):
    return np.asarray(chunks, np.float32).reshape(-1, 1)


class TieError(AssertionError):
    pass


class TieLog:
    def __init__(self, margin):
        self.margin, self.ties, self.selections, self.min_gap = margin, 0, 0, math.inf
        self.slots = set()  # flat index >> 6 of the selected finite candidates (the top-k kernels' 64-lane slots)
        self.groups = []  # the flat indices of every maximal run of exactly tied finite values, in rank order
        self.pairs = []  # (flat index of the higher-ranked, of the lower-ranked) of every exact tie among finite values

    def see(self, v, i, k):
        """v, i: values sorted descending along the last dim and their indices; the first k are selected."""
        n = v.shape[-1]
        m = min(k, n - 1)
        hi, lo = v[..., :m], v[..., 1: m + 1]
        tie = hi == lo
        gap = (hi.double() - lo.double())[~tie]
        self.selections += 1
        self.ties += int(tie.sum())
        self.slots |= set((i[..., :k][v[..., :k] > -1e19] >> 6).unique().tolist())
        fin = tie & (hi > -1e19)
        self.pairs += list(zip(i[..., :m][fin].tolist(), i[..., 1: m + 1][fin].tolist()))
        for row_t, row_i in zip(fin.reshape(-1, m).tolist(), i.reshape(-1, n).tolist()):  # maximal runs of ties
            run = []
            for j, t in enumerate(row_t + [False]):
                if t:
                    run = run or [row_i[j]]
                    run.append(row_i[j + 1])
                elif run:
                    self.groups.append(run)
                    run = []
        if gap.numel():
            g = float(gap.min())
            self.min_gap = min(self.min_gap, g)
            if not g > self.margin:
                raise TieError(f"a selection separated by {g:.3e} <= {self.margin:.0e} that is no exact tie")


@contextlib.contextmanager
def pinned_topk(margin=TIE_MARGIN):
    """Tensor.topk as a stable descending sort (ties -> lower index), every selection checked by a TieLog."""
    log = TieLog(margin)
    real = torch.Tensor.topk

    def topk(self, k, dim=-1, largest=True, sorted=True):
        assert largest and sorted
        v, i = torch.sort(self, dim=dim, descending=True, stable=True)
        log.see(v.movedim(dim, -1), i.movedim(dim, -1), k)
        v, i = v.narrow(dim, 0, k), i.narrow(dim, 0, k)
        rv, ri = real(self, k, dim, largest, sorted)
        assert torch.equal(rv, v)  # the values never depend on the tie rule
        return v, i

    torch.Tensor.topk = topk
    try:
        yield log
    finally:
        torch.Tensor.topk = real


def ref_fast_beam(script, lp, beam, n_best, alpha, min_len, margin=TIE_MARGIN):
    """ref_cpu.fast_beam on the stub over chunks 0..C-1 -> (results per chunk, stub, tie log).  stub.hyp_counts:
    the scores of each finished chunk's hypothesis list, in arrival order, when it was sorted (the module's `sorted`
    is watched, not changed), in the order the chunks finished."""
    stub = Stub(script, lp)
    stub.hyp_scores = []

    def watching_sorted(it, **kw):
        stub.hyp_scores.append([h[0] for h in it])
        return sorted(it, **kw)

    ref_cpu.sorted = watching_sorted
    try:
        with pinned_topk(margin) as log:
            res = ref_cpu.fast_beam(stub, chunk_src(range(script.C)), np.ones(script.C, np.int64), beam_size=beam,
                                    n_best=n_best, max_length=script.S, min_length=min_len, alpha=alpha)
    finally:
        del ref_cpu.sorted
    return res, stub, log


def fast_props(script, res, stub, log, beam, n_best):
    """What a scripted --fast run exercised, from the reference run alone."""
    tr = fast_trace(stub, script.C, beam, script.S)
    order = [c for s, t in enumerate(tr) for c in t["alive"] if c not in t["after"]]
    n_hyp = np.zeros(script.C, np.int64)
    n_hyp[order] = [len(h) for h in stub.hyp_scores]
    evictions = drops = 0  # arrivals at a full list that displace an entry / that are worse than every entry
    for h in stub.hyp_scores:
        for i in range(n_best, len(h)):
            worst = sorted(h[:i], reverse=True)[n_best - 1]
            evictions += h[i] > worst
            drops += h[i] <= worst
    steps_run = tr[-1]["steps_run"]
    V = script.V
    return dict(
        trace=tr, steps=len(tr), steps_run=steps_run, n_hyp=n_hyp, evictions=evictions, drops=drops, slots=log.slots,
        # the best hypothesis is shorter than the chunk's run: it finished while the top beam had not
        other_first=[c for c in range(script.C) if len(res[c][0][1]) < steps_run[c]],
        equal_scores=[c for c in range(script.C) for a, b in zip(res[c], res[c][1:])
                      if a[0] == b[0] and not np.array_equal(a[1], b[1])],
        cross_beam_ties=sum(1 for a, b in log.pairs if a // V != b // V),
        in_beam_ties=sum(1 for a, b in log.pairs if a // V == b // V and a != b),
        # two tied candidates that one lane of the top-k kernels holds (flat indices 64 apart)
        same_lane_ties=sum(1 for g in log.groups for a in g for b in g if a < b and (b - a) % 64 == 0))


def fast_trace(stub, C, beam, S):
    """Per step of a ref_cpu.fast_beam run on chunks 0..C-1: alive[s] = chunks decoded at step s; after[s] =
    chunks still alive after step s; done / steps_run / n_alive as the device keeps them after step s; anc[s] =
    {new global row: parent global row} of the step's reorder (alive chunks only)."""
    n = len(stub.steps)
    alive = [sorted(set(c.tolist())) for c in stub.steps]
    out = []
    steps_run = np.zeros(C, np.int32)
    for s in range(n):
        after = alive[s + 1] if s + 1 < n else []
        for c in alive[s]:
            if c not in after:
                steps_run[c] = s + 1
        done = np.array([0 if c in after else 1 for c in range(C)], np.int32)
        anc = {}
        if s < len(stub.selects):
            chunk, idx = stub.selects[s]
            for p, i in enumerate(idx.tolist()):
                anc[int(chunk[i]) * beam + p % beam] = int(chunk[i]) * beam + i % beam
        tok = {}  # global row -> the token it feeds the next step
        if s + 1 < n:
            for p, (c, t) in enumerate(zip(stub.steps[s + 1].tolist(), stub.toks[s + 1].tolist())):
                tok[c * beam + p % beam] = t
        out.append(dict(alive=alive[s], after=after, done=done, steps_run=steps_run.copy(), n_alive=len(after),
                        anc=anc, tok=tok))
    return out


class RecBeam(ref_cpu.ClassicBeam):
    """ClassicBeam that registers itself and logs, after every advance, done() and its best finished score."""
    made = []

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.log = []
        self.blocked = 0
        RecBeam.made.append(self)

    def _blocked(self, j):
        r = super()._blocked(j)
        self.blocked += bool(r)
        return r

    def advance(self, word_probs, attn_out):
        super().advance(word_probs, attn_out)
        self.log.append((self.done(), max((f[0] for f in self.finished), default=-math.inf), len(self.finished)))


LP_KIND = {"none": 0, "wu": 1, "avg": 2}
COV_KIND = {"none": 0, "wu": 1, "summary": 2}


def ref_classic_beam(script, lp, groups, beam, n_best, min_len, opts, lengths, margin=TIE_MARGIN):
    """ref_cpu.classic_beam on the stub, one call per group (a reference batch: a list of chunk ids).
    opts: ref_cpu.classic_beam's keyword options; lengths [C]: each chunk's source length (the attention cut of
    chunk j of a batch is lengths[batch[j // beam]], translator.py:902-907).  Returns (results per chunk, the
    RecBeam of every chunk, cut per chunk, tie log)."""
    res, beams, cut = {}, {}, {}
    orig = ref_cpu.ClassicBeam
    ref_cpu.ClassicBeam = RecBeam
    try:
        with pinned_topk(margin) as log:
            for g in groups:
                RecBeam.made = []
                stub = Stub(script, lp)
                out = ref_cpu.classic_beam(stub, chunk_src(g), np.asarray([lengths[c] for c in g], np.int64),
                                           beam_size=beam, n_best=n_best, max_length=script.S, min_length=min_len,
                                           **opts)
                for j, c in enumerate(g):
                    res[c], beams[c], cut[c] = out[j], RecBeam.made[j], int(lengths[g[j // beam]])
    finally:
        ref_cpu.ClassicBeam = orig
    return res, beams, cut, log


def ulp32(x):
    return float(np.spacing(np.abs(np.float32(x))))


# ------------------------------------------------------------------ the cases
# Seeds picked on the CPU (fp64 head, SEED_MARGIN) by trying 0, 1, 2, ... until the run keeps the margin and
# shows what its case is about (fast_props / classic_props); test_search_scheme.py re-checks every one.
B2 = ((5, 2.0), (6, 2.0))
FAST_GRID = [(2, 6), (5, 9), (8, 9), (4, 32), (8, 32)]
FAST_GRID_SEEDS = {(2, 6, 0.0, 0): 0, (2, 6, 0.0, 3): 0, (2, 6, 0.6, 0): 0, (2, 6, 0.6, 3): 0, (5, 9, 0.0, 0): 0,
                   (5, 9, 0.0, 3): 0, (5, 9, 0.6, 0): 0, (5, 9, 0.6, 3): 0, (8, 9, 0.0, 0): 1, (8, 9, 0.0, 3): 1,
                   (8, 9, 0.6, 0): 3, (8, 9, 0.6, 3): 3, (4, 32, 0.0, 0): 1, (4, 32, 0.0, 3): 5, (4, 32, 0.6, 0): 1,
                   (4, 32, 0.6, 3): 5, (8, 32, 0.0, 0): 1, (8, 32, 0.0, 3): 16, (8, 32, 0.6, 0): 1,
                   (8, 32, 0.6, 3): 16}


def fast_grid_script(beam, V, alpha, min_len):
    C, S = (2, 6) if V == 32 else (3, 8)
    return Script(C, S, V, FAST_GRID_SEEDS[(beam, V, alpha, min_len)], eos_bias=1.5 if V == 32 else 0.5)


# name: (Script arguments, beam, n_best, alpha, min_len, what the reference run must show)
FAST_SCENARIOS = {
    "ties": (dict(C=3, S=8, V=9, seed=0, dup=((5, 6),), boost=B2, eos_bias=0.5), 5, 2, 0.0, 0,
             lambda p, res, S: p["cross_beam_ties"] > 0 and p["in_beam_ties"] > 0 and p["steps"] >= 4),
    "other_beam_first": (dict(C=3, S=8, V=9, seed=5, eos_bias=0.0), 5, 1, 0.0, 0,
                         lambda p, res, S: len(p["other_first"]) >= 2),
    "evict_equal_scores": (dict(C=3, S=8, V=9, seed=1, dup=((5, 6),), boost=B2, eos_bias=1.0), 5, 2, 0.6, 0,
                           lambda p, res, S: p["equal_scores"] and p["evictions"] > 0 and p["drops"] > 0),
    "no_eos": (dict(C=2, S=6, V=9, seed=0, eos_bias=-1e4), 5, 2, 0.6, 0,
               lambda p, res, S: p["steps"] == S and all(len(h[1]) == S for r in res for h in r)),
    "one_step": (dict(C=3, S=1, V=9, seed=0), 5, 2, 0.0, 0, lambda p, res, S: p["steps"] == 1),
    "different_steps": (dict(C=4, S=8, V=9, seed=0, eos_bias=0.5), 5, 2, 0.6, 0,
                        lambda p, res, S: len(set(p["steps_run"].tolist())) >= 3 and p["steps"] >= 5),
    "ties_in_one_lane": (dict(C=2, S=6, V=32, seed=0, dup=((5, 6), (5, 7)),
                              boost=((5, 2.0), (6, 2.0), (7, 2.0)), eos_bias=1.5), 4, 2, 0.6, 0,
                         lambda p, res, S: p["same_lane_ties"] > 0 and p["steps"] >= 3),
    "all_256_candidates": (dict(C=2, S=6, V=32, seed=0, eos_bias=1.5), 8, 8, 0.6, 0,
                           lambda p, res, S: p["slots"] >= {0, 1, 2, 3}),
}


def classic_cases():
    """name -> dict(script, groups, beam, n_best, min_len, opts, lengths, need)"""
    import itertools
    cases = {}

    def add(name, beam=5, V=9, n_best=2, min_len=0, T=0, eos_bias=0.5, S=8, need=None, extra=None, **opts):
        big = V == 32
        C, groups = (3, [[0], [1, 2]]) if big else (5, [[0, 1], [2, 3, 4]])
        lengths = [max(T - 1, 0) if c in groups[0] else T // 2 for c in range(C)] if T else [1] * C
        cases[name] = dict(script=dict(C=C, S=6 if big else S, V=V, T=T, eos_bias=1.5 if big else eos_bias,
                                       **(extra or {})),
                           groups=groups, beam=beam, n_best=n_best, min_len=min_len, opts=opts, lengths=lengths,
                           need=need)

    for lp in ("none", "wu", "avg"):
        for beam, V in ((5, 9), (8, 32)):
            add(f"lp_{lp}_{beam}x{V}", beam, V, need="groups_differ", length_penalty=lp, alpha=0.6)
    for i, (cov, sw, T) in enumerate(itertools.product(("wu", "summary"), (False, True), (1, 64, 65, 130))):
        add(f"cov_{cov}_{'stepwise' if sw else 'scoring'}_T{T}", T=T, coverage_penalty=cov, stepwise_penalty=sw,
            beta=0.1, length_penalty=("none", "wu", "avg")[i % 3], alpha=0.6, need="cov_matters" if T > 1 else None)
    for n in (1, 2, 3):
        for ex in ((), (4, 5)):
            add(f"ngram{n}_{'excl' if ex else 'all'}", S=10, eos_bias=-1.0, need="blocked", block_ngram_repeat=n,
                exclusion_tokens=ex)
    add("min_len", min_len=3, eos_bias=1.5, need="masked")
    add("top_up", n_best=5, eos_bias=-2.0, need="top_up")
    add("late_better", n_best=1, need="late_better", length_penalty="avg")
    add("ties", need="ties", extra=dict(dup=((5, 6),), boost=B2), length_penalty="wu", alpha=0.6)
    add("ties_in_one_lane", beam=4, V=32, need="same_lane_ties", length_penalty="wu", alpha=0.6,
        extra=dict(dup=((5, 6), (5, 7)), boost=((5, 2.0), (6, 2.0), (7, 2.0))))
    add("three_groups_of_one", need="groups_differ")
    cases["three_groups_of_one"]["groups"] = [[0], [1, 2, 3], [4]]
    return cases


CLASSIC_SEEDS = {"lp_none_8x32": 3, "lp_wu_8x32": 3, "lp_avg_8x32": 3, "cov_wu_scoring_T130": 2,
                 "cov_wu_stepwise_T65": 1, "cov_summary_stepwise_T64": 1, "cov_summary_stepwise_T65": 1,
                 "ngram1_excl": 1, "ngram2_all": 1, "ngram3_all": 3, "ngram3_excl": 3, "min_len": 2, "top_up": 1,
                 "late_better": 6, "ties_in_one_lane": 3}  # every other case: seed 0


def classic_case(name):
    k = classic_cases()[name]
    return Script(seed=CLASSIC_SEEDS.get(name, 0), **k["script"]), k


def same_tokens(a, b):
    """two result lists of one chunk: equal lengths and token arrays"""
    return len(a) == len(b) and all(np.array_equal(p[1], q[1]) for p, q in zip(a, b))


def classic_props(res, beams, groups):
    """What a scripted classic run exercised, from the reference's beams."""
    late = []
    for c, b in beams.items():
        first = next((i for i, e in enumerate(b.log) if e[0]), None)
        if first is not None and first < len(b.log) - 1 and b.log[-1][1] > b.log[first][1]:
            late.append(c)
    steps = {c: len(b.prev_ks) for c, b in beams.items()}
    return dict(steps_run=steps, late_better=late, blocked=sum(b.blocked for b in beams.values()),
                top_up=[c for c, b in beams.items() if b.log[-1][2] < b.n_best],
                groups_differ=len({steps[g[0]] for g in groups}) > 1,
                sibling_continues=[c for c, b in beams.items() if any(e[0] for e in b.log[:-1])])


def classic_need(script, lp, k, res, beams, log):
    """Asserts that the reference run of a classic case shows what the case is about; returns classic_props."""
    p = classic_props(res, beams, k["groups"])
    V = script.V
    p["same_lane_ties"] = sum(1 for g in log.groups for a in g for b in g if a < b and (b - a) % 64 == 0)
    p["ties"] = (any(a // V != b // V for a, b in log.pairs) and any(a // V == b // V for a, b in log.pairs)
                 and any(a[0] == b[0] and not np.array_equal(a[1], b[1]) for r in res.values() for a, b in zip(r, r[1:])))
    assert max(p["steps_run"].values()) >= 3 and p["sibling_continues"], p
    rerun = lambda min_len, opts: ref_classic_beam(script, lp, k["groups"], k["beam"], k["n_best"], min_len, opts,
                                                   k["lengths"], margin=0)[0]
    if k["need"] == "masked":
        r0 = rerun(0, k["opts"])
        assert any(not same_tokens(res[c], r0[c]) for c in res)
    elif k["need"] == "cov_matters":
        r0 = rerun(k["min_len"], dict(k["opts"], coverage_penalty="none"))
        assert max(abs(a[0] - b[0]) for c in res for a, b in zip(res[c], r0[c])) > 0.01
    elif k["need"]:
        assert p[k["need"]], (k["need"], p)
    return p


# ------------------------------------------------------------------ sampling cases
SAMPLE_R = 4096
SAMPLE_EOS = 3
# (temp, topk, step) -> the draw's seed: the first from 1 up whose 4096 draws all stay 1e-4 of the sum away from
# every CDF boundary of the row below (fp64 head); the test asserts 1e-5 on the device's log-probs
SAMPLE_SEEDS = {(1.0, -1, 0): 74, (1.0, -1, 5): 2, (0.7, 2, 0): 11, (0.7, 2, 5): 14, (1.5, 3, 0): 20,
                (1.5, 3, 5): 8, (1.0, 6, 0): 74, (1.0, 6, 5): 2}
SAMPLE_TIE = dict(script=1, dup=(1, 4), topk=2, step=2, seed=7)        # tokens 1 and 4 tie at ranks 2 and 3
SAMPLE_TIE_IN = dict(script=0, dup=(1, 4), topk=3, step=2, seed=3)     # tokens 1 and 4 tie at ranks 1 and 2
SAMPLE_MIN_LEN = dict(min_len=3, seeds={1: 80, 4: 140})                 # step -> seed; EOS is a likely token


def sampling_script(kind="plain"):
    """One row (X[0, 0, 0]) and a V = 6 head with a flat enough distribution that every token is drawn."""
    if kind in ("tie", "tie_in"):
        t = SAMPLE_TIE if kind == "tie" else SAMPLE_TIE_IN
        return Script(1, 1, 6, t["script"], dup=(t["dup"],), spread=0.1)
    return Script(1, 1, 6, 0, spread=0.1, eos_bias=1.5 if kind == "min_len" else 0.0)
