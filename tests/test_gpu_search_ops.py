"""The output head and the search kernels (csrc/search.hip, csrc/head.hpp), op by op, needs an MI355X.

Head, embedding and attention softmax against fp64; argmax, sampling, the --fast beam and the classic Beam
against oracle/ref_cpu.py's own searches run on the scripted model of tests/search_util.py, whose log-probs are
the device head's (one greedy-head launch over the table rows), so both searches start from the same bits.

Bounds.  fp64 comparisons: a case's max error stays within 4 E32, E32 the max error against fp64 of the same
operation materialised in fp32 on the CPU (test_gpu_enc_layer0.py's rule; measured ratios: DESIGN.md section
4); log-probs also within golden_util.logp_close.  Searches: tokens, lengths, order and every state field exact;
--fast scores within 1 ulp of the reference's fp32, classic scores within 1e-3 + 1e-5 rel
(test_beam_options_vs_golden's).  Every selection of a reference run is an exact tie or wider than TIE_MARGIN,
or the test fails (search_util.pinned_topk).
"""
import numpy as np
import pytest
import torch

from nanodecoder_amd import _lib
from tests import golden_util as gu
from tests import search_util as U

pytestmark = pytest.mark.gpu

FILL = -7.25


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(_dev())


def _head(w, emb, pe):
    from nanodecoder_amd.engine import SearchHead
    return SearchHead(w["ln_g"], w["ln_b"], w["gw"], w["gb"], emb, pe, device=_dev())


def _script_head(sc, S=None):
    """S: the steps the test runs when they are more than the script's (the position table must cover them)"""
    return _head(sc.head(), sc.emb, sc.pe if S is None else U.sinusoid_pe(S + 1))


def _greedy(head, x, step, S, min_len, eos, **kw):
    from nanodecoder_amd.engine import op_greedy_head
    out, ne = op_greedy_head(head, _t(x) if isinstance(x, np.ndarray) else x, step, S, min_len, eos, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, ne


_LP = {}


def _device_lp(sc, key):
    """The device head's log-probs of every table row [C, S, V, V], one launch, computed once per script."""
    if key not in _LP:
        out, _ = _greedy(_script_head(sc), sc.X.reshape(-1, U.D), 0, 1, 0, sc.eos)
        _LP[key] = out["logp"].reshape(sc.C, sc.S, sc.V, sc.V).copy()
    return _LP[key]


# ================================================================= head vs fp64
HEAD_KINDS = ("normal", "mean100", "constant", "spread50", "specials")


def _head_case(V, R, kind):
    rng = np.random.default_rng(1000 * V + 10 * R + HEAD_KINDS.index(kind))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    w = dict(ln_g=f(1.0 + 0.1 * rng.standard_normal(U.D)), ln_b=f(0.1 * rng.standard_normal(U.D)),
             gw=f(rng.standard_normal((V, U.D)) / 16.0), gb=f(0.1 * rng.standard_normal(V)))
    x = rng.standard_normal((R, U.D))
    if kind == "mean100":
        x += 100.0
    elif kind == "constant":  # zero variance: the row normalises to ln_b
        x = np.repeat(rng.standard_normal((R, 1)) * 3.0, U.D, axis=1)
    elif kind == "spread50":  # logits of standard deviation 12.8: about 50 between the extremes
        w["gw"] = f(w["gw"] * 12.8)
    elif kind == "specials":  # synth's generator: the specials biased by -1e4
        w["gb"][: max(1, min(3, V - 1))] = -1e4
    return w, f(x)


@pytest.mark.parametrize("kind", HEAD_KINDS)
@pytest.mark.parametrize("R", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("V", [1, 6, 8, 9, 17, 32])
def test_head_vs_fp64(V, R, kind):
    w, x = _head_case(V, R, kind)
    emb = np.zeros((V, U.D), np.float32)
    out, _ = _greedy(_head(w, emb, None), x, 0, 1, 0, 0)
    got = out["logp"].reshape(R, V).astype(np.float64)
    ref = U.head_fp64(x, **w)
    e32 = np.abs(U.head_fp32(x, **w).astype(np.float64) - ref).max()
    err = np.abs(got - ref).max()
    print(f"head V={V} R={R} {kind}: E32 {e32:.3e} err {err:.3e} err/E32 {err / e32 if e32 else 0.0:.3f}")
    assert np.isfinite(got).all()
    assert gu.logp_close(got, ref).all(), (err, e32)
    assert err <= 4.0 * e32, (err, e32)


def test_head_is_deterministic_across_row_positions():
    """One row at several positions (other waves, other workgroups, another launch size): bit-equal log-probs.
    The scripted model's tables depend on it."""
    w, x = _head_case(17, 9, "normal")
    x[[1, 4, 6]] = x[0]
    head = _head(w, np.zeros((17, U.D), np.float32), None)
    a = _greedy(head, x, 0, 1, 0, 0)[0]["logp"].reshape(9, 17)
    b = _greedy(head, x[:1], 0, 1, 0, 0)[0]["logp"].reshape(1, 17)
    for r in (1, 4, 6):
        assert gu.same_f32(a[r], a[0])
    assert gu.same_f32(b[0], a[0])


# ================================================================= embed_row
def _forcing_head(V, rng):
    """A head (identity LayerNorm) and rows x[r] whose argmax is tok[r]: row r is tok[r]'s generator row, far
    ahead of the others' nearly orthogonal ones."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    w = dict(ln_g=np.ones(U.D, np.float32), ln_b=np.zeros(U.D, np.float32),
             gw=f(rng.standard_normal((V, U.D)) / 4.0), gb=np.zeros(V, np.float32))
    return w, lambda tok: f(w["gw"][tok] * 8.0)


@pytest.mark.parametrize("with_pe", [True, False])
def test_embed_row(with_pe):
    """Every token of a V = 17 vocabulary once (0, 7: the last preloaded row, 8: the first dependent load,
    V - 1), one row each, over two workgroups' worth of rows and a ragged third."""
    from nanodecoder_amd.engine import NextRows
    V, S, step = 17, 6, 2
    rng = np.random.default_rng(40)
    tok = rng.permutation(V)
    R = V
    assert {0, 7, 8, V - 1} <= set(tok.tolist())
    emb = (rng.standard_normal((V, U.D)) * 0.5).astype(np.float32)
    pe = U.sinusoid_pe(S + 1) if with_pe else None
    w, rows = _forcing_head(V, rng)
    ne = NextRows(R, _dev(), fill=FILL)
    out, ne = _greedy(_head(w, emb, pe), rows(tok), step, S, 0, 1, ne=ne)
    assert (out["tok"] == tok).all()
    want = U.embed_ref(emb, pe, tok, step + 1)
    assert gu.same_f32(ne.rows().cpu().numpy(), want)
    assert (ne.tok.cpu().numpy()[:R] == tok).all() and (ne.tok.cpu().numpy()[R:] == -1).all()
    part = ne.part.cpu().numpy()
    mu64, q64 = U.row_stats(want, np.float64)
    mu32, q32 = U.row_stats(want, np.float32)
    for name, got, r64, r32 in (("mean", part[:R, 0, 0], mu64, mu32), ("M2", part[:R, 0, 1], q64, q32)):
        e32 = np.abs(r32.astype(np.float64) - r64).max()
        err = np.abs(got.astype(np.float64) - r64)
        print(f"embed pe={with_pe} {name}: E32 {e32:.3e} err {err.max():.3e} err/E32 {err.max() / e32:.3f}")
        assert (err <= np.maximum(4.0 * e32, np.spacing(np.abs(r64).astype(np.float32)))).all(), (name, err, e32)
    # nothing else is written: the other partial slots, the padding rows
    assert (part[:, 1:] == FILL).all() and (part[R:] == FILL).all()
    assert (ne.x.cpu().numpy().reshape(-1) == FILL).sum() == (ne.x.shape[0] - R) * U.D


def test_embed_row_skipped_after_the_last_step():
    from nanodecoder_amd.engine import NextRows
    V, R, S = 9, 5, 4
    rng = np.random.default_rng(7)
    pe = np.concatenate([U.sinusoid_pe(S), np.full((1, U.D), 7e7, np.float32)])  # a sentinel row at index S
    w, rows = _forcing_head(V, rng)
    tok = np.array([8, 0, 4, 7, 8])
    ne = NextRows(R, _dev(), fill=FILL)
    ne.tok.fill_(-5)
    out, ne = _greedy(_head(w, rng.standard_normal((V, U.D)).astype(np.float32), pe), rows(tok), S - 1, S, 0, 1,
                      ne=ne)
    assert (out["tok"] == tok).all() and (out["out_tokens"][:, S - 1] == tok).all()
    assert (ne.x.cpu().numpy() == FILL).all() and (ne.part.cpu().numpy() == FILL).all()
    assert (ne.tok.cpu().numpy() == -5).all()


# ================================================================= greedy
def _argmax_case(eos, dup, boost, seed=3, V=9, R=6):
    sc = U.Script(R, 4, V, seed, eos=eos, dup=dup, boost=boost, spread=0.1)
    return sc, sc.X[:, 1, 0]


def _expect_argmax(lp, eos, masked):
    """first index of the maximum of each row (EOS at -1e20 when masked); every runner-up that is no exact tie
    with the winner is further than TIE_MARGIN below it"""
    m = lp.copy()
    if masked:
        m[:, eos] = np.float32(-1e20)
    best = m.argmax(1)
    top = m.max(1, keepdims=True)
    gap = (top - m).astype(np.float64)
    assert ((gap == 0) | (gap > U.TIE_MARGIN)).all()
    return best, m[np.arange(len(m)), best]


@pytest.mark.parametrize("name,eos,dup,boost,masked,want", [
    ("tie 7/8: the first wins", 3, ((7, 8),), ((7, 20.0), (8, 20.0)), False, 7),
    ("tie 2/5: the first wins", 3, ((2, 5),), ((2, 20.0), (5, 20.0)), False, 2),
    ("EOS 3 is the argmax: masked", 3, (), ((3, 20.0),), True, None),
    ("EOS 3 is the argmax: past min_len", 3, (), ((3, 20.0),), False, 3),
    ("EOS 0 is the argmax: masked", 0, (), ((0, 20.0),), True, None),
    ("EOS 0 is the argmax: past min_len", 0, (), ((0, 20.0),), False, 0),
    ("EOS 3 ties with 6 and comes first: masked", 3, ((3, 6),), ((3, 20.0), (6, 20.0)), True, 6),
    ("EOS 3 ties with 6 and comes first: past min_len", 3, ((3, 6),), ((3, 20.0), (6, 20.0)), False, 3),
    ("EOS 0 ties with 4: masked", 0, ((0, 4),), ((0, 20.0), (4, 20.0)), True, 4),
    ("EOS 8 ties with 7 and comes second: masked", 8, ((7, 8),), ((7, 20.0), (8, 20.0)), True, 7),
])
def test_greedy_argmax_ties_and_min_len(name, eos, dup, boost, masked, want):
    sc, x = _argmax_case(eos, dup, boost)
    S, step = 4, 1
    out, _ = _greedy(_script_head(sc), x, step, S, 2 if masked else 1, eos)
    lp = out["logp"][:, step]
    best, score = _expect_argmax(lp, eos, masked)
    if want is not None:
        assert (best == want).all(), name  # the case is what it says
    else:
        assert (lp.argmax(1) == eos).all() and (best != eos).all(), name
    for a, b in dup:
        assert gu.same_f32(lp[:, a], lp[:, b])
    assert (out["tok"] == best).all() and (out["out_tokens"][:, step] == best).all(), name
    assert gu.same_f32(out["score"], score), name


def test_greedy_layouts_over_three_steps():
    """out_tokens[r * S + step], score, the dump [R][S][V] and the next rows over a 3-step run of R = 5 rows
    (two workgroups), against ref_cpu.greedy on the stub."""
    from nanodecoder_amd.engine import NextRows
    from oracle import ref_cpu
    sc = U.Script(5, 3, 9, seed=11, eos_bias=1.0)
    lp = _device_lp(sc, "greedy3")
    with U.pinned_topk() as log:
        ref = ref_cpu.greedy(U.Stub(sc, lp), U.chunk_src(range(5)), np.ones(5), max_length=3, min_length=1)
    head, X = _script_head(sc), _t(sc.X)
    R, S, V = 5, 3, 9
    out = dict(tok=torch.full((R,), sc.bos, dtype=torch.int32, device=_dev()),
               out_tokens=torch.full((R, S), -1, dtype=torch.int32, device=_dev()),
               score=torch.zeros(R, device=_dev()), logp=torch.full((R, S, V), FILL, device=_dev()))
    ne = NextRows(R, _dev(), fill=FILL)
    rows = torch.arange(R, device=_dev())
    from nanodecoder_amd.engine import op_greedy_head
    for s in range(S):
        x = X[rows, s, out["tok"].long().clamp(0, V - 1)]
        op_greedy_head(head, x, s, S, 1, sc.eos, out=out, ne=ne)
        torch.cuda.synchronize()
        tok = out["tok"].cpu().numpy()
        assert (tok == ref["tokens"][:, s]).all(), s
        assert (out["out_tokens"].cpu().numpy()[:, s + 1:] == -1).all()
        assert (out["logp"].cpu().numpy()[:, s + 1:] == FILL).all()
        if s + 1 < S:
            assert gu.same_f32(ne.rows().cpu().numpy(), U.embed_ref(sc.emb, sc.pe, tok, s + 1))
            assert (ne.tok.cpu().numpy()[:R] == tok).all()
    assert (out["out_tokens"].cpu().numpy() == ref["tokens"]).all()
    assert gu.same_f32(out["logp"].cpu().numpy(), ref["logp"])
    assert gu.same_f32(out["score"].cpu().numpy(), ref["scores"])
    assert log.selections == 3


# ================================================================= sampling
def _sample(sc, temp, topk, step, seed, min_len=0, S=8):
    x = np.repeat(sc.X[0, 0, :1], U.SAMPLE_R, axis=0)
    seed_t = torch.tensor([seed], dtype=torch.int64, device=_dev())
    out, _ = _greedy(_script_head(sc, S), x, step, S, min_len, U.SAMPLE_EOS, temp=temp, topk=topk, seed=seed_t)
    lp = out["logp"][:, step]
    assert (lp.view(np.uint32) == lp[0].view(np.uint32)).all()  # one row, one set of log-probs
    return out, lp[0]


def _check_draws(out, lp, temp, topk, step, seed, eos=None):
    u = U.draw_uniform_rows(seed, U.SAMPLE_R, step)
    pick, l, kept, margin = U.sample_ref(lp, temp, topk, u, eos=eos)
    print(f"sampling temp={temp} topk={topk} step={step}: min margin {margin.min():.3e}, "
          f"draws {np.bincount(pick, minlength=l.size).tolist()}")
    assert margin.min() > 1e-5  # no draw sits on a CDF boundary: no exemptions
    assert (out["tok"] == pick).all() and (out["out_tokens"][:, step] == pick).all()
    assert gu.same_f32(out["score"], l[pick])  # float32(lp) / float32(temp), bitwise
    assert kept[out["tok"]].all()
    return pick, kept


@pytest.mark.parametrize("step", [0, 5])
@pytest.mark.parametrize("temp,topk", [(1.0, -1), (0.7, 2), (1.5, 3), (1.0, 6)])
def test_sampling_is_the_inverse_cdf_pick(temp, topk, step):
    sc = U.sampling_script()
    seed = U.SAMPLE_SEEDS[(temp, topk, step)]
    out, lp = _sample(sc, temp, topk, step, seed)
    pick, kept = _check_draws(out, lp, temp, topk, step, seed)
    assert set(pick.tolist()) == set(np.flatnonzero(kept).tolist())  # every kept token is drawn, no other


def test_sampling_keeps_both_members_of_a_tie_at_the_kth_value():
    t = U.SAMPLE_TIE
    sc = U.sampling_script("tie")
    out, lp = _sample(sc, 1.0, t["topk"], t["step"], t["seed"])
    a, b = t["dup"]
    order = np.argsort(-lp, kind="stable")
    assert lp[a] == lp[b] and sorted(order[t["topk"] - 1: t["topk"] + 1].tolist()) == [a, b]
    pick, kept = _check_draws(out, lp, 1.0, t["topk"], t["step"], t["seed"])
    assert kept.sum() == t["topk"] + 1
    n = np.bincount(out["tok"], minlength=sc.V)
    assert n[a] > 0 and n[b] > 0              # both tied tokens are drawn
    assert (n[~kept] == 0).all()              # a token outside the kept set never is


def test_sampling_counts_a_tie_inside_the_top_k_once_per_member():
    """The two most likely tokens tie and top-k is 3: the kept set is the pair and the third token, no fourth."""
    t = U.SAMPLE_TIE_IN
    sc = U.sampling_script("tie_in")
    out, lp = _sample(sc, 1.0, t["topk"], t["step"], t["seed"])
    a, b = t["dup"]
    assert lp[a] == lp[b] and sorted(np.argsort(-lp, kind="stable")[:2].tolist()) == [a, b]
    pick, kept = _check_draws(out, lp, 1.0, t["topk"], t["step"], t["seed"])
    n = np.bincount(out["tok"], minlength=sc.V)
    assert kept.sum() == t["topk"] and (n[kept] > 0).all() and (n[~kept] == 0).all()


@pytest.mark.parametrize("step", [1, 4])
def test_sampling_honours_min_len(step):
    m = U.SAMPLE_MIN_LEN
    sc = U.sampling_script("min_len")
    seed = m["seeds"][step]
    out, lp = _sample(sc, 1.0, -1, step, seed, min_len=m["min_len"])
    masked = step < m["min_len"]
    _check_draws(out, lp, 1.0, -1, step, seed, eos=U.SAMPLE_EOS if masked else None)
    n = np.bincount(out["tok"], minlength=sc.V)
    assert (n[U.SAMPLE_EOS] == 0) if masked else (n[U.SAMPLE_EOS] > 100)


# ================================================================= the --fast beam
PER_ROW = ("cum", "tok", "pen", "prev_pen")
PER_ROW2 = ("seq", "anc", "blk", "cov")
PER_CHUNK = ("done", "top_fin", "n_hyp", "steps_run")
PER_HYP = ("hyp_score", "hyp_len", "hyp_tok", "hyp_anc")


def _snapshot(st, ne):
    torch.cuda.synchronize()
    s = {k: v.cpu().numpy() for k, v in st.t.items() if k != "attn"}
    s["ne_x"], s["ne_part"], s["ne_tok"] = ne.rows().cpu().numpy(), ne.part.cpu().numpy(), ne.tok.cpu().numpy()
    return s


def _chunk_bytes(s, c, beam, n_best):
    """every field of chunk c (and its rows of the next input), as bytes"""
    r, h = slice(c * beam, (c + 1) * beam), slice(c * n_best, (c + 1) * n_best)
    parts = [s[k][r] for k in PER_ROW + ("ne_x", "ne_part", "ne_tok")] + [s[k][:, r] for k in PER_ROW2]
    parts += [s[k][c: c + 1] for k in PER_CHUNK] + [s[k][h] for k in PER_HYP]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def _fast_setup(sc, beam, n_best):
    from nanodecoder_amd.engine import BeamOpState, NextRows, op_beam_init
    st = BeamOpState(sc.C, beam, n_best, sc.S, _dev(), fill=-3)
    ne = NextRows(sc.C * beam, _dev(), fill=FILL)
    op_beam_init(st, sc.bos)
    return st, ne


def _fast_step(sc, head, X, st, ne, s, min_len, alpha, **kw):
    from nanodecoder_amd.engine import op_beam_step
    chunk = torch.arange(sc.C * st.beam, device=_dev()) // st.beam
    x = X[chunk, s, st["tok"].long().clamp(0, sc.V - 1)]
    op_beam_step(head, x, st, ne, s, min_len, sc.eos, alpha, **kw)


def _run_fast(sc, beam, n_best, alpha, min_len):
    """S steps of the device beam on the scripted model: the state after init and after every step, and the
    finish kernel's output."""
    from nanodecoder_amd.engine import op_beam_finish
    head, X = _script_head(sc), _t(sc.X)
    st, ne = _fast_setup(sc, beam, n_best)
    snaps = [_snapshot(st, ne)]
    for s in range(sc.S):
        _fast_step(sc, head, X, st, ne, s, min_len, alpha)
        snaps.append(_snapshot(st, ne))
    out = [t.cpu().numpy() for t in op_beam_finish(st)]
    torch.cuda.synchronize()
    return snaps, out


def _check_results(out, res, C, S, close):
    tokens, scores, lens = out
    for c in range(C):
        for i, h in enumerate(res[c]):
            n = len(h[1])
            assert lens[c, i] == n, (c, i, lens[c], [len(x[1]) for x in res[c]])
            assert (tokens[c, i, :n] == h[1]).all() and (tokens[c, i, n:] == -1).all(), (c, i, tokens[c, i], h[1])
            assert close(float(scores[c, i]), h[0]), (c, i, scores[c, i], h[0])


def _check_fast(sc, key, beam, n_best, alpha, min_len):
    """The device run against ref_cpu.fast_beam: state after every step, ancestry, finished lists."""
    lp = _device_lp(sc, key)
    alpha = float(np.float32(alpha))  # the entry takes alpha as fp32: the reference's penalty gets the same number
    res, stub, log = U.ref_fast_beam(sc, lp, beam, n_best, alpha, min_len)  # raises on a near tie
    p = U.fast_props(sc, res, stub, log, beam, n_best)
    tr = p["trace"]
    snaps, out = _run_fast(sc, beam, n_best, alpha, min_len)
    C, S, V = sc.C, sc.S, sc.V
    assert snaps[0]["n_alive"][0] == C
    for s in range(S):
        before, after = snaps[s], snaps[s + 1]
        for c in range(C):
            if before["done"][c]:  # a finished chunk: no field moves, nor do its rows of the next input
                assert _chunk_bytes(after, c, beam, n_best) == _chunk_bytes(before, c, beam, n_best), (s, c)
        if s >= len(tr):
            assert after["n_alive"][0] == 0 and after["steps_done"][0] == len(tr)
            continue
        t = tr[s]
        assert (after["done"] == t["done"]).all(), (s, after["done"], t["done"])
        assert (after["steps_run"] == t["steps_run"]).all(), (s, after["steps_run"], t["steps_run"])
        assert after["n_alive"][0] == t["n_alive"], (s, after["n_alive"], t["n_alive"])
        assert ((after["tok"] >= 0) & (after["tok"] < V)).all()
        cur, nxt = s & 1, (s & 1) ^ 1
        for dst, par in t["anc"].items():  # the reference's select history
            assert after["anc"][nxt][dst][s] == par, (s, dst)
            assert (after["anc"][nxt][dst][:s] == before["anc"][cur][par][:s]).all(), (s, dst)
            assert (after["seq"][nxt][dst][:s] == before["seq"][cur][par][:s]).all(), (s, dst)
        for row, tok in t["tok"].items():
            assert after["tok"][row] == tok and after["seq"][nxt][row][s] == tok, (s, row)
            if s + 1 < S:
                assert gu.same_f32(after["ne_x"][row], U.embed_ref(sc.emb, sc.pe, tok, s + 1)), (s, row)
    assert snaps[-1]["steps_done"][0] == len(tr) and (snaps[-1]["done"] == 1).all()
    assert (snaps[-1]["n_hyp"] == p["n_hyp"]).all(), (snaps[-1]["n_hyp"], p["n_hyp"])
    _check_results(out, res, C, S, lambda got, ref: abs(got - ref) <= U.ulp32(ref))
    return p, snaps, res


@pytest.mark.parametrize("min_len", [0, 3])
@pytest.mark.parametrize("alpha", [0.0, 0.6])
@pytest.mark.parametrize("n_best", [1, 2, "beam"])
@pytest.mark.parametrize("beam,V", U.FAST_GRID)
def test_fast_beam_grid(beam, V, n_best, alpha, min_len):
    sc = U.fast_grid_script(beam, V, alpha, min_len)
    p, _, _ = _check_fast(sc, ("grid", beam, V, sc.seed), beam, beam if n_best == "beam" else n_best, alpha, min_len)
    if (beam, V) == (8, 32):
        assert p["slots"] >= {0, 1, 2, 3}  # candidates 128..255 (the third and fourth 64-lane slots) are selected


@pytest.mark.parametrize("name", sorted(U.FAST_SCENARIOS))
def test_fast_beam_scenario(name):
    kw, beam, n_best, alpha, min_len, shows = U.FAST_SCENARIOS[name]
    sc = U.Script(**kw)
    p, snaps, res = _check_fast(sc, ("scenario", name), beam, n_best, alpha, min_len)
    assert shows(p, res, sc.S), {k: v for k, v in p.items() if k != "trace"}
    if name == "other_beam_first":  # hypotheses on the list, the top beam not finished: the chunk goes on
        assert any(((s["n_hyp"] >= n_best) & (s["top_fin"] == 0) & (s["done"] == 0)).any() for s in snaps[1:])
    if name == "evict_equal_scores":
        assert (snaps[-1]["n_hyp"] > n_best).any()
    if name == "no_eos":
        assert (snaps[-1]["steps_run"] == sc.S).all() and (snaps[-1]["hyp_len"] == sc.S).all()


def test_fast_beam_chunk_list():
    """The tail form: a launch over a permuted chunk list with a -1 entry (ccap < C) advances the listed chunks
    exactly as the full launch does and leaves every field of the others bit for bit."""
    from nanodecoder_amd.engine import op_beam_finish
    kw, beam, n_best, alpha, min_len, _ = U.FAST_SCENARIOS["different_steps"]
    sc = U.Script(**kw)
    full, out_full = _run_fast(sc, beam, n_best, alpha, min_len)
    assert not full[1]["done"].any()  # every chunk is alive at step 1
    head, X = _script_head(sc), _t(sc.X)
    st, ne = _fast_setup(sc, beam, n_best)
    _fast_step(sc, head, X, st, ne, 0, min_len, alpha)
    s0 = _snapshot(st, ne)
    lists = [([2, -1, 0], [1, 3]), ([-1, 3, 1], [])]
    for clist, absent in lists:
        _fast_step(sc, head, X, st, ne, 1, min_len, alpha, clist=_t(np.array(clist, np.int32)), ccap=3)
        s1 = _snapshot(st, ne)
        for c in range(sc.C):
            want = s0 if c in absent else full[2]
            assert _chunk_bytes(s1, c, beam, n_best) == _chunk_bytes(want, c, beam, n_best), (clist, c)
    assert s1["n_alive"][0] == full[2]["n_alive"][0]
    for s in range(2, sc.S):
        _fast_step(sc, head, X, st, ne, s, min_len, alpha)
    end = _snapshot(st, ne)
    assert all(_chunk_bytes(end, c, beam, n_best) == _chunk_bytes(full[-1], c, beam, n_best) for c in range(sc.C))
    assert end["steps_done"][0] == full[-1]["steps_done"][0] and end["n_alive"][0] == 0
    for a, b in zip([t.cpu().numpy() for t in op_beam_finish(st)], out_full):
        assert a.tobytes() == b.tobytes()


# ================================================================= the classic Beam
def _classic_opts(o):
    return _lib.NdClassicOpts(length_penalty=U.LP_KIND[o.get("length_penalty", "none")], alpha=o.get("alpha", 0.0),
                              beta=o.get("beta", 0.0), coverage_penalty=U.COV_KIND[o.get("coverage_penalty", "none")],
                              stepwise_penalty=int(o.get("stepwise_penalty", False)),
                              block_ngram_repeat=o.get("block_ngram_repeat", 0),
                              ignore_mask=sum(1 << t for t in o.get("exclusion_tokens", ())))


def _run_classic(sc, k, cut):
    from nanodecoder_amd.engine import BeamOpState, NextRows, op_beam_finish, op_beam_init, op_beam_step
    C, S, V, T, beam, n_best = sc.C, sc.S, sc.V, sc.T, k["beam"], k["n_best"]
    head, X, ATT = _script_head(sc), _t(sc.X), _t(sc.ATT)
    st = BeamOpState(C, beam, n_best, S, _dev(), T=T, fill=-3)
    ne = NextRows(C * beam, _dev(), fill=FILL)
    group = np.zeros(C, np.int32)
    for g, chunks in enumerate(k["groups"]):
        group[chunks] = g
    if T:
        st["cut"].copy_(_t(np.array([cut[c] for c in range(C)], np.int32)))
        st["attn"].fill_(0.5)
    opts = _classic_opts(k["opts"])
    op_beam_init(st, sc.bos, group=_t(group))
    chunk = torch.arange(C * beam, device=_dev()) // beam
    snaps = [_snapshot(st, ne)]
    for s in range(S):
        tok = st["tok"].long().clamp(0, V - 1)
        if T:
            st["attn"][:, s, :] = ATT[chunk, s, tok]
        op_beam_step(head, X[chunk, s, tok], st, ne, s, k["min_len"], sc.eos, opts=opts)
        snaps.append(_snapshot(st, ne))
    out = [t.cpu().numpy() for t in op_beam_finish(st, opts=opts)]
    torch.cuda.synchronize()
    return snaps, out, group


@pytest.mark.parametrize("name", sorted(U.classic_cases()))
def test_classic_beam(name):
    sc, k = U.classic_case(name)
    k["opts"].update({o: float(np.float32(v)) for o, v in k["opts"].items() if o in ("alpha", "beta")})  # as the ABI
    lp = _device_lp(sc, ("classic", repr(k["script"]), sc.seed))
    res, beams, cut, log = U.ref_classic_beam(sc, lp, k["groups"], k["beam"], k["n_best"], k["min_len"], k["opts"],
                                              k["lengths"])  # raises on a near tie
    p = U.classic_need(sc, lp, k, res, beams, log)
    snaps, out, group = _run_classic(sc, k, cut)
    C, S, beam, n_best = sc.C, sc.S, k["beam"], k["n_best"]
    steps = p["steps_run"]  # the reference's len(prev_ks): advance() calls per chunk
    finished = {g: all(beams[c].log[-1][0] for c in chunks) for g, chunks in enumerate(k["groups"])}
    for s in range(S):
        before, after = snaps[s], snaps[s + 1]
        for c in range(C):
            b = beams[c]
            if s >= steps[c]:  # the chunk's batch finished at an earlier step: nothing of it moves
                assert _chunk_bytes(after, c, beam, n_best) == _chunk_bytes(before, c, beam, n_best), (s, c)
            assert after["steps_run"][c] == min(s + 1, steps[c]), (s, c, after["steps_run"], steps)
            if s < steps[c]:  # the step's next_ys and prev_ks, beam by beam
                rows, nxt = slice(c * beam, (c + 1) * beam), (s & 1) ^ 1
                assert (after["seq"][nxt][rows, s] == b.next_ys[s + 1].numpy()).all(), (s, c)
                assert (after["anc"][nxt][rows, s] == c * beam + b.prev_ks[s].numpy()).all(), (s, c)
            assert after["done"][c] == int(b.log[min(s, steps[c] - 1)][0]), (s, c)
        alive = sum(1 for g, chunks in enumerate(k["groups"]) if not (finished[g] and s + 1 >= steps[chunks[0]]))
        assert after["n_alive"][0] == alive, (s, after["n_alive"], alive)
        for g, chunks in enumerate(k["groups"]):
            want = steps[chunks[0]] if finished[g] and s + 1 >= steps[chunks[0]] else 0
            assert after["grp_done"][g] == want, (s, g, after["grp_done"])
    if all(finished.values()):
        assert snaps[-1]["steps_done"][0] == max(steps.values())
    _check_results(out, res, C, S, lambda got, ref: abs(got - ref) <= 1e-3 + 1e-5 * abs(ref))
    if name == "late_better":  # the better hypothesis that arrived after the chunk was done is the one reported
        c = p["late_better"][0]
        first = next(i for i, e in enumerate(beams[c].log) if e[0])
        assert abs(out[1][c, 0] - beams[c].log[-1][1]) <= 1e-3 and out[1][c, 0] > beams[c].log[first][1] + 1e-3


# ================================================================= attention capture
@pytest.mark.parametrize("rpc", [1, 5])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 512])
def test_attn_step_softmax_vs_fp64(T, rpc):
    from nanodecoder_amd.engine import op_attn_step_softmax
    spans = sorted({1, T - 1, T})
    C, ld = len(spans), T + 3
    rng = np.random.default_rng(T * 10 + rpc)
    a = (rng.standard_normal((C * rpc, ld)) * 3.0).astype(np.float32)
    got = op_attn_step_softmax(_t(a), _t(np.array(spans, np.int32)), rpc, T)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert gu.same_f32(got[:, T:], a[:, T:])  # past the row: untouched
    err = e32 = 0.0
    for r in range(C * rpc):
        L = spans[r // rpc]
        assert (got[r, L:T] == 0).all(), r  # zeros past the span
        if L:
            ref = torch.softmax(torch.from_numpy(a[r, :L]).double(), 0).numpy()
            f32 = torch.softmax(torch.from_numpy(a[r, :L]), 0).numpy().astype(np.float64)
            err, e32 = max(err, np.abs(got[r, :L] - ref).max()), max(e32, np.abs(f32 - ref).max())
    print(f"attn softmax T={T} rpc={rpc}: E32 {e32:.3e} err {err:.3e} err/E32 {err / e32 if e32 else 0.0:.3f}")
    assert err <= 4.0 * e32, (err, e32)


def test_beam_attn_gather_is_a_gather():
    from nanodecoder_amd.engine import BeamOpState, op_beam_attn_gather
    C, beam, n_best, S, Ts, max_len, T = 2, 3, 2, 5, 7, 4, 5
    rng = np.random.default_rng(5)
    st = BeamOpState(C, beam, n_best, S, _dev(), T=Ts)
    hyp_len = np.array([0, 1, max_len, 3], np.int32)
    hyp_anc = rng.integers(0, C * beam, (C * n_best, S)).astype(np.int32)
    attn = rng.standard_normal((C * beam, S, Ts)).astype(np.float32)
    st["hyp_len"].copy_(_t(hyp_len))
    st["hyp_anc"].copy_(_t(hyp_anc))
    st["attn"].copy_(_t(attn))
    got = op_beam_attn_gather(st, max_len, T)
    torch.cuda.synchronize()
    want = np.zeros((C * n_best, max_len, T), np.float32)
    for h in range(C * n_best):
        for t in range(hyp_len[h]):
            want[h, t] = attn[hyp_anc[h, t], t, :T]
    assert gu.same_f32(got.cpu().numpy().reshape(want.shape), want)
