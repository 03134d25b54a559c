"""Several candidate targets per chunk on one encoder pass (needs an MI355X): nd_score_candidates against the
CPU oracle's forced-token loop and against nd_score_targets on the replicated chunks, its K = 1 case, the
independence of the slots, empty slots, the posterior kernel on scripted scores, the pool, the timed form,
the refusals and the Translator surface."""
import ctypes
import types

import numpy as np
import pytest
import torch

from nanodecoder_amd import frontend, synth
from tests import cand_util as cu
from tests import golden_util as gu
from tests import score_util as su

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MAX_BATCH, MAX_STEPS = 16, 72
# (chunks of the fixture, candidate kinds per chunk, L): K * L = 176 query rows per chunk, across the 128-row
# query group and no multiple of the 32-row wave block; and 130 rows, two past the group
CASES = {"mixed": ((2, 3, 5), (0, 1, 2, 3), 44), "boundary": ((4,), (0, 1), 65)}


def _engine(cfg, W, **kw):
    from nanodecoder_amd.engine import Engine
    return Engine(cfg, W, device=0, max_batch=MAX_BATCH, max_steps=MAX_STEPS, **kw)


def _gold_tokens(z, i):
    return z["gold"][i, : z["gold_len"][i] - 1].tolist()


def _case(z, cfg, chunks, kinds, L):
    """dict(src, lengths, spans, cand [B, K, L], cand_len [B, K]) of fixture chunks ``chunks``, each with the
    candidates ``kinds`` (indices into cand_util.KINDS) of its gold row."""
    cands = [[cu.candidates_of(_gold_tokens(z, i))[k] for k in kinds] for i in chunks]
    cand, cand_len = cu.pack(cands, len(kinds), L, cfg.pad_idx, cfg.eos_idx)
    idx = list(chunks)
    return dict(src=z["src"][idx], lengths=z["lengths"][idx], spans=np.full(len(idx), z["src"].shape[1], np.int32),
                cand=cand, cand_len=cand_len)


def _replicated(d):
    """The case as nd_score_targets takes it: every chunk copied K times, one gold row each."""
    B, K, L = d["cand"].shape
    rep = np.repeat(np.arange(B), K)
    return dict(src=d["src"][rep], lengths=d["lengths"][rep], spans=d["spans"][rep], gold=d["cand"].reshape(B * K, L),
                gold_len=d["cand_len"].reshape(B * K))


def _cand(eng, d, **kw):
    r = eng.score_candidates(d["src"], d["lengths"], d["spans"], cand=d["cand"], cand_len=d["cand_len"], **kw)
    torch.cuda.synchronize()
    return r


@pytest.fixture(scope="module")
def fixture():
    return su.load_fixture()


@pytest.fixture(scope="module")
def oracle(fixture):
    """The CPU oracle's forced-token scores of every case's B * K sequences (the chunk rows repeated), for
    both fixture models, computed once."""
    from oracle import ref_cpu
    out = {}
    for name, z in fixture.items():
        cfg, W = su.fixture_model(z)
        model = ref_cpu.RefModel(cfg, W)
        for case, (chunks, kinds, L) in CASES.items():
            r = _replicated(_case(z, cfg, chunks, kinds, L))
            out[name, case] = su.oracle_score(model, r["src"], r["lengths"], r["gold"], r["gold_len"])
    return out


def _check_against_oracle_and_replicated(fixture, oracle, name, case, exact, graphs):
    z = fixture[name]
    cfg, W = su.fixture_model(z)
    chunks, kinds, L = CASES[case]
    d = _case(z, cfg, chunks, kinds, L)
    rep = _replicated(d)
    B, K = d["cand_len"].shape
    eng = _engine(cfg, W, graphs=graphs)
    try:
        eng.set_exact_fp32(exact)
        r = _cand(eng, d, return_tok_logp=True, return_logp=True)
        assert int(r["overflow"].item()) == 0
        t = eng.score_targets(rep["src"], rep["lengths"], rep["spans"], gold=rep["gold"], gold_len=rep["gold_len"],
                              return_tok_logp=True, return_logp=True)
        torch.cuda.synchronize()
        sc, tl, lp = r["scores"].cpu().numpy(), r["tok_logp"].cpu().numpy(), r["logp"].cpu().numpy()
        post, best = r["post"].cpu().numpy(), r["best"].cpu().numpy()
        t_sc, t_tl, t_lp = (t[k].cpu().numpy() for k in ("scores", "tok_logp", "logp"))
    finally:
        eng.close()
    assert sc.shape == (B, K) and tl.shape == (B, K, L) and lp.shape == (B, K, L, cfg.vocab)
    assert post.shape == (B, K) and best.shape == (B,)
    live = np.arange(L)[None, None, :] < d["cand_len"][:, :, None]
    o_sc, o_tl, o_lp = (a.reshape((B, K) + a.shape[1:]) for a in oracle[name, case])
    t_sc, t_tl, t_lp = (a.reshape((B, K) + a.shape[1:]) for a in (t_sc, t_tl, t_lp))
    print(name, case, "exact" if exact else "split", "graphs" if graphs else "eager",
          "max |score - oracle|", np.abs(sc - o_sc).max(), "max |score - replicated|", np.abs(sc - t_sc).max(),
          "max |logp - oracle| live", np.abs(lp - o_lp)[live][:, 4:].max(),
          "max |logp - replicated| live", np.abs(lp - t_lp)[live][:, 4:].max(), "scores", sc)
    for w_sc, w_tl, w_lp in ((o_sc, o_tl, o_lp), (t_sc, t_tl, t_lp)):
        assert gu.logp_close(sc, w_sc).all()
        assert gu.logp_close(tl, w_tl).all()
        assert gu.logp_close(lp, w_lp)[live].all()
    assert (tl[~live] == 0).all()
    # the posterior and the best slot: the host rule on the call's own scores
    w_post, w_best = frontend.candidate_posterior(sc, d["cand_len"])
    print("max |post - host rule|", np.abs(post - w_post).max(), "best", best)
    assert (best == w_best).all()
    assert (np.abs(post - w_post) <= 1e-5 + 1e-6 * np.abs(w_post)).all()
    return sc


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", su.MODELS)
def test_candidates_match_oracle_and_replicated_call(fixture, oracle, name, exact, graphs):
    """Chunks 2, 3, 5 with the four candidates each, L = 44."""
    sc = _check_against_oracle_and_replicated(fixture, oracle, name, "mixed", exact, graphs)
    # slot 0 of chunk 2 is the fixture's gold row: the reference's own score
    assert gu.logp_close(sc[0, 0], fixture[name]["score"][2])


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", su.MODELS)
def test_candidates_two_rows_past_the_query_group(fixture, oracle, name, exact, graphs):
    """Chunk 4 alone (gold_len 65), K = 2 (the gold row and the substitution), L = 65: 130 query rows."""
    sc = _check_against_oracle_and_replicated(fixture, oracle, name, "boundary", exact, graphs)
    assert gu.logp_close(sc[0, 0], fixture[name]["score"][4])


@pytest.mark.parametrize("exact", [False, True])
def test_one_candidate_is_score_targets_bitwise(fixture, exact):
    z = fixture["transformer_pe"]
    cfg, W = su.fixture_model(z)
    B, T = z["src"].shape
    spans = np.full(B, T, np.int32)
    eng = _engine(cfg, W)
    try:
        eng.set_exact_fp32(exact)
        a = eng.score_targets(z["src"], z["lengths"], spans, gold=z["gold"], gold_len=z["gold_len"],
                              return_tok_logp=True)
        b = eng.score_candidates(z["src"], z["lengths"], spans, cand=z["gold"][:, None, :],
                                 cand_len=z["gold_len"][:, None], return_tok_logp=True)
        torch.cuda.synchronize()
        assert torch.equal(a["scores"], b["scores"][:, 0]) and torch.equal(a["tok_logp"], b["tok_logp"][:, 0])
        assert (b["post"] == 0).all() and (b["best"] == 0).all()
    finally:
        eng.close()


@pytest.mark.parametrize("exact", [False, True])
def test_slots_do_not_see_each_other(fixture, exact):
    """Two slots that hold the same candidate get the same bits, and permuting a chunk's slots permutes its
    results bit for bit."""
    z = fixture["transformer_pe"]
    cfg, W = su.fixture_model(z)
    L = 44
    d = _case(z, cfg, (2, 3), (0, 1, 0, 3), L)  # slots 0 and 2: the gold row twice
    perms = np.array([[2, 0, 3, 1], [3, 2, 1, 0]])
    p = dict(d, cand=np.take_along_axis(d["cand"], perms[:, :, None], 1),
             cand_len=np.take_along_axis(d["cand_len"], perms, 1))
    eng = _engine(cfg, W)
    try:
        eng.set_exact_fp32(exact)
        a = _cand(eng, d, return_tok_logp=True)
        b = _cand(eng, p, return_tok_logp=True)
        assert torch.equal(a["scores"][:, 0], a["scores"][:, 2]) and torch.equal(a["tok_logp"][:, 0], a["tok_logp"][:, 2])
        pt = torch.from_numpy(perms).to(DEV)
        assert torch.equal(b["scores"], torch.gather(a["scores"], 1, pt))
        assert torch.equal(b["tok_logp"], torch.gather(a["tok_logp"], 1, pt[:, :, None].expand(-1, -1, L)))
        assert torch.isfinite(a["scores"]).all()
    finally:
        eng.close()


def test_empty_slots(fixture):
    """A chunk with two of its four slots filled: the empty slots (cand_len 0, junk ids, out-of-range ones
    included) read -inf, take no part in the posterior and do not change the filled slots' bits."""
    z = fixture["transformer_pe"]
    cfg, W = su.fixture_model(z)
    full = _case(z, cfg, (2, 3), (0, 1, 2, 3), 44)
    part = dict(full, cand=full["cand"].copy(), cand_len=full["cand_len"].copy())
    part["cand_len"][0, 2:] = 0
    part["cand"][0, 2:] = np.random.default_rng(4).choice([0, 1, 2, 3, 4, 7, 8, 1000, -5, 2 ** 31 - 1], (2, 44))
    eng = _engine(cfg, W)
    try:
        a = _cand(eng, full, return_tok_logp=True)
        b = _cand(eng, part, return_tok_logp=True)
        assert int(b["overflow"].item()) == 0
        assert torch.equal(a["scores"][0, :2], b["scores"][0, :2]) and torch.equal(a["scores"][1], b["scores"][1])
        assert torch.equal(a["tok_logp"][0, :2], b["tok_logp"][0, :2])
        sc, post, best = b["scores"].cpu().numpy(), b["post"].cpu().numpy(), b["best"].cpu().numpy()
        tl = b["tok_logp"].cpu().numpy()
    finally:
        eng.close()
    assert (sc[0, 2:] == -np.inf).all() and (post[0, 2:] == -np.inf).all() and (tl[0, 2:] == 0).all()
    assert np.isfinite(sc[0, :2]).all() and np.isfinite(sc[1]).all()
    w_post, w_best = frontend.candidate_posterior(sc, part["cand_len"])
    assert (best == w_best).all() and best[0] in (0, 1)
    fin = np.isfinite(w_post)
    assert (np.isfinite(post) == fin).all()
    assert (np.abs(post[fin] - w_post[fin]) <= 1e-5 + 1e-6 * np.abs(w_post[fin])).all()
    assert abs(np.exp(post[0, :2].astype(np.float64)).sum() - 1.0) < 1e-5  # over the two filled slots only


@pytest.mark.parametrize("in_place", [False, True])
def test_cand_posterior_on_scripted_scores(in_place):
    from nanodecoder_amd import _lib
    L = _lib.lib()
    scores, cand_len, want_best = cu.scripted_rows()
    B, K = scores.shape
    s = torch.from_numpy(scores).to(DEV)
    cl = torch.from_numpy(cand_len).to(DEV)
    out = s if in_place else torch.full((B, K), 7.0, device=DEV)
    post = torch.full((B, K), 7.0, device=DEV)
    best = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.nd_cand_posterior(P(s), P(cl), B, K, P(out), P(post), P(best),
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.nd_last_error()
    torch.cuda.synchronize()
    out, post, best = out.cpu().numpy(), post.cpu().numpy(), best.cpu().numpy()
    live = cand_len > 0
    assert best.tolist() == want_best.tolist()
    assert (out[~live] == -np.inf).all() and gu.same_f32(out[live], scores[live])
    w_post, w_best = frontend.candidate_posterior(scores, cand_len)
    assert (post[~live] == -np.inf).all()
    assert np.isnan(post[4, :3]).all()  # the NaN row: never best, every live post NaN
    ok = live & ~np.isnan(w_post)
    print("max |post - fp64|", np.abs(post[ok] - w_post[ok]).max(), post[3])
    assert (np.abs(post[ok] - w_post[ok]) <= 1e-5 + 1e-6 * np.abs(w_post[ok])).all()
    assert post[2, 1] == 0.0 and post[3, 2] > post[3, 0] > post[3, 1] > post[3, 3]
    # the nullable outputs
    out2 = torch.full((B, K), 7.0, device=DEV)
    assert L.nd_cand_posterior(P(torch.from_numpy(scores).to(DEV)), P(cl), B, K, P(out2), None, None, None) == 0
    torch.cuda.synchronize()
    assert gu.same_f32(out2.cpu().numpy(), out)


def test_pool_candidates_match_single_engine_bitwise(fixture):
    from nanodecoder_amd.engine import EnginePool
    z = fixture["transformer_pe"]
    cfg, W = su.fixture_model(z)
    batches = [_case(z, cfg, (2, 3, 5), (0, 1, 2, 3), 44), _case(z, cfg, (5, 3, 2), (3, 2, 1, 0), 44),
               _case(z, cfg, (1, 2), (0, 1), 33)]
    eng = _engine(cfg, W)
    try:
        single = [_cand(eng, b, return_tok_logp=True) for b in batches]
    finally:
        eng.close()
    pool = EnginePool(cfg, W, device=0, lanes=3, max_batch=MAX_BATCH, max_steps=MAX_STEPS)
    try:
        rs = [pool.score_candidates(b["src"], b["lengths"], b["spans"], cand=b["cand"], cand_len=b["cand_len"],
                                    return_tok_logp=True) for b in batches]
        pool.synchronize()
        torch.cuda.synchronize()
        assert sorted(r["lane"] for r in rs) == [0, 1, 2]
        for r, s, b in zip(rs, single, batches):
            assert all(torch.equal(r[k], s[k]) for k in ("scores", "post", "best", "tok_logp"))
            assert r["inputs"][3] is b["cand"] and r["inputs"][4] is b["cand_len"]
    finally:
        pool.close()


@pytest.mark.parametrize("graphs", [True, False])
def test_timed_calls_are_the_same_launches(fixture, graphs):
    """With nd_set_timing a scoring call runs as two pieces, the encoder side and the decoder side, and
    nd_last_timing reports both: the results keep their bits, for the candidates call and for its K = 1 sibling."""
    z = fixture["transformer_pe"]
    cfg, W = su.fixture_model(z)
    d = _case(z, cfg, (2, 3, 5), (0, 1, 2, 3), 44)
    rep = _replicated(d)
    eng = _engine(cfg, W, graphs=graphs)
    try:
        def both():
            a = _cand(eng, d, return_tok_logp=True)
            ta = eng.last_timing()
            b = eng.score_targets(rep["src"], rep["lengths"], rep["spans"], gold=rep["gold"], gold_len=rep["gold_len"],
                                  return_tok_logp=True)
            torch.cuda.synchronize()
            return a, b, ta, eng.last_timing()
        a0, b0, _, _ = both()
        eng.set_timing(True)
        a1, b1, ta, tb = both()
        eng.set_timing(False)
        a2, b2, _, _ = both()
        print("timed: candidates encode / decode ms", ta, "replicated", tb)
        for a, b in ((a1, b1), (a2, b2)):
            assert all(torch.equal(a[k], a0[k]) for k in ("scores", "post", "best", "tok_logp"))
            assert torch.equal(b["scores"], b0["scores"]) and torch.equal(b["tok_logp"], b0["tok_logp"])
        assert min(ta) > 0 and min(tb) > 0
    finally:
        eng.close()


def test_refusals_with_a_context(fixture):
    """B * K > max_batch, K = 0, L > max_steps and a null d_score return ND_ERR_ARG and touch no buffer; an
    average-attention decoder is refused by name."""
    from nanodecoder_amd import _lib
    z = fixture["transformer_pe"]
    cfg, W = su.fixture_model(z)
    sig = torch.zeros(8, 512, device=DEV)
    ints = torch.full((8 * 4 * 80,), 1, dtype=torch.int32, device=DEV)
    outs = torch.full((8 * 4 * 80,), 7.0, device=DEV)
    best = torch.full((8,), 7, dtype=torch.int32, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(eng, B, K, L, score=True):
        return eng._L.nd_score_candidates(eng._h, P(sig), P(ints), P(ints), P(ints), P(ints), B, 512, K, L,
                                          P(outs) if score else None, P(outs), P(best), P(outs), None, None)

    eng = _engine(cfg, W)
    try:
        for args, msg in (((5, 4, 8), b"B * K out of range"), ((2, 0, 8), b"K out of range"),
                          ((2, 4, MAX_STEPS + 1), b"L out of range"), ((17, 1, 8), b"B out of range")):
            assert call(eng, *args) == _lib.ND_ERR_ARG and msg in eng._L.nd_last_error(), args
        assert call(eng, 2, 4, 8, score=False) == _lib.ND_ERR_ARG and b"null buffer" in eng._L.nd_last_error()
        torch.cuda.synchronize()
        assert (outs == 7.0).all() and (best == 7).all()
    finally:
        eng.close()
    acfg = synth.ModelConfig(self_attn_type="average")
    aeng = _engine(acfg, synth.make_weights(acfg, seed=15))
    try:
        with pytest.raises(NotImplementedError):
            aeng.score_candidates(z["src"], z["lengths"], cand=np.ones((6, 2, 8), np.int32),
                                  cand_len=np.ones((6, 2), np.int32))
        assert call(aeng, 2, 4, 8) == _lib.ND_ERR_ARG and b"average-attention" in aeng._L.nd_last_error()
        assert b"nd_score_candidates" in aeng._L.nd_last_error()
        torch.cuda.synchronize()
        assert (outs == 7.0).all() and (best == 7).all()
    finally:
        aeng.close()


def test_translator_score_candidates(fixture):
    """The six fixture chunks with 1 to 4 candidates each through an engine of max_batch 8 (several calls):
    slot 0, the gold row, scores what Translator.score gives it."""
    from nanodecoder_amd.translator import Translator
    z = fixture["transformer_pe"]
    cfg, W = su.fixture_model(z)
    opt = types.SimpleNamespace(gpu=0, beam_size=1, max_length=100, batch_size=6, engine_max_batch=8)
    tr = Translator(cfg, W, opt)
    try:
        chunks = gu.chunks_of(z)
        gold = [_gold_tokens(z, i) for i in range(len(chunks))]
        counts = [1, 4, 3, 2, 2, 4]  # chunk 0's gold row is a lone EOS: itself only
        cands = [cu.candidates_of(g)[:n] if g else [g] for g, n in zip(gold, counts)]
        cands[1][0] = " ".join(cfg.itos[t] for t in cands[1][0])  # a token string among the id lists
        got = tr.score_candidates(chunks, cands, batch_size=6)
        per = tr.score(chunks, gold, batch_size=6)
    finally:
        tr.engine.close()
    assert [len(g[0]) for g in got] == counts and [len(g[1]) for g in got] == counts
    for i, (sc, post, best) in enumerate(got):
        print("chunk", i, "scores", sc, "post", post, "best", best, "score()", per[i][0])
        assert gu.logp_close(np.float32(sc[0]), np.float32(per[i][0]))
        assert gu.logp_close(np.float32(sc[0]), z["score"][i])
        assert np.isfinite(sc).all() and np.isfinite(post).all()
        assert best == int(np.argmax(np.array(sc, np.float32)))
        w_post, _ = frontend.candidate_posterior(np.array(sc, np.float32), np.ones(len(sc)))
        assert (np.abs(np.array(post) - w_post) <= 1e-5 + 1e-6 * np.abs(w_post)).all()
