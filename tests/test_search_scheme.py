"""The scripted model of the op-level search tests (tests/search_util.py), on the CPU: the stub answers
ref_cpu's searches from its tables and carries chunk ids through tile and reorder; the pinned top-k is the
stable lower-index rule and refuses a near tie; the Python restatement of draw_uniform matches splitmix64's
published outputs; and every committed seed keeps SEED_MARGIN with the fp64 head and shows what its case is
about (the GPU tests assert the same on the device's own log-probs with TIE_MARGIN)."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu
from tests import search_util as U


# ----------------------------------------------------------------- draw_uniform
GOLDEN = 0x9E3779B97F4A7C15
# the first three outputs of splitmix64 seeded with 0 (Vigna's reference implementation; the test vector
# java.util.SplittableRandom and the xoshiro seeding examples quote)
SPLITMIX_0 = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_draw_uniform_is_splitmix64_top_24_bits():
    for step, z in enumerate(SPLITMIX_0):
        assert U.draw_uniform(0, 0, step) == (z >> 40) / 2.0 ** 24
    assert U.draw_uniform(0, 0, 0) == 14819496 / 16777216  # 0xE220A8
    # a seed shifts the state; a row adds row * 2^32 to the counter, i.e. golden * row * 2^32 to the state
    assert U.draw_uniform(GOLDEN, 0, 0) == U.draw_uniform(0, 0, 1)
    for seed, row, step in [(1, 1, 0), (12345, 7, 3), (2 ** 64 - 1, 4095, 99)]:
        shifted = (seed + GOLDEN * (row << 32)) % 2 ** 64
        assert U.draw_uniform(seed, row, step) == U.draw_uniform(shifted, 0, step)
        assert 0.0 <= U.draw_uniform(seed, row, step) < 1.0
    # the counter wraps at 64 bits like the device's unsigned arithmetic
    assert U.draw_uniform(5, 2 ** 32, 0) == U.draw_uniform(5, 0, 0)


def test_draw_uniform_rows_matches_scalar():
    for seed, step in [(0, 0), (74, 5), (2 ** 63 + 11, 99)]:
        u = U.draw_uniform_rows(seed, 300, step)
        assert [U.draw_uniform(seed, r, step) for r in range(300)] == u.tolist()


def test_sample_ref_by_hand():
    """lp = log of (1/2, 1/4, 1/8, 1/8): cdf 1/2, 3/4, 7/8, 1; top-k 2 keeps the first two; a tie at the k-th
    value keeps both members."""
    lp = np.log(np.array([0.5, 0.25, 0.125, 0.125], np.float32))
    u = np.array([0.0, 0.49, 0.51, 0.74, 0.76, 0.874, 0.876, 0.999])
    pick, l, kept, margin = U.sample_ref(lp, 1.0, -1, u)
    assert pick.tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and kept.all() and (l == lp).all()
    assert abs(margin[1] - 0.01) < 1e-6 and abs(margin[5] - 0.001) < 1e-6
    pick, _, kept, _ = U.sample_ref(lp, 1.0, 2, np.array([0.0, 0.66, 0.67, 0.999]))
    assert kept.tolist() == [True, True, False, False] and pick.tolist() == [0, 0, 1, 1]
    _, _, kept, _ = U.sample_ref(lp, 1.0, 3, np.array([0.5]))
    assert kept.all()  # ranks 3 and 4 tie: both stay
    # temp 1/2 squares the probabilities: EOS (token 0) masked, the rest 1/16, 1/64, 1/64: cdf 0, 4/6, 5/6, 1
    pick, l, kept, _ = U.sample_ref(lp, 0.5, -1, np.array([0.5, 0.7, 0.9]), eos=0)
    assert l[0] == np.float32(-1e20) / np.float32(0.5) and pick.tolist() == [1, 2, 3]


# ----------------------------------------------------------------- the stub
def _tiny():
    sc = U.Script(3, 4, 6, seed=9, T=5)
    return sc, sc.cpu_lp()


def test_stub_answers_from_the_tables_and_carries_chunks():
    sc, lp = _tiny()
    stub = U.Stub(sc, lp)
    src = torch.as_tensor(U.chunk_src([2, 0]))
    st = stub.decoder_state(ref_cpu.tile(stub.encode(src, None), 3), ref_cpu.tile(src, 3))
    assert st["chunk"].tolist() == [2, 2, 2, 0, 0, 0]
    tok = torch.tensor([1, 5, 0, 2, 2, 4])
    out = stub.decode_step(st, tok, 2)
    for r, (c, t) in enumerate(zip([2, 2, 2, 0, 0, 0], tok.tolist())):
        assert np.array_equal(out[r].numpy(), lp[c, 2, t]) and np.array_equal(st["attn"][r].numpy(), sc.ATT[c, 2, t])
    out[0, 0] = 7.0  # the searches write into what they get: the table must not change
    assert lp[2, 2, 1, 0] != 7.0 and stub.lp[2, 2, 1, 0] != 7.0
    stub.reorder(st, torch.tensor([4, 3, 3, 1]))
    assert st["chunk"].tolist() == [0, 0, 0, 2]


def test_greedy_on_the_stub_follows_the_table_by_hand():
    sc, lp = _tiny()
    stub = U.Stub(sc, lp)
    with U.pinned_topk(0.0):
        out = ref_cpu.greedy(stub, U.chunk_src([0, 1, 2]), np.ones(3), max_length=sc.S)
    for c in range(3):
        t = sc.bos
        for s in range(sc.S):
            assert np.array_equal(out["logp"][c, s], lp[c, s, t])
            t = int(np.argmax(lp[c, s, t]))
            assert out["tokens"][c, s] == t


def test_duplicates_are_bit_equal():
    sc = U.Script(2, 3, 9, seed=0, T=4, dup=((5, 6),))
    lp = sc.cpu_lp()
    assert np.array_equal(lp[..., 5], lp[..., 6])              # duplicate generator rows: equal logits
    assert np.array_equal(lp[:, :, 5, :], lp[:, :, 6, :])      # equal X rows: equal rows of log-probs
    assert np.array_equal(sc.ATT[:, :, 5], sc.ATT[:, :, 6])


def test_pinned_topk_is_the_lower_index_rule_and_refuses_near_ties():
    x = torch.tensor([[1.0, 3.0, 3.0, 0.5, 3.0, -1e20, -1e20]])
    with U.pinned_topk(1e-4) as log:
        v, i = x.topk(4)
    assert i.tolist() == [[1, 2, 4, 0]] and v.tolist() == [[3.0, 3.0, 3.0, 1.0]]
    assert log.ties == 2 and log.pairs == [(1, 2), (2, 4)] and log.min_gap == 0.5
    with pytest.raises(U.TieError):
        with U.pinned_topk(1e-4):
            torch.tensor([2.0, 2.00005, 1.0]).topk(1)
    with U.pinned_topk(1e-4):  # a near tie below the first value not selected is no selection
        torch.tensor([2.0, 1.5, 1.0, 1.00005]).topk(2)
    with U.pinned_topk(1e-4):  # masked candidates tie exactly
        torch.tensor([0.0, float("-inf"), float("-inf")]).topk(2)
    assert torch.Tensor.topk is not None and "pinned" not in repr(torch.Tensor.topk)


# ----------------------------------------------------------------- committed seeds
@pytest.mark.parametrize("beam,V", U.FAST_GRID)
def test_fast_grid_seeds_keep_the_margin(beam, V):
    for alpha in (0.0, 0.6):
        for min_len in (0, 3):
            sc = U.fast_grid_script(beam, V, alpha, min_len)
            lp = sc.cpu_lp()
            for n_best in sorted({1, 2, beam}):
                res, stub, log = U.ref_fast_beam(sc, lp, beam, n_best, alpha, min_len, margin=U.SEED_MARGIN)
                p = U.fast_props(sc, res, stub, log, beam, n_best)
                assert p["steps"] >= 3 and (n_best > 1 or len(set(p["steps_run"].tolist())) >= 2)
                if (beam, V) == (8, 32):
                    assert p["slots"] >= {0, 1, 2, 3}  # candidates 128..255 are selected
            if min_len:
                r0 = U.ref_fast_beam(sc, lp, beam, 1, alpha, 0, margin=0)[0]
                r1 = U.ref_fast_beam(sc, lp, beam, 1, alpha, min_len, margin=0)[0]
                assert any(not U.same_tokens(a, b) for a, b in zip(r0, r1))  # the mask matters


@pytest.mark.parametrize("name", sorted(U.FAST_SCENARIOS))
def test_fast_scenario_seeds(name):
    kw, beam, n_best, alpha, min_len, shows = U.FAST_SCENARIOS[name]
    sc = U.Script(**kw)
    res, stub, log = U.ref_fast_beam(sc, sc.cpu_lp(), beam, n_best, alpha, min_len, margin=U.SEED_MARGIN)
    assert shows(U.fast_props(sc, res, stub, log, beam, n_best), res, sc.S)


@pytest.mark.parametrize("name", sorted(U.classic_cases()))
def test_classic_case_seeds(name):
    sc, k = U.classic_case(name)
    lp = sc.cpu_lp()
    res, beams, cut, log = U.ref_classic_beam(sc, lp, k["groups"], k["beam"], k["n_best"], k["min_len"], k["opts"],
                                              k["lengths"], margin=U.SEED_MARGIN)
    U.classic_need(sc, lp, k, res, beams, log)
    if k["script"]["T"]:
        assert all(cut[c] < sc.T for c in cut)


def test_sampling_seeds_keep_the_margin():
    sc = U.sampling_script()
    lp = U.head_fp64(sc.X[0, 0, :1], **sc.head()).astype(np.float32)[0]
    for (temp, topk, step), seed in U.SAMPLE_SEEDS.items():
        pick, _, kept, margin = U.sample_ref(lp, temp, topk, U.draw_uniform_rows(seed, U.SAMPLE_R, step))
        assert margin.min() > 1e-4 and set(pick.tolist()) == set(np.flatnonzero(kept).tolist())
    for kind, t, first in (("tie", U.SAMPLE_TIE, U.SAMPLE_TIE["topk"] - 1), ("tie_in", U.SAMPLE_TIE_IN, 0)):
        sc = U.sampling_script(kind)
        lp = U.head_fp64(sc.X[0, 0, :1], **sc.head()).astype(np.float32)[0]
        a, b = t["dup"]
        assert lp[a] == lp[b] and sorted(np.argsort(-lp, kind="stable")[first: first + 2].tolist()) == [a, b]
        _, _, kept, margin = U.sample_ref(lp, 1.0, t["topk"], U.draw_uniform_rows(t["seed"], U.SAMPLE_R, t["step"]))
        assert margin.min() > 1e-4 and kept.sum() == t["topk"] + (kind == "tie")
