"""Decoder attention, FFN, P16 GEMM, encoder attention and encoder layer-0 op entries whose refusal comes from the launcher, most
of them after the kernel attributes are set (needs an MI355X): each returns ND_ERR_ARG and launches nothing
(the output keeps its sentinel)."""
import ctypes

import pytest
import torch

from nanodecoder_amd import _lib

pytestmark = pytest.mark.gpu

C, T = 2, 16
PAD = ctypes.c_float(0.0)


@pytest.fixture(scope="module")
def bufs():
    dev = torch.device("cuda", 0)
    f = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
    return dict(q=f(16 * 2048), kv=f(C * T * 1600), bank=f(C * 512 * 256), ks=f(C * 512), part=f(2 * 64 * 8 * 272),
                em=torch.zeros(C, dtype=torch.int32, device=dev), signal=f(C * T) + 1.0,
                span=torch.full((C,), T, dtype=torch.int32, device=dev),
                clist=torch.arange(C + 1, dtype=torch.int32, device=dev).clamp(max=C - 1),
                out=torch.full((16 * 2048,), -7.25, dtype=torch.float32, device=dev))


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _refused(bufs, rc, what):
    L = _lib.lib()
    assert rc == _lib.ND_ERR_ARG, (rc, L.nd_last_error())
    err = L.nd_last_error()
    assert err.startswith(what + b": ") and b"bad arguments" not in err, err  # the launcher's refusal
    torch.cuda.synchronize()
    assert bool((bufs["out"] == -7.25).all()), "a refused call launched a kernel"


@pytest.mark.parametrize("rpc,t", [(9, T), (1, 513)])
def test_ctx_attention_refuses(bufs, rpc, t):
    b = bufs
    rc = _lib.lib().nd_op_dec_ctx_attention(_p(b["q"]), _p(b["kv"]), 512, 0, _p(b["signal"]), _p(b["span"]), PAD,
                                            _p(b["out"]), C, rpc, t, None)
    _refused(b, rc, b"dec_ctx_attention")


@pytest.mark.parametrize("ccap,nsplit", [(0, 1), (C + 1, 1), (C, 65)])
def test_ctx_attention_list_refuses(bufs, ccap, nsplit):
    b = bufs
    rc = _lib.lib().nd_op_dec_ctx_attention_list(_p(b["q"]), _p(b["kv"]), 512, 0, 0, _p(b["signal"]), _p(b["span"]),
                                                 PAD, _p(b["out"]), C, 1, T, _p(b["clist"]), ccap, nsplit,
                                                 _p(b["part"]), None, None)
    _refused(b, rc, b"dec_ctx_attention_list")


@pytest.mark.parametrize("rpc,ldT", [(2, T), (1, T - 1)])
def test_mem_attention_refuses(bufs, rpc, ldT):
    b = bufs
    rc = _lib.lib().nd_op_dec_mem_attention(_p(b["q"]), _p(b["bank"]), _p(b["signal"]), _p(b["span"]), PAD,
                                            _p(b["out"]), C, rpc, T, ldT, 0, None)
    _refused(b, rc, b"dec_mem_attention")


def test_bank_d8_refuses_long_chunk(bufs):
    b = bufs
    rc = _lib.lib().nd_op_dec_bank_d8(_p(b["q"]), _p(b["bank"]), _p(b["ks"]), _p(b["em"]), _p(b["signal"]),
                                      _p(b["span"]), PAD, _p(b["out"]), C, 513, None, 0, None)
    _refused(b, rc, b"dec_bank_d8")


def _enc_ffn(b, y, x, F):
    w = _p(b["q"])
    return _lib.lib().nd_op_enc_ffn(y, w, 1.0, w, w, 1.0, w, x, _p(b["part"]), 16, F, None, None)


def test_enc_ffn_refuses_ragged_d_ff(bufs):
    _refused(bufs, _enc_ffn(bufs, _p(bufs["q"]), _p(bufs["out"]), 48), b"enc_ffn")  # F % 32 != 0


def test_enc_ffn_refuses_in_place(bufs):
    _refused(bufs, _enc_ffn(bufs, _p(bufs["out"]), _p(bufs["out"]), 64), b"enc_ffn")  # x == y without the Wo fold


def test_enc_ffn_wo_refuses_attention_rows_as_output(bufs):
    b = bufs
    w, x = _p(b["q"]), _p(b["out"])
    rc = _lib.lib().nd_op_enc_ffn_wo(x, _p(b["kv"]), w, 1.0, w, w, 1.0, w, w, 1.0, w, x, _p(b["part"]), None, 1.0,
                                     None, None, 16, 64, None, None)  # att == x
    _refused(b, rc, b"enc_ffn_wo")


@pytest.mark.parametrize("M,nsplit,slab", [
    (24, 1, True),    # P16 rows come in blocks of 16
    (16, 3, True),    # more splits than d_ff has 32-wide chunks (F = 64)
    (16, 2, False),   # a split launch needs its slab
])
def test_dec_ffn_refuses(bufs, M, nsplit, slab):
    b = bufs
    w = _p(b["q"])
    rc = _lib.lib().nd_op_dec_ffn(_p(b["kv"]), w, 1.0, w, w, 1.0, w, _p(b["out"]), _p(b["part"]), M, 64, nsplit,
                                  _p(b["bank"]) if slab else None, _p(b["em"]), None, 1, None, None)
    _refused(b, rc, b"dec_ffn")


@pytest.mark.parametrize("N,K", [(24, 256), (16, 384)])  # N % 16 != 0; no kernel for this K
def test_gemm_p16_refuses(bufs, N, K):
    b = bufs
    rc = _lib.lib().nd_op_gemm_p16(_p(b["kv"]), _p(b["bank"]), _p(b["q"]), None, _p(b["out"]), 16, N, K, None, 0,
                                   None, 0, None, None)
    _refused(b, rc, b"gemm_p16")


def test_gemm_p16_split_refuses_partial_count(bufs):
    b = bufs
    rc = _lib.lib().nd_op_gemm_p16_split(_p(b["kv"]), _p(b["bank"]), 1.0, _p(b["q"]), None, _p(b["out"]), 16, 16, 256,
                                         _p(b["part"]), 3, None, 0, None, None)  # 3 partials do not tile 256 columns
    _refused(b, rc, b"gemm_p16_split")


def test_enc_attention_refuses_long_chunk(bufs):
    b = bufs
    rc = _lib.lib().nd_op_enc_attention(_p(b["bank"]), _p(b["signal"]), _p(b["span"]), _p(b["out"]), C, 513, None)
    _refused(b, rc, b"enc_attention")


@pytest.mark.parametrize("t,null", [(513, None), (0, None), (-1, None), (T, "signal"), (T, "span"), (T, "w_in"),
                                    (T, "b_in"), (T, "nwqkv"), (T, "nbqkv"), (T, "out")])
def test_enc_layer0_refuses(bufs, t, null):
    """T outside 1..512 or a null input: refused before the preparation's launch (nothing written)."""
    b = bufs
    a = dict(signal=_p(b["signal"]), span=_p(b["span"]), w_in=_p(b["q"]), b_in=_p(b["q"]), nwqkv=_p(b["bank"]),
             nbqkv=_p(b["q"]), out=_p(b["out"]))
    if null:
        a[null] = None
    prep = torch.full((6 * 256 + 48,), -7.25, dtype=torch.float32, device=b["out"].device)
    scal = torch.full((4,), -7.25, dtype=torch.float64, device=b["out"].device)
    rc = _lib.lib().nd_op_enc_layer0(a["signal"], a["span"], a["w_in"], a["b_in"], a["nwqkv"], a["nbqkv"], a["out"],
                                     C, t, _p(prep), _p(scal), ctypes.c_void_p(prep.data_ptr() + 6 * 256 * 4), None)
    _refused(b, rc, b"enc_layer0")
    assert bool((prep == -7.25).all()) and bool((scal == -7.25).all())


# ----------------------------------------------------------------- output head and search entries
SV, SS, SC = 9, 4, 3  # vocabulary, steps, chunks of the search refusals


def _search_state(b, beam=4, n_best=2, T=0):
    from nanodecoder_amd.engine import BeamOpState
    return BeamOpState(SC, min(beam, 8), n_best, SS, b["out"].device, T=T)


def _head_args(b, V):
    w = _p(b["q"])
    return (_p(b["kv"]), w, w, w, w, V)


def _next_args(b):
    return (_p(b["bank"]), None, _p(b["out"]), _p(b["part"]), None)  # emb, pe, ne_x, ne_part, ne_tok


@pytest.mark.parametrize("V,temp,topk,sample", [
    (0, 1.0, -1, False), (33, 1.0, -1, False),                        # V outside [1, 32]
    (SV, 0.0, -1, True), (SV, 1.0, 1, True), (SV, 1.0, SV + 1, True),  # sampling that is argmax, or keeps > V
])
def test_greedy_head_refuses(bufs, V, temp, topk, sample):
    b = bufs
    seed = torch.ones(1, dtype=torch.int64, device=b["out"].device)
    rc = _lib.lib().nd_op_greedy_head(*_head_args(b, V), SS, 0, 0, 0, 4, *_next_args(b), _p(b["em"]), _p(b["clist"]),
                                      _p(b["ks"]), None, temp, topk, _p(seed) if sample else None, None)
    _refused(b, rc, b"greedy_head")


@pytest.mark.parametrize("V,beam,n_best,ccap", [
    (0, 4, 2, None), (33, 4, 2, None),  # V outside [1, 32]
    (SV, 9, 2, None),                   # beam > 8
    (32, 9, 2, None),                   # beam * V > 256
    (SV, 4, 5, None),                   # n_best > beam
    (SV, 4, 2, 0), (SV, 4, 2, SC + 1),  # ccap outside [1, C]
])
def test_beam_step_refuses(bufs, V, beam, n_best, ccap):
    b = bufs
    st = _search_state(b, beam, n_best)
    rc = _lib.lib().nd_op_beam_step(*_head_args(b, V), *_next_args(b), st.ref(), SC, beam, n_best, 0, SS, 0, 0, 0.0,
                                    _p(b["clist"]) if ccap is not None else None, ccap or 0, None)
    _refused(b, rc, b"beam_step")


@pytest.mark.parametrize("V,beam,n_best,cov,T,ngram", [
    (6, 8, 2, 0, 0, 0),    # V < beam: step 0 has V candidates only
    (SV, 9, 2, 0, 0, 0),   # beam > 8
    (SV, 4, 5, 0, 0, 0),   # n_best > beam
    (SV, 4, 2, 1, 0, 0),   # a coverage penalty without attn / cut / cov
    (SV, 4, 2, 0, 0, SS + 1),  # an n-gram longer than the run
])
def test_beam_classic_step_refuses(bufs, V, beam, n_best, cov, T, ngram):
    b = bufs
    st = _search_state(b, beam, n_best, T)
    opts = _lib.NdClassicOpts(coverage_penalty=cov, beta=0.1, block_ngram_repeat=ngram)
    rc = _lib.lib().nd_op_beam_classic_step(*_head_args(b, V), *_next_args(b), st.ref(), SC, beam, n_best, 0, SS, 0,
                                            0, ctypes.byref(opts), None)
    _refused(b, rc, b"beam_classic_step")


def test_beam_classic_finish_refuses_more_hypotheses_than_beams(bufs):
    b = bufs
    st = _search_state(b, 4, 2)
    opts = _lib.NdClassicOpts()
    tokens = torch.full((SC * 5 * SS,), -7, dtype=torch.int32, device=b["out"].device)
    rc = _lib.lib().nd_op_beam_classic_finish(st.ref(), SC, 4, 5, SS, ctypes.byref(opts), _p(tokens), _p(b["out"]),
                                              _p(b["em"]), None)
    _refused(b, rc, b"beam_classic_finish")
    assert bool((tokens == -7).all())


@pytest.mark.parametrize("attn,T,max_len", [(False, 4, SS), (True, 9, SS), (True, 4, SS + 1)])
def test_beam_attn_gather_refuses(bufs, attn, T, max_len):
    """no captured attention; rows wider than the capture's; more steps than the state holds"""
    b = bufs
    st = _search_state(b, 4, 2, T=8 if attn else 0)
    rc = _lib.lib().nd_op_beam_attn_gather(st.ref(), SC, 2, SS, max_len, T, _p(b["out"]), None)
    _refused(b, rc, b"beam_attn_gather")


@pytest.mark.parametrize("R,rpc,t", [(0, 1, 4), (4, 0, 4), (4, 1, 0)])
def test_attn_step_softmax_refuses(bufs, R, rpc, t):
    b = bufs
    rc = _lib.lib().nd_op_attn_step_softmax(_p(b["out"]), 16, _p(b["span"]), R, rpc, t, None)
    _refused(b, rc, b"attn_step_softmax")
