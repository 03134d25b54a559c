"""Decoder self-attention, GEMM and LSTM op entries, host side (no GPU): the refusals that come before any HIP
call.  The buffers are small host arrays standing in for device pointers: a refused call never reads them."""
import ctypes

import pytest

from nanodecoder_amd import _lib, build


@pytest.fixture(scope="module")
def L():
    build.build()
    return _lib.lib()


def _buf(n=16):
    return ctypes.cast((ctypes.c_float * n)(), ctypes.c_void_p)


def _refused(L, rc, what):
    assert rc == _lib.ND_ERR_ARG, rc
    assert what in L.nd_last_error()


def test_self_attention_refuses_step_at_max_steps(L):
    rc = L.nd_op_dec_self_attention(_buf(), _buf(), None, 0, 8, 8, _buf(), 2, None)
    _refused(L, rc, b"dec_self_attention: ")


@pytest.mark.parametrize("tok0,hist_ld,step", [
    (2, 8, 10),   # keys up to step - 1 need hist[r][0 .. step - 2]: hist_ld < step - 1
    (7, 16, 3),   # tok0 >= V
])
def test_self_attention_table_refuses(L, tok0, hist_ld, step):
    V, steps, R = 7, 16, 2
    rc = L.nd_op_dec_self_attention_table(_buf(), steps, V, _buf(), tok0, _buf(), hist_ld, _buf(), step, steps,
                                          _buf(), R, None)
    _refused(L, rc, b"dec_self_attention_table: ")
    assert b"bad arguments" not in L.nd_last_error()  # the launcher's refusal, not the entry's null checks


@pytest.mark.parametrize("R,rpc", [(18, 9), (7, 2)])  # more rows per chunk than the kernels hold; R % rpc != 0
def test_self_attention_beam_refuses(L, R, rpc):
    rc = L.nd_op_dec_self_attention_beam(_buf(), _buf(), _buf(), 8, 1, 8, _buf(), R, rpc, None, None)
    _refused(L, rc, b"dec_self_attention_beam: ")


@pytest.mark.parametrize("M,N,K,norm", [
    (8, 64, 48, 0),   # K % 32 != 0
    (8, 64, 64, 1),   # the LayerNorm prologue serves K == 256 only
    (8, 48, 32, 0),   # N is no multiple of the narrowest tile (64)
])
def test_gemm_refuses(L, M, N, K, norm):
    rc = L.nd_op_gemm(_buf(), _buf(), _buf(), None, _buf(), M, N, K, norm, 0, None)
    _refused(L, rc, b"gemm: ")


def test_gemm_split_refuses_null_image(L):
    rc = L.nd_op_gemm_split(_buf(), None, 1.0, _buf(), None, _buf(), 8, 64, 32, 0, 0, None)
    _refused(L, rc, b"gemm_split: ")


@pytest.mark.parametrize("wih0,bn_scale,bn_shift", [
    (False, False, False),  # layer 0 computes its projections from signal, wih0 and bsum
    (True, True, False),    # BatchNorm needs both of scale and shift
    (True, False, True),
])
def test_lstm_layer_refuses(L, wih0, bn_scale, bn_shift):
    opt = lambda on: _buf() if on else None
    for entry in (L.nd_op_lstm_layer, L.nd_op_lstm_layer_f32):  # the split-fp16 form and the exact-fp32 one
        rc = entry(None, _buf(), opt(wih0), _buf(), _buf(), _buf(), 1, 4, _buf(), opt(bn_scale), opt(bn_shift), 1, None)
        _refused(L, rc, b"lstm_layer: ")


@pytest.mark.parametrize("entry", ["nd_op_lstm_layer", "nd_op_lstm_layer_f32"])
@pytest.mark.parametrize("kw", [dict(B=0), dict(T=0), dict(xp=False), dict(whh=False), dict(len=False),
                                dict(out=False)])
def test_lstm_layer_refuses_bad_arguments(L, entry, kw):
    """no rows, no steps, a null among the projected form's required pointers"""
    a = dict(xp=True, whh=True, len=True, out=True, B=1, T=4)
    a.update(kw)
    opt = lambda on: _buf() if on else None
    rc = getattr(L, entry)(opt(a["xp"]), None, None, None, opt(a["whh"]), opt(a["len"]), a["B"], a["T"],
                           opt(a["out"]), None, None, 0, None)
    _refused(L, rc, b"lstm_layer: bad arguments")


def _enc_attention_ex(L, qkv=True, signal=True, span=True, out=True, B=1, T=4, exact=0):
    opt = lambda on: _buf() if on else None
    return L.nd_op_enc_attention_ex(opt(qkv), opt(signal), opt(span), opt(out), B, T, exact, None, None)


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("kw", [dict(qkv=False), dict(signal=False), dict(span=False), dict(out=False), dict(B=0)])
def test_enc_attention_ex_refuses_bad_arguments(L, kw, exact):
    """each null pointer, no chunks: the entry's own checks, for either form"""
    _refused(L, _enc_attention_ex(L, exact=exact, **kw), b"enc_attention_ex: bad arguments")


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("T", [0, 513])
def test_enc_attention_ex_launcher_refuses_chunk_length(L, T, exact):
    _refused(L, _enc_attention_ex(L, T=T, exact=exact), b"enc_attention_ex: ")
    assert b"bad arguments" not in L.nd_last_error()


# ----------------------------------------------------------------- output head and search entries
def _state(null=None):
    """An nd_beam_state whose members all point at one small host array (never read by a refused call)."""
    keep = (ctypes.c_float * 16)()
    p = ctypes.cast(keep, ctypes.c_void_p).value
    st = _lib.NdBeamState()
    for name, kind in _lib.NdBeamState._fields_:
        if name == "T":
            st.T = 4
        elif name in ("seq", "anc", "cov", "blk"):
            getattr(st, name)[0] = getattr(st, name)[1] = p
        else:
            setattr(st, name, p)
    if null:
        setattr(st, null, None)
    st._keep = keep
    return st


def _greedy_head(L, V=9, S=4, step=0, eos=3, R=2, x=True, temp=1.0, topk=-1, seed=False):
    b = _buf()
    return L.nd_op_greedy_head(b if x else None, b, b, b, b, V, S, step, 0, eos, R, b, None, b, b, None, b, b, b,
                               None, temp, topk, b if seed else None, None)


@pytest.mark.parametrize("kw", [dict(step=4), dict(step=-1), dict(eos=9), dict(eos=-1), dict(R=0), dict(S=0),
                                dict(x=False)])
def test_greedy_head_refuses_bad_arguments(L, kw):
    """a step outside [0, S), EOS outside the vocabulary (the mask would write past the row's log-probs), no rows,
    a null input: the entry's own checks"""
    _refused(L, _greedy_head(L, **kw), b"greedy_head: bad arguments")


@pytest.mark.parametrize("kw", [dict(V=0), dict(V=33, eos=3), dict(seed=True, temp=0.0), dict(seed=True, topk=1),
                                dict(seed=True, topk=10)])
def test_greedy_head_launcher_refuses(L, kw):
    _refused(L, _greedy_head(L, **kw), b"greedy_head: ")
    assert b"bad arguments" not in L.nd_last_error()


def _beam_step(L, classic, V=9, beam=4, n_best=2, step=0, S=4, eos=3, C=3, null=None, ccap=None, opts=None):
    b, st = _buf(), _state(null)
    head = (b, b, b, b, b, V, b, None, b, b, None, ctypes.byref(st), C, beam, n_best, step, S, 0, eos)
    if classic:
        o = opts if opts is not None else _lib.NdClassicOpts()
        return L.nd_op_beam_classic_step(*head, ctypes.byref(o), None)
    return L.nd_op_beam_step(*head, 0.6, b if ccap is not None else None, ccap or 0, None)


@pytest.mark.parametrize("classic", [False, True])
@pytest.mark.parametrize("kw", [dict(step=4), dict(eos=9), dict(C=0), dict(null="cum"), dict(null="hyp_anc")])
def test_beam_step_refuses_bad_arguments(L, classic, kw):
    what = b"beam_classic_step: bad arguments" if classic else b"beam_step: bad arguments"
    _refused(L, _beam_step(L, classic, **kw), what)


def test_beam_classic_step_refuses_bad_arguments(L):
    _refused(L, _beam_step(L, True, null="grp_done"), b"beam_classic_step: bad arguments")
    _refused(L, _beam_step(L, True, opts=_lib.NdClassicOpts(length_penalty=3)), b"beam_classic_step: bad arguments")
    _refused(L, _beam_step(L, True, opts=_lib.NdClassicOpts(coverage_penalty=-1)), b"beam_classic_step: bad arguments")


@pytest.mark.parametrize("classic,kw", [
    (False, dict(V=33)), (False, dict(beam=9)), (False, dict(V=32, beam=9)), (False, dict(n_best=5)),
    (False, dict(ccap=0)), (False, dict(ccap=4)),
    (True, dict(V=6, beam=8)), (True, dict(n_best=5)), (True, dict(null="attn", opts=_lib.NdClassicOpts(coverage_penalty=1))),
])
def test_beam_step_launcher_refuses(L, classic, kw):
    _refused(L, _beam_step(L, classic, **kw), b"beam_classic_step: " if classic else b"beam_step: ")
    assert b"bad arguments" not in L.nd_last_error()


def test_beam_init_and_finish_refuse_bad_arguments(L):
    b, st, o = _buf(), _state(), _lib.NdClassicOpts()
    _refused(L, L.nd_op_beam_init(ctypes.byref(st), 3, 9, 2, None), b"beam_init: bad arguments")
    _refused(L, L.nd_op_beam_init(None, 3, 4, 2, None), b"beam_init: bad arguments")
    _refused(L, L.nd_op_beam_classic_init(ctypes.byref(st), None, 3, 4, 2, None), b"beam_classic_init: bad arguments")
    _refused(L, L.nd_op_beam_finish(ctypes.byref(st), 3, 0, 4, b, b, b, None), b"beam_finish: bad arguments")
    _refused(L, L.nd_op_beam_finish(ctypes.byref(st), 3, 2, 4, None, b, b, None), b"beam_finish: bad arguments")
    _refused(L, L.nd_op_beam_classic_finish(ctypes.byref(st), 3, 4, 2, 4, None, b, b, b, None),
             b"beam_classic_finish: bad arguments")
    _refused(L, L.nd_op_beam_classic_finish(ctypes.byref(st), 3, 4, 5, 4, ctypes.byref(o), b, b, b, None),
             b"beam_classic_finish: ")
    assert b"bad arguments" not in L.nd_last_error()  # n_best > beam: the launcher's


def test_attention_capture_entries_refuse(L):
    b, st = _buf(), _state()
    _refused(L, L.nd_op_attn_step_softmax(None, 16, b, 4, 1, 4, None), b"attn_step_softmax: bad arguments")
    _refused(L, L.nd_op_attn_step_softmax(b, 3, b, 4, 1, 4, None), b"attn_step_softmax: bad arguments")  # ld < T
    _refused(L, L.nd_op_attn_step_softmax(b, 16, b, 0, 1, 4, None), b"attn_step_softmax: ")
    _refused(L, L.nd_op_beam_attn_gather(ctypes.byref(st), 3, 2, 4, 4, 4, None, None), b"beam_attn_gather: bad arguments")
    _refused(L, L.nd_op_beam_attn_gather(ctypes.byref(st), 3, 2, 4, 4, 5, b, None), b"beam_attn_gather: ")  # T > st.T
    _refused(L, L.nd_op_beam_attn_gather(ctypes.byref(_state("attn")), 3, 2, 4, 4, 4, b, None), b"beam_attn_gather: ")
