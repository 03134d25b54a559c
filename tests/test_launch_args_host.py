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
    rc = L.nd_op_lstm_layer(None, _buf(), opt(wih0), _buf(), _buf(), _buf(), 1, 4, _buf(), opt(bn_scale),
                            opt(bn_shift), 1, None)
    _refused(L, rc, b"lstm_layer: ")
