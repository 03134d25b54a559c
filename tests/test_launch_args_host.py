"""Decoder self-attention op entries, host side (no GPU): the refusals that come before any HIP call.  The
buffers are small host arrays standing in for device pointers: a refused call never reads them."""
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
