"""Decoder attention op entries that set kernel attributes before they validate (needs an MI355X): each
refusal returns ND_ERR_ARG from the launcher and launches nothing (the output keeps its sentinel)."""
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
