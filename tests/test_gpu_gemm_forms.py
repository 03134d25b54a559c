"""Every reachable form of every GEMM kernel family (needs an MI355X): for each route of launch_gemm and
launch_gemm_p16, each (LN, RELU, RESID) combination the route admits, on fp32 and on split-fp16 weights, at the
smallest shape that takes the route.  Each case asserts the route (nd_gemm_routes) and compares with the fp64
product to the 2e-4 absolute bound of test_gemm_vs_fp64 / test_gemm_p16_vs_fp64 (same input scaling).  A
shape's inputs and fp64 products are made once (on the GPU) and shared by its cases.

Forms no op entry can reach, so not run here:
  * the LayerNorm forms of the k-step-64 tile (gemm_f32_kernel<64, 64, 2, 2, 64>) and of the long-K and split-K
    P16 kernels (gemm_p16_kernel<1, 8, .>, gemm_p16k_kernel): the LN prologue needs K == 256, these run from
    K == 512 / 1024 on;
  * gemm_f32_kernel<256, 256, 2, 4, 32, H3 = false> with LN: fp32 weights at K == 256 on 256 x 256 tiles take the
    ring kernel (gemm_f32d_kernel) unless the call has P16 operands or the q24 epilogue, and both need a split
    image (its non-LN forms run at K == 32, below the ring's three k steps);
  * gemm_f32_kernel<128, .> and <256, .> on P16 operands are the same instantiations as on row-major ones (p16io
    is a runtime field), so the large-M route is run on the 64 x 64 tile only.
"""
import functools
import itertools

import pytest
import torch

from nanodecoder_amd import _lib

pytestmark = pytest.mark.gpu

BOUND = 2e-4
EPI = list(itertools.product([False, True], repeat=3))  # (ln, relu, res)
NO_LN = [e for e in EPI if not e[0]]


@functools.lru_cache(maxsize=None)
def _inputs(M, N, K):
    """The shape's operands on the GPU and its fp64 products {ln: LN?(A) W^T + b}."""
    g = torch.Generator().manual_seed(M + N + K)
    dev = torch.device("cuda", 0)
    t = dict(A=torch.randn(M, K, generator=g), W=torch.randn(N, K, generator=g) / K ** 0.5,
             b=torch.randn(N, generator=g), lg=1 + 0.1 * torch.randn(K, generator=g),
             lb=0.1 * torch.randn(K, generator=g))
    t = {k: v.to(dev) for k, v in t.items()}
    t["R"] = torch.randn(M, N, generator=torch.Generator(dev).manual_seed(M + N + K), device=dev)
    a, w, b = t["A"].double(), t["W"].double(), t["b"].double()
    t["ref"] = {False: a @ w.t() + b}
    if K == 256:
        t["ref"][True] = torch.nn.functional.layer_norm(a, (K,), t["lg"].double(), t["lb"].double(), 1e-6) @ w.t() + b
    return t


def _check(out, t, ln, relu, res):
    ref = t["ref"][ln]
    if relu:
        ref = ref.clamp_min(0)
    if res:
        ref = ref + t["R"].double()
    err = (out.double() - ref).abs().max().item()
    assert err < BOUND, err


def _routes_are(**want):
    torch.cuda.synchronize()
    got = {k: v for k, v in _lib.gemm_routes(reset=True).items() if v}
    assert got == want, got


def _cases(*groups):
    out = []
    for name, M, N, K, epis, splits in groups:
        for (ln, relu, res), split in itertools.product(epis, splits):
            k = K[ln] if isinstance(K, dict) else K
            out.append(pytest.param(name, M, N, k, ln, relu, res, split,
                                    id=f"{name}-{M}x{N}x{k}-{'ln' if ln else ''}{'relu' if relu else ''}"
                                       f"{'res' if res else ''}-{'split' if split else 'f32'}"))
    return out


K_LN = {False: 32, True: 256}
ROW_MAJOR = _cases(
    ("tile64", 37, 64, K_LN, EPI, [False, True]),
    ("tile64", 37, 64, 1024, NO_LN, [False, True]),                   # the k-step-64 tile
    ("tile128", 8192, 1024, K_LN, EPI, [False, True]),
    ("tile256", 4096, 4096, {False: 64, True: 256}, EPI, [False, True]),  # fp32: the ring kernel
    ("tile256", 4096, 4096, 32, NO_LN, [False]),                      # fp32 below the ring's k steps
)


@pytest.mark.parametrize("route,M,N,K,ln,relu,res,split", ROW_MAJOR)
def test_row_major_forms(route, M, N, K, ln, relu, res, split):
    from nanodecoder_amd.engine import op_gemm
    t = _inputs(M, N, K)
    _lib.gemm_routes(reset=True)
    out = op_gemm(t["A"], t["W"], t["b"], t["R"] if res else None, t["lg"] if ln else None, t["lb"] if ln else None,
                  relu, split=split)
    _routes_are(**{route: 1})
    _check(out, t, ln, relu, res)


def _p16_operands(t, ln, res):
    from nanodecoder_amd.engine import op_fold_layernorm, pack_p16, row_partials
    Wd, bd, part_in = t["W"], t["b"], None
    if ln:
        Wd, bd = op_fold_layernorm(Wd, bd, t["lg"], t["lb"])
        A = t["A"]
        part_in = row_partials(torch.cat([A, A.new_zeros((-A.shape[0]) % 16, A.shape[1])]))
    return pack_p16(t["A"]), Wd, bd, pack_p16(t["R"]) if res else None, part_in


P16 = _cases(
    ("p16_small", 16, 16, 256, EPI, [False, True]),
    ("p16s_2x4", 1024, 256, 256, EPI, [False, True]),
    ("p16s_2x2", 1376, 96, 256, EPI, [False, True]),
    ("p16_longk", 16, 16, 512, NO_LN, [False, True]),
    ("p16_longk", 16, 16, 1024, NO_LN, [False, True]),
    ("p16_longk", 16, 16, 2048, NO_LN, [False, True]),
    ("p16_big", 2048, 512, 256, EPI, ["rm"]),
)


@pytest.mark.parametrize("route,M,N,K,ln,relu,res,split", P16)
def test_p16_forms(route, M, N, K, ln, relu, res, split):
    from nanodecoder_amd.engine import op_gemm_p16, op_pack_p16h, op_split_weight, pack_p16, unpack_p16
    t = _inputs(M, N, K)
    Ap, Wd, bd, Rp, part_in = _p16_operands(t, ln, res)
    Wh, sc = op_pack_p16h(Wd) if split else (None, 1.0)
    Wr, sr = op_split_weight(Wd) if split == "rm" else (None, 1.0)
    _lib.gemm_routes(reset=True)
    Cp, _ = op_gemm_p16(Ap, pack_p16(Wd), bd, M, N, K, Rp, part_in, relu, None, Wh=Wh, wscale=sc, Wh_rm=Wr,
                        wscale_rm=sr)
    _routes_are(**({"p16_big": 1, "tile64": 1} if route == "p16_big" else {route: 1}))
    _check(unpack_p16(Cp, M), t, ln, relu, res)


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("split", [False, True])
def test_p16_splitk_forms(res, split):
    from nanodecoder_amd.engine import op_gemm_p16_splitk, op_gemm_p16_splitk_f32, op_pack_p16h, pack_p16, unpack_p16
    M, N, K = 160, 32, 1024
    t = _inputs(M, N, K)
    Ap, Rp = pack_p16(t["A"]), pack_p16(t["R"]) if res else None
    _lib.gemm_routes(reset=True)
    if split:
        Wh, sc = op_pack_p16h(t["W"])
        Cp, _, _ = op_gemm_p16_splitk(Ap, Wh, sc, t["b"], M, N, K, Rp)
    else:
        Cp, _, _ = op_gemm_p16_splitk_f32(Ap, pack_p16(t["W"]), t["b"], M, N, K, Rp)
    _routes_are(p16_splitk=1)
    _check(unpack_p16(Cp, M), t, False, False, res)


@pytest.mark.parametrize("M,N,route", [(2048, 128, "p16s_2x4"), (48, 3200, "p16s_2x2")])
@pytest.mark.parametrize("split", [False, True])
def test_retired_p16_routes_stay_zero(M, N, route, split):
    """K == 256 with LN at the shapes a reading of launch_gemm_p16's ladder line by line would send to the
    p16_ln128 / p16_n64 tiles: (N/128) ceil(M/16) >= 128 implies (N/64) ceil(M/32) >= 128, and (N/64) ceil(M/16)
    >= 128 implies (N/32) ceil(M/32) >= 128, so the LDS-staged kernels above them take every such shape."""
    from nanodecoder_amd.engine import op_gemm_p16, op_pack_p16h, pack_p16, unpack_p16
    t = _inputs(M, N, 256)
    Ap, Wd, bd, _, part_in = _p16_operands(t, True, False)
    Wh, sc = op_pack_p16h(Wd) if split else (None, 1.0)
    _lib.gemm_routes(reset=True)
    Cp, _ = op_gemm_p16(Ap, pack_p16(Wd), bd, M, N, 256, None, part_in, False, None, Wh=Wh, wscale=sc)
    torch.cuda.synchronize()
    routes = _lib.gemm_routes(reset=True)
    assert routes["p16_n64"] == 0 and routes["p16_ln128"] == 0
    assert {k: v for k, v in routes.items() if v} == {route: 1}
    _check(unpack_p16(Cp, M), t, True, False, False)
