"""The fused FFN block at op level (csrc/ffn.hip enc_ffn_kernel: nd_op_enc_ffn,
nd_op_enc_ffn_wo in place without and with the QKV fold, nd_op_dec_ffn)
against the fp64 reference of the same block (tests/ffn_util.py), needs an
MI355X.

Bar, per case, form and output (x, and qkv of the "wo_qkv" form):

    err = max |got - fp64|  <=  K (E32 + sqrt(n_acc) 2^-25 max|ref|)
    and  err < 2e-4 max(1, max|ref| / 8),      K = 8.

E32 is the error against fp64 of the same block in plain fp32 on the CPU;
n_acc the number of fp32 roundings the residual-carrying accumulator takes
(3 d_ff / 32, 24 more under the Wo fold; the decoder form: split 0's share
plus nsplit).  tests/test_ffn_scheme.py derives the bar and K on the CPU from
a numpy model of the scheme (which stays within a quarter of it) and shows
that the model with one lo term left out of one chunk is beyond it.  The row
statistics answer to fp64 statistics of the returned x itself: mean within
2^-22 max|x_row|, M2 within 1e-5 relative plus 256 (2^-23 max|x_row|)^2.
Neither bar is taken from a kernel.  Measured: at most 0.49 of the bar (x), 0.52
(qkv), 0.53 and 0.03 (mean, M2); per case in DESIGN.md section 5.

Every output buffer carries guard rows past M, pre-filled; no index leaves them.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import ffn_util as U

pytestmark = pytest.mark.gpu

D = U.D
FILL = -7.25
GUARD = 32      # rows past M (M16 for the decoder form: two P16 row groups)
FORMS = pytest.mark.parametrize("form", U.FORMS)
WEIGHTS = ("W1", "b1", "W2", "b2", "lg", "lb")


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _w(case):
    """The case's weights on the device, uploaded once per case."""
    if "_dev" not in case:
        case["_dev"] = {k: _t(case[k]) for k in WEIGHTS + ("Wo", "bo", "Wq", "bq", "lq", "lqb")}
    return case["_dev"]


def _run(case, form, nsplit=1, y=None, att=None, tickets=None, skip=None, skip_rpc=1, null_slab=False):
    """One launch of a form on a case (y / att: rows to use instead of the case's).  dict of x [M, 256],
    mean and m2 [M], qkv [M, 768] or None, the guard word, the tickets, and `clean`: every guard row of x, part
    and qkv and every part slot past the first still holds FILL."""
    from nanodecoder_amd import _lib
    from nanodecoder_amd import engine as E
    w = _w(case)
    y = case["y"] if y is None else y
    att = case["att"] if att is None else att
    M = y.shape[0]
    dev = _dev()
    full = lambda rows, *s: torch.full((rows,) + s, FILL, dtype=torch.float32, device=dev)
    args = [w[k] for k in WEIGHTS]
    qkv = None
    if form == "dec":
        yp = E.pack_p16(_t(y))
        M16 = yp.shape[0]
        xb, part = full(M16 + GUARD, D), full(M16 + GUARD, 16, 2)
        if null_slab:
            # nsplit = 1 needs neither slab nor tickets: the raw entry with both null
            assert nsplit == 1 and skip is None
            W1f, b1f = E.op_fold_layernorm(w["W1"], w["b1"], w["lg"], w["lb"])
            w1h, w1s = E.op_pack_p16h(W1f)
            w2h, w2s = E.op_pack_p16h(w["W2"])
            ov = torch.zeros(1, dtype=torch.int32, device=dev)
            p = lambda t: ctypes.c_void_p(t.data_ptr())
            s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(_lib.lib().nd_op_dec_ffn(p(yp), p(w1h), w1s, p(b1f), p(w2h), w2s, p(w["b2"]), p(xb), p(part),
                                                M16, case["F"], 1, None, None, None, 1, p(ov), s), "nd_op_dec_ffn")
        else:
            x_, _, ov, tickets = E.op_dec_ffn(yp, *args, nsplit, skip=skip, skip_rpc=skip_rpc, tickets=tickets, x=xb,
                                              part=part)
            assert x_ is xb
        torch.cuda.synchronize()
        x = E.unpack_p16(xb[:M16])[:M].cpu().numpy()
        rows = M16
    else:
        part = full(M + GUARD, 16, 2)
        if form == "none":
            xb = full(M + GUARD, D)
            x_, _, ov = E.op_enc_ffn(_t(y), *args, x=xb, part=part)
        else:
            xb = full(M + GUARD, D)
            xb[:M] = _t(y)
            kw = dict(att=_t(att), Wo=w["Wo"], bo=w["bo"], inplace=True, part=part)
            if form == "wo_qkv":
                qkv = full(M + GUARD, U.NQ)
                x_, _, ov, q_ = E.op_enc_ffn(xb[:M], *args, Wq=w["Wq"], bq=w["bq"], lnq_g=w["lq"], lnq_b=w["lqb"],
                                             qkv=qkv, **kw)
                assert q_ is qkv
            else:
                x_, _, ov = E.op_enc_ffn(xb[:M], *args, **kw)
        torch.cuda.synchronize()
        assert x_.data_ptr() == xb.data_ptr()
        x = xb[:M].cpu().numpy()
        rows = M
    part = part.cpu().numpy()
    clean = bool((xb[rows:] == FILL).all().item()) and bool((part[rows:] == FILL).all()) \
        and bool((part[:, 1:] == FILL).all())
    if qkv is not None:
        qkv = qkv.cpu().numpy()
        clean = clean and bool((qkv[M:] == FILL).all())
        qkv = qkv[:M]
    return dict(x=x, mean=part[:M, 0, 0], m2=part[:M, 0, 1], qkv=qkv, word=int(ov.item()), tickets=tickets,
                clean=clean)


def _check(case, form, out, nsplit=1):
    """x, the statistics and qkv of a launch against the module's bars; the guard rows and unused part slots
    keep their fill; the guard word stays 0."""
    name = f"{case['name']} [{form}{f' nsplit {nsplit}' if form == 'dec' else ''}]"
    assert out["word"] == 0, name
    assert out["clean"], name
    ys = U.yardsticks(case, form in ("wo", "wo_qkv"))
    for which in ("x", "qkv") if form == "wo_qkv" else ("x",):
        assert np.isfinite(out[which]).all(), name
        err = U.error(case, form, out[which], which)
        new, old = U.bars(case, form, which, nsplit)
        e32, mx = (ys["e32"], ys["mx"]) if which == "x" else (ys["e32q"], ys["mxq"])
        print(f"{name} {which}: max|ref| {mx:.4g}  E32 {e32:.3e}  err {err:.3e}  err/E32 {err / e32:.2f}  "
              f"err/bar {err / new:.3f}")
        assert err < old, (name, which, err, old)
        assert err <= new, (name, which, err, new)
    rm, rq = U.stats_miss(out["x"], out["mean"], out["m2"])
    print(f"{name} statistics: mean {rm:.3f}  M2 {rq:.3f} of their bars")
    assert rm <= 1.0, (name, rm)
    assert rq <= 1.0, (name, rq)


def _same(a, b, rows_a, rows_b, name):
    for k in ("x", "mean", "m2", "qkv"):
        if a[k] is not None:
            assert np.array_equal(a[k][rows_a], b[k][rows_b], equal_nan=True), (name, k)


@FORMS
@pytest.mark.parametrize("group", U.GROUPS)
def test_cases_vs_fp64(group, form):
    """Every case of a group in a form (the decoder form over two splits where d_ff has two chunks)."""
    for case in U.cases(group):
        ns = min(2, case["F"] // U.HC) if form == "dec" else 1
        _check(case, form, _run(case, form, ns), ns)


@FORMS
def test_rows_do_not_depend_on_their_block(form):
    """Rows of a case run at M = 131 are, bit for bit, the same rows run alone at M = 16 from offset 0 of a
    block: rows 100 .. 115 (the middle of block 0) and 115 .. 130 (across the block boundary into the ragged
    block)."""
    case = U.unit_case(131, 160)
    ns = 2 if form == "dec" else 1
    whole = _run(case, form, ns)
    _check(case, form, whole, ns)
    for r0 in (100, 115):
        rows = slice(r0, r0 + 16)
        alone = _run(case, form, ns, y=case["y"][rows], att=case["att"][rows])
        assert alone["clean"]
        _same(whole, alone, rows, slice(None), (form, r0))


@pytest.mark.parametrize("form,what", [(f, "y") for f in U.FORMS] + [("wo", "att"), ("wo_qkv", "att")])
def test_a_nan_row_stays_in_its_row(form, what):
    """One row of y (of att, in the forms that read attention rows) set to NaN changes no bit of any other
    row; the other rows stay finite."""
    case = U.unit_case(131, 64)
    ns = 2 if form == "dec" else 1
    bad = 77
    rows = np.array([r for r in range(case["M"]) if r != bad])
    dirty_in = case[what].copy()
    dirty_in[bad] = np.nan
    clean = _run(case, form, ns)
    dirty = _run(case, form, ns, **{what: dirty_in})
    assert dirty["clean"]
    assert np.isnan(dirty["x"][bad]).all()
    assert np.isfinite(dirty["x"][rows]).all() and np.isfinite(dirty["mean"][rows]).all()
    if dirty["qkv"] is not None:
        assert np.isfinite(dirty["qkv"][rows]).all()
    _same(clean, dirty, rows, rows, (form, what))


DEC_SHAPES = [(16, 32, 1), (144, 96, 1), (144, 96, 2), (272, 96, 3), (16, 160, 5), (144, 160, 3), (272, 160, 2),
              (272, 2048, 1), (16, 2048, 2), (144, 2048, 3), (272, 2048, 64)]


@pytest.mark.parametrize("M,F,ns", DEC_SHAPES)
def test_dec_splits_vs_fp64(M, F, ns):
    """The decoder form per nsplit (one chunk per split at nsplit = d_ff / 32, uneven shares such as 5 chunks
    over 3 splits, a ragged last row block at M = 144 and 272), each held to the fp64 bar; the tickets back
    at zero after a launch; a second launch on the same tickets bitwise equal; nsplit = 1 also with null slab
    and tickets."""
    case = U.unit_case(M, F)
    a = _run(case, "dec", ns)
    assert int(a["tickets"].abs().sum().item()) == 0
    _check(case, "dec", a, ns)
    b = _run(case, "dec", ns, tickets=a["tickets"])
    assert int(b["tickets"].abs().sum().item()) == 0 and b["clean"]
    _same(a, b, slice(None), slice(None), (M, F, ns))
    if ns == 1:
        c = _run(case, "dec", 1, null_slab=True)
        assert c["clean"] and c["word"] == 0
        _same(a, c, slice(None), slice(None), (M, F, "null slab"))


@pytest.mark.parametrize("ns", [1, 3])
def test_dec_skip_leaves_a_dead_row_block_untouched(ns):
    """With a skip vector whose chunks cover all of row block 1, that block's rows of x and of the statistics
    keep the fill; the other blocks are bit for bit what they are without it; the tickets are back at zero."""
    M, rpc = 272, 4
    case = U.unit_case(M, 96)
    done = np.zeros(M // rpc, np.int32)
    done[128 // rpc:256 // rpc] = 1
    done[3] = 1                       # one finished chunk inside a live block: the block is computed whole
    a = _run(case, "dec", ns)
    b = _run(case, "dec", ns, tickets=a["tickets"], skip=_t(done), skip_rpc=rpc)
    assert b["clean"] and int(b["tickets"].abs().sum().item()) == 0
    dead = slice(128, 256)
    live = np.r_[0:128, 256:M]
    assert (b["x"][dead] == FILL).all() and (b["mean"][dead] == FILL).all() and (b["m2"][dead] == FILL).all()
    _same(a, b, live, live, ns)
