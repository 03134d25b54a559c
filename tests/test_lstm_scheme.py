"""The BiLSTM recurrence's split-fp16 arithmetic (lstm_dir_kernel, csrc/lstm.hip, H3 form) restated in numpy,
CPU only: what the scheme costs against fp64, and that the GPU suite's bar (tests/test_gpu_lstm.py) sees a
single lost term of it.

Per direction, W_hh is scaled by 2^sh, sh = min(14 - ex, 116) with max |W| = f 2^ex, f in [0.5, 1) (frexp):
max |W| 2^sh lies in [2^13, 2^14) down to max |W| = 2^-102, and 2^sh and the unscale 2^-sh / 2^10 stay finite
and normal below that, down to the smallest float.  The scaled weight is split once, hi = fp16(w), lo = fp16(w - hi).  Each
step h_{t-1} (|h| < 1) is scaled by 2^10 and split the same way (lo stays clear of the fp16 subnormals), the
product is h_hi W_lo + h_lo W_hi + h_hi W_hi accumulated in fp32 on the MFMA (every fp16 x fp16 product is
exact in fp32), and the gate is fma(sum, 2^-sh / 2^10, x).  The cell's sigmoid and tanh run on the hardware
exp2 and reciprocal (1 ulp each; rounded correctly here): sigmoid(x) = rcp(1 + exp2(-x log2 e)),
tanh(x) = sign(x) (1 - t) rcp(1 + t), t = exp2(-2 |x| log2 e).

Conditions on the GPU suite's cases (tests/lstm_util.py):
(a) the scheme as written stays within the split form's bar, 8 max(E32, floor), against fp64;
(b) on the cases marked discriminating, the scheme with h_lo W_hi dropped, and with h_hi W_lo dropped, lands at
    10x that bar or more: the bar cannot hide the loss of one cross term;
(c) the scale is finite for every max |W| down to the smallest normal float (the unclamped rule 2^(14 - ex)
    overflows below 2^-114: every product inf or NaN).
"""
import numpy as np
import pytest

from tests import lstm_util as U

F16, F32, F64 = np.float16, np.float32, np.float64
HSCALE = 1024.0
LOG2E = F32(1.4426950408889634)


def scale_shift(m, clamp=True):
    """sh of a direction whose max |W_hh| is m (fp32)."""
    if not m > 0:
        return 0
    sh = 14 - int(np.frexp(F32(m))[1])
    return min(sh, 116) if clamp else sh


def _split(x):
    hi = x.astype(F16)
    return hi, (x - hi.astype(F32)).astype(F16)


def exp_fast(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2((x * LOG2E).astype(F32).astype(F64)).astype(F32)


def rcp(x):
    with np.errstate(divide="ignore"):
        return (1.0 / x.astype(F64)).astype(F32)


def sig_fast(x):
    return rcp((F32(1) + exp_fast(-x)).astype(F32))


def tanh_fast(x):
    t = exp_fast(F32(-2) * np.abs(x))
    return np.copysign(((F32(1) - t).astype(F32) * rcp((F32(1) + t).astype(F32))).astype(F32), x)


def scheme(c, drop=None, hscale=HSCALE, fast=True):
    """The layer on the kernel's arithmetic, [B, T, 256] float32.  drop: "h_lo*W_hi" or "h_hi*W_lo" leaves that
    term out; hscale 1 enters h unscaled."""
    planes, unscale = [], []
    for d in range(2):
        W = c["whh"][d]
        sh = scale_shift(np.abs(W).max())
        Ws = (W * F32(2.0 ** sh)).astype(F32)
        assert np.isfinite(Ws).all()
        planes.append(tuple(p.astype(F64).T for p in _split(Ws)))
        unscale.append(2.0 ** -sh / hscale)

    def recurrent(d, h):
        hi, lo = (p.astype(F64) for p in _split((h * F32(hscale)).astype(F32)))
        whi, wlo = planes[d]
        z = hi @ whi
        if drop != "h_hi*W_lo":
            z = z + hi @ wlo
        if drop != "h_lo*W_hi":
            z = z + lo @ whi
        return z.astype(F32).astype(F64) * unscale[d]  # the fp32 accumulator; the unscale is a power of two

    kw = dict(sigmoid=sig_fast, tanh=tanh_fast) if fast else {}
    return U.bilstm(c, F32, recurrent=recurrent, gate_sum=lambda x, z: (x.astype(F64) + z).astype(F32), **kw)


def err(c, ref, got):
    valid = U.valid_rows(c)
    assert np.isfinite(got[valid]).all()
    return float(np.abs(got.astype(F64) - ref)[valid].max())


@pytest.mark.parametrize("name", list(U.CASES))
def test_scheme_within_the_gpu_bar(name):
    """(a), and on the discriminating cases (b)."""
    c = U.case(name)
    ref, e32, floor = U.refs(name)
    bar = U.bar(name, "split")
    e = err(c, ref, scheme(c))
    print(f"{name}: E32 {e32:.3e} floor {floor:.3e} bar {bar:.3e}  scheme {e:.3e} ({e / max(e32, floor):.2f})")
    assert e <= bar, (name, e, bar)
    if U.CASES[name][1]:
        for drop in ("h_lo*W_hi", "h_hi*W_lo"):
            eb = err(c, ref, scheme(c, drop=drop))
            print(f"  without {drop}: {eb:.3e} = {eb / bar:.1f} bars")
            assert eb >= 10 * bar, (name, drop, eb, bar)


def test_discriminating_cases_are_the_issue_ones():
    assert {n for n, (_, d) in U.CASES.items() if d} == {f"group_B{b}" for b in (4, 5, 7, 8, 6, 16, 17, 33)} | {"long_512"}


def test_scale_rule():
    """(c): max |W| 2^sh in [2^13, 2^14) while sh is unclamped; 2^sh and 2^-sh / 2^10 finite and normal for every
    max |W| from the smallest normal float up; the unclamped rule overflows to inf below 2^-114."""
    tiny = float(np.finfo(F32).tiny)
    for m in (3.0e38, 16384.0, 8192.0, 1.0, 0.15, 0.125, 2.0 ** -20, 1.9 * 2.0 ** -102):
        s = F32(m) * F32(2.0 ** scale_shift(m))
        assert 2.0 ** 13 <= s < 2.0 ** 14, m
    assert scale_shift(0.0) == 0
    for m in (2.0 ** -102, 2.0 ** -113, 1.5 * 2.0 ** -114, 2.0 ** -120, tiny, 1.0, 3.0e38):
        sh = scale_shift(m)
        with np.errstate(over="ignore"):
            wsc, un = F32(2.0 ** sh), F32(F32(2.0 ** -sh) / F32(HSCALE))
        assert np.isfinite(wsc) and wsc >= tiny and np.isfinite(un) and un >= tiny, m
        assert float(wsc) * float(un) * HSCALE == 1.0 and F32(m) * wsc < 2.0 ** 14, m
    with np.errstate(over="ignore"):
        assert np.isinf(F32(2.0 ** scale_shift(2.0 ** -120, clamp=False)))
        assert np.isinf(F32(2.0 ** scale_shift(1.9 * 2.0 ** -115, clamp=False)))
        assert np.isfinite(F32(2.0 ** scale_shift(2.0 ** -114, clamp=False)))


def test_whh_zero_is_the_closed_form_and_tiny_weights_change_nothing():
    """W_hh = 0 leaves the cell's own recurrence, c_t = f_t c_{t-1} + i_t g_t with gates of the projections
    alone; max |W_hh| = 2^-120 gives the same output to the last bit of fp64, in the reference and in the scheme."""
    c0, ct = U.case("whh_zero"), U.case("whh_tiny")
    ref = U.refs("whh_zero")[0]
    B, T, H = c0["B"], c0["T"], U.H
    want = np.zeros_like(ref)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))  # noqa: E731
    for d, p in enumerate(U.projections(c0)):
        for b in range(B):
            cell = np.zeros(H)
            n = int(c0["lens"][b])
            for t in (range(n) if d == 0 else range(n - 1, -1, -1)):
                z = p[b, t]
                cell = sig(z[H:2 * H]) * cell + sig(z[:H]) * np.tanh(z[2 * H:3 * H])
                want[b, t, d * H:(d + 1) * H] = sig(z[3 * H:]) * np.tanh(cell)
    assert np.abs(want - ref).max() < 1e-15
    assert np.abs(ct["whh"]).max() == 2.0 ** -120 and np.array_equal(U.refs("whh_tiny")[0], ref)
    assert np.array_equal(scheme(ct), scheme(c0))


def test_h_scale_is_observable_on_the_small_h_case():
    """Why the GPU suite keeps "small_h": with the output gate nearly closed (h ~ 1e-4) and W_hh entries up to
    16, entering h unscaled pushes its lo part into the fp16 subnormals; the gate sums lose ~1e-5 and h, itself
    ~1e-4, about 1e-4 of that.  The case's bar scales with its output (E32 ~ 5e-11), so the loss shows: the
    scheme as written stays within the bar, the scheme without the 2^10 does not (about 1.4 bars)."""
    c = U.case("small_h")
    ref = U.refs("small_h")[0]
    bar = U.bar("small_h", "split")
    e_scaled, e_plain = err(c, ref, scheme(c)), err(c, ref, scheme(c, hscale=1.0))
    print(f"small h: max|h| {np.abs(ref).max():.2e} bar {bar:.3e}  h 2^10 {e_scaled:.3e}  h unscaled {e_plain:.3e}")
    assert np.abs(ref).max() < 3e-4 and np.abs(c["whh"]).max() > 15
    assert e_scaled <= bar < e_plain


def test_yardstick_forms_agree():
    """torch.nn.LSTM and the numpy fp32 recurrence (used where a length is 0) are the same layer: both within
    fp32 rounding of the fp64 reference, on a layer-0 and a projected case with BatchNorm."""
    for name in ("bn_layer0", "bn_xp", "group_B5"):
        c = U.case(name)
        ref, e32, floor = U.refs(name)
        e_np = err(c, ref, U.bilstm(c, F32))
        assert e32 < 2e-6 and e_np < 2e-6, (name, e32, e_np)
        assert not U.yardstick(c)[~U.valid_rows(c)].any()
