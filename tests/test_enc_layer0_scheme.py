"""Encoder layer 0's closed form (csrc/attention.hip enc_attention_rank2_kernel,
embed_qkv_prep_kernel / prepare_embed_qkv; kernels.hpp EmbedQkv) restated in
numpy, CPU only: why it is written about s0 and not about s = 0.

The layer reads x = s w + b, so with w', b' the centred embedding weight and
bias its LayerNorm'd row is (s w' + b') r, r = rsqrt(var(s) + eps), and q, k, v
are y a + r c + b'' with y = s r, a = W' w', c = W' b'.  Written this way
(`shift=False`, the form before the fix) two things cancel when w' and b' are
nearly collinear: the expanded variance s^2 m_ww + 2 s m_wb + m_bb near its
minimum m_bb - m_wb^2 / m_ww at s0 = -m_wb / m_ww, and then a y + c r =
r (s a + c) with c ~ -s0 a.  The shipped form (`shift=True`) takes s' = s - s0
and b_perp = b' + s0 w', which is orthogonal to w': the variance is
s'^2 m_ww + m_perp, a sum of non-negative terms, and c = W' b_perp is no
multiple of a.  s0 is rounded to fp32 before b_perp is formed, so
s w' + b' = s' w' + b_perp holds exactly for the s0 the kernel subtracts.
The shift is taken once cos^2(w', b') > 1/16; up to there the form about s = 0
loses at most 1 / (1 - cos^2) <= 16/15 to the cancellation, and s0 = 0 leaves a
well-conditioned model's results bit for bit as they were (s - 0 is s).

The fp32 emulation rounds every operation to fp32 (numpy: libm exp2, exact
division and sqrt, no fused multiply-add); the GPU's exp2 / rcp / rsq and its
fmas differ from it by about an ulp per operation, and the kernel adds a
chunk's keys in order where numpy adds pairwise, which at 512 keys is the
larger difference (tests/test_gpu_enc_layer0.py measures the kernel itself;
DESIGN.md section 5 has the figures).
"""
import math

import numpy as np
import pytest
import torch

from tests import enc_layer0_util as U

D, H, DH = U.D, U.H, U.DH
COS = (None, 0.9, 0.99, 0.999, 0.9999, 0.99999)
EDGE = (0.2, 0.3)  # either side of the rule's threshold cos = 1/4
T, B = 130, 4


def fold(wts):
    """(W diag(g), b + W beta) in double (launch_fold_layernorm)."""
    W = wts["wqkv"].astype(np.float64)
    return W * wts["ln_g"].astype(np.float64), wts["bqkv"].astype(np.float64) + W @ wts["ln_b"].astype(np.float64)


def prepare(wts, shift, dt):
    """The load-time preparation in double (prepare_embed_qkv), its results
    rounded to dt as the kernel holds them."""
    nw, nb = fold(wts)
    if dt == np.float32:  # the folded weight and bias are fp32 arrays on the device
        nw, nb = nw.astype(np.float32).astype(np.float64), nb.astype(np.float32).astype(np.float64)
    w, b = wts["w_in"].astype(np.float64), wts["b_in"].astype(np.float64)
    wc, bc = w - w.mean(), b - b.mean()
    ww, wb = wc @ wc, wc @ bc
    # the shipped rule: the shift from cos^2 > 1/16 on; below, s0 = 0 (the old form, bit for bit)
    s0 = float(np.float32(-wb / ww)) if shift and ww > 0 and 16 * wb * wb > ww * (bc @ bc) else 0.0
    bp = bc + s0 * wc
    a, c = (nw @ wc).astype(dt), (nw @ bp).astype(dt)
    m = np.array([ww / D, wc @ bp / D, bp @ bp / D]).astype(dt)
    sc = math.log2(math.e) / math.sqrt(DH)
    coef = np.zeros((H, 6))
    for h in range(H):
        q, k = slice(h * DH, (h + 1) * DH), slice(D + h * DH, D + (h + 1) * DH)
        aq, cq, bq = a[q].astype(np.float64), c[q].astype(np.float64), nb[q]
        ak, ck = a[k].astype(np.float64), c[k].astype(np.float64)
        coef[h] = np.array([aq @ ak, cq @ ak, bq @ ak, aq @ ck, cq @ ck, bq @ ck]) * sc
    return dict(a=a, c=c, m=m, s0=dt(s0), coef=coef.astype(dt), bias=nb.astype(dt))


def closed_form(sig, span, wts, shift, dt):
    """The kernel's arithmetic in dt: [B, T, 256], rows t >= span NaN."""
    P = prepare(wts, shift, dt)
    a, c, (mww, mwb, mbb), s0, coef, bias = P["a"], P["c"], P["m"], P["s0"], P["coef"], P["bias"]
    eps, two = dt(U.LN_EPS), dt(2.0)
    out = np.full(sig.shape + (D,), np.nan, dt)

    def yr(s):
        sp = s.astype(dt) - s0
        r = dt(1.0) / np.sqrt(sp * (sp * mww + two * mwb) + mbb + eps)
        return sp * r, r

    for i in range(sig.shape[0]):
        L = min(int(span[i]), sig.shape[1])
        if L <= 0:
            continue
        s = sig[i, :L]
        y, r = yr(s)
        keys = s != 0  # the mask reads the raw sample
        ky, kr = (y[keys], r[keys]) if keys.any() else yr(np.zeros(1, np.float32))  # all masked: one key, s = 0
        al = coef[:, 0] * y[:, None] + (coef[:, 1] * r[:, None] + coef[:, 2])   # [L, H]
        be = coef[:, 3] * y[:, None] + (coef[:, 4] * r[:, None] + coef[:, 5])
        lg = al[:, :, None] * ky + be[:, :, None] * kr                            # [L, H, keys], log2 units
        e = np.exp2(lg - lg.max(-1, keepdims=True)).astype(dt)
        inv = dt(1.0) / e.sum(-1)
        ey, er = (e * ky).sum(-1) * inv, (e * kr).sum(-1) * inv                  # [L, H]
        av, cv, bv = (v[2 * D:].reshape(H, DH) for v in (a, c, bias))
        out[i, :L] = (av * ey[:, :, None] + cv * er[:, :, None] + bv).reshape(L, D)
    return out


def case(cos, qk_scale=1.0, seed=0):
    wts = U.make_weights(cos, seed=11 + seed, qk_scale=qk_scale)
    _, s0 = U.measured_cos_s0(wts)
    sig = U.clustered_signal(B, T, s0, seed=5 + seed)
    sig[1, ::7] = 0.0
    span = np.array([T, T, 77, T - 1])
    return wts, sig, span


def errors(cos, qk_scale=1.0):
    """max abs error against fp64 of (the fp32 materialised path, the old
    closed form, the shipped closed form), and max |ref|."""
    wts, sig, span = case(cos, qk_scale)
    ref = U.materialised(sig, span, **wts).numpy()
    live = ~np.isnan(ref)
    e32 = np.abs(U.materialised(sig, span, **wts, dtype=torch.float32).numpy().astype(np.float64) - ref)[live].max()
    old = np.abs(closed_form(sig, span, wts, False, np.float32).astype(np.float64) - ref)[live].max()
    new = np.abs(closed_form(sig, span, wts, True, np.float32).astype(np.float64) - ref)[live].max()
    return e32, old, new, np.abs(ref[live]).max()


@pytest.fixture(scope="module")
def table():
    t = {(c, 1.0): errors(c) for c in COS}
    t[(None, 4.0)] = errors(None, 4.0)
    t.update({(c, 1.0): errors(c) for c in EDGE})
    for k, (e32, old, new, mx) in t.items():
        print(f"cos {k[0]} qk x{k[1]}: max|ref| {mx:.2f}  E32 {e32:.2e}  old {old:.2e} ({old / e32:.2f} E32)  "
              f"shipped {new:.2e} ({new / e32:.2f} E32)")
    return t


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("cos", COS)
def test_closed_form_is_the_layer_in_fp64(cos, shift):
    """Algebra: in fp64 both parametrisations are the materialised layer."""
    wts, sig, span = case(cos)
    ref = U.materialised(sig, span, **wts).numpy()
    got = closed_form(sig, span, wts, shift, np.float64)
    live = ~np.isnan(ref)
    assert np.array_equal(np.isnan(got), ~live)
    assert np.abs(got - ref)[live].max() < 1e-11


def test_shift_identity_is_exact_for_the_rounded_s0():
    """s w' + b' = (s - s0) w' + b_perp to double rounding for the fp32 s0 the kernel subtracts."""
    wts, sig, _ = case(0.9999)
    w, b = wts["w_in"].astype(np.float64), wts["b_in"].astype(np.float64)
    wc, bc = w - w.mean(), b - b.mean()
    s0 = float(prepare(wts, True, np.float32)["s0"])
    s = sig[0].astype(np.float64)[:, None]
    assert np.abs((s * wc + bc) - ((s - s0) * wc + (bc + s0 * wc))).max() < 1e-15
    m = prepare(wts, True, np.float64)["m"]
    assert abs(m[1]) <= 2.0 ** -24 * abs(s0) * m[0] * 1.01  # w' . b_perp: only s0's rounding is left


def test_old_form_degrades_with_collinearity(table):
    """About s = 0 the fp32 error grows with cos(w', b'): past the whole 1e-4
    budget of the encoder memory at 0.9999, while the materialised fp32 path
    (the reference model's arithmetic) stays at a few 1e-6."""
    old = [table[(c, 1.0)][1] for c in COS]
    e32 = [table[(c, 1.0)][0] for c in COS]
    assert old[0] < 1e-5 and old[1] < 1e-5            # fine where the suite's random weights sit
    assert all(b > 2 * a for a, b in zip(old[2:], old[3:]))  # about x sqrt(10) .. x 10 per added nine
    assert old[4] > 1e-4 and old[5] > 1e-3
    assert old[4] > 4 * e32[4] and old[5] > 4 * e32[5]
    assert max(e32) < 1e-4 / 2


def test_shipped_form_does_not(table):
    """About s0 the fp32 error stays below the materialised fp32 path's own
    (E32) at every collinearity and with sharp attention (Wq, Wk x 4).  The
    bound 1.0 is the claim itself (no worse than the arithmetic it replaces);
    the largest ratio measured here is recorded in DESIGN.md section 5."""
    for k, (e32, _, new, mx) in table.items():
        assert new <= 1.0 * e32, (k, new, e32)
        assert new < 1e-5 * max(1.0, mx / 4.0), (k, new)
    flat = [table[(c, 1.0)][2] for c in COS]
    assert max(flat) < 3 * min(flat), flat  # no trend with cos


def test_the_rule_shifts_from_a_quarter_on(table):
    """s0 = 0 up to cos^2 = 1/16 (there the shipped form IS the old one, bit for
    bit), the shift beyond; the two sides of the threshold are equally good."""
    for cos, shifted in ((None, False), (EDGE[0], False), (EDGE[1], True), (0.9, True)):
        wts, sig, span = case(cos)
        assert (prepare(wts, True, np.float32)["s0"] != 0) == shifted
        same = np.array_equal(closed_form(sig, span, wts, True, np.float32),
                              closed_form(sig, span, wts, False, np.float32), equal_nan=True)
        assert same == (not shifted)
    lo, hi = table[(EDGE[0], 1.0)], table[(EDGE[1], 1.0)]
    assert lo[2] <= lo[0] and hi[2] <= hi[0]


def test_constant_weight_and_zero_bias_stay_finite():
    """m_ww = 0 exactly (constant w_in: s0 = 0, every row LN(b)) and b_in = 0
    (m_wb = m_bb = 0: r = rsqrt(s^2 m_ww + eps)) in fp32."""
    for kw in (dict(w_const=True), dict(b_zero=True)):
        wts = U.make_weights(None, seed=3, **kw)
        sig = U.clustered_signal(2, 65, 0.0, seed=1)
        span = np.array([65, 40])
        ref = U.materialised(sig, span, **wts).numpy()
        got = closed_form(sig, span, wts, True, np.float32)
        live = ~np.isnan(ref)
        assert np.isfinite(got[live]).all()
        assert np.abs(got.astype(np.float64) - ref)[live].max() < 1e-5
        if "w_const" in kw:
            P = prepare(wts, True, np.float32)
            assert P["m"][0] == 0 and P["s0"] == 0 and not P["a"].any()
