"""The fused FFN block's arithmetic (csrc/ffn.hip enc_ffn_kernel, all four
forms) as a numpy model on the CPU, against the fp64 reference of the same
block (tests/ffn_util.py).  This file settles the bar tests/test_gpu_ffn.py
holds the kernel to; nothing here runs the kernel.

The bar, per case, form and output (x, and qkv of the "wo_qkv" form):

    err = max |got - fp64|  <=  K (E32 + sqrt(n_acc) 2^-25 max|ref|)
    and  err < 2e-4 max(1, max|ref| / 8)

E32 is the error against fp64 of the same block in plain fp32 torch on the
CPU.  n_acc counts the fp32 roundings the accumulator that carries the
residual takes, from the scheme's description: the residual and b2 are the
accumulators' initial value, so they are rounded at each of the three MFMA
terms of each d_ff chunk of 32 (3 F / 32), at 24 more terms under the Wo fold,
and in the decoder form at split 0's share of the chunks plus the nsplit
additions of the sum in split order; the term is a random walk of that many
half-ulp roundings at max|ref|.  Plain fp32 rounds the residual once.  The
qkv output answers to the same formula with its own E32 and its own max|ref|
(ffn_util.acc_term).  The second bound is the ceiling of
test_enc_ffn_fused_vs_fp64, kept.

K = 8: the smallest power of two for which the model stays within a quarter
of the bar on every case, form and output.  The model's worst ratio is 0.22 of
the bar on x (residual scale 64 under the Wo fold at d_ff 2048; 0.44 at
K = 4) and 0.21 on qkv (the offset rows), 0.03-0.17 on the unit cases.  A
quarter is left for what the model does not have: the hardware's rsq, the
MFMA's roundings inside a k-block, summation orders.  (Measured on an MI355X:
the kernel is at most 0.49 of the bar on x and 0.52 on qkv, the offset rows,
which are also at 0.72 of qkv's 2e-4 ceiling; 1.9-2.9 times the model where
the accumulator carries a residual through d_ff 2048 and equal to the model
to three digits where it carries none; DESIGN.md section 5 has the table.)

Teeth: with ONE lo term left out of ONE chunk (the prologue's chunk 0, a
middle one, the last step's; phase 1 or phase 2; the first or last slice of
the Wo or QKV fold) the model is beyond the bar at d_ff 2048 (7.7e-5..1.1e-4
against 2.8e-5..5.9e-5; every one of them under the old 2e-4) and at d_ff 32
(6.7e-4..9.8e-4 against 1.4e-5..3.2e-5).

The residual's accumulation loss is the scheme: on the `residual` cases the
model sits at 2.8-10.5 E32 (scale 64, d_ff 2048: 1.95e-4 against E32 1.85e-5)
and the accumulation term, not E32, is what carries them.

The statistics answer to their own bar against fp64 statistics of the fp32 x
that was returned: mean within 2^-22 max|x_row|, M2 within 1e-5 relative plus
256 (2^-23 max|x_row|)^2.  A one-pass variance in fp32 misses it on the
`offset` rows by a factor of 150 and more.
"""
import numpy as np
import pytest

from tests import ffn_util as U

R_MODEL = 0.25


def _splits(case, form):
    if form != "dec":
        return (1,)
    return tuple(sorted({n for n in (1, 2, 3, case["F"] // U.HC) if n <= case["F"] // U.HC}))


@pytest.mark.parametrize("group", U.GROUPS)
def test_model_within_a_quarter_of_the_bar(group):
    worst = 0.0
    for case in U.cases(group):
        rows = U.model_rows(case)
        for form in U.FORMS:
            ys = U.yardsticks(case, form in ("wo", "wo_qkv"))
            assert ys["hidden"] < 0.9 * U.F16_LIMIT and np.abs(case["att"]).max() < 0.9 * U.F16_LIMIT, case["name"]
            for ns in _splits(case, form):
                out = U.emulate(case, form, ns, rows=rows)
                assert out["hmax"] < U.F16_LIMIT
                for which in ("x", "qkv") if form == "wo_qkv" else ("x",):
                    assert np.isfinite(out[which]).all(), case["name"]
                    err = U.error(case, form, out[which], which, rows)
                    new, old = U.bars(case, form, which, ns)
                    e32, mx = (ys["e32"], ys["mx"]) if which == "x" else (ys["e32q"], ys["mxq"])
                    print(f"{case['name']} [{form} nsplit {ns}] {which}: max|ref| {mx:.4g}"
                          f"  E32 {e32:.3e}  model {err:.3e}  model/E32 {err / e32:.2f}  model/bar {err / new:.3f}")
                    worst = max(worst, err / new)
                    assert err <= R_MODEL * new, (case["name"], form, ns, which, err, new)
                    assert err < old, (case["name"], form, ns, which, err, old)
                rm, rq = U.stats_miss(out["x"], out["mean"], out["m2"])
                assert rm <= 1.0 and rq <= 1.0, (case["name"], form, ns, rm, rq)
    print(f"{group}: worst model/bar {worst:.3f}")


def test_k_is_the_smallest_power_of_two():
    """K = 8 holds every case within a quarter (the test above); at K / 2 the worst case does not."""
    case = next(c for c in U.cases("residual") if "scale 64" in c["name"])
    rows = U.model_rows(case)
    err = U.error(case, "wo", U.emulate(case, "wo", rows=rows)["x"], rows=rows)
    assert err > R_MODEL * U.bars(case, "wo")[0] / 2.0
    assert U.K_BAR == 8.0


def _teeth_case(F):
    return next(c for c in U.cases("unit") if c["M"] == 48 and c["F"] == F)


def _drops(F):
    n = F // U.HC
    chunks = sorted({0, n // 2, n - 1})
    return ([("W1", j) for j in chunks] + [("W2", j) for j in chunks] + [("Wo", 0), ("Wo", 7), ("Wq", 0), ("Wq", 23)])


@pytest.mark.parametrize("term", U.LO_TERMS)
@pytest.mark.parametrize("F", [32, 2048])
def test_one_dropped_term_in_one_chunk_exceeds_the_bar(F, term):
    """One lo term left out of one chunk: first, middle and last d_ff chunk of W1 and of W2, the first and
    last slice of the Wo and of the QKV fold.  Beyond the bar in every form that runs the chunk; at d_ff
    2048 every one of them is under the old 2e-4 bar."""
    case = _teeth_case(F)
    for which, j in _drops(F):
        forms = (("wo_qkv", 1),) if which in ("Wo", "Wq") else (("none", 1), ("wo_qkv", 1), ("dec", min(3, F // U.HC)))
        for form, ns in forms:
            out = U.emulate(case, form, ns, drop=(which, j, term))
            w = "qkv" if which == "Wq" else "x"
            err = U.error(case, form, out[w], w)
            new, old = U.bars(case, form, w, ns)
            print(f"{case['name']} [{form} nsplit {ns}] without {term} of {which} chunk {j}: {w} err {err:.3e}  "
                  f"bar {new:.3e}  old bar {old:.3e}")
            assert err > min(new, old), (which, j, term, form, err, new)
            if F == 2048 and which in ("W1", "W2"):
                assert err < 2e-4, (which, j, term, form, err)   # what the old bar let through


def test_residual_cases_rest_on_the_accumulation_term():
    """The loss against plain fp32 on the residual cases, as a ratio; the accumulation term of the bar is
    larger than E32 there and the model is beyond E32 itself: K E32 alone, held to a quarter, would refuse the
    shipped scheme."""
    for case in U.cases("residual"):
        rows = U.model_rows(case)
        for form in ("none", "wo"):
            ys = U.yardsticks(case, form == "wo")
            err = U.error(case, form, U.emulate(case, form, rows=rows)["x"], rows=rows)
            walk = U.acc_term(case, form)
            print(f"{case['name']} [{form}]: E32 {ys['e32']:.3e}  accumulation term {walk:.3e}  model {err:.3e}  "
                  f"model/E32 {err / ys['e32']:.2f}")
            assert walk > ys["e32"], (case["name"], form)
            assert err > R_MODEL * U.K_BAR * ys["e32"], (case["name"], form)


def test_one_pass_variance_misses_the_statistics_bar():
    """Two-pass statistics of the model's x hold the bar on every offset row; sum x^2 - 256 mean^2 in fp32
    does not."""
    for case in U.cases("offset"):
        for form in ("none", "wo"):
            out = U.emulate(case, form)
            rm, rq = U.stats_miss(out["x"], out["mean"], out["m2"])
            _, rq1 = U.stats_miss(out["x"], *U.one_pass_stats(out["x"]))
            print(f"{case['name']} [{form}]: two-pass mean {rm:.3f} M2 {rq:.3f} of their bars; one-pass M2 {rq1:.1f}")
            assert rm <= 1.0 and rq <= 1.0
            assert rq1 > 1.0


def test_constant_rows_normalise_to_zero():
    """A constant row has var 0 and LN(y) = 0: x = y + W2 relu(b1') + b2, in the model as in fp64."""
    case = U.cases("offset")[0]
    const = np.flatnonzero((case["y"] == U.CONST).all(axis=1))
    assert len(const) == 3
    out = U.emulate(case, "none")
    _, b1f = U.fold_ln(case["W1"], case["b1"], case["lg"], case["lb"])
    want = U.CONST + np.maximum(b1f.astype(np.float64), 0) @ case["W2"].astype(np.float64).T + case["b2"]
    assert np.abs(out["x"][const] - want[None, :]).max() < 4 * 2.0 ** -24 * 128
    assert np.array_equal(out["x"][const[0]], out["x"][const[1]])
