"""The BiLSTM recurrence (lstm_dir_kernel through nd_op_lstm_layer, the split-fp16 form, and
nd_op_lstm_layer_f32, the exact-fp32 form) against the fp64 layer of tests/lstm_util.py, needs an MI355X.

Bound, per case: E32 is the max abs error against fp64 of the same layer in fp32 on the CPU (torch.nn.LSTM over
the same packed inputs), floor = 2^-23 max |ref| one fp32 rounding of the output.  The fp32 form must stay
within 4 max(E32, floor), the project's standing rule; the split form within 8 max(E32, floor): the same 4,
doubled for the hardware exp2 / reciprocal in its activations (tests/test_lstm_scheme.py restates that form on
the CPU: its products cost nothing over fp32, and one lost cross term of the split lands 29 - 216 bars out on
the cases marked discriminating).  Neither bound is taken from the kernel.  Measured ratios: DESIGN.md section
3, the BiLSTM recurrence under "Split-fp16 products" (worst 2.06 in fp32, 1.62 in the split form).

Every case runs twice per form, on an `out` prefilled with a sentinel and on a zeroed one:
- rows t < len are fully overwritten and within the bar;
- every value of a row t >= len is the sentinel or exactly 0 (a full 4-sequence group of the split form stores 0
  into padding row `step` of a finished sequence; nothing else writes there), and exactly 0 on the zeroed `out`;
- the two runs agree to the bit.
"""
import numpy as np
import pytest
import torch

from tests import lstm_util as U

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
FORMS = ("split", "f32")
H = U.H


def _run(c, form, fill):
    from nanodecoder_amd.engine import op_lstm_layer
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in c.items() if isinstance(v, np.ndarray)}
    out = torch.full((c["B"] * c["T"], 2 * H), fill, dtype=torch.float32, device=dev)
    kw = dict(xp=t["xp"]) if c.get("xp") is not None else dict(signal=t["signal"], wih0=t["wih0"], bsum=t["bsum"])
    if c.get("bn_scale") is not None:
        kw.update(bn_scale=t["bn_scale"], bn_shift=t["bn_shift"])
    got = op_lstm_layer(t["whh"], t["lens"], c["T"], out=out, exact=form == "f32", **kw)
    torch.cuda.synchronize()
    assert got is out
    return out.cpu().numpy().reshape(c["B"], c["T"], 2 * H)


def _check(name, form, ref=None):
    c = U.case(name)
    ref0, e32, floor = U.refs(name)
    ref = ref0 if ref is None else ref
    bar = U.bar(name, form)
    valid = U.valid_rows(c)
    got, got0 = _run(c, form, SENTINEL), _run(c, form, 0.0)
    pad = got[~valid]
    assert ((pad == SENTINEL) | (pad == 0)).all(), f"{name} {form}: a row past its length was written"
    assert not got0[~valid].any(), f"{name} {form}: rows past a length must stay zero"
    assert np.isfinite(got[valid]).all(), (name, form)
    assert (got[valid] != SENTINEL).all(), f"{name} {form}: a valid row was not fully written"
    assert np.array_equal(got[valid], got0[valid]), f"{name} {form}: two runs of the same call differ"
    err = float(np.abs(got.astype(np.float64) - ref)[valid].max())
    print(f"lstm {form} {name}: E32 {e32:.3e} floor {floor:.3e} err {err:.3e} ratio {err / max(e32, floor):.2f} "
          f"(bar {U.FACTOR[form]:.0f})")
    assert err <= bar, (name, form, err, bar)
    return got


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(U.CASES))
def test_lstm_layer_vs_fp64(name, form):
    _check(name, form)


@pytest.mark.parametrize("form", FORMS)
def test_tiny_weights_match_zero_weights(form):
    """max |W_hh| = 2^-120 (the power-of-two weight scale must stay finite): the W_hh = 0 output, which is the
    closed form without recurrence (tests/test_lstm_scheme.py)."""
    assert np.array_equal(U.case("whh_tiny")["xp"], U.case("whh_zero")["xp"])
    _check("whh_tiny", form, ref=U.refs("whh_zero")[0])


def _placed(base, seq, B, slot, seed):
    """`seq` (one sequence's inputs and length) in slot `slot` of a batch of B beside random neighbours of other
    lengths; the weights are `base`'s."""
    T, layer0 = base["T"], base.get("xp") is None
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, T + 1, B)
    lens[(slot + 1) % B] = T  # a longer neighbour: the sequence ends inside the group's loop
    c = U.make(B, T, lens, layer0, False, seed=seed)
    for k in ("whh", "wih0", "bsum", "bn_scale", "bn_shift"):
        if base.get(k) is not None:
            c[k] = base[k]
    c["lens"][slot] = seq["len"]
    if layer0:
        c["signal"][slot] = seq["x"]
    else:
        c["xp"].reshape(B, T, -1)[slot] = seq["x"]
    return c


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("layer0", [False, True])
def test_sequence_is_independent_of_its_placement(layer0, form):
    """One sequence in different slots, batch sizes and company (slots of full and partly filled groups of
    either form, first and last in the batch): its rows are bit-identical within a form."""
    T, n = 40, 23
    base = U.make(4, T, [T] * 4, layer0, True, seed=90 + layer0)
    seq = dict(len=n, x=(base["signal"][2] if layer0 else base["xp"].reshape(4, T, -1)[2]).copy())
    first = None
    for B, slot in ((4, 0), (4, 3), (5, 4), (7, 2), (9, 5), (17, 16), (33, 20)):
        c = _placed(base, seq, B, slot, seed=100 * B + slot)
        got = _run(c, form, 0.0)[slot]
        assert not got[n:].any() and np.isfinite(got).all()
        if first is None:
            first = got
            ref = U.bilstm(c)[slot]
            assert np.abs(got[:n] - ref[:n]).max() < 1e-5  # the sequence itself, loosely: the bars are the cases'
        else:
            assert np.array_equal(got, first), (B, slot)
