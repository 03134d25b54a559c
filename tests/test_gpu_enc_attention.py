"""The encoder's self-attention kernels at op level (nd_op_enc_attention_ex:
enc_attention_h3_kernel, split-fp16 and persistent, and with exact the fp32
enc_attention_kernel) against the fp64 reference of the same attention
(tests/enc_attn_util.py), needs an MI355X.

Bar, per case: err = max |out - fp64| over the rows t < span must satisfy

    err <= K max(E32, 2^-21 max|V|)   and   err < 1e-4 max(1, max|ref| / 4).

E32 is the error against fp64 of the same attention in plain fp32 on the CPU
(the reference model's own arithmetic) on the same inputs.  The floor stands
where fp32 is exact and E32 = 0 (T = 1, a span of one key: the output is v
itself): a value split into fp16 hi + lo keeps 22 bits, and both P and V are
split.  The second bound is test_enc_attention_vs_oracle's ceiling, kept.
Neither is taken from a kernel.  K = 4: the numpy model of the shipped scheme
(tests/test_enc_attn_scheme.py) stays within 0.8 of the yardstick on every
case here, and 4 leaves 5x for what it does not model (hardware exp2 and rcp,
the MFMA's summation order).  The exact form is the reference arithmetic apart
from summation order and answers to the same bar.  The same model with one lo
term left out, even on one k-step only, is beyond this bar
(test_dropped_term_exceeds_the_bar).  Measured ratios: DESIGN.md section 5.

Every span is at least 1 and every index stays inside the buffers.
"""
import numpy as np
import pytest
import torch

from tests import enc_attn_util as U

pytestmark = pytest.mark.gpu

D = U.D
FILL = -7.25
GUARD = 64
FORMS = pytest.mark.parametrize("exact", [False, True], ids=["h3", "exact"])


def _dev():
    return torch.device("cuda", 0)


def _run(qkv, sig, span, exact):
    """(out [B*T + GUARD, 256] numpy, pre-filled with FILL; the guard word after the call)."""
    from nanodecoder_amd.engine import op_enc_attention
    dev = _dev()
    t = lambda a: a.to(dev) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sig = t(sig)
    B, T = sig.shape
    out = torch.full((B * T + GUARD, D), FILL, dtype=torch.float32, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    got = op_enc_attention(t(qkv), sig, t(np.asarray(span, np.int32)), exact=exact, ovf=ovf, out=out)
    torch.cuda.synchronize()
    assert got is out
    return out.cpu().numpy(), int(ovf.item())


def _check(case, exact, out=None):
    """A case's output against fp64 within the module's bar; rows at or past span and the guard rows keep the
    fill; the guard word stays 0.  Returns out."""
    name = f"{case['name']} [{'exact' if exact else 'h3'}]"
    B, T = case["sig"].shape
    if out is None:
        out, word = _run(case["qkv"], case["sig"], case["span"], exact)
        assert word == 0, name
    _, live, e32, mx, vmax = U.yardsticks(case)
    body = out[:B * T].reshape(B, T, D)
    assert (body[~live] == FILL).all() and (out[B * T:] == FILL).all(), name
    assert np.isfinite(body[live]).all(), name
    err = U.error(case, body)
    new, old = U.bars(case)
    print(f"{name}: max|ref| {mx:.3f}  E32 {e32:.3e}  floor {U.FLOOR * vmax:.3e}  err {err:.3e}  "
          f"err/E32 {err / e32 if e32 else float('inf'):.3f}  err/bar {err / new:.3f}")
    assert err < old, (name, err, old)
    assert err <= new, (name, err, new)
    return out


@FORMS
@pytest.mark.parametrize("group", U.GROUPS)
def test_cases_vs_fp64(group, exact):
    for case in U.cases(group):
        _check(case, exact)


@FORMS
def test_poison_rows_past_span(exact):
    """NaN in every qkv row and sample at t >= span changes no bit of the rows t < span."""
    for case in U.cases("ragged"):
        B, T = case["sig"].shape
        _, live, *_ = U.yardsticks(case)
        clean, w0 = _run(*U.poisoned(case, 0.0), case["span"], exact)
        dirty, w1 = _run(*U.poisoned(case, np.nan), case["span"], exact)
        assert w0 == 0 and w1 == 0, case["name"]
        assert np.isfinite(dirty[:B * T].reshape(B, T, D)[live]).all(), case["name"]
        assert np.array_equal(clean, dirty), case["name"]
        _check(case, exact, dirty)


def _persistent_batch():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = min(128, (2 * cus + 8) // 8 + 1)      # 8 B > 2 CUs + 8: some workgroup walks three items
    return U.persistent_case(B), min(8 * B, cus)


@FORMS
def test_persistent_grid_vs_fp64_and_alone(exact):
    """More (chunk, head) items than twice the persistent grid: every chunk within its own bar, and six
    chunks bit for bit what they are when run alone (an item owes nothing to the item its workgroup walked
    before it, nor to the prefetch issued under that item's key loop)."""
    case, grid = _persistent_batch()
    B, T = case["sig"].shape
    out, word = _run(case["qkv"], case["sig"], case["span"], exact)
    assert word == 0
    assert (out[B * T:] == FILL).all()
    for b in range(B):
        _check(U.sub_case(case, b), exact, np.concatenate([out[b * T:(b + 1) * T], out[B * T:]]))
    # a short chunk whose workgroups' previous items (grid items earlier: grid / 8 chunks) were a long one's
    back = max(1, grid // 8)
    after_long = max(range(back, B), key=lambda b: int(case["span"][b - back]) - int(case["span"][b]))
    assert case["span"][after_long - back] > case["span"][after_long]
    probes = [0, B - 1, B // 6, B // 2, (5 * B) // 6, after_long]
    assert len(set(probes)) == 6
    for b in probes:
        one = U.sub_case(case, b)
        alone, _ = _run(one["qkv"], one["sig"], one["span"], exact)
        assert np.array_equal(alone[:T], out[b * T:(b + 1) * T]), (b, int(case["span"][b]))


@FORMS
def test_repeatable(exact):
    for case in U.cases("shapes"):
        a, _ = _run(case["qkv"], case["sig"], case["span"], exact)
        b, _ = _run(case["qkv"], case["sig"], case["span"], exact)
        assert np.array_equal(a, b), case["name"]


def _guard_word(qkv, sig, span, edits, exact=False):
    """The guard word after a call on qkv (device) with elements (row, column, value) set."""
    q = qkv.clone()
    for row, col, val in edits:
        q[row, col] = val
    return _run(q, sig, span, exact)[1]


def test_range_guard():
    """The split-fp16 form raises the guard word for one live K or V element of 7e4 and for one live Q
    element whose scaled value reaches the fp16 limit, in the first chunk and in the last chunk of a batch
    that workgroups reach on a later pass; values just inside the range, and the same values in rows at or
    past a chunk's span (positions that do not exist for it), leave it 0.  The fp32 form never writes it.
    Outputs are not compared here."""
    big_q = float(np.float32(U.Q_LIMIT * 1.001))
    B, T = 2, 96
    rng = np.random.default_rng(77)
    dev = _dev()
    qkv = torch.from_numpy(rng.standard_normal((B * T, 3 * D)).astype(np.float32)).to(dev)
    sig = torch.from_numpy(U._signal(rng, B, T)).to(dev)
    span = np.array([T, 40], np.int32)
    live = {"K": (5, D + 37, 7e4), "V": (70, 2 * D + 200, -7e4), "Q": (33, 101, big_q), "Q last row": (T - 1, 3, -big_q)}
    assert _guard_word(qkv, sig, span, []) == 0
    for what, edit in live.items():
        assert _guard_word(qkv, sig, span, [edit]) == 1, what
        assert _guard_word(qkv, sig, span, [edit], exact=True) == 0, what
    inside = [(5, D + 37, 65000.0), (70, 2 * D + 200, -65000.0), (33, 101, float(np.float32(U.Q_LIMIT * 0.99)))]
    assert _guard_word(qkv, sig, span, inside) == 0
    # chunk 1 (span 40): rows 40 .. 95 do not exist for it
    for what, (row, col, val) in {"K": (40, D + 37, 7e4), "V": (64, 2 * D + 200, 7e4), "Q": (41, 101, big_q),
                                   "Q wave 1": (70, 5, big_q), "Q last row": (T - 1, 3, big_q)}.items():
        assert _guard_word(qkv, sig, span, [(T + row, col, val)]) == 0, what + " past the span"
    # the last chunk of the persistent batch: an item of a workgroup's second or third pass
    case, _ = _persistent_batch()
    PB, PT = case["sig"].shape
    qkv, sig = torch.from_numpy(case["qkv"]).to(dev), torch.from_numpy(case["sig"]).to(dev)
    last = (PB - 1) * PT
    assert case["span"][PB - 1] > 2
    assert _guard_word(qkv, sig, case["span"], []) == 0
    for what, edit in {"K": (last + 1, D + 250, 7e4), "V": (last, 2 * D + 9, 7e4), "Q": (last + 2, 77, big_q)}.items():
        assert _guard_word(qkv, sig, case["span"], [edit]) == 1, what + " in the last chunk"
