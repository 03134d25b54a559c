"""The split-fp16 encoder attention's arithmetic (csrc/attention.hip
enc_attention_h3_kernel) as a numpy model on the CPU, against the fp64
reference of the same attention (tests/enc_attn_util.py).

Two statements.  The scheme itself is as accurate as plain fp32: on every case
of the GPU test its error is within R_EMU of max(E32, 2^-21 max|V|), E32 being
the error of the fp32 reference arithmetic on the same inputs (the floor
stands where fp32 is exact and E32 = 0: a span of one key, whose output is v
itself, split into 22 bits).  And the bar the GPU test holds the kernel to,
K times that yardstick, has teeth: with any one lo term left out, on both
k-steps or on the second alone, the same model is beyond it.
"""
import numpy as np
import pytest

from tests import enc_attn_util as U


@pytest.mark.parametrize("group", U.GROUPS)
def test_scheme_within_fp32(group):
    worst = 0.0
    for case in U.cases(group):
        out = U.emulate_h3(case["qkv"], case["sig"], case["span"])
        ref, live, e32, mx, vmax = U.yardsticks(case)
        assert np.isfinite(out[live]).all() and np.isnan(out[~live]).all(), case["name"]
        err = U.error(case, out)
        ratio = err / max(e32, U.FLOOR * vmax)
        worst = max(worst, ratio)
        print(f"{case['name']}: max|ref| {mx:.3f}  E32 {e32:.3e}  floor {U.FLOOR * vmax:.3e}  emu {err:.3e}  "
              f"ratio {ratio:.3f}")
        assert ratio <= U.R_EMU, (case["name"], err, e32)
    print(f"{group}: worst ratio {worst:.3f} (R_EMU {U.R_EMU})")


def test_persistent_case_within_fp32():
    case = U.persistent_case(66)
    out = U.emulate_h3(case["qkv"], case["sig"], case["span"])
    _, live, e32, _, vmax = U.yardsticks(case)
    assert np.isfinite(out[live]).all()
    ratio = U.error(case, out) / max(e32, U.FLOOR * vmax)
    print(f"{case['name']}: ratio {ratio:.3f}")
    assert ratio <= U.R_EMU


def test_bar_constants():
    """K = 4 while the emulation stays within 0.8 of the yardstick, 5 R_EMU beyond."""
    assert U.K_BAR == (4.0 if U.R_EMU <= 0.8 else 5.0 * U.R_EMU)


def _teeth_cases():
    return [c for c in U.cases("range") if c["name"] in ("range scale1", "range scale4")]


@pytest.mark.parametrize("step", [None, 1], ids=["whole", "step1"])
@pytest.mark.parametrize("term", U.DROPS)
def test_dropped_term_exceeds_the_bar(term, step):
    """One lo term left out of every tile, or of every tile's second k-step
    only: beyond the GPU test's bar at scale 1 and at scale 4."""
    for case in _teeth_cases():
        err = U.error(case, U.emulate_h3(case["qkv"], case["sig"], case["span"], drop=(term, step)))
        new, old = U.bars(case)
        print(f"{case['name']} without {term} ({'both k-steps' if step is None else 'k-step 1'}): err {err:.3e}  "
              f"new bar {new:.3e}  old bar {old:.3e}")
        assert err > min(new, old), (case["name"], term, step, err, new, old)
