"""The razor-thin Schmidl-Cox cases of tests/sc_margin_cases.py must hold by themselves, without a GPU: the captures have the dynamic
range they claim, few cases are dropped as ambiguous, exact rational arithmetic on the f32 samples agrees with the oracle at every
razor lag, and the cases discriminate -- a detector that decides on plain f64 prefix differences (what a streaming kernel computes
when it takes no further care) gets cases wrong on every burst capture at eps_min and none on the ordinary capture."""
import math

import pytest

import sc_margin_cases as smc
from util import wide


@pytest.mark.parametrize("n,late", smc.SIZES)
def test_construction(orc, n, late):
    sz = smc.build(orc, n, late)
    print(f"N = {n}: oracle error of M(d_k) against exact arithmetic {sz.oracle_err:.2e}, eps_min {sz.eps_min:.2e}, "
          f"record lags {sz.records}, min window / total energy 2^{[round(math.log2(r), 1) for r in sz.ratios]}")
    # the oracle is far more exact than the thinnest margin, and that margin is two decades clear of its error
    assert sz.eps_min == max(1e-12, 100.0 * sz.oracle_err) and sz.eps_min < 1e-9
    assert all(len(lags) == (6 if n == 64 else 2) for lags in sz.records)
    # dynamic range: the ordinary capture's windows hold a good share of its energy, the bursts push that to 2^-9, 2^-15, 2^-17
    assert sz.ratios[0] > 2.0 ** -5
    for ratio, lg in zip(sz.ratios[1:], smc.RATIO_LOG2[1:]):
        assert abs(math.log2(ratio) - lg) <= 1.0, (n, ratio, lg)
    # every case of every capture: 3 eps x 2 signs per record lag, few dropped, and exact arithmetic confirms the oracle
    for ci in range(len(smc.CAPTURES)):
        cases = [c for c in sz.cases if c.cap == ci]
        assert len(cases) == 6 * len(sz.records[ci])
        dropped = sum(not c.kept for c in cases)
        assert dropped <= smc.MAX_DROP_SHARE * len(cases), (n, ci, dropped, len(cases))
    for c in sz.cases:
        if c.kept:
            assert c.exact_crosses == c.oracle_crosses == (c.sign < 0), c
    # a threshold's rows: each kept case's own row is there with a verdict
    for t in sz.thresholds:
        for c in sz.cases:
            if c.kept and (c.d, c.eps, c.sign) == (t.d, t.eps, t.sign):
                assert t.rows[c.cap] is not None and t.thr == c.thr


@pytest.mark.parametrize("n,late", smc.SIZES)
def test_cases_catch_a_prefix_difference_detector(orc, n, late):
    """Only d_hat, the CFO and the metric of the peak leave a detector.  A search over d_k + W + 64 lags returns the same peak whether
    the crossing is found at d_k or a lag later, so each threshold is also searched over d_k + 1 lags: the razor lag is then the
    last one, and the decision there is the answer itself (d_k, or -1 for nothing found)."""
    sz = smc.build(orc, n, late)
    kept = {(c.cap, c.d, c.eps, c.sign) for c in sz.cases if c.kept}
    wrong = {eps: [0] * len(smc.CAPTURES) for eps in smc.EPS_FIXED + (sz.eps_min,)}
    wrong_wide = 0
    for t in sz.thresholds:
        for ci in range(len(smc.CAPTURES)):
            if (ci, t.d, t.eps, t.sign) in kept:
                assert t.razor[ci][0] == (t.d if t.sign < 0 else -1)
                wrong[t.eps][ci] += smc.prefix_detector(sz.caps[ci], sz.S, sz.W, t.d + 1, t.thr) != t.razor[ci][0]
                wrong_wide += smc.prefix_detector(sz.caps[ci], sz.S, sz.W, t.n_lags, t.thr) != t.rows[ci][0]
    print(f"N = {n}: wrong decisions of the prefix-difference detector per capture {smc.CAPTURES}: "
          + ", ".join(f"eps {eps:.0e}: {w}" for eps, w in wrong.items()) + f"; over d_k + W + 64 lags: {wrong_wide}")
    assert wrong[sz.eps_min][0] == 0, wrong
    # (the late set exists to reach k_sc_cf<256>, beyond the sizes the cases were specified for: behind its 2^-9 burst the emulation's
    # error is about eps_min itself and may fall either way, so only the two larger bursts are required to catch it)
    assert all(w >= 1 for w in wrong[sz.eps_min][2 if late else 1:]), wrong
    assert wrong[1e-6] == [0] * len(smc.CAPTURES), wrong          # the margins every detector gets right
