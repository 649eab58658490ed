"""The definitions alone are homogeneous in the input (no GPU): the f64 oracle and the numpy definitions of the extensions return the
same bits when the capture of tests/gain_cases.py arrives at any of its gains -- except the quantities that are powers or amplitudes
by definition, which come out exactly g (H) or g^2 (noise_var, gain, the wide-CFO metrics, the oracle's P) times.  This is what entitles
tests/test_gpu_gain.py to demand bits of the kernels, and not a tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfo_wide_ref as cw  # noqa: E402
import chest_ref  # noqa: E402
import gain_cases as gc  # noqa: E402
import quality_ref as qr  # noqa: E402
import soft_ref as sr  # noqa: E402
from util import wide  # noqa: E402

SHAPES = pytest.mark.parametrize("n,mod,nbytes", gc.CPU_SHAPES)


def test_scaling_is_exact_and_refuses_what_is_not():
    x = np.array([1.0 + 2.0j, -3.5e-7 + 0j, 0j], np.complex64)
    for g in gc.GAINS:
        y = gc.scaled(x, g)
        assert y.dtype == np.complex64 and np.array_equal(wide(y), wide(x) * g)
    with pytest.raises(AssertionError):
        gc.scaled(x, 3.0)                                        # x * 3 / 3 != x
    with pytest.raises(AssertionError):
        gc.scaled(np.array([1e-35], np.complex64), 2.0 ** -20)   # subnormal
    assert gc.same(gc.times(np.float32([3.0, -0.0]), 4.0), np.float32([12.0, -0.0]))


@SHAPES
def test_the_baseline_is_right(orc, n, mod, nbytes):
    c = gc.cpu_case(n, mod, nbytes)
    assert c["sync"][0] == c["delay"] + c["S"] + 9                # the plateau's end, found behind the FIR channel's 9-sample bulk delay
    assert c["dec"]["status"] == 0 and c["dec"]["bytes"] == c["pay"]
    assert c["rx"].size % 2 == 1


@SHAPES
def test_the_oracle_is_homogeneous(orc, n, mod, nbytes):
    c = gc.cpu_case(n, mod, nbytes)
    d0, p0, m0, f0 = c["sync"]
    for g in gc.GAINS:
        x = wide(gc.scaled(c["rx"], g))
        d, p, m, f = orc.sc_sync(x, c["S"], 3, 0, 0.5)
        assert d == d0 and gc.same(np.float64([m, f]), np.float64([m0, f0])), g
        assert gc.same(np.complex128([p]), gc.times(np.complex128([p0]), g * g)), g           # only P itself scales, by g^2
        dec = orc.decode_sc(x, True, mod, n)
        assert (dec["status"], dec["offset"], dec["bytes"]) == (0, c["dec"]["offset"], c["pay"]), g
        assert gc.same(np.float64([dec["f_delta"], dec["metric"]]), np.float64([c["dec"]["f_delta"], c["dec"]["metric"]])), g


@SHAPES
def test_the_channel_estimates_scale_with_the_input(orc, n, mod, nbytes):
    c = gc.cpu_case(n, mod, nbytes)
    smooth0 = chest_ref.smooth(c["hk"], c["trn"], n)
    for g in gc.GAINS:
        x = wide(gc.scaled(c["rx"], g))
        hk = gc.channel_estimate(orc, x, c["dec"]["offset"], c["dec"]["f_delta"], c["trn"], n)
        assert gc.same(hk, gc.times(c["hk"], g)), g
        assert gc.same(chest_ref.smooth(hk, c["trn"], n), gc.times(smooth0, g)), g


@SHAPES
def test_link_quality_is_homogeneous(orc, n, mod, nbytes):
    c = gc.cpu_case(n, mod, nbytes)
    nd = orc.data_carriers(n, True)
    n_points = -(-8 * (16 + nbytes) // mod)
    args = dict(syms_per_frame=-(-n_points // nd), first_symbol=10, n_points=n_points, offset=[c["dec"]["offset"]], f_delta=[c["dec"]["f_delta"]])
    base = qr.quality(wide(c["rx"])[None, :], n, True, mod, c["trn"], hk=c["hk"], **args)
    assert base[0, qr.Q_VALID] == 1 and base[0, qr.Q_POINTS] == n_points and 0 < base[0, qr.Q_EVM2] < 0.1 and base[0, qr.Q_SNR] > 10
    for g in gc.GAINS:
        got = qr.quality(wide(gc.scaled(c["rx"], g))[None, :], n, True, mod, c["trn"], hk=gc.times(c["hk"], g), **args)
        for k in (qr.Q_VALID, qr.Q_SNR, qr.Q_LLR_UNIT, qr.Q_EVM2, qr.Q_POINTS):
            assert gc.same(got[:, k], base[:, k]), (g, qr.NAMES[k])
        for k in (qr.Q_NOISE_VAR, qr.Q_GAIN):
            assert gc.same(got[:, k], gc.times(base[:, k], g * g)), (g, qr.NAMES[k])


@SHAPES
def test_wide_cfo_is_homogeneous(orc, n, mod, nbytes):
    c = gc.cpu_case(n, mod, nbytes)
    args = (n, c["trn"], [c["dec"]["offset"]], [c["dec"]["f_delta"]])
    m0, f0, g0 = cw.cfo_wide(wide(c["rx"]), *args)
    assert m0[0] == 0 and g0[0, 0] > 2 * g0[0, 1] > 0             # the link's CFO lies inside the Schmidl-Cox range
    for g in gc.GAINS:
        m, f, G = cw.cfo_wide(wide(gc.scaled(c["rx"], g)), *args)
        assert np.array_equal(m, m0) and gc.same(f, f0) and gc.same(G, gc.times(g0, g * g)), g


@SHAPES
def test_llrs_are_homogeneous(orc, n, mod, nbytes):
    """the equalised points of the data symbols, the weights w_k and the int8 LLRs, with hk = g hk_1"""
    c = gc.cpu_case(n, mod, nbytes)
    S, off = c["S"], c["dec"]["offset"]
    bins = sr.data_bins(orc, n, True)

    def run(g):
        x = orc.cfo_rotate(wide(gc.scaled(c["rx"], g))[off:], c["dec"]["f_delta"], 0)[10 * S:(10 + c["D"]) * S]
        hk = gc.times(c["hk"], g)
        by, soft = orc.rx_demod(x, n, True, mod, hk=hk, want_soft=True)
        w = sr.channel_weights(hk[None, :], bins)
        return by, soft, w, sr.frame_llrs(soft.reshape(1, -1, len(bins)), mod, 32.0, w)

    by0, soft0, w0, llr0 = run(1.0)
    assert by0[16:16 + nbytes] == c["pay"] and np.abs(llr0).max() >= 16
    for g in gc.GAINS:
        by, soft, w, llr = run(g)
        assert by == by0 and gc.same(soft, soft0) and gc.same(w, w0) and np.array_equal(llr, llr0), g
