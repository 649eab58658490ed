"""CPU certificate of the pilot-table families of tests/pilot_cases.py -- the conditions under which tests/test_gpu_pilots.py may ask what
it asks -- and the host-side pieces that go with them.  No kernel is launched; every measured value is printed.

  1. every family differs from the default table of its N;
  2. `holes` has max(3, N / 32) dead bins, none on a pilot, at least one on a data carrier, and cond(R) <= 10 -- so the WLS stage may
     be held to its usual bar under it -- and ofdm_chest_matrix meets the bar of test_chest_cpu.py on it;
  3. the header orc.encode builds under `unit_loud` has its signed maximum at the planted imaginary part while abs of its minimum is
     larger; under `stdrng` and the default the maximum lies in block 0, the locking signal;
  4. on the f64 definition of the wide CFO acquisition the true m wins with a best-to-runner-up ratio >= 2 under every family on the
     captures the GPU test uses: the condition under which an exact m may be demanded of an f32 kernel;
  5. ofdm_chest_matrix on a table that is zero on the whole guard band either refuses or returns an inverse, max |R got - I| <= 1e-6.
     The bound is a condition, not a measurement: the device keeps the matrix in f32, a residual beyond that is no usable table;
  6. api._ctx_key, the cache key of the free functions, takes explicit tables by value;
  7. include/ofdm_hip.h says what a zero training bin means."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chest_ref as cr  # noqa: E402
import pilot_cases as pc  # noqa: E402

COND_CAP = 10.0
WIDE_RATIO = 2.0
RESIDUAL = 1e-6


@pytest.fixture(scope="module")
def lib():
    from ofdm_amd import build

    lib = C.CDLL(build.build())
    lib.ofdm_chest_matrix.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    return lib


def _chest_matrix(lib, trn):
    n = trn.size
    got = np.zeros((n // 4, n // 4), np.complex128)
    rc = lib.ofdm_chest_matrix(n, n // 4, np.ascontiguousarray(trn).ctypes.data, got.ctypes.data)
    return rc, got


@pytest.mark.parametrize("n", pc.SIZES)
def test_every_family_differs_from_the_default(orc, n):
    dpre, dtrn = pc.tables("default", n)
    np.testing.assert_array_equal(dpre, orc.default_preamble(n + n // 4))
    np.testing.assert_array_equal(dtrn, orc.default_training(n))
    for name in pc.FAMILIES:
        pre, trn = pc.tables(name, n)
        assert pre.shape == dpre.shape and trn.shape == dtrn.shape and pre.dtype == trn.dtype == np.complex128
        assert np.isfinite(pre).all() and np.isfinite(trn).all() and np.all(pre != 0)      # (a zero preamble sample breaks frequency_correction)
        assert np.abs(trn - dtrn).max() > 0.1, name
        assert (name == "holes") == bool(np.array_equal(pre, dpre)), name                  # holes keeps the default preamble, no other does
        again = pc.tables(name, n)
        assert np.array_equal(again[0], pre) and np.array_equal(again[1], trn)             # seeded
    assert np.all(np.abs(np.abs(pc.tables("unit_loud", n)[1]) - 1.0) < 1e-15)


@pytest.mark.parametrize("n", pc.SIZES)
def test_holes_is_inside_the_domain_of_the_wls_stage(orc, lib, n):
    trn = pc.tables("holes", n)[1]
    dead = pc.dead_bins(trn)
    cls = np.array([orc.carrier_class(int(k), n, True) for k in dead])
    assert dead.size == max(3, n // 32) and not np.any(cls == 2) and np.sum(cls == 0) >= 1, (dead, cls)
    live = np.abs(trn[trn != 0])
    assert live.min() >= 0.5 and live.max() <= 1.0
    conds = {}
    for name in ("default",) + pc.FAMILIES:
        conds[name] = float(np.linalg.cond(cr.rmatrix(pc.tables(name, n)[1], n)))
    print(f"n_fft {n}: cond(R) " + ", ".join(f"{k} {v:.2f}" for k, v in conds.items()) + f"; holes: {dead.size} dead bins, {int(np.sum(cls == 0))} on data carriers")
    assert conds["holes"] <= COND_CAP                     # (another SEED in pilot_cases.py if not: the cap stays)
    R = cr.rmatrix(trn, n)
    rc, got = _chest_matrix(lib, trn)
    assert rc == 0
    want = np.linalg.inv(R)
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"n_fft {n}: ofdm_chest_matrix under holes, relative error {err:.2e}")
    assert err <= conds["holes"] * 1e-13                  # the bar of test_chest_matrix_is_numpys_inverse
    assert np.abs(R @ got - np.eye(n // 4)).max() <= RESIDUAL


@pytest.mark.parametrize("n", pc.SIZES)
def test_where_the_header_peaks(orc, n):
    S = n + n // 4
    quiet = b"\x5a" * 5
    for name in ("default",) + pc.FAMILIES:
        pre, trn = pc.tables(name, n)
        tx = orc.encode(quiet, True, 6, n, preamble=pre, training=trn)
        hdr = tx[:10 * S]
        value, at, part = pc.signed_peak(hdr)
        low = min(hdr.real.min(), hdr.imag.min())
        print(f"n_fft {n} {name}: header's signed maximum {value:.4f} in {part} of sample {at} (block {at // S}), minimum {low:.4f}; the frame's {pc.signed_peak(tx)[0]:.4f}")
        assert pc.signed_peak(tx)[:2] == (value, at) and value == 1.0      # a frame that is no louder than its header
        if name == "unit_loud":
            neg, pos = pc.loud_positions(n)
            assert part == "im" and 1 <= at // S <= 4 and at % S == pos
            # the planted pair, scaled by 1 / 0.95 as normalize scales it: abs would have found -0.99, in a real part
            assert abs(hdr[S + pos] - pc.LOUD_POS / 0.95) < 1e-12 and abs(hdr[S + neg] - pc.LOUD_NEG / 0.95) < 1e-12
            assert low == hdr.real.min() == hdr[S + neg].real and abs(low) > value
            assert np.abs(hdr[:S]).max() < 0.5 / 0.95 + 1e-12                # the locking signal is not the peak
        else:
            assert at // S == 0 and part == "re", name                       # the locking signal


@pytest.mark.parametrize("n", sorted(pc.WIDE_SNR))
def test_true_m_wins_by_a_factor_of_two_under_every_family(n):
    for name in ("default",) + pc.FAMILIES:
        k = pc.cfo_wide_case(name, n)
        m, fd, g = k["ref"]
        ratio = g[:, 0] / g[:, 1]
        print(f"n_fft {n} {name}: m {m.tolist()}, best-to-runner-up ratios {np.round(ratio, 2).tolist()}, complex64 restatement {k['dist']:.1e}")
        assert np.array_equal(m, np.array(pc.WIDE_M)) and np.array_equal(m, k["m"]), name
        assert np.isfinite(g).all() and ratio.min() >= WIDE_RATIO, (name, ratio.min())
        S = n + n // 4
        assert np.array_equal(fd, np.where(m != 0, k["f0"] + 2.0 * np.pi * m / S, k["f0"]))


@pytest.mark.parametrize("n", [64, 128, 256, 1024])
def test_chest_matrix_on_a_band_nulled_table_refuses_or_inverts(orc, lib, n):
    """N = 256 is where the recursion used to run to its end on rounding residue: rc 0 with max |R got - I| = 2.9e-3 at cond(R) 2.2e14.
    N = 64 and 128 (cond 7e2, 4e6) are answered with a true inverse, N >= 512 (cond >= 5e16) fail a pivot."""
    trn = pc.band_nulled(n)
    assert all((trn[k] == 0) == (orc.carrier_class(k, n, True) == 1) for k in range(n))
    R = cr.rmatrix(trn, n)
    cond = float(np.linalg.cond(R))
    rc, got = _chest_matrix(lib, trn)
    resid = float(np.abs(R @ got - np.eye(n // 4)).max()) if rc == 0 else None
    print(f"n_fft {n}: band-nulled table, cond(R) {cond:.3g}, ofdm_chest_matrix -> {rc}" + ("" if resid is None else f", max |R got - I| {resid:.2e}"))
    assert rc == -1 or (rc == 0 and resid <= RESIDUAL)
    if n >= 256:
        assert rc == -1                                   # singular to rounding: outside the stage's domain


def test_ctx_key_takes_tables_by_value():
    from ofdm_amd import api

    pre, trn = pc.tables("unit_loud", 64)
    base = api._ctx_key(64, api.QAM64, True)
    k1 = api._ctx_key(64, api.QAM64, True, training=trn, preamble=pre)
    hash(k1)                                              # (an ndarray in the key used to raise TypeError: unhashable type)
    assert k1 == api._ctx_key(64, api.QAM64, 1, preamble=pre.copy(), training=trn.copy())             # the same tables: one context
    assert k1 == api._ctx_key(64, api.QAM64, True, training=list(trn), preamble=pre.astype(np.complex128))
    other = trn.copy()
    other[17] += 1e-12
    keys = {base, k1, api._ctx_key(64, api.QAM64, True, training=other, preamble=pre), api._ctx_key(64, api.QAM64, True, training=trn),
            api._ctx_key(64, api.QAM64, True, training=pc.tables("holes", 64)[1], preamble=pre),
            api._ctx_key(64, api.QAM64, True, pilots="stdrng"), api._ctx_key(64, api.QAM64, True, _replica=1, training=trn, preamble=pre),
            api._ctx_key(64, api.QAM64, True, training=trn, preamble=pre, cfo_mode=api.CFO_ABS)}
    assert len(keys) == 8                                 # different tables, a missing table, another replica or option: different contexts
    assert base == api._ctx_key(64, api.QAM64, True) and api._ctx_key(64, api.QAM64, True, cfo_mode=2) == api._ctx_key(64, api.QAM64, True, cfo_mode=2)
    assert trn.tobytes() == pc.tables("unit_loud", 64)[1].tobytes()                                    # the key does not touch its arguments
    assert hash(api._ctx_key(64, api.QAM64, True, tuning={"grid_cap": 3})) == hash(api._ctx_key(64, api.QAM64, True, tuning={"grid_cap": 3}))
    assert api._ctx_key(64, api.QAM64, True, tuning={"grid_cap": 3}) != api._ctx_key(64, api.QAM64, True, tuning={"grid_cap": 1})


def test_header_says_what_a_zero_training_bin_means():
    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    for text in ("A ZERO TRAINING BIN", "demaps by the NaN rule", "makes every LLR of the frame 0", "H' is finite in every bin",
                 "zero on a whole band", "H[k] is non-finite (NaN) in exactly those bins", "max |R rinv - I| <= 1e-6"):
        assert text in hdr, text
