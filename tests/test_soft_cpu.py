"""CPU checks of the soft-decision extension (OFDM_ECC_HAMMING74_SOFT, ofdm_rx_llr_batch, ofdm_hamming74_decode_soft): the boundary
accepts the new ecc value and declares the two entry points, and the numpy restatement tests/soft_ref.py agrees with hand-worked
values and with the kernels' closed form.  No kernel is launched here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import soft_ref as sr  # noqa: E402

NEW = ("ofdm_rx_llr_batch", "ofdm_hamming74_decode_soft")


@pytest.fixture(scope="module")
def lib():
    from ofdm_amd import build

    return C.CDLL(build.build())


def _create(lib, ecc):
    from ofdm_amd import Params

    p = Params()
    lib.ofdm_default_params(C.byref(p))
    p.ecc = ecc
    h = C.c_void_p()
    rc = lib.ofdm_create(C.byref(p), None, None, 0, None, C.byref(h))
    if rc == 0:
        lib.ofdm_destroy(h)
    return rc


def test_create_accepts_soft_hamming(lib):
    import torch

    assert _create(lib, 2) == (0 if torch.cuda.is_available() else -3)   # OFDM_ERR_NO_DEVICE without a GPU, never INVALID


def test_create_still_rejects_ecc_3_and_above(lib):
    assert [_create(lib, e) for e in (3, 4, -1, 100)] == [-1] * 4


def test_new_entry_points_are_on_every_surface(lib):
    import ofdm_amd
    from ofdm_amd import api

    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in ofdm_amd.SIGNATURES
        assert re.search(r"\bint " + n + r"\(", hdr) and ("pub fn " + n + "(") in rs
    assert re.search(r"OFDM_ECC_HAMMING74_SOFT = 2\b", hdr) and "pub const OFDM_ECC_HAMMING74_SOFT: i32 = 2;" in rs
    m = re.search(r"#define OFDM_SOFT_LLR_SCALE ([0-9.]+)f", hdr)
    assert m and float(m.group(1)) == api.SOFT_LLR_SCALE
    assert (ofdm_amd.ECC_HAMMING74_SOFT, ofdm_amd.SOFT_LLR_SCALE) == (2, api.SOFT_LLR_SCALE)


def test_soft_entry_points_reject_bad_arguments_without_a_context(lib):
    lib.ofdm_rx_llr_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_int64]
    lib.ofdm_hamming74_decode_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    assert lib.ofdm_rx_llr_batch(None, None, 1, 80, 80, 0, 1, None, None, None, 0, 16.0, None, 64) == -1
    assert lib.ofdm_hamming74_decode_soft(None, None, 56, None) == -1


def test_bpsk_and_qpsk_llr_is_v():
    v = np.array([-3.5, -1.0, -0.25, 0.0, 0.5, 1.0, 2.75])
    np.testing.assert_array_equal(sr.axis_llr(v, 1)[:, 0], v)
    np.testing.assert_array_equal(sr.point_llr(v + 0j, 1)[:, 0], v)
    z = np.array([0.3 - 0.7j, -1.2 + 0.1j])
    np.testing.assert_allclose(sr.point_llr(z, 2), [[0.3, -0.7], [-1.2, 0.1]], rtol=0, atol=1e-12)   # I bit, then Q bit


def test_16qam_closed_forms_by_hand():
    # M = 4: levels -3 -1 1 3, Gray 00 01 11 10.  MSB: v for |v| <= 2, 2v -+ 2 beyond; LSB: 2 - |v|
    for v, want in ((0.5, (0.5, 1.5)), (-0.5, (-0.5, 1.5)), (3.0, (4.0, -1.0)), (-2.5, (-3.0, -0.5)), (1.0, (1.0, 1.0)),
                    (-1.0, (-1.0, 1.0)), (2.0, (2.0, 0.0)), (5.0, (8.0, -3.0))):
        np.testing.assert_allclose(sr.axis_llr(np.array([v]), 2)[0], want, atol=1e-12)
    # a 16-QAM point at x = 1/3 (level 2, v = 1) on I and x = -1 (level 0, v = -3) on Q: bits I(1, 1), Q(0, 0)
    np.testing.assert_allclose(sr.point_llr(np.array([1 / 3 - 1j]), 4)[0], [1.0, 1.0, -4.0, -1.0], atol=1e-12)


def test_noiseless_weakest_bit_has_unit_magnitude():
    for m in (1, 2, 3, 4):
        M = 1 << m
        lam = sr.axis_llr(2.0 * np.arange(M) - (M - 1), m)
        assert np.abs(lam).min() == 1.0
        bits = np.stack([sr.gray_bit(np.arange(M), m, b) for b in range(m)], -1)
        assert ((lam > 0) == (bits == 1)).all()                    # positive means bit 1


def test_closed_form_is_the_brute_force_minimum():
    v = np.concatenate([np.linspace(-20, 20, 40001), np.arange(-17, 18, 1.0)])   # every level and boundary, dense in between
    for m in (1, 2, 3, 4):
        np.testing.assert_allclose(sr.axis_llr_closed(v, m), sr.axis_llr(v, m), rtol=0, atol=1e-9)


def test_quantise_and_weights():
    np.testing.assert_array_equal(sr.quantise([0.5, 1.5, -2.5, 200.0, -1e9, np.nan, np.inf, -np.inf]), [0, 2, -2, 127, -127, 0, 0, 0])
    hk = np.array([[1.0, 2.0, 0.0, 1j]])
    np.testing.assert_allclose(sr.channel_weights(hk, np.array([0, 1, 3])), [[0.5, 2.0, 0.5]])


def test_soft_hamming_restatement_by_hand():
    rng = np.random.default_rng(3)
    d = rng.integers(0, 16, 16)
    bits = np.array([(sr.ham_codeword(x) >> i) & 1 for x in d for i in range(7)])
    llr = (2 * bits - 1) * 20
    got = sr.ham_decode_soft(llr)
    np.testing.assert_array_equal(got, (d[0::2] | (d[1::2] << 4)).astype(np.uint8))
    assert (sr.ham_decode_soft(np.zeros(56, np.int8)) == 0).all()          # every codeword ties: the smallest nibble
    one = np.zeros(56, np.int64)
    one[3] = 5   # only d3 carries weight: every nibble with bit 3 set ties at +5, the smallest of them is 8
    assert sr.ham_decode_soft(one)[0] == 8
    assert sr.ham_decode_soft(np.zeros(55)).size == 0
