"""CPU checks of the convolutional mode (OFDM_ECC_CONV_K7, ofdm_conv_k7_encode, ofdm_conv_k7_decode_soft): the boundary accepts
the new ecc value and declares the two entry points on every surface, and the numpy restatement tests/conv_ref.py gives the known
answers, inverts noiseless codewords and is maximum likelihood by brute force.  No kernel is launched here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as cr  # noqa: E402

NEW = ("ofdm_conv_k7_encode", "ofdm_conv_k7_decode_soft")
KNOWN = (("", "0000"), ("61", "fb689c03"), ("616263", "fb68708c8bb89c03"), ("0001020304050607", "0000fb34ecd317e7b04f487b5f9ca4a80300"))


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


def test_create_accepts_conv_k7_and_nothing_around_it(lib):
    import torch

    assert _create(lib, 5) == (0 if torch.cuda.is_available() else -3)   # OFDM_ERR_NO_DEVICE without a GPU, never INVALID
    assert [_create(lib, e) for e in (6, 8, 9)] == [-1] * 3


def test_new_entry_points_are_on_every_surface(lib):
    import ofdm_amd

    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ofdm_host.hpp")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in ofdm_amd.SIGNATURES
        assert re.search(r"\bint " + n + r"\(", hdr) and ("pub fn " + n + "(") in rs and (n + "(") in hpp
    assert re.search(r"OFDM_ECC_CONV_K7 = 5\b", hdr) and "pub const OFDM_ECC_CONV_K7: i32 = 5;" in rs
    assert re.search(r"3 and 4 are\s+REJECTED", hdr)
    assert ofdm_amd.ECC_CONV_K7 == 5
    assert lib.ofdm_abi_version() == 1


def test_entry_points_reject_a_null_context(lib):
    i64 = C.c_int64
    lib.ofdm_conv_k7_encode.argtypes = [C.c_void_p, C.c_void_p, i64, i64, i64, C.c_void_p, i64]
    lib.ofdm_conv_k7_decode_soft.argtypes = [C.c_void_p, C.c_void_p, i64, i64, i64, C.c_int32, C.c_void_p, i64]
    assert lib.ofdm_conv_k7_encode(None, None, 1, 4, 4, None, 10) == -1
    assert lib.ofdm_conv_k7_decode_soft(None, None, 1, 16, 8, 1, None, 1) == -1


def test_encoder_known_answers():
    for pay, code in KNOWN:
        assert bytes(cr.encode(bytes.fromhex(pay))).hex() == code
    for p in (0, 1, 5, 100):
        assert cr.encode(bytes(p)).size == 2 * (p + 1)


def test_viterbi_inverts_noiseless_codewords():
    rng = np.random.default_rng(1)
    for p in (0, 1, 2, 7, 40):
        pay = rng.integers(0, 256, p, dtype=np.uint8).tobytes()
        bits = np.unpackbits(cr.encode(pay), bitorder="little").astype(np.int64)
        for amp in (1, 37, 127):
            for term in (True, False):
                got = cr.viterbi((2 * bits - 1) * amp, term)
                assert bytes(got) == pay + b"\0", (p, amp, term)


def test_viterbi_is_maximum_likelihood_by_brute_force():
    rng = np.random.default_rng(2)
    checked = 0
    for case in range(40):
        term = case % 2 == 0
        T = 16 if term else 8                    # 2^10 terminated inputs of 16 bits, 2^8 free inputs of 8 bits
        llr = rng.integers(-128, 128, 2 * T) if case % 4 < 2 else rng.integers(-6, 7, 2 * T)
        best, unique = cr.brute_force(llr, term)
        if not unique:
            continue
        np.testing.assert_array_equal(cr.viterbi(llr, term), np.packbits(best, bitorder="little"))
        checked += 1
    assert checked >= 25


def test_both_tie_rules():
    # all-zero LLRs: every decision ties (p0 is kept), every final metric ties (state 0 wins) -> the all-zero path
    for T in (8, 13, 64, 200):
        for term in (True, False):
            got = cr.viterbi(np.zeros(2 * T, np.int8), term)
            assert got.size == T // 8 and not got.any()
    assert cr.viterbi(np.zeros(14), True).size == 0


def test_batch_form_is_the_scalar_form():
    rng = np.random.default_rng(3)
    for T in (0, 5, 8, 77, 300):
        llr = rng.integers(-128, 128, (6, 2 * T + 3))
        for term in (True, False):
            want = np.stack([cr.viterbi(r[: 2 * T], term) for r in llr]) if T >= 8 else np.zeros((6, 0), np.uint8)
            np.testing.assert_array_equal(cr.viterbi_batch(llr[:, : 2 * T], term), want)


def test_noisy_channel_figure_of_the_issue():
    # 64 frames of 100 bytes at a noise level that flips about a tenth of the channel bits: a few hundred payload bit errors of 51 200
    rng = np.random.default_rng(4)
    pay = rng.integers(0, 256, (64, 100), dtype=np.uint8)
    bits = np.stack([np.unpackbits(cr.encode(p.tobytes()), bitorder="little") for p in pay]).astype(np.float64)
    rx = (2 * bits - 1) + rng.normal(0, 0.8, bits.shape)
    flipped = ((rx > 0) != (bits > 0)).mean()
    assert 0.08 < flipped < 0.13
    llr = np.clip(np.rint(rx * 24), -127, 127).astype(np.int64)
    got = cr.viterbi_batch(llr, True)[:, :100]
    errs = int(np.unpackbits(got ^ pay).sum())
    assert errs < 0.02 * pay.size * 8, errs          # against about 10 % uncoded
