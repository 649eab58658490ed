"""CPU checks of the framed convolutional modes (OFDM_ECC_CONV_K7F_R12 / _R23 / _R34) and the punctured stage entry points
(ofdm_conv_k7_kept_bits, ofdm_conv_k7_encode_punctured, ofdm_conv_k7_decode_punctured): the boundary accepts the new ecc values and
declares the entry points on every surface, and the numpy restatement tests/framed_ref.py -- the definition of these modes, parity
unpinned by the reference -- punctures as the header says, inverts noiseless streams, is maximum likelihood by brute force, rejects
damaged length blocks and orders the three rates on a noisy channel.  No kernel is launched here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as cr  # noqa: E402
import framed_ref as fr  # noqa: E402

NEW = ("ofdm_conv_k7_kept_bits", "ofdm_conv_k7_encode_punctured", "ofdm_conv_k7_decode_punctured")


@pytest.fixture(scope="module")
def lib():
    from ofdm_amd import build

    lib = C.CDLL(build.build())
    i64 = C.c_int64
    lib.ofdm_conv_k7_kept_bits.restype = i64
    lib.ofdm_conv_k7_kept_bits.argtypes = [i64, C.c_int32]
    lib.ofdm_conv_k7_encode_punctured.argtypes = [C.c_void_p, C.c_void_p, i64, i64, i64, C.c_int32, C.c_void_p, i64]
    lib.ofdm_conv_k7_decode_punctured.argtypes = [C.c_void_p, C.c_void_p, i64, i64, i64, C.c_int32, C.c_int32, C.c_void_p, i64]
    return lib


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


def test_create_accepts_the_framed_modes_and_nothing_above_them(lib):
    import torch

    want = 0 if torch.cuda.is_available() else -3          # OFDM_ERR_NO_DEVICE without a GPU, never INVALID
    assert [_create(lib, e) for e in (10, 11, 12)] == [want] * 3
    assert [_create(lib, e) for e in (13, 14, 99)] == [-1] * 3
    assert [_create(lib, e) for e in (3, 4, 6, 7, 8, 9, -1, 100)] == [-1] * 8


def test_new_surface_is_on_every_layer(lib):
    import ofdm_amd
    from ofdm_amd import api

    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ofdm_host.hpp")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in ofdm_amd.SIGNATURES
        assert re.search(r"\bint(64_t)? " + n + r"\(", hdr) and ("pub fn " + n + "(") in rs and (n + "(") in hpp
    for name, value in (("ECC_CONV_K7F_R12", 10), ("ECC_CONV_K7F_R23", 11), ("ECC_CONV_K7F_R34", 12),
                        ("CONV_RATE_1_2", 0), ("CONV_RATE_2_3", 1), ("CONV_RATE_3_4", 2)):
        assert re.search(r"\bOFDM_%s = %d\b" % (name, value), hdr), name
        assert ("pub const OFDM_%s: i32 = %d;" % (name, value)) in rs, name
        assert getattr(api, name) == value and getattr(ofdm_amd, name) == value
    # what the earlier modes pinned stays
    assert re.search(r"OFDM_ECC_CONV_K7 = 5\b", hdr) and re.search(r"3 and 4 are\s+REJECTED", hdr)
    assert "No puncturing" not in hdr and "punctured rates and framed modes" in hdr
    assert lib.ofdm_abi_version() == 1
    assert (fr.RATE_1_2, fr.RATE_2_3, fr.RATE_3_4) == (api.CONV_RATE_1_2, api.CONV_RATE_2_3, api.CONV_RATE_3_4)


def test_kept_bits_is_the_restatement(lib):
    for rate in fr.RATES:
        for T in list(range(51)) + [8 * (560 + 1), 8 * (1304 + 1)]:
            assert lib.ofdm_conv_k7_kept_bits(T, rate) == fr.kept(T, rate), (T, rate)
    for rate in (-1, 3, 99):
        assert lib.ofdm_conv_k7_kept_bits(16, rate) < 0
    assert lib.ofdm_conv_k7_kept_bits(-1, 0) < 0
    # the table of the header: period and mask
    assert [fr.kept(T, 1) for T in range(5)] == [0, 2, 3, 5, 6] and [fr.kept(T, 2) for T in range(7)] == [0, 2, 3, 4, 6, 7, 8]
    for rate in fr.RATES:       # max_steps inverts kept
        for bits in range(0, 80):
            T = fr.max_steps(bits, rate)
            assert fr.kept(T, rate) <= bits < fr.kept(T + 1, rate)
    assert [fr.coded_len(p, 0) for p in (0, 1, 560)] == [18 + 2, 18 + 4, 18 + 2 * 561]
    assert fr.coded_len(560, 1) == 18 + (12 * 561 + 7) // 8 and fr.coded_len(1304, 2) == 18 + (fr.kept(8 * 1305, 2) + 7) // 8


def test_entry_points_reject_a_null_context(lib):
    assert lib.ofdm_conv_k7_encode_punctured(None, None, 1, 4, 4, 1, None, 10) == -1
    assert lib.ofdm_conv_k7_decode_punctured(None, None, 1, 16, 8, 2, 1, None, 1) == -1
    assert lib.ofdm_conv_k7_encode_punctured(None, None, 0, 0, 0, 0, None, 0) == -1
    assert lib.ofdm_conv_k7_decode_punctured(None, None, 0, 0, 0, 0, 1, None, 0) == -1


def test_punctured_encode_is_the_code_with_the_masked_bits_deleted():
    rng = np.random.default_rng(10)
    for p in (0, 1, 2, 3, 11, 100):
        pay = rng.integers(0, 256, p, dtype=np.uint8).tobytes()
        full = np.unpackbits(cr.encode(pay), bitorder="little")
        for rate, period in ((0, ((1, 1),)), (1, ((1, 1), (1, 0))), (2, ((1, 1), (1, 0), (0, 1)))):
            keep = [int(full[2 * t + k]) for t in range(full.size // 2) for k in (0, 1) if period[t % len(period)][k]]
            assert len(keep) == fr.kept(8 * (p + 1), rate)
            want = np.packbits(np.array(keep, np.uint8), bitorder="little")
            got = fr.encode_punctured(pay, rate)
            np.testing.assert_array_equal(got, want)
            assert got.size == fr.body_len(p, rate)
            if rate == 0:
                np.testing.assert_array_equal(got, cr.encode(pay))
            stream = fr.encode_stream(pay, rate)
            assert stream.size == fr.coded_len(p, rate)
            np.testing.assert_array_equal(stream[:18], cr.encode(p.to_bytes(4, "little") + (p ^ 0xFFFFFFFF).to_bytes(4, "little")))
            np.testing.assert_array_equal(stream[18:], got)


def test_noiseless_streams_are_inverted():
    rng = np.random.default_rng(11)
    cases = 0
    for p in (0, 1, 2, 7, 40):
        pay = rng.integers(0, 256, p, dtype=np.uint8).tobytes()
        for rate in fr.RATES:
            T = 8 * (p + 1)
            bits = np.unpackbits(fr.encode_punctured(pay, rate), bitorder="little")[: fr.kept(T, rate)].astype(np.int64)
            for term in (True, False):
                got = fr.viterbi_punctured((2 * bits - 1) * 37, T, rate, term)
                assert bytes(got) == pay + b"\0", (p, rate, term)
                cases += 1
            llr = (2 * np.unpackbits(fr.encode_stream(pay, rate), bitorder="little").astype(np.int64) - 1) * 37
            assert fr.decode_stream(llr, fr.coded_len(p, rate), rate) == (0, pay)
    assert cases == 30


def test_punctured_viterbi_is_maximum_likelihood_by_brute_force():
    rng = np.random.default_rng(12)
    checked = 0
    for case in range(72):
        term, rate = case % 2 == 0, 1 + (case // 2) % 2
        T = 16 if term else 8
        n = fr.kept(T, rate)
        llr = rng.integers(-128, 128, n) if case % 8 < 4 else rng.integers(-6, 7, n)
        full = fr.depuncture(llr, T, rate)
        assert np.count_nonzero(full) <= n and full.size == 2 * T
        best, unique = cr.brute_force(full, term)          # a dropped position weighs nothing: ML over the kept ones
        if not unique:
            continue
        np.testing.assert_array_equal(fr.viterbi_punctured(llr, T, rate, term), np.packbits(best, bitorder="little"))
        checked += 1
    assert checked >= 25


def test_every_single_byte_change_of_a_length_block_is_rejected():
    for p in (0, 1, 560, 0x01020304, 0xFFFFFFFF):
        good = p.to_bytes(4, "little") + (p ^ 0xFFFFFFFF).to_bytes(4, "little") + b"\0"
        assert fr.length_block_value(good) == p
        for i in range(9):
            for delta in (1, 0x80, 0xFF, 0x5A):
                bad = bytearray(good)
                bad[i] ^= delta
                assert fr.length_block_value(bytes(bad)) is None, (p, i, delta)
    llr = (2 * np.unpackbits(fr.encode_stream(b"abc", 1), bitorder="little").astype(np.int64) - 1) * 37
    assert fr.decode_stream(llr, 17, 1) == (fr.HEADER_STATUS, b"")          # too little body
    wrong = np.concatenate([cr.encode(bytes([3, 0, 0, 0, 0xFC, 0xFF, 0xFF, 0x7F])), fr.encode_punctured(b"abc", 1)])
    llr = (2 * np.unpackbits(wrong, bitorder="little").astype(np.int64) - 1) * 37
    assert fr.decode_stream(llr, wrong.size, 1) == (fr.HEADER_STATUS, b"")  # a wrong complement


def test_cut_stream_delivers_the_unterminated_prefix():
    rng = np.random.default_rng(13)
    pay = rng.integers(0, 256, 60, dtype=np.uint8).tobytes()
    for rate in fr.RATES:
        stream = fr.encode_stream(pay, rate)
        llr = (2 * np.unpackbits(stream, bitorder="little").astype(np.int64) - 1) * 37
        avail = stream.size - 7
        st, got = fr.decode_stream(llr[: 8 * avail], avail, rate)
        T = fr.max_steps(8 * (avail - 18), rate)
        assert st == 0 and len(got) == min(60, T // 8) < 60
        assert got[:-2] == pay[: len(got) - 2]             # the open end may be wrong, what lies before it is not


def _noisy(rng, bits, sigma):
    rx = (2 * bits.astype(np.float64) - 1) + rng.normal(0, sigma, bits.shape)
    return np.clip(np.rint(24 * rx), -127, 127).astype(np.int64), int(((rx > 0) != (bits > 0)).sum())


def test_noisy_channel_figures_of_the_issue():
    """64 frames x 100 bytes, BPSK with Gaussian noise, LLR = clip(rint(24 rx)).  At sigma 0.6 (about 4.7 % raw flips) the payload bit
    errors of 51 200 are ordered rate 1/2 <= 2/3 <= 3/4, and the weakest rate still stays under half of what the uncoded payload would
    lose (the raw flip rate times 51 200 bits).  Measured with this draw order and seed (default_rng(14)): raw flips 4.73 %, payload bit
    errors 0 / 48 / 759 at rate 1/2 / 2/3 / 3/4, against a bound of 0.5 x 0.0473 x 51 200 = 1 211 (the issue's own draw: 0 / 59 / 877)."""
    rng = np.random.default_rng(14)
    pay = rng.integers(0, 256, (64, 100), dtype=np.uint8)
    errs, flips, sent = {}, 0, 0
    for rate in fr.RATES:
        T = 8 * 101
        e = 0
        for row in pay:
            bits = np.unpackbits(fr.encode_punctured(row.tobytes(), rate), bitorder="little")[: fr.kept(T, rate)]
            llr, fl = _noisy(rng, bits, 0.6)
            flips, sent = flips + fl, sent + bits.size
            got = fr.viterbi_punctured(llr, T, rate, True)[:100]
            e += int(np.unpackbits(got ^ row).sum())
        errs[rate] = e
    raw = flips / sent
    print(f"sigma 0.6: raw flips {raw:.4f}, payload bit errors of 51200 by rate {errs}")
    assert 0.04 < raw < 0.055
    assert errs[0] <= errs[1] <= errs[2] < 0.5 * raw * pay.size * 8, (errs, raw)


def test_length_block_survives_where_uncoded_bits_do_not():
    """sigma 0.5 flips about 2.3 % of the channel bits: 128 uncoded header bits survive in about 5 % of frames, the 72-step block
    in 200 of 200."""
    rng = np.random.default_rng(15)
    ok = 0
    for trial in range(200):
        p = int(rng.integers(0, 1 << 16))
        bits = np.unpackbits(fr.length_block(p), bitorder="little")
        llr, _ = _noisy(rng, bits, 0.5)
        ok += fr.length_block_value(cr.viterbi(llr, True)) == p
    assert ok == 200
