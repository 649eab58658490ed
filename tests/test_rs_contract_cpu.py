"""The host RS(255,223) decoder (ofdm_rs255_decode, ofdm_amd/csrc/outer_code.hip) held to its contract by construction: "a block
decodes to the unique code word within 16 byte errors or fails, a function of the input alone".  The blocks and their answers are
tests/rs_cases.py -- every error position, every weight 2 .. 16 in the patterns k_rs255_decode's lanes care about, the nearest other
code word, 17 .. 40 errors and noise -- and no reference decoder is involved: the judge is an encoder, restated there and pinned here
to ofdm_rs255_encode.  tests/test_gpu_rs_contract.py runs the same blocks on the device.  No kernel is launched here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rs_cases as rc  # noqa: E402
import rs_vectors as rv  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from ofdm_amd import build

    lib = C.CDLL(build.build())
    i64, vp = C.c_int64, C.c_void_p
    lib.ofdm_rs255_encode.argtypes = [vp, i64, vp]
    lib.ofdm_rs255_decode.argtypes = [vp, i64, vp, vp]
    return lib


def test_the_judging_encoder_is_the_library_s(lib):
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, (33, rc.K), dtype=np.uint8)
    data[32] = 0
    data[32, rc.K - 1] = 1                                              # e_222: its code word is the generator polynomial
    words = rc.encode(data)
    assert words.shape == (33, rc.N)
    for d, w in zip(data, words):
        assert rv.host_encode(lib, bytes(d))[:rc.N] == bytes(w)         # (host_encode appends the always-present empty block)
    assert bytes(words[32, rc.K - 1:]) == bytes(rc.GEN.astype(np.uint8)) and not words[32, :rc.K - 1].any()
    assert rc.GEN.size == 33 and rc.GEN.all() and rc.GEN[0] == 1


def test_families_are_what_they_say():
    cs = rc.cases()
    assert rc.family_counts(cs) == rc.COUNTS == {"A": 765, "B": 480, "C": 24, "D": 1024, "E": 17}
    assert cs is rc.cases()                                             # built once, shared
    for family, block, expectation in cs:
        assert block.shape == (rc.N,) and block.dtype == np.uint8
        assert (expectation[0] == "either") == (family == "D")
    judged = [c for c in cs if c[2][0] == "is"]                         # the answer is a code word exactly `fixed` bytes from the input
    answers = rc.encode(np.array([np.frombuffer(e[1], np.uint8) for _, _, e in judged]))
    distance = (answers != np.array([b for _, b, _ in judged])).sum(axis=1)
    assert distance.tolist() == [e[2] for _, _, e in judged]
    a = [c for c in cs if c[0] == "A"]
    word = rc.encode(np.frombuffer(a[0][2][1], np.uint8))               # family A's one code word
    assert all(e[1] == a[0][2][1] for _, _, e in a)
    hit = sorted((int(np.flatnonzero(b != word)[0]), int((b ^ word).max())) for _, b, _ in a)
    assert hit == [(pos, v) for pos in range(rc.N) for v in (0x01, 0x80, 0xFF)]   # every position with every value
    b_weights = sorted(e[2] for f, _, e in cs if f == "B")
    assert b_weights == sorted(list(range(2, 17)) * 32)
    c_fixed = [e[2] for f, _, e in cs if f == "C"]
    assert c_fixed == [16] * 24


def test_host_decoder_keeps_the_contract_on_every_block(lib):
    cs = rc.cases()
    tally = rc.judge_all(cs, [rv.host_block(lib, block) for _, block, _ in cs])
    d = tally["D"]
    print(f"family D: {d.get('decoded', 0)} of {sum(d.values())} blocks beyond capacity decoded to another code word (not capped)")
    assert sum(d.values()) == rc.COUNTS["D"]


def test_a_block_s_count_follows_from_its_bytes(lib):
    """rs_cases.check_uncounted, which judges the blocks of a device row of three, gives every block the host decoder's own count"""
    cs = rc.cases()
    results = [rv.host_block(lib, block) for _, block, _ in cs]
    distance = rc.distances(np.array([b for _, b, _ in cs]), np.array([np.frombuffer(d, np.uint8) for d, _ in results]))
    for (family, block, expectation), (delivered, fixed), dist in zip(cs, results, distance):
        assert rc.check_uncounted(block, delivered, expectation, dist) == fixed, family
    family, block, expectation = next(c for c in cs if c[0] == "D")
    assert rc.check_uncounted(block, bytes(block[:rc.K]), expectation) == -1
    with pytest.raises(AssertionError):                                 # neither unchanged nor a code word within 16
        rc.check_uncounted(block, bytes([block[0] ^ 1]) + bytes(block[1:rc.K]), expectation)


def test_the_check_refuses_what_breaks_the_contract():
    """the judge itself: answers that break each arm are refused"""
    cs = rc.cases()
    family, block, (_, data, fixed) = next(c for c in cs if c[0] == "B")
    assert rc.check(block, data, fixed, ("is", data, fixed)) == "is"
    wrong = bytes([data[0] ^ 1]) + data[1:]
    for delivered, count in ((wrong, fixed), (data, fixed + 1), (bytes(block[:rc.K]), -1)):
        with pytest.raises(AssertionError):
            rc.check(block, delivered, count, ("is", data, fixed))
    either = ("either",)
    assert rc.check(block, bytes(block[:rc.K]), -1, either) == "failed"
    assert rc.check(block, data, fixed, either) == "decoded"
    assert data != bytes(block[:rc.K])                                  # (the first block of B has its errors in the data bytes)
    for delivered, count in ((data, -1), (data, fixed - 1), (wrong, fixed), (data, 0), (data, 17)):
        with pytest.raises(AssertionError):
            rc.check(block, delivered, count, either)
