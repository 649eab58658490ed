"""CPU checks of the LDPC(648) modes of rates 2/3, 3/4 and 5/6 (OFDM_ECC_LDPC648_R23 / _R34 / _R56 = 41 / 42 / 43, with the frame check
105 / 106 / 107): the tables' properties and that every layer states the same ones, the host encoder and decoder of the library held
to tests/ldpc_rates_ref.py bit for bit (iteration counts included) on the sets tests/test_gpu_ldpc_rates.py decodes on the device,
rate 0 held to the functions that have no `rate`, the tables' quality through the real shortening and puncturing, the frame stream,
and the boundary: the new exports on every layer and which ecc values ofdm_create takes.  No kernel is launched here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldpc_rates_ref as rr  # noqa: E402
import ldpc_rates_vectors as rv  # noqa: E402
import ldpc_ref as lr  # noqa: E402

NEW = ("ofdm_ldpc648_info_bytes", "ofdm_ldpc648_coded_len_rate", "ofdm_ldpc648_encode_rate", "ofdm_ldpc648_decode_rate",
       "ofdm_ldpc648_encode_rate_batch", "ofdm_ldpc648_decode_rate_batch")
BLOCKS = (88, 87, 85, 81)
ROW_DEGREES = (None, [11, 10, 10, 11, 12, 11, 11, 11], [14, 14, 14, 15, 14, 14], [20, 20, 21, 20])


@pytest.fixture(scope="module")
def lib():
    from ofdm_amd import build

    lib = C.CDLL(build.build())
    i64, i32, vp = C.c_int64, C.c_int32, C.c_void_p
    lib.ofdm_ldpc648_info_bytes.restype = i32
    lib.ofdm_ldpc648_info_bytes.argtypes = [i32]
    lib.ofdm_ldpc648_coded_len_rate.restype = i64
    lib.ofdm_ldpc648_coded_len_rate.argtypes = [i64, i32]
    lib.ofdm_ldpc648_encode_rate.argtypes = [vp, i64, i32, vp]
    lib.ofdm_ldpc648_decode_rate.argtypes = [vp, i64, i32, i32, vp, vp]
    lib.ofdm_ldpc648_encode_rate_batch.argtypes = [vp, vp, i64, i64, i64, i32, vp, i64]
    lib.ofdm_ldpc648_decode_rate_batch.argtypes = [vp, vp, i64, i64, i64, i32, i32, vp, i64, vp]
    lib.ofdm_ldpc648_coded_len.restype = i64
    lib.ofdm_ldpc648_coded_len.argtypes = [i64]
    lib.ofdm_ldpc648_encode.argtypes = [vp, i64, vp]
    lib.ofdm_ldpc648_decode.argtypes = [vp, i64, i32, vp, vp]
    return lib


def host_encode(lib, rate, info):
    k = rr.INFO_BYTES[rate]
    info = np.ascontiguousarray(info, np.uint8).reshape(-1, k)
    out = np.full((info.shape[0], rr.CODE_BYTES), 0x5A, np.uint8)
    assert lib.ofdm_ldpc648_encode_rate(info.ctypes.data, info.shape[0], rate, out.ctypes.data) == 0
    return out


def host_decode(lib, rate, llr, max_iter):
    llr = np.ascontiguousarray(llr, np.int8).reshape(-1, rr.SENT_BITS)
    out = np.full((llr.shape[0], rr.INFO_BYTES[rate]), 0xA5, np.uint8)
    iters = np.full(llr.shape[0], -7, np.int32)
    assert lib.ofdm_ldpc648_decode_rate(llr.ctypes.data, llr.shape[0], max_iter, rate, out.ctypes.data, iters.ctypes.data) == 0
    return out, iters


# ------------------------------------------------------------------------------------------------ the codes
@pytest.mark.parametrize("rate", (1, 2, 3))
def test_table_properties(rate):
    code = rr.CODES[rate]
    t = code.table
    rows = (None, 8, 6, 4)[rate]
    assert t.shape == (rows, 24) and int((t >= 0).sum()) == BLOCKS[rate] and t.max() < rr.Z
    assert (t >= 0).sum(axis=1).tolist() == ROW_DEGREES[rate] and max(ROW_DEGREES[rate]) <= 21
    h = code.parity_check_matrix()
    m = 27 * rows
    assert h.shape == (m, 648) and int(h.sum()) == BLOCKS[rate] * 27
    assert lr.gf2_rank(h) == m == (None, 216, 162, 108)[rate]               # full rank
    assert lr.gf2_rank(h[:, 648 - m:]) == m                                 # the parity half is invertible
    overlap = h.astype(np.int64) @ h.astype(np.int64).T                     # two rows sharing two columns = a 4-cycle
    np.fill_diagonal(overlap, 0)
    assert overlap.max() <= 1
    # the parity half: shifts 1 / 0 / 1 in the first, middle and last row of the first parity column, then the dual diagonal
    k = 24 - rows
    assert [int(v) for v in t[:, k]] == [1 if l in (0, rows - 1) else 0 if l == rows // 2 else -1 for l in range(rows)]
    for j in range(1, rows):
        assert [int(v) for v in t[:, k + j]] == [0 if l in (j - 1, j) else -1 for l in range(rows)]
    # what travels: 640 bits, the shortened and punctured counts of the header
    assert code.sent.size == 640 and np.unique(code.sent).size == 640
    assert (code.shortened.size, code.punctured.size) == ((8, 0), (6, 2), (4, 4))[rate - 1]
    assert (code.k, code.info_bits, code.parity_sent) == ((53, 424, 216), (60, 480, 160), (67, 536, 104))[rate - 1]


def test_rate_0_is_ldpc_ref():
    code = rr.CODES[0]
    assert code.table is lr.TABLE and code.k == lr.INFO_BYTES and code.m == lr.M
    np.testing.assert_array_equal(code.parity_check_matrix(), lr.parity_check_matrix())
    rng = np.random.default_rng(12)
    info = rng.integers(0, 256, (16, 40), dtype=np.uint8)
    np.testing.assert_array_equal(code.encode(info), lr.encode(info))
    llr = rv.pool(0)[0]
    for max_iter in rv.MAX_ITERS:
        a, b = rv.reference(0, max_iter), lr.decode(llr, max_iter)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    for p in (0, 1, 32, 33, 560):
        pay = bytes(rng.integers(0, 256, p, dtype=np.uint8))
        np.testing.assert_array_equal(code.stream(pay), lr.stream(pay))
    assert [code.row_bytes(b) for b in (0, 79, 80, 1000)] == [lr.row_bytes(b) for b in (0, 79, 80, 1000)]


def _tables_in(text, start, count):
    """the first `count` runs of rows of 24 entries ("-" or -1 = a zero block) in text behind `start`"""
    rows = []
    for ln in text[text.index(start):].splitlines():
        tok = re.findall(r"-1|-|\d+", re.sub(r"[{},*]", " ", ln))
        plain = re.sub(r"[{},*\s]|-1|-|\d+", "", ln)
        if len(tok) == 24 and not plain:
            rows.append([-1 if v in ("-", "-1") else int(v) for v in tok])
    want = [rr.TABLES[r].shape[0] for r in (1, 2, 3)][:count]
    out, at = [], 0
    for n in want:
        out.append(np.array(rows[at:at + n]))
        at += n
    return out


def test_every_layer_states_the_same_tables():
    txt = open(os.path.join(ROOT, "ofdm_amd", "csrc", "ldpc_table.h")).read()
    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    for got in (_tables_in(txt, "kLdpcShiftR23[8][kLdpcCols] = {", 3), _tables_in(hdr, "LDPC(648), rates 2/3, 3/4 and 5/6 (OFDM_ECC", 3)):
        for rate in (1, 2, 3):
            np.testing.assert_array_equal(got[rate - 1], rr.TABLES[rate])
    doc = hdr[hdr.index("LDPC(648), rates 2/3, 3/4 and 5/6 (OFDM_ECC"):][:6000]
    assert "NOT the matrices of 802.11n" in doc and "NOT the matrices of 802.11n" in txt and "NOT the matrices of 802.11n" in rr.__doc__


# ------------------------------------------------------------------------------------------------ the encoder
@pytest.mark.parametrize("rate", rr.RATES)
def test_host_encoder_is_the_reference_and_makes_codewords(lib, rate):
    code = rr.CODES[rate]
    info = np.random.default_rng(50 + rate).integers(0, 256, (48, code.k), dtype=np.uint8)
    info[0] = np.arange(code.k)
    info[1] = 0xFF
    info[2] = 0
    x = code.codeword_bits(info)
    h = code.parity_check_matrix().astype(np.int64)
    assert not ((x.astype(np.int64) @ h.T) & 1).any()                       # H x = 0 over the full 648 bits
    assert not x[:, code.shortened].any()
    got = host_encode(lib, rate, info)
    np.testing.assert_array_equal(got, code.encode(info))
    np.testing.assert_array_equal(got[:, :code.k], info)                    # systematic
    np.testing.assert_array_equal(np.unpackbits(got, axis=1, bitorder="little"), x[:, code.sent])


# ------------------------------------------------------------------------------------------------ the decoder
@pytest.mark.parametrize("max_iter", rv.MAX_ITERS)
@pytest.mark.parametrize("rate", rr.RATES)
def test_host_decoder_is_the_reference(lib, rate, max_iter):
    llr = rv.pool(rate)[0]
    want, want_it = rv.reference(rate, max_iter)
    got, got_it = host_decode(lib, rate, llr, max_iter)
    np.testing.assert_array_equal(got_it, want_it)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("rate", rr.RATES)
def test_the_pool_holds_every_class(rate):
    """what the host and the device decoders are compared on: words that converge at iteration 1, late and never, and the corners"""
    llr, info, kind = rv.pool(rate)
    kind = np.array(kind)
    by, it = rv.reference(rate, 20)
    print(f"rate {rate}: iterations by kind " + ", ".join(f"{k}: {sorted(it[kind == k].tolist())}" for k in sorted(set(kind))))
    assert (it[kind == "clean"] == 1).all() and (by[kind == "clean"] == info[kind == "clean"]).all()
    assert (it[kind == "junk"] == 0).all()
    assert it[kind == "zero"] == 1 and not by[kind == "zero"].any()           # all-zero LLRs: the all-zero word at once
    assert it[kind == "low"] == 1 and not by[kind == "low"].any()             # all -128: the all-zero word at full confidence
    assert it[kind == "high"] == 0                                            # all +127: the all-ones word is no code word of any rate
    noisy = np.char.startswith(kind, "noisy")
    assert (it[noisy] == 0).any() and (it[noisy] >= 4).any() and (it[noisy] == 1).any()
    conv = it > 0
    assert (by[conv & noisy] == info[conv & noisy]).all()                     # no converged word differs from what was sent
    assert kind[:8].tolist() == ["clean", "junk", "junk", "clean", "zero", "low", "junk", "clean"]
    it1 = rv.reference(rate, 1)[1]
    assert set(it1.tolist()) == {0, 1} and (it1 == 1).sum() < (it > 0).sum()


@pytest.mark.parametrize("rate", rr.RATES)
def test_rate_0_and_every_rate_through_the_rate_functions(lib, rate):
    """rate 0 through the _rate functions = the functions without a rate, byte for byte; every rate: K and coded_len"""
    code = rr.CODES[rate]
    assert lib.ofdm_ldpc648_info_bytes(rate) == code.k
    if rate:
        return
    rng = np.random.default_rng(3)
    info = rng.integers(0, 256, (32, 40), dtype=np.uint8)
    old = np.zeros((32, 80), np.uint8)
    assert lib.ofdm_ldpc648_encode(info.ctypes.data, 32, old.ctypes.data) == 0
    np.testing.assert_array_equal(host_encode(lib, 0, info), old)
    llr = np.ascontiguousarray(rv.pool(0)[0])
    for max_iter in (1, 5, 20):
        out = np.zeros((llr.shape[0], 40), np.uint8)
        its = np.zeros(llr.shape[0], np.int32)
        assert lib.ofdm_ldpc648_decode(llr.ctypes.data, llr.shape[0], max_iter, out.ctypes.data, its.ctypes.data) == 0
        got, got_it = host_decode(lib, 0, llr, max_iter)
        np.testing.assert_array_equal(got, out)
        np.testing.assert_array_equal(got_it, its)
    for p in (0, 31, 32, 33, 560, 1304):
        assert lib.ofdm_ldpc648_coded_len_rate(p, 0) == lib.ofdm_ldpc648_coded_len(p)


QUALITY_EBN0_DB = (None, 3.5, 4.0, 5.0)


@pytest.mark.parametrize("rate", (1, 2, 3))
def test_table_quality_through_shortening_and_puncturing(rate):
    """200 random info words a rate, BPSK + AWGN, L = clip(rint(32 y)), Eb/N0 3.5 / 4.0 / 5.0 dB with the rate taken as 8 K / 640: at most
    2 of 200 may fail to converge within 20 iterations and none may converge to a wrong word."""
    code = rr.CODES[rate]
    rng = np.random.default_rng(2026 + rate)
    info = rng.integers(0, 256, (200, code.k), dtype=np.uint8)
    llr = rv.awgn_llr(code, info, QUALITY_EBN0_DB[rate], rng)
    by, it = code.decode(llr, 20)
    failed = int((it == 0).sum())
    wrong = int(((it > 0) & (by != info).any(axis=1)).sum())
    print(f"rate {rate} at {QUALITY_EBN0_DB[rate]} dB: {failed} of 200 unconverged, {wrong} converged to a wrong word, mean iterations "
          f"{it[it > 0].mean():.2f}")
    assert failed <= 2 and wrong == 0


def test_argument_checks(lib):
    llr = np.zeros(640, np.int8)
    out = np.zeros(80, np.uint8)
    for rate in (-1, 4, 41):
        assert lib.ofdm_ldpc648_info_bytes(rate) == -1 and lib.ofdm_ldpc648_coded_len_rate(10, rate) == -1
        assert lib.ofdm_ldpc648_encode_rate(out.ctypes.data, 1, rate, out.ctypes.data) == -1
        assert lib.ofdm_ldpc648_decode_rate(llr.ctypes.data, 1, 20, rate, out.ctypes.data, None) == -1
        assert lib.ofdm_ldpc648_encode_rate_batch(None, None, 0, 0, 0, rate, None, 0) == -1
    for rate in rr.RATES:
        for bad in (0, -1, 65):
            assert lib.ofdm_ldpc648_decode_rate(llr.ctypes.data, 1, bad, rate, out.ctypes.data, None) == -1
        assert lib.ofdm_ldpc648_decode_rate(llr.ctypes.data, -1, 20, rate, out.ctypes.data, None) == -1
        assert lib.ofdm_ldpc648_decode_rate(None, 1, 20, rate, out.ctypes.data, None) == -1
        assert lib.ofdm_ldpc648_decode_rate(None, 0, 20, rate, None, None) == 0
        assert lib.ofdm_ldpc648_decode_rate(llr.ctypes.data, 1, 64, rate, out.ctypes.data, None) == 0      # iters is optional
        assert lib.ofdm_ldpc648_encode_rate(None, 0, rate, None) == 0 and lib.ofdm_ldpc648_encode_rate(None, 1, rate, out.ctypes.data) == -1
        assert lib.ofdm_ldpc648_coded_len_rate(-1, rate) == -1
        # the batch calls check their arguments before they need a device
        assert lib.ofdm_ldpc648_encode_rate_batch(None, None, 1, 80, 1, rate, None, 80) == -1
        assert lib.ofdm_ldpc648_decode_rate_batch(None, None, 1, 640, 1, 20, rate, None, 80, None) == -1


# ------------------------------------------------------------------------------------------------ the frame stream
def _llrs_of(stream_bytes, amp=40):
    bits = np.unpackbits(np.asarray(stream_bytes, np.uint8), bitorder="little").astype(np.int64)
    return (amp * (2 * bits - 1)).astype(np.int8)


@pytest.mark.parametrize("rate", (1, 2, 3))
def test_stream_build_and_coded_len(lib, rate):
    code = rr.CODES[rate]
    k = code.k
    for p in (0, 1, k - 8, k - 7, 2 * k - 8, 560):
        pay = bytes(np.random.default_rng(p).integers(0, 256, p, dtype=np.uint8))
        info = code.info_stream(pay)
        B = -(-(p + 8) // k)
        assert info.size == k * B == k * code.codewords(p)
        assert info[:4].tobytes() == p.to_bytes(4, "little") and info[4:8].tobytes() == (p ^ 0xFFFFFFFF).to_bytes(4, "little")
        assert info[8:8 + p].tobytes() == pay and not info[8 + p:].any()
        s = code.stream(pay)
        assert s.size == code.coded_len(p) == 80 * B == lib.ofdm_ldpc648_coded_len_rate(p, rate)
        np.testing.assert_array_equal(s.reshape(B, 80), host_encode(lib, rate, info))
    assert [code.coded_len(p) // 80 for p in (0, 1, k - 8, k - 7, 2 * k - 8)] == [1, 1, 1, 2, 2]
    assert code.coded_len(560) // 80 == (None, 11, 10, 9)[rate]
    assert [code.row_bytes(b) for b in (0, 79, 80, 159, 160)] == [0, 0, k - 8, k - 8, 2 * k - 8]


@pytest.mark.parametrize("rate", (1, 2, 3))
def test_receive_rule_every_branch(rate):
    code = rr.CODES[rate]
    k = code.k
    rng = np.random.default_rng(11 + rate)
    pay = bytes(rng.integers(0, 256, 2 * k + 5, dtype=np.uint8))    # 3 code words
    assert code.codewords(len(pay)) == 3
    llr = _llrs_of(code.stream(pay))
    assert code.receive(llr, 240) == (0, pay)                        # whole
    assert code.receive(llr, 239) == (0, pay[:2 * k - 8])            # cut: the prefix of the two whole code words
    assert code.receive(llr, 80) == (0, pay[:k - 8])
    for body in (79, 0, -16):
        assert code.receive(llr, body) == (rr.HEADER_STATUS, b"")    # no whole code word
    junk = rng.integers(-128, 128, 640, dtype=np.int8)
    assert code.decode(junk)[1][0] == 0
    bad0 = llr.copy(); bad0[:640] = junk
    assert code.receive(bad0, 240) == (rr.HEADER_STATUS, b"")        # code word 0 does not converge
    bad2 = llr.copy(); bad2[1280:1920] = junk
    assert code.receive(bad2, 240) == (rr.UNCORRECTABLE_STATUS, b"")  # a later one does not
    assert code.receive(bad2, 160) == (0, pay[:2 * k - 8])           # ... but lies behind the cut
    info = code.info_stream(pay).copy(); info[5] ^= 0x10             # length words not complementary
    assert code.receive(_llrs_of(code.encode(info.reshape(-1, k)).reshape(-1)), 240) == (rr.HEADER_STATUS, b"")
    for p in (1000, 0xFFFFFFFF):                                     # p claiming more code words than the frame holds
        info = code.info_stream(pay).copy()
        info[:4] = np.frombuffer(p.to_bytes(4, "little"), np.uint8)
        info[4:8] = np.frombuffer((p ^ 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)
        st, out = code.receive(_llrs_of(code.encode(info.reshape(-1, k)).reshape(-1)), 240)
        assert st == 0 and out == info[8:].tobytes() and len(out) == 3 * k - 8


# ------------------------------------------------------------------------------------------------ the boundary
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


def test_create_accepts_the_six_modes_and_nothing_around_them(lib):
    import torch

    want = 0 if torch.cuda.is_available() else -3          # OFDM_ERR_NO_DEVICE without a GPU, never INVALID
    assert [_create(lib, e) for e in (41, 42, 43, 105, 106, 107)] == [want] * 6
    rejected = (37, 40, 44, 45, 61, 62, 63, 104, 108, 125)
    assert [_create(lib, e) for e in rejected] == [-1] * len(rejected)
    assert [_create(lib, e) for e in (16, 80)] == [want] * 2  # rate 1/2 as before


def test_new_surface_is_on_every_layer(lib):
    import ofdm_amd
    from ofdm_amd import api

    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ofdm_host.hpp")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in ofdm_amd.SIGNATURES
        assert re.search(r"\b(int|int32_t|int64_t) " + n + r"\(", hdr) and ("pub fn " + n + "(") in rs and (n + "(") in hpp, n
    for name, value in (("LDPC648_R23", 41), ("LDPC648_R34", 42), ("LDPC648_R56", 43)):
        assert re.search(r"\bOFDM_ECC_%s = %d\b" % (name, value), hdr) and "pub const OFDM_ECC_%s: i32 = %d;" % (name, value) in rs
        assert getattr(api, "ECC_" + name) == getattr(ofdm_amd, "ECC_" + name) == value
        assert api._with_fcs(value, True) == 64 + value
    assert api.LDPC_INFO_BYTES == rr.INFO_BYTES == tuple(lib.ofdm_ldpc648_info_bytes(r) for r in rr.RATES)
    import inspect
    assert inspect.signature(api.Context.ldpc_encode).parameters["rate"].default == 0
    assert inspect.signature(api.Context.ldpc_decode).parameters["rate"].default == 0
    assert "kernels_ldpc.hip" in ofdm_amd.build.SOURCES
    assert ofdm_amd.build.EXTRA_FLAGS["kernels_ldpc.hip"] == ["-fno-slp-vectorize"]
