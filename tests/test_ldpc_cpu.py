"""CPU checks of the LDPC(648,324) mode (OFDM_ECC_LDPC648 = 16, with the frame check 80): the table's properties, the three known
answers, the host encoder and decoder of the library held to tests/ldpc_ref.py bit for bit (iteration counts included) on the sets
tests/test_gpu_ldpc.py decodes on the device, every branch of the receive rule in the reference, and the boundary: the five new
exports on every layer, coded_len, and which ecc values ofdm_create takes.  No kernel is launched here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldpc_ref as lr  # noqa: E402
import ldpc_vectors as lv  # noqa: E402

NEW = ("ofdm_ldpc648_coded_len", "ofdm_ldpc648_encode", "ofdm_ldpc648_decode", "ofdm_ldpc648_encode_batch", "ofdm_ldpc648_decode_batch")
# info -> the 40 parity bytes, computed with a GF(2) inverse of the parity half (not with the back-substitution of the library)
KATS = ((bytes(range(40)), "08e71a7c4a39f145219fcb02d9c773209884af579f8dcbf7b55f6baaa04a9df0d8e5c0cd24c9a196"),
        (b"\xff" * 40, "3f0c7f00cf0322781e103f0c7f079e07c40fbbdf7dd8fd0e440f78df853ffc2efc21781ef0c0f380"),
        (b"\x00" * 39 + b"\x80", "200840802000030401182008c0004100060806304030800186000430042080210001040108200840"))


@pytest.fixture(scope="module")
def lib():
    from ofdm_amd import build

    lib = C.CDLL(build.build())
    i64, i32, vp = C.c_int64, C.c_int32, C.c_void_p
    lib.ofdm_ldpc648_coded_len.restype = i64
    lib.ofdm_ldpc648_coded_len.argtypes = [i64]
    lib.ofdm_ldpc648_encode.argtypes = [vp, i64, vp]
    lib.ofdm_ldpc648_decode.argtypes = [vp, i64, i32, vp, vp]
    lib.ofdm_ldpc648_encode_batch.argtypes = [vp, vp, i64, i64, i64, vp, i64]
    lib.ofdm_ldpc648_decode_batch.argtypes = [vp, vp, i64, i64, i64, i32, vp, i64, vp]
    return lib


def host_encode(lib, info):
    info = np.ascontiguousarray(info, np.uint8).reshape(-1, lr.INFO_BYTES)
    out = np.zeros((info.shape[0], lr.CODE_BYTES), np.uint8)
    assert lib.ofdm_ldpc648_encode(info.ctypes.data, info.shape[0], out.ctypes.data) == 0
    return out


def host_decode(lib, llr, max_iter):
    llr = np.ascontiguousarray(llr, np.int8).reshape(-1, lr.SENT_BITS)
    out = np.full((llr.shape[0], lr.INFO_BYTES), 0xA5, np.uint8)
    iters = np.full(llr.shape[0], -7, np.int32)
    assert lib.ofdm_ldpc648_decode(llr.ctypes.data, llr.shape[0], max_iter, out.ctypes.data, iters.ctypes.data) == 0
    return out, iters


# ------------------------------------------------------------------------------------------------ the code
def test_table_properties():
    assert lr.TABLE.shape == (12, 24) and int((lr.TABLE >= 0).sum()) == 88 and lr.TABLE.max() < lr.Z
    h = lr.parity_check_matrix()
    assert h.shape == (324, 648) and int(h.sum()) == 88 * 27
    assert lr.gf2_rank(h) == 324
    assert lr.gf2_rank(h[:, 324:]) == 324                     # the parity half is invertible: the parity of an info word is unique
    overlap = h.astype(np.int64) @ h.astype(np.int64).T       # two rows sharing two columns = a 4-cycle
    np.fill_diagonal(overlap, 0)
    assert overlap.max() <= 1
    deg = (lr.TABLE >= 0).sum(axis=0).tolist()
    assert deg == [12, 3, 3, 3, 12, 3, 3, 3, 12, 3, 3, 3, 3] + [2] * 11


def test_shared_header_states_the_same_table():
    txt = open(os.path.join(ROOT, "ofdm_amd", "csrc", "ldpc_table.h")).read()
    body = txt[txt.index("kLdpcShift[kLdpcRows][kLdpcCols] = {"):]
    body = body[body.index("{") + 1:body.index("};")]
    rows = re.findall(r"\{([^{}]*)\}", body)
    got = np.array([[int(v) for v in r.split(",")] for r in rows])
    np.testing.assert_array_equal(got, lr.TABLE)
    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    doc = hdr[hdr.index("LDPC(648,324) (north-star extension"):]
    lines = [ln.strip(" *").split() for ln in doc.splitlines()[1:40]]
    tab = [ln for ln in lines if len(ln) == 24 and all(re.fullmatch(r"-|\d+", t) for t in ln)]
    np.testing.assert_array_equal(np.array([[-1 if t == "-" else int(t) for t in ln] for ln in tab]), lr.TABLE)
    assert "unverified" in doc[:4000].lower() and "unverified" in txt.lower()


@pytest.mark.parametrize("info,parity", KATS)
def test_known_answers(lib, info, parity):
    a = np.frombuffer(info, np.uint8)
    want = info + bytes.fromhex(parity)
    assert lr.encode(a[None])[0].tobytes() == want
    assert host_encode(lib, a)[0].tobytes() == want


def test_random_info_encodes_to_codewords(lib):
    info = np.random.default_rng(5).integers(0, 256, (64, 40), dtype=np.uint8)
    x = lr.codeword_bits(info)
    h = lr.parity_check_matrix().astype(np.int64)
    assert not ((x.astype(np.int64) @ h.T) & 1).any()
    assert not x[:, 320:324].any()
    code = host_encode(lib, info)
    np.testing.assert_array_equal(code, lr.encode(info))
    np.testing.assert_array_equal(code[:, :40], info)                       # systematic
    sent = np.unpackbits(code, axis=1, bitorder="little")
    np.testing.assert_array_equal(sent, np.concatenate([x[:, :320], x[:, 324:644]], axis=1))


# ------------------------------------------------------------------------------------------------ the decoder
@pytest.mark.parametrize("max_iter", lv.MAX_ITERS)
@pytest.mark.parametrize("name", ("clean", "corner", "noisy"))
def test_host_decoder_is_the_reference(lib, name, max_iter):
    want, want_it = lv.reference(name, max_iter)
    got, got_it = host_decode(lib, lv.llr_set(name), max_iter)
    np.testing.assert_array_equal(got_it, want_it)
    np.testing.assert_array_equal(got, want)


def test_clean_and_corner_rows_decode_as_stated():
    info, _ = lv.clean()
    by, it = lv.reference("clean", 20)
    assert (it == 1).all() and (by == info).all()                            # noiseless +-32: the first iteration's checks hold
    by, it = lv.reference("corner", 20)
    assert it[0] == 1 and not by[0].any()                                    # all-zero LLRs: converges at iteration 1 to zeros
    assert it[1] == 1 and not by[1].any()                                    # all -128: the all-zero code word at full confidence
    assert it[2] == 0                                                        # all +127: the all-ones word is no code word


def test_noisy_set_has_both_classes_and_no_wrong_convergence():
    info, llr = lv.noisy()
    assert llr.shape[0] >= 400
    by, it = lv.reference("noisy", lr.MAX_ITER)
    bad = int((it == 0).sum())
    print(f"noisy set at {lv.NOISY_EBN0_DB} dB: {bad} of {it.size} unconverged at {lr.MAX_ITER} iterations, mean iterations of the rest "
          f"{it[it > 0].mean():.2f}")
    assert 0.10 * it.size <= bad <= 0.90 * it.size
    for max_iter in lv.MAX_ITERS:
        by, it = lv.reference("noisy", max_iter)
        conv = it > 0
        assert (by[conv] == info[conv]).all(), max_iter                      # no converged code word differs from what was sent
        assert ((it >= 0) & (it <= max_iter)).all()
        if max_iter >= 5:
            assert conv.any() and (~conv).any(), max_iter                    # both classes (no row of this set converges in ONE iteration)


def test_decode_argument_checks(lib):
    llr = np.zeros(640, np.int8)
    out = np.zeros(40, np.uint8)
    for bad in (0, -1, 65):
        assert lib.ofdm_ldpc648_decode(llr.ctypes.data, 1, bad, out.ctypes.data, None) == -1
    assert lib.ofdm_ldpc648_decode(llr.ctypes.data, -1, 20, out.ctypes.data, None) == -1
    assert lib.ofdm_ldpc648_decode(None, 1, 20, out.ctypes.data, None) == -1
    assert lib.ofdm_ldpc648_decode(None, 0, 20, None, None) == 0
    assert lib.ofdm_ldpc648_decode(llr.ctypes.data, 1, 64, out.ctypes.data, None) == 0      # iters is optional
    assert lib.ofdm_ldpc648_encode(None, 0, None) == 0 and lib.ofdm_ldpc648_encode(None, 1, out.ctypes.data) == -1
    # the batch calls check their arguments before they need a device
    for fn, args in ((lib.ofdm_ldpc648_encode_batch, (None, None, 1, 40, 1, None, 80)),
                     (lib.ofdm_ldpc648_decode_batch, (None, None, 1, 640, 1, 20, None, 40, None))):
        assert fn(*args) == -1


# ------------------------------------------------------------------------------------------------ the frame stream
def _llrs_of(stream_bytes, amp=40):
    bits = np.unpackbits(np.asarray(stream_bytes, np.uint8), bitorder="little").astype(np.int64)
    return (amp * (2 * bits - 1)).astype(np.int8)


def test_stream_build(lib):
    for p in (0, 1, 31, 32, 33, 72, 73, 560):
        pay = bytes(np.random.default_rng(p).integers(0, 256, p, dtype=np.uint8))
        info = lr.info_stream(pay)
        B = -(-(p + 8) // 40)
        assert info.size == 40 * B == 40 * lr.codewords(p)
        assert info[:4].tobytes() == p.to_bytes(4, "little") and info[4:8].tobytes() == (p ^ 0xFFFFFFFF).to_bytes(4, "little")
        assert info[8:8 + p].tobytes() == pay and not info[8 + p:].any()
        s = lr.stream(pay)
        assert s.size == lr.coded_len(p) == 80 * B == lib.ofdm_ldpc648_coded_len(p)
        np.testing.assert_array_equal(s.reshape(B, 80), host_encode(lib, info))


def test_receive_rule_every_branch():
    rng = np.random.default_rng(11)
    pay = bytes(rng.integers(0, 256, 100, dtype=np.uint8))          # 3 code words
    s = lr.stream(pay)
    llr = _llrs_of(s)
    assert lr.receive(llr, 240) == (0, pay)                          # whole
    assert lr.receive(llr, 240 + 79) == (0, pay)                     # a started 80 bytes behind it do not count
    assert lr.receive(llr, 239) == (0, pay[:72])                     # cut: the prefix of the two whole code words
    assert lr.receive(llr, 80) == (0, pay[:32])
    for body in (79, 0, -16):
        assert lr.receive(llr, body) == (lr.HEADER_STATUS, b"")      # no whole code word
    junk = rng.integers(-128, 128, 640, dtype=np.int8)
    assert lr.decode(junk)[1][0] == 0
    bad0 = llr.copy(); bad0[:640] = junk
    assert lr.receive(bad0, 240) == (lr.HEADER_STATUS, b"")          # code word 0 does not converge
    bad2 = llr.copy(); bad2[1280:1920] = junk
    assert lr.receive(bad2, 240) == (lr.UNCORRECTABLE_STATUS, b"")   # a later one does not
    assert lr.receive(bad2, 160) == (0, pay[:72])                    # ... but lies behind the cut
    # a valid code word whose length words are not complementary
    info = lr.info_stream(pay).copy(); info[5] ^= 0x10
    forged = _llrs_of(lr.encode(info.reshape(-1, 40)).reshape(-1))
    assert lr.receive(forged, 240) == (lr.HEADER_STATUS, b"")
    # p claiming more code words than the frame holds, 0xFFFFFFFF included (64-bit arithmetic)
    for p in (1000, 0xFFFFFFFF):
        info = lr.info_stream(pay).copy()
        info[:4] = np.frombuffer(p.to_bytes(4, "little"), np.uint8)
        info[4:8] = np.frombuffer((p ^ 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)
        forged = _llrs_of(lr.encode(info.reshape(-1, 40)).reshape(-1))
        st, out = lr.receive(forged, 240)
        assert st == 0 and out == info[8:].tobytes() and len(out) == 112
    # p smaller than the stream: only its code words are decoded, junk behind them is not looked at
    info = lr.info_stream(pay).copy()
    info[:4] = np.frombuffer((20).to_bytes(4, "little"), np.uint8)
    info[4:8] = np.frombuffer((20 ^ 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)
    forged = _llrs_of(lr.encode(info.reshape(-1, 40)).reshape(-1)); forged[640:] = np.resize(junk, forged.size - 640)
    assert lr.receive(forged, 240) == (0, pay[:20])
    assert [lr.row_bytes(b) for b in (0, 79, 80, 159, 160, 1000)] == [0, 0, 32, 32, 72, 472]


# ------------------------------------------------------------------------------------------------ the boundary
def test_coded_len(lib):
    assert [lib.ofdm_ldpc648_coded_len(p) for p in (0, 31, 32, 33, 560, 1304)] == [80, 80, 80, 160, 1200, 2640]
    assert [lr.coded_len(p) for p in (0, 31, 32, 33, 560, 1304)] == [80, 80, 80, 160, 1200, 2640]
    assert lib.ofdm_ldpc648_coded_len(-1) == -1


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


def test_create_accepts_the_ldpc_modes_and_nothing_around_them(lib):
    import torch

    want = 0 if torch.cuda.is_available() else -3          # OFDM_ERR_NO_DEVICE without a GPU, never INVALID
    assert [_create(lib, e) for e in (16, 80)] == [want] * 2
    rejected = (13, 14, 15, 17, 18, 19, 33, 36, 40, 79, 81)
    assert [_create(lib, e) for e in rejected] == [-1] * len(rejected)


def test_new_surface_is_on_every_layer(lib):
    import ofdm_amd
    from ofdm_amd import api

    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ofdm_host.hpp")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in ofdm_amd.SIGNATURES
        assert re.search(r"\b(int|int64_t) " + n + r"\(", hdr) and ("pub fn " + n + "(") in rs and (n + "(") in hpp
    assert hasattr(api.Context, "ldpc_encode") and hasattr(api.Context, "ldpc_decode")
    assert re.search(r"\bOFDM_ECC_LDPC648 = 16\b", hdr) and "pub const OFDM_ECC_LDPC648: i32 = 16;" in rs
    assert re.search(r"#define OFDM_LDPC_MAX_ITER 20\b", hdr) and "pub const OFDM_LDPC_MAX_ITER: i32 = 20;" in rs
    assert api.ECC_LDPC648 == ofdm_amd.ECC_LDPC648 == 16 and api.LDPC_MAX_ITER == lr.MAX_ITER == 20
    assert api._with_fcs(api.ECC_LDPC648, True) == 80
    assert "kernels_ldpc.hip" in ofdm_amd.build.SOURCES and ofdm_amd.build.EXTRA_FLAGS["kernels_ldpc.hip"] == ["-fno-slp-vectorize"]
