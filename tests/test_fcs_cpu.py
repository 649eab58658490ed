"""CPU-only checks of the CRC-32 frame check (ecc = OFDM_ECC_FCS + mode): the exported host CRC against zlib, the reference rule of
tests/fcs_ref.py against the facts include/ofdm_hip.h states about it, ofdm_create's acceptance of the new ecc values, and the
presence of the new surface on every layer of the boundary.  No kernel is launched here."""
import ctypes as C
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fcs_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofdm_fcs_wrap_batch", "ofdm_fcs_check_batch")
CONSTANTS = (("ECC_FCS", 64), ("FRAME_FCS", -6))


@pytest.fixture(scope="module")
def lib():
    from ofdm_amd import build

    lib = C.CDLL(build.build())
    lib.ofdm_crc32.restype = C.c_uint32
    lib.ofdm_crc32.argtypes = [C.c_void_p, C.c_int64]
    return lib


# ---------------------------------------------------------------------------------------------------------- ofdm_crc32
def test_crc32_is_zlib(lib):
    rng = np.random.default_rng(32)
    for n in list(range(71)) + [255, 568, 1312, 70001]:
        for odd in (0, 1, 3):                                   # the base address: aligned, and odd
            buf = rng.integers(0, 256, n + 8, dtype=np.uint8)
            view = buf[odd:odd + n]
            assert lib.ofdm_crc32(view.ctypes.data, n) == (zlib.crc32(bytes(view)) & 0xFFFFFFFF), (n, odd)
    kat = np.frombuffer(b"123456789", np.uint8).copy()
    assert lib.ofdm_crc32(kat.ctypes.data, 9) == 0xCBF43926
    zero4 = np.zeros(4, np.uint8)
    assert lib.ofdm_crc32(zero4.ctypes.data, 4) == 0x2144DF1C
    assert lib.ofdm_crc32(None, 9) == 0 and lib.ofdm_crc32(None, 0) == 0
    assert lib.ofdm_crc32(kat.ctypes.data, -1) == 0
    assert lib.ofdm_crc32(kat.ctypes.data, 0) == 0               # zlib.crc32(b"") == 0


def test_python_crc32_wrapper():
    from ofdm_amd import api

    for msg in (b"", b"a", b"123456789", bytes(range(256)) * 3):
        assert api.crc32(msg) == (zlib.crc32(msg) & 0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------- the rule
def test_reference_round_trip_and_padding():
    rng = np.random.default_rng(7)
    for p in (0, 1, 2, 3, 4, 5, 31, 32, 223, 560):
        pay = bytes(rng.integers(0, 256, p, dtype=np.uint8))
        env = fcs_ref.wrap(pay)
        assert len(env) == p + fcs_ref.OVERHEAD
        assert struct.unpack_from("<I", env, 0)[0] == p and env[4:4 + p] == pay
        assert fcs_ref.check(env) == pay
        for pad in (bytes(3), bytes(223), bytes(rng.integers(0, 256, 3, dtype=np.uint8)), bytes(rng.integers(0, 256, 223, dtype=np.uint8))):
            assert fcs_ref.check(env + pad) == pay                # bytes behind 8 + p are not looked at


def test_reference_rejects_every_single_bit_change():
    rng = np.random.default_rng(8)
    env = fcs_ref.wrap(bytes(rng.integers(0, 256, 32, dtype=np.uint8)))
    assert len(env) == 40
    row = env + bytes(700)
    assert fcs_ref.check(row) == env[4:36]
    for bit in range(320):                                        # the bits of the length word included
        bad = bytearray(row)
        bad[bit >> 3] ^= 1 << (bit & 7)
        assert fcs_ref.check(bytes(bad)) is None, bit


def test_reference_rejects_zero_short_and_forged_rows():
    assert fcs_ref.check(bytes(708)) is None                      # crc32 of four zero bytes is 0x2144DF1C, not 0
    assert zlib.crc32(bytes(4)) == 0x2144DF1C
    for L in range(8):
        assert fcs_ref.check(bytes(L)) is None and fcs_ref.check(fcs_ref.wrap(b"")[:L]) is None
    assert fcs_ref.check(fcs_ref.wrap(b"")) == b""
    rng = np.random.default_rng(9)
    L = 64
    body = bytes(rng.integers(0, 256, L, dtype=np.uint8))

    def forged(p, fix_crc):
        row = bytearray(struct.pack("<I", p) + body[4:])
        if fix_crc and 8 + p <= L:
            struct.pack_into("<I", row, 4 + p, zlib.crc32(bytes(row[:4 + p])) & 0xFFFFFFFF)
        return bytes(row)

    assert fcs_ref.check(forged(L - 8, True)) == body[4:L - 4]    # p = L - 8 with a matching check: the boundary case
    assert fcs_ref.check(forged(L - 8, False)) is None
    for p in (L - 7, 2 ** 31, 0xFFFFFFFF):
        assert fcs_ref.check(forged(p, True)) is None, p


# ---------------------------------------------------------------------------------------------------------- ofdm_create
def _create(lib, ecc):
    from ofdm_amd import Params

    p = Params()
    assert lib.ofdm_default_params(C.byref(p)) == 0
    p.ecc = ecc
    h = C.c_void_p()
    rc = lib.ofdm_create(C.byref(p), None, None, 0, None, C.byref(h))
    if rc == 0:
        lib.ofdm_destroy.argtypes = [C.c_void_p]
        lib.ofdm_destroy(h)
    return rc


def test_create_accepts_every_fcs_value_and_no_other(lib):
    base = _create(lib, 0)
    assert base in (0, -3)                                        # -3: no GPU here
    for m in fcs_ref.BASE_MODES:
        assert _create(lib, m) == base, m
        assert _create(lib, fcs_ref.ECC_FCS + m) == base, m
    assert sorted(fcs_ref.ECC_FCS + m for m in fcs_ref.BASE_MODES) == [64, 65, 66, 69, 74, 75, 76, 80, 84, 94, 95, 96, 105, 106, 107]
    for bad in (63, 67, 68, 70, 77, 85, 93, 97, 128, 64 + 64):
        assert _create(lib, bad) == -1, bad
    for bad in (3, 4, 6, 7, 8, 9, 13, 14, 21, 29, 33, 40, 99, 100, -1):   # what was rejected stays rejected
        assert _create(lib, bad) == -1, bad


# ---------------------------------------------------------------------------------------------------------- the boundary
def test_new_surface_is_on_every_layer(lib):
    import ofdm_amd
    from ofdm_amd import api

    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ofdm_host.hpp")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in ofdm_amd.SIGNATURES
        assert re.search(r"\bint " + n + r"\(", hdr) and ("pub fn " + n + "(") in rs and (n + "(") in hpp
    assert hasattr(lib, "ofdm_crc32") and "ofdm_crc32" in ofdm_amd.SIGNATURES
    assert re.search(r"\buint32_t ofdm_crc32\(", hdr) and "pub fn ofdm_crc32(" in rs and "ofdm_crc32(" in hpp
    assert hasattr(api.Context, "fcs_wrap") and hasattr(api.Context, "fcs_check") and callable(api.crc32) and callable(ofdm_amd.crc32)
    for f in (api.encode, api.decode, api.decode_long):
        assert "fcs" in f.__code__.co_varnames[:f.__code__.co_argcount + f.__code__.co_kwonlyargcount], f.__name__
    for name, value in CONSTANTS:
        assert re.search(r"\bOFDM_%s = %d\b" % (name, value), hdr), name
        assert ("pub const OFDM_%s: i32 = %d;" % (name, value)) in rs, name
        assert getattr(api, name) == value and getattr(ofdm_amd, name) == value
        assert ("OFDM_" + name) in hpp, name
    assert re.search(r"#define OFDM_FCS_OVERHEAD 8\b", hdr) and "pub const OFDM_FCS_OVERHEAD: i64 = 8;" in rs and api.FCS_OVERHEAD == 8
    assert "frame check sequence" in hdr and "0xEDB88320" in hdr and "0xCBF43926" in hdr
    # what the earlier modes pinned stays
    assert re.search(r"3 and 4 are\s+REJECTED", hdr) and "punctured rates and framed modes" in hdr
    assert "spoils the frame's WHOLE estimate" in hdr
    assert re.search(r"int32_t reserved\[4\];", hdr) and "pub reserved: [i32; 4]," in rs
    assert "33 upwards are rejected" not in hdr                   # 64 + mode is a mode now
    assert "--fcs" in open(os.path.join(ROOT, "tools", "ofdm_loopback.cpp")).read()
    assert "kernels_fcs.hip" in open(os.path.join(ROOT, "ofdm_amd", "build.py")).read()
    assert lib.ofdm_abi_version() == 1


def test_entry_points_reject_a_null_context(lib):
    assert lib.ofdm_fcs_wrap_batch(None, None, 1, 4, None, 4, None, 12, None) == -1
    assert lib.ofdm_fcs_check_batch(None, None, 1, 12, None, 12, None, 4, None, None) == -1
    assert lib.ofdm_fcs_wrap_batch(None, None, 0, 0, None, 0, None, 8, None) == -1
    assert lib.ofdm_fcs_check_batch(None, None, 0, 0, None, 0, None, 0, None, None) == -1
