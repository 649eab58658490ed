"""CPU checks of the batched Reed-Solomon(255,223) surface and the RS-outer frame modes (OFDM_ECC_RS255 = 20 + inner): the boundary
accepts the four new ecc values and nothing around them, the two stage entry points and the five new constants are declared on
every layer, and the host decoder -- the definition k_rs255_decode is held to -- agrees with the oracle's
decipher_transmission_bytes on the very vectors tests/test_gpu_rs.py decodes on the device, 17-error and random blocks included.
No kernel is launched here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rs_vectors as rv  # noqa: E402

NEW = ("ofdm_rs255_encode_batch", "ofdm_rs255_decode_batch")
CONSTANTS = (("ECC_RS255", 20), ("ECC_RS255_K7F_R12", 30), ("ECC_RS255_K7F_R23", 31), ("ECC_RS255_K7F_R34", 32),
             ("FRAME_UNCORRECTABLE", -5))


@pytest.fixture(scope="module")
def lib():
    from ofdm_amd import build

    lib = C.CDLL(build.build())
    i64, vp = C.c_int64, C.c_void_p
    lib.ofdm_rs255_encode_batch.argtypes = [vp, vp, i64, i64, vp, i64, vp, i64]
    lib.ofdm_rs255_decode_batch.argtypes = [vp, vp, i64, i64, vp, i64, vp, i64, vp, vp]
    lib.ofdm_rs255_encode.argtypes = [vp, i64, vp]
    lib.ofdm_rs255_decode.argtypes = [vp, i64, vp, vp]
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


def test_create_accepts_the_rs_modes_and_nothing_around_them(lib):
    import torch

    want = 0 if torch.cuda.is_available() else -3          # OFDM_ERR_NO_DEVICE without a GPU, never INVALID
    assert [_create(lib, e) for e in (20, 30, 31, 32)] == [want] * 4
    rejected = list(range(21, 30)) + [33, 40]
    assert [_create(lib, e) for e in rejected] == [-1] * len(rejected)


def test_new_surface_is_on_every_layer(lib):
    import ofdm_amd
    from ofdm_amd import api

    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ofdm_host.hpp")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in ofdm_amd.SIGNATURES
        assert re.search(r"\bint " + n + r"\(", hdr) and ("pub fn " + n + "(") in rs and (n + "(") in hpp
    assert hasattr(api.Context, "rs255_encode") and hasattr(api.Context, "rs255_decode")
    for name, value in CONSTANTS:
        assert re.search(r"\bOFDM_%s = %d\b" % (name, value), hdr), name
        assert ("pub const OFDM_%s: i32 = %d;" % (name, value)) in rs, name
        assert getattr(api, name) == value and getattr(ofdm_amd, name) == value
        assert ("OFDM_" + name) in hpp, name
    # what the earlier modes pinned stays
    assert re.search(r"3 and 4 are\s+REJECTED", hdr) and "punctured rates and framed modes" in hdr
    assert lib.ofdm_abi_version() == 1


def test_entry_points_reject_a_null_context(lib):
    assert lib.ofdm_rs255_encode_batch(None, None, 1, 4, None, 4, None, 255) == -1
    assert lib.ofdm_rs255_decode_batch(None, None, 1, 255, None, 255, None, 446, None, None) == -1
    assert lib.ofdm_rs255_encode_batch(None, None, 0, 0, None, 0, None, 255) == -1
    assert lib.ofdm_rs255_decode_batch(None, None, 0, 0, None, 0, None, 223, None, None) == -1


@pytest.mark.parametrize("n_code", rv.N_CODES)
def test_host_decoder_is_the_oracle_on_the_gpu_vectors(lib, orc, n_code):
    rows = rv.decoder_rows(lib, n_code)
    kinds = set()
    for lens in (None, rv.row_lengths(n_code)):
        for r in range(rv.ROWS):
            length = n_code if lens is None else rv.clamp(lens[r], n_code)
            data, out_len, fixed = rv.host_row(lib, rows[r], length)
            assert out_len == 223 * (length // 255 + 1) == len(data)
            want = orc.decipher_transmission_bytes(bytes(rows[r, :length]))
            # the whole-row host call and the oracle say the same: None <=> OFDM_ERR_UNCORRECTABLE <=> a block the reference fails
            code = np.ascontiguousarray(rows[r, :length])
            out = np.zeros(out_len, np.uint8)
            total = C.c_int32(-7)
            rc = lib.ofdm_rs255_decode(C.c_void_p(code.ctypes.data) if length else None, length, C.c_void_p(out.ctypes.data), C.byref(total))
            if want is None:
                assert rc == -6 and fixed == -1, (n_code, r, length)
                kinds.add("bad")
            else:
                assert rc == 0 and fixed == total.value >= 0, (n_code, r, length)
                assert bytes(out) == want == data, (n_code, r, length)
                kinds.add("fixed" if fixed else "clean")
    if n_code >= 255:
        assert kinds == {"bad", "fixed", "clean"}, (n_code, kinds)     # the vectors reach every outcome


def test_vectors_carry_the_cases_they_name(lib):
    rows = rv.decoder_rows(lib, 765)                                   # three whole blocks a row: every kind
    seen = {}
    for r in range(rv.ROWS):
        for b in range(3):
            seen[rv.KINDS[(r + rv.ROWS * b) % len(rv.KINDS)]] = rv.host_block(lib, rows[r, b * 255:(b + 1) * 255])[1]
    assert set(seen) == set(rv.KINDS)
    assert (seen["clean"], seen["e1"], seen["e2"], seen["e15"], seen["e16"], seen["forced"], seen["parity"], seen["zero"]) == \
        (0, 1, 2, 15, 16, 4, 5, 0)
    assert seen["e17"] == -1 and seen["random"] == -1                  # (a miscorrection has probability ~1e-14 per block)


def test_python_row_sizing_uses_the_library_s_step_count(lib):
    """Context.decode_row_bytes sizes RS-mode rows with api.conv_max_steps: it must be the inverse of ofdm_conv_k7_kept_bits, as the
    library's own conv_max_steps is"""
    from ofdm_amd import api

    lib.ofdm_conv_k7_kept_bits.restype = C.c_int64
    lib.ofdm_conv_k7_kept_bits.argtypes = [C.c_int64, C.c_int32]
    for rate in (api.CONV_RATE_1_2, api.CONV_RATE_2_3, api.CONV_RATE_3_4):
        for bits in list(range(0, 400)) + [8 * (1064 - 18), 8 * (9000 - 18) + 3]:
            T = api.conv_max_steps(bits, rate)
            assert lib.ofdm_conv_k7_kept_bits(T, rate) <= bits < lib.ofdm_conv_k7_kept_bits(T + 1, rate), (rate, bits, T)
