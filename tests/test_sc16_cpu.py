"""EXT-9 without a GPU: the host functions ofdm_sc16_widen / ofdm_sc16_narrow against tests/sc16_ref.py bit for bit, the argument
checks every sc16 entry point makes before it touches a device, and the surface on every layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sc16_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [1.0 / 32768.0, 1.0, 3.0517578e-5, 3.1e-5, 1e-3]   # 3.0517578e-5 rounds to 2^-15 in f32; 3.1e-5 and 1e-3 are no powers of two
EDGES = [-32768, -32767, -1, 0, 1, 32767]
NEW = ["ofdm_sc16_widen", "ofdm_sc16_narrow", "ofdm_sc16_widen_batch", "ofdm_sc16_narrow_batch", "ofdm_rx_demod_sc16_batch",
       "ofdm_rx_decode_sc16_batch", "ofdm_rx_demod_sc16_host", "ofdm_rx_decode_sc16_host"]


@pytest.fixture(scope="module")
def lib(ofdm):
    return ofdm.load()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _widen(lib, q, scale):
    out = np.full(q.shape[:-1], np.nan, np.complex64)
    assert lib.ofdm_sc16_widen(q.ctypes.data, out.size, scale, out.ctypes.data) == 0
    return out


def _narrow(lib, z, scale):
    out = np.full(z.shape + (2,), 12345, np.int16)
    clipped = C.c_int64(-1)
    assert lib.ofdm_sc16_narrow(z.ctypes.data, z.size, scale, out.ctypes.data, C.byref(clipped)) == 0
    return out, clipped.value


@pytest.mark.parametrize("scale", SCALES)
def test_host_widen_is_numpy_bit_for_bit(lib, scale):
    rng = np.random.default_rng(16)
    comp = np.concatenate([rng.integers(-32768, 32768, 4096 - len(EDGES), dtype=np.int16), np.array(EDGES, np.int16)])
    q = np.ascontiguousarray(comp.reshape(-1, 2))
    got = _widen(lib, q, scale)
    want = sc16_ref.widen(q, scale)
    np.testing.assert_array_equal(_bits(got.view(np.float32)), _bits(want.view(np.float32)))
    np.testing.assert_array_equal(_bits(got.view(np.float32)), _bits(q.astype(np.float32) * np.float32(scale)).reshape(-1))


def test_host_narrow_is_the_definition(lib):
    inf, nan = np.inf, np.nan
    comp = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 32767.4, -32767.4, 32767.5, -32767.5, 32768.0, -32768.0, 1e9, -1e9, inf, -inf, nan, 0.0,
            32767.0, -32767.0]
    z = np.array(comp, np.float32).view(np.complex64).copy()
    got, clipped = _narrow(lib, z, 1.0)
    want, want_clipped = sc16_ref.narrow(z, 1.0)
    np.testing.assert_array_equal(got, want)
    # ties to even; 32767.4 is in range; 32767.5 rounds to 32768: clipped; -32768 is never produced; NaN gives 0 and counts
    assert got.reshape(-1).tolist() == [0, 0, 2, -2, 2, -2, 32767, -32767, 32767, -32767, 32767, -32767, 32767, -32767, 32767, -32767, 0, 0,
                                        32767, -32767]
    assert clipped == want_clipped == 9
    # a scale that is no power of two, on a seeded row: the single rounded product decides the ties
    rng = np.random.default_rng(17)
    z = (rng.standard_normal(2048) + 1j * rng.standard_normal(2048)).astype(np.complex64)
    for scale in (12000.0, 30000.0 / 3.1):
        got, clipped = _narrow(lib, z, scale)
        want, want_clipped = sc16_ref.narrow(z, scale)
        np.testing.assert_array_equal(got, want)
        assert clipped == want_clipped and got.min() >= -32767
    assert sc16_ref.narrow(z, 30000.0 / 3.1)[1] > 0       # the second scale does clip: the count is exercised
    out = np.zeros((1, 2), np.int16)
    assert lib.ofdm_sc16_narrow(z.ctypes.data, 1, 1.0, out.ctypes.data, None) == 0   # clipped is optional


def test_narrow_inverts_widen_for_every_int16_but_the_lowest(lib):
    v = np.arange(-32767, 32768, dtype=np.int16)
    q = np.ascontiguousarray(np.stack([v, v[::-1]], axis=-1))
    back, clipped = _narrow(lib, _widen(lib, q, 2.0 ** -15), 2.0 ** 15)
    np.testing.assert_array_equal(back, q)
    assert clipped == 0
    low = np.array([[-32768, -32768]], np.int16)
    back, clipped = _narrow(lib, _widen(lib, low, 2.0 ** -15), 2.0 ** 15)
    assert back.tolist() == [[-32767, -32767]] and clipped == 2


@pytest.mark.parametrize("scale", [0.0, -1.0, np.inf, np.nan])
def test_bad_scale_is_refused_on_the_host(lib, scale):
    q = np.zeros((4, 2), np.int16)
    z = np.zeros(4, np.complex64)
    assert lib.ofdm_sc16_widen(q.ctypes.data, 4, scale, z.ctypes.data) == -1
    assert lib.ofdm_sc16_narrow(z.ctypes.data, 4, scale, q.ctypes.data, None) == -1
    assert lib.ofdm_sc16_widen(None, 4, 1.0, z.ctypes.data) == -1 and lib.ofdm_sc16_widen(q.ctypes.data, -1, 1.0, z.ctypes.data) == -1
    assert lib.ofdm_sc16_widen(None, 0, 1.0, None) == 0


def test_null_context_is_invalid_on_every_device_entry_point(lib):
    s = 1.0 / 32768.0
    assert lib.ofdm_sc16_widen_batch(None, None, 1, 8, 8, s, None, 8) == -1
    assert lib.ofdm_sc16_narrow_batch(None, None, 1, 8, 8, s, None, 8, None) == -1
    assert lib.ofdm_rx_demod_sc16_batch(None, None, 1, 640, 640, s, 0, 8, None, None, None, 0, None, 48, None) == -1
    assert lib.ofdm_rx_decode_sc16_batch(None, None, 1, 2000, 2000, s, 0, 8, None, 64, None, None, None, None, None) == -1
    assert lib.ofdm_rx_demod_sc16_host(None, None, 1, 640, 640, s, 0, 8, None, 48, 0) == -1
    assert lib.ofdm_rx_decode_sc16_host(None, None, 1, 2000, 2000, s, 0, 8, None, 64, None, None, None, None, None, 0) == -1


def test_the_surface_is_on_every_layer(ofdm):
    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ofdm_host.hpp")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in ofdm.SIGNATURES, n
        assert re.search(r"pub fn %s\s*\(" % n, rs), n
    assert "typedef struct { int16_t re, im; } ofdm_sc16;" in hdr and "#define OFDM_SC16_DEFAULT_SCALE (1.0f / 32768.0f)" in hdr
    assert "pub struct ofdm_sc16 { pub re: i16, pub im: i16 }" in rs and "pub const OFDM_SC16_DEFAULT_SCALE: f32 = 1.0 / 32768.0;" in rs
    for n in ("ofdm_rx_decode_sc16_host", "ofdm_rx_demod_sc16_host", "ofdm_sc16_widen", "ofdm_sc16_narrow"):
        assert n in hpp, n
    from ofdm_amd import api, build

    assert api.SC16_DEFAULT_SCALE == 1.0 / 32768.0 == float(sc16_ref.DEFAULT_SCALE) and ofdm.SC16_DEFAULT_SCALE == api.SC16_DEFAULT_SCALE
    for m in ("sc16_widen", "sc16_narrow", "rx_demod_sc16", "decode_batch_sc16", "demod_host_sc16", "decode_host_sc16"):
        assert callable(getattr(api.Context, m)), m
    assert callable(api.sc16_widen) and callable(api.sc16_narrow) and ofdm.sc16_widen is api.sc16_widen
    assert "kernels_sc16.hip" in build.SOURCES and "kernels_n64_sc16.hip" in build.SOURCES
    assert "--sc16" in open(os.path.join(ROOT, "tools", "ofdm_loopback.cpp")).read()


def test_module_level_functions_are_the_host_functions():
    from ofdm_amd import api

    rng = np.random.default_rng(18)
    q = rng.integers(-32768, 32768, (3, 50, 2), dtype=np.int16)
    z = api.sc16_widen(q, 3.1e-5)
    assert z.shape == (3, 50) and z.dtype == np.complex64
    np.testing.assert_array_equal(_bits(z.view(np.float32)), _bits(sc16_ref.widen(q, 3.1e-5).view(np.float32)))
    back, clipped = api.sc16_narrow(z, 1.0 / 3.1e-5)
    want, want_clipped = sc16_ref.narrow(z, 1.0 / 3.1e-5)
    np.testing.assert_array_equal(back, want)
    assert clipped == want_clipped
    with pytest.raises(api.OfdmError):
        api.sc16_widen(np.zeros((4, 2), np.int32))
