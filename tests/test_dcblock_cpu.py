"""The DC blocker (EXT-15, include/ofdm_hip.h "a DC blocker in front of detection") without a GPU.

  1. the host functions ofdm_dc_block / ofdm_dc_block_sc16 equal the numpy definition (tests/dcblock_ref.py) bit for bit, on an input on
     which another summation order gives other bits; the stateful mirror of the handle equals the one-shot rule however it is cut;
  2. the properties: a constant leaves exactly 0 from block 1 on, a NaN spoils the M blocks behind its own block and nothing else;
  3. every error code, and the surface in every layer;
  4. the reason to exist, on the f64 oracle alone (tests/dcblock_cases.py): unfiltered, a DC term fires the detector inside the noise lead
     and the frame behind it is lost; filtered with the default window every frame is timed on the sample of the DC-free capture and its
     hard-bit errors stay within e_0 + max(0.02 e_0, 8) of the DC-free capture of the same noise; noise plus DC alone detects unfiltered
     and not filtered; the band of windows that lock is mapped and printed (holds the table), the default is in it.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dcblock_cases as K
import dcblock_ref as D
import sc16_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofdm_dc_block_default", "ofdm_dc_block", "ofdm_dc_block_sc16", "ofdm_dcblock_create", "ofdm_dcblock_destroy", "ofdm_dcblock_reset",
       "ofdm_dcblock_push", "ofdm_dcblock_push_sc16", "ofdm_dcblock_state", "ofdm_stream_set_dc_block", "ofdm_stream_get_dc_block")
MS = (1, 4, 60, 1024)


def sizes(M):
    return (0, 1, 63, 64, 65, 127, 128, 64 * (M + 3) + 17)


def bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


wide = K.wide


@pytest.fixture(scope="module")
def api():
    from ofdm_amd import api as _api

    return _api


# ---------------------------------------------------------------------------------------------------------- 1: the definition
def test_the_wide_input_tells_summation_orders_apart():
    x = wide(64 * 40, 7)
    mag = np.abs(x[x != 0])
    assert mag.max() / mag.min() > 2.0 ** 70
    tree = D.block_sums(x)
    parts = x.view(np.float32).reshape(-1, 64, 2).astype(np.float64)
    plain = parts.sum(axis=1)                                             # numpy's own order
    serial = np.zeros_like(tree)
    for i in range(64):                                                   # left to right
        serial += parts[:, i]
    for other in (plain, serial):
        assert (tree.view(np.int64) != other.view(np.int64)).any()
        # ... and the difference reaches the f32 output: a filter that sums in that order is told apart from the definition
        assert (D.means(other[:-1], 1, len(other), 4).view(np.int32) != D.means(tree[:-1], 1, len(tree), 4).view(np.int32)).any()


@pytest.mark.parametrize("M", MS)
def test_host_functions_are_the_numpy_definition(api, M):
    for n in sizes(M):
        x = wide(n, 100 + n % 97)
        ref = D.dc_block(x, M)
        assert np.array_equal(bits(api.dc_block_host(x, M)), bits(ref)), (M, n)
        q, scale = np.random.default_rng(n + M).integers(-32768, 32768, (n, 2)).astype(np.int16), 0.7 / 32768
        xw = D.widen(q, scale)
        assert np.array_equal(bits(xw), bits(sc16_ref.widen(q, scale)))
        assert np.array_equal(bits(api.dc_block_host(q, M, scale=scale)), bits(D.dc_block(xw, M))), (M, n)
        assert np.array_equal(bits(api.dc_block_host(q, M, scale=scale)), bits(api.dc_block_host(xw, M))), (M, n)


@pytest.mark.parametrize("M", MS)
def test_the_handle_mirror_is_the_one_shot_rule_however_it_is_cut(M):
    n = 64 * (M + 3) + 17
    x = wide(n, 11 + M)
    ref = bits(D.dc_block(x, M))
    rng = np.random.default_rng(M)
    cuts = {"63": [63] * (n // 63) + [n % 63], "64": [64] * (n // 64) + [n % 64], "65": [65] * (n // 65) + [n % 65],
            "997": [997] * (n // 997) + [n % 997], "random": []}
    if n <= 64 * 63 + 17:
        cuts["1"] = [1] * n
    else:                                           # single samples across the first block boundaries, the rest in one piece
        cuts["1"] = [1] * 200 + [n - 200]
    left = n
    while left:
        m = int(min(rng.integers(0, 300), left))
        cuts["random"].append(m)
        left -= m
    for what, parts in cuts.items():
        h, at, got = D.Handle(M), 0, []
        for m in parts:
            got.append(h.push(x[at: at + m]))
            at += m
        assert at == n and h.total == n and len(h.sums) <= M and len(h.open) == n % 64
        assert np.array_equal(bits(np.concatenate(got)), ref), (M, what)
        h.reset()
        assert np.array_equal(bits(h.push(x[:200])), bits(D.dc_block(x[:200], M)))       # a reset starts a new stream at 0


# ---------------------------------------------------------------------------------------------------------- 2: properties
@pytest.mark.parametrize("M", MS)
def test_a_constant_leaves_exactly_zero_and_a_nan_spoils_m_blocks(api, M):
    n = 64 * (M + 3) + 17
    x = np.full(n, np.complex64(0.375 - 1.25j))
    for y in (api.dc_block_host(x, M), D.dc_block(x, M)):
        assert np.array_equal(bits(y[:64]), bits(x[:64])) and not bits(y[64:]).any()         # +0.0 in both parts
    x = wide(n, 3)
    at = 64 + 5                                                                              # a NaN in block 1
    x[at] = np.complex64(complex(np.nan, 1.0))
    y, ref = api.dc_block_host(x, M), D.dc_block(x, M)
    clean = D.dc_block(np.where(np.arange(n) == at, np.complex64(1j), x), M)
    spoiled = np.zeros(n, bool)
    spoiled[at] = True
    spoiled[128: 128 + 64 * M] = True                                                        # blocks 2 .. 1 + M, whose means hold block 1
    for got in (y, ref):
        assert np.array_equal(np.isnan(got.real), spoiled) and not np.isnan(got.imag).any()
        assert np.array_equal(bits(got[~spoiled]), bits(clean[~spoiled]))                    # nothing else is touched
    # host and numpy: the same samples are NaN (which NaN is unspecified), every other bit equal
    keep = ~np.isnan(y.view(np.float32))
    assert np.array_equal(keep, ~np.isnan(ref.view(np.float32))) and np.array_equal(y.view(np.uint32)[keep], ref.view(np.uint32)[keep])


# ---------------------------------------------------------------------------------------------------------- 3: errors and surface
def test_error_codes_without_a_gpu(api):
    import ofdm_amd
    from ofdm_amd import build

    lib = C.CDLL(build.build())
    for f in NEW:
        fn = getattr(lib, f)
        fn.restype, fn.argtypes = ofdm_amd.SIGNATURES[f]
    INVALID = -1
    assert lib.ofdm_dc_block_default(64, 16) == 4 and lib.ofdm_dc_block_default(1024, 256) == 60 and lib.ofdm_dc_block_default(4096, 1024) == 240
    assert [api.dc_block_default(n) for n in (64, 128, 256, 512, 1024, 2048, 4096)] == [D.default_blocks(n) for n in (64, 128, 256, 512, 1024, 2048, 4096)]
    for bad in ((0, 0), (100, 25), (64, 8), (8192, 2048), (32, 8), (-64, -16)):
        assert lib.ofdm_dc_block_default(*bad) == INVALID, bad
    x, y = np.zeros(128, np.complex64), np.zeros(128, np.complex64)
    q = np.zeros((128, 2), np.int16)
    p = lambda a: a.ctypes.data
    assert lib.ofdm_dc_block(p(x), 128, 4, p(y)) == 0 and lib.ofdm_dc_block(None, 0, 4, None) == 0
    for M in (0, -1, 1025):
        assert lib.ofdm_dc_block(p(x), 128, M, p(y)) == INVALID and lib.ofdm_dc_block_sc16(p(q), 128, 1.0, M, p(y)) == INVALID
    assert lib.ofdm_dc_block(p(x), -1, 4, p(y)) == INVALID and lib.ofdm_dc_block(None, 128, 4, p(y)) == INVALID
    assert lib.ofdm_dc_block(p(x), 128, 4, None) == INVALID
    UNSUPPORTED = -2                                                # a stream beyond 2^40 samples: refused before anything is read or allocated
    assert lib.ofdm_dc_block(p(x), 2 ** 40 + 1, 4, p(y)) == UNSUPPORTED and lib.ofdm_dc_block_sc16(p(q), 2 ** 40 + 1, 1.0, 4, p(y)) == UNSUPPORTED
    assert lib.ofdm_dc_block_sc16(p(q), 128, 1.0, 4, p(y)) == 0 and lib.ofdm_dc_block_sc16(None, 0, 1.0, 4, None) == 0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.ofdm_dc_block_sc16(p(q), 128, bad, 4, p(y)) == INVALID
    assert lib.ofdm_dc_block_sc16(None, 128, 1.0, 4, p(y)) == INVALID and lib.ofdm_dc_block_sc16(p(q), 128, 1.0, 4, None) == INVALID
    with pytest.raises(api.OfdmError):
        api.dc_block_host(q, 4)                                     # int16 without a scale
    with pytest.raises(api.OfdmError):
        api.dc_block_host(x, 0)
    # NULL handles and contexts: invalid, never a crash
    h, t, m = C.c_void_p(), C.c_int64(7), C.c_int32(7)
    assert lib.ofdm_dcblock_create(None, None, 4, 4096) == INVALID
    assert lib.ofdm_dcblock_create(C.byref(h), None, 4, 4096) == INVALID and not h.value
    assert lib.ofdm_dcblock_destroy(None) == INVALID and lib.ofdm_dcblock_reset(None) == INVALID
    assert lib.ofdm_dcblock_push(None, p(x), 128, p(y)) == INVALID and lib.ofdm_dcblock_push_sc16(None, p(q), 128, 1.0, p(y)) == INVALID
    assert lib.ofdm_dcblock_state(None, C.byref(t), C.byref(m)) == INVALID
    assert lib.ofdm_stream_set_dc_block(None, 4) == INVALID and lib.ofdm_stream_get_dc_block(None, C.byref(m)) == INVALID


def test_surface_in_every_layer():
    import ofdm_amd

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofdm_hip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ofdm_host.hpp")).read()
    api_src = open(os.path.join(ROOT, "ofdm_amd", "api.py")).read()
    for f in NEW:
        assert re.search(r"\bint %s\(" % f, hdr), f
        assert f in ofdm_amd.SIGNATURES, f
        assert re.search(r"pub fn %s\s*\(" % f, rs), f
        assert f in hpp, f
        assert f in api_src, f
        # no new function is an `ofdm_ctx *ctx` entry point: the handle, or plain values, come first
        assert not re.search(r"\b%s\(\s*(const\s+)?ofdm_ctx\s*\*" % f, hdr), f
    assert "typedef struct ofdm_dcblock ofdm_dcblock;" in hdr and "class DcBlock" in hpp and "struct DcBlock" in rs
    assert "set_dc_block" in hpp and "kernels_dcblock.hip" in open(os.path.join(ROOT, "ofdm_amd", "build.py")).read()
    for name in ("dc_block_default", "dc_block_host", "def dc_filter", "def dc_block", "class DcBlock", "dc_blocks"):
        assert name in api_src, name


# ---------------------------------------------------------------------------------------------------------- 4: the reason to exist
@pytest.mark.parametrize("name", list(K.CASES))
def test_seeds_are_the_first_whose_dc_free_frames_lock(orc, name):
    assert K.seed_of(orc, name) == K.SEEDS[name]


@pytest.mark.parametrize("name", list(K.CASES))
def test_dc_loses_the_frames_and_the_filter_brings_them_back(orc, name):
    """Measured here (the figures the test prints; also in DESIGN.md): e_f - e_0 between -4 and +3 bits over the four cases and three DC
    terms (n64_qam64: 62 -> 58 and 64 -> 67; n256_qam64: 37 -> 37 and 25 -> 23; n1024_qam64: 11 -> 11 and 6 -> 7; n64_qpsk: 0 -> 0), every
    frame timed on the DC-free capture's sample."""
    c = K.capture(orc, name, K.SEEDS[name])
    M = D.default_blocks(c.n_fft)
    base = K.frames(orc, c, c.x.astype(np.complex64))                  # DC-free, unfiltered: the same noise
    assert all(e is not None for _, e in base)
    for f in K.DC_FACTORS:
        x = K.with_dc(c, f)
        d = orc.sc_sync(x, L=c.S)[0]
        un = K.frames(orc, c, x)
        print(name, "dc", f, "rho %.1f" % K.rho(c, f), "unfiltered d", d, "lead", c.lead, "errors", [e for _, e in un], "DC-free", [e for _, e in base])
        if K.rho(c, f) >= K.RHO_FIRES:                                  # 1: fires inside the lead, the decode fails
            assert 0 <= d < c.lead - c.S, (name, f, d)
            r, e = un[0]
            assert r["offset"] < c.starts[0] - c.S and (e is None or e > 0.25 * 8 * len(c.coded[0])), (name, f, r["offset"], e)
            assert r["bytes"] != c.payloads[0]
        else:                                                           # below the bound: the DC-free behaviour
            assert K.locks(orc, c, x), (name, f)
        fl = K.frames(orc, c, D.dc_block(x, M))
        for k, ((r, e), (r0, e0)) in enumerate(zip(fl, base)):
            print(name, "dc", f, "frame", k, "offset", r["offset"], "DC-free", r0["offset"], "e_f", e, "e_0", e0)
            assert r["offset"] == r0["offset"], (name, f, k)            # 2: timed on the sample of the DC-free capture
            assert e <= e0 + max(0.02 * e0, 8), (name, f, k, e, e0)     # 3


@pytest.mark.parametrize("name", list(K.CASES))
def test_noise_plus_dc_alone(orc, name):
    c = K.capture(orc, name, K.SEEDS[name])
    M = D.default_blocks(c.n_fft)
    rng = np.random.default_rng(5)
    n = 12 * c.S + 2000
    noise = np.sqrt(c.sigma2 / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    assert orc.sc_sync(noise.astype(np.complex64), L=c.S)[0] < 0
    for f in K.DC_FACTORS:
        x = (noise + f * c.rms * K.DC_PHASE).astype(np.complex64)
        if K.rho(c, f) >= K.RHO_FIRES:
            assert orc.sc_sync(x, L=c.S)[0] >= 0, (name, f)             # 4: unfiltered it detects ...
        assert orc.sc_sync(D.dc_block(x, M), L=c.S)[0] < 0, (name, f)   # ... filtered it detects nothing


@pytest.mark.parametrize("name", list(K.CASES))
def test_the_band_of_windows_and_the_default_in_it(orc, name):
    c = K.capture(orc, name, K.SEEDS[name])
    rows = []
    for r in K.BAND:
        M = K.blocks_of(c, r)
        ok = all(K.locks(orc, c, D.dc_block(K.with_dc(c, f), M)) for f in K.DC_FACTORS)
        rows.append((r, M, ok))
    print(name, "window r S -> (blocks, every frame locks):", rows)
    assert dict((r, ok) for r, _, ok in rows)[3] and K.blocks_of(c, 3) == D.default_blocks(c.n_fft)    # 5: only the default is asserted
