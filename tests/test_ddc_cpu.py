"""The digital down-converter (EXT-16, include/ofdm_hip.h "a digital down-converter") without a GPU.

  1. the host functions ofdm_ddc / ofdm_ddc_sc16 equal the numpy definition (tests/ddc_ref.py) bit for bit, on an input and taps on which
     another order of the additions, or a multiply followed by an add, gives other bits;
  2. the rotor tables are numpy's within one f32 ulp; the phase rule is the integer definition far beyond 2^32 samples; phase_inc is
     taken mod 2^20; the stateful mirror of the handle equals the one-shot rule however the stream is cut;
  3. the properties: the identity converter returns its input's bits, a NaN spoils exactly the outputs whose window holds it, M(n), the
     design (the table of DESIGN.md, EXT-16, is printed here);
  4. every error code, and the surface in every layer;
  5. the reason to exist, on the f64 oracle alone (tests/ddc_cases.py): plain decimation of a wide-band capture loses the first frame to
     the noise lead and leaves more than a quarter of every frame's bits wrong, also of the frames it times right;
     converted with the default design every frame is timed on the sample the narrow-band capture is timed on and the QPSK case keeps
     the narrow-band capture's error count; the finding about an adjacent channel of the same modem is measured and printed.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ddc_cases as K
import ddc_ref as R
import sc16_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofdm_ddc_rotor_tables", "ofdm_ddc_out_len", "ofdm_ddc_inc_for", "ofdm_ddc_design", "ofdm_ddc", "ofdm_ddc_sc16", "ofdm_ddc_create",
       "ofdm_ddc_destroy", "ofdm_ddc_reset", "ofdm_ddc_push", "ofdm_ddc_push_sc16", "ofdm_ddc_state", "ofdm_stream_set_ddc", "ofdm_stream_get_ddc")
DECIMS = (1, 2, 3, 4, 8, 64)
INVALID, UNSUPPORTED = -1, -2


def taps_of(D):
    return [T for T in (D, 4 * D + 1, 24 * D, 257, 4096) if D <= T <= 4096]


def lengths(D, T):
    return (0, T - 1, T, T + D - 1, T + D, 5 * T + 17)


def bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


@pytest.fixture(scope="module")
def api():
    from ofdm_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def rot(api):
    return api.ddc_rotor_tables()


@pytest.fixture(scope="module")
def lib():
    import ofdm_amd
    from ofdm_amd import build

    lib = C.CDLL(build.build())
    for f in NEW:
        fn = getattr(lib, f)
        fn.restype, fn.argtypes = ofdm_amd.SIGNATURES[f]
    return lib


# ---------------------------------------------------------------------------------------------------------- 1: the definition
def other_orders(v, D, h, M):
    """the same filter with its additions in another order, or without the fma: descending k, pairwise, multiply then add"""
    last = (M - 1) * D
    col = lambda k: v[k: k + last + 1: D]
    out = {}
    for part in ("real", "imag"):
        g = lambda k: np.ascontiguousarray(getattr(col(k), part))
        acc = np.zeros(M, np.float32)
        for k in range(h.size - 1, -1, -1):
            acc = R.fma32(h[k], g(k), acc)
        out.setdefault("descending", []).append(acc)
        terms = [R.fma32(h[k], g(k), np.zeros(M, np.float32)) for k in range(h.size)]
        while len(terms) > 1:
            terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
        out.setdefault("pairwise", []).append(terms[0])
        acc = np.zeros(M, np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            for k in range(h.size):
                acc = acc + h[k] * g(k)                 # two roundings
        out.setdefault("multiply then add", []).append(acc)
    return {k: (re + 1j * im).astype(np.complex64) for k, (re, im) in out.items()}


def test_the_wide_input_tells_orders_of_accumulation_apart(rot):
    D, T, n = 4, 96, 96 + 4 * 400
    x, h = K.wide(n, 7), K.wide_taps(T, 8)
    mag = np.abs(x[x != 0])
    assert mag.max() / mag.min() > 2.0 ** 70 and abs(float(h.astype(np.float64).sum())) < 0.05 * float(np.abs(h).sum())
    v = R.mix(x, 0, 12345, *rot)
    M = R.out_len(n, D, T)
    want = R.fir(v, D, h, M)
    for what, y in other_orders(v, D, h, M).items():
        differ = int((bits(y) != bits(want)).any(axis=None) and (bits(y).reshape(-1, 2) != bits(want).reshape(-1, 2)).any(axis=1).sum())
        print(what, "differs in", differ, "of", M, "outputs")
        assert differ > M // 10, what
    # ... and so does a mixer whose inner product is contracted into the fma's own rounding (one rounding less)
    p = R.phases(0, n, 12345)
    r = R.cmul(rot[0][p >> 10], rot[1][p & 1023])
    exact = (x.astype(np.complex128) * r.astype(np.complex128)).astype(np.complex64)
    assert (bits(exact) != bits(v)).any()


@pytest.mark.parametrize("D", DECIMS)
def test_host_functions_are_the_numpy_definition(api, rot, D):
    rng = np.random.default_rng(D)
    for T in taps_of(D):
        h = K.wide_taps(T, 20 + T)
        for n in lengths(D, T):
            inc = int(rng.integers(0, R.PHASE_MOD))
            x = K.wide(n, 100 + n % 97)
            got = api.ddc_host(x, D, inc, h)
            assert got.size == R.out_len(n, D, T) == api.ddc_out_len(n, D, T), (D, T, n)
            assert np.array_equal(bits(got), bits(R.ddc(x, D, inc, h, *rot))), (D, T, n)
            if T > 24 * D and T != D and n != T + D:
                continue                                # sc16, the long filters (257, 4096): one length each, the same code behind another load
            q, scale = rng.integers(-32768, 32768, (n, 2)).astype(np.int16), 0.7 / 32768
            xw = R.widen(q, scale)
            assert np.array_equal(bits(xw), bits(sc16_ref.widen(q, scale)))
            got = api.ddc_host(q, D, inc, h, scale=scale)
            assert np.array_equal(bits(got), bits(R.ddc_sc16(q, scale, D, inc, h, *rot))), (D, T, n)
            assert np.array_equal(bits(got), bits(api.ddc_host(xw, D, inc, h))), (D, T, n)


# ---------------------------------------------------------------------------------------------------------- 2: rotor, phase, cuts
def test_rotor_tables_are_numpys_within_one_ulp(rot):
    for got, want in zip(rot, R.tables()):
        assert got.shape == (1024,) and got.dtype == np.complex64
        g, w = got.view(np.float32), want.view(np.float32)
        assert (np.abs(g.astype(np.float64) - w.astype(np.float64)) <= np.spacing(np.abs(w)).astype(np.float64)).all()
    assert rot[0][0] == 1 and rot[1][0] == 1 and rot[0][256] .imag == 1 and rot[0][512].real == -1


def test_the_phase_rule_far_beyond_2_to_the_32():
    n0 = 2 ** 33 + 7
    for inc in (1, 786432, 314573, R.PHASE_MOD - 1, 5 + 3 * R.PHASE_MOD, -7):
        want = [((n0 + i) * inc) % R.PHASE_MOD for i in range(3000)]              # python integers: the definition
        assert R.phases(n0, 3000, inc).tolist() == want
        # what the host and the device compute: the low 32 bits of the index times the increment mod 2^20, in 32-bit arithmetic
        low = ((np.arange(3000, dtype=np.uint64) + np.uint64(n0)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        assert ((low * np.uint32(inc % R.PHASE_MOD)) & np.uint32(R.PHASE_MOD - 1)).tolist() == want


def test_phase_inc_is_taken_mod_2_to_the_20(api, lib, rot):
    x, h = K.wide(700, 3), K.wide_taps(9, 4)
    want = R.ddc(x, 2, 314573, h, *rot)
    out, n_out = np.zeros(400, np.complex64), C.c_int64()
    for inc in (314573, 314573 + R.PHASE_MOD, 314573 - R.PHASE_MOD, 314573 - 2048 * R.PHASE_MOD):
        assert lib.ofdm_ddc(x.ctypes.data, 700, 2, inc, h.ctypes.data, 9, out.ctypes.data, 400, C.byref(n_out)) == 0
        assert n_out.value == want.size and np.array_equal(bits(out[: want.size]), bits(want)), inc
        assert np.array_equal(bits(api.ddc_host(x, 2, inc, h)), bits(want))
    assert api.ddc_inc_for(0.25) == R.inc_for(0.25) == 786432 and api.ddc_inc_for(-0.3) == R.inc_for(-0.3) == 314573
    assert api.ddc_inc_for(0.0) == 0 and api.ddc_inc_for(0.5) == api.ddc_inc_for(-0.5) == 1 << 19
    # a tone at f0 comes down to 0: the output is the filter's gain at 0 times the tone's amplitude, up to the rotor's 2^-20 grid
    n = np.arange(4000)
    tone = np.exp(2j * np.pi * 0.25 * n).astype(np.complex64)
    y = api.ddc_host(tone, 4, api.ddc_inc_for(0.25))
    assert np.abs(y - 1).max() < 1e-5


@pytest.mark.parametrize("D,T", [(1, 1), (2, 9), (3, 72), (4, 96), (8, 192), (64, 64)])
def test_the_handle_mirror_is_the_one_shot_rule_however_it_is_cut(rot, D, T):
    n = 5 * T + 17 + 2000
    x, h, inc = K.wide(n, 11 + D), K.wide_taps(T, 12 + D), 314573
    ref = bits(R.ddc(x, D, inc, h, *rot))
    rng = np.random.default_rng(D)
    eq = lambda m: [m] * (n // m) + [n % m]
    lead = max(T - 3, 0)
    cuts = {"1": [lead] + [1] * (2 * D + 6) + [n - lead - (2 * D + 6)],            # single samples across the first outputs
            "D": eq(D), "997": eq(997), "random": []}
    if D > 1:
        cuts["D-1"] = eq(D - 1) if D > 2 else [1] * 300 + [n - 300]
    left = n
    while left:
        m = int(min(rng.integers(0, 600), left))                                   # empty pushes included
        cuts["random"].append(m)
        left -= m
    for what, parts in cuts.items():
        f, at, got = R.Handle(D, inc, h, *rot), 0, []
        for m in parts:
            got.append(f.push(x[at: at + m]))
            at += m
            assert f.carry.size <= max(T - 1, 0) and f.total_out == R.out_len(at, D, T)
        assert at == n and f.total_in == n
        assert np.array_equal(bits(np.concatenate(got)), ref), (D, T, what)
        f.reset()
        assert np.array_equal(bits(f.push(x[: 2 * T + 5])), bits(R.ddc(x[: 2 * T + 5], D, inc, h, *rot)))   # a reset starts a new stream at 0


# ---------------------------------------------------------------------------------------------------------- 3: properties
def test_the_identity_converter_returns_the_inputs_bits(api, rot):
    x = K.wide(1000, 5)
    one = np.ones(1, np.float32)
    for y in (api.ddc_host(x, 1, 0, one), R.ddc(x, 1, 0, one, *rot)):
        keep = x.view(np.float32) != 0                  # (-0.0 comes out as +0.0: the sum starts from +0.0)
        assert np.array_equal(y.view(np.uint32)[keep], x.view(np.uint32)[keep]) and not y.view(np.float32)[~keep].any()


@pytest.mark.parametrize("D,T", [(1, 5), (3, 13), (4, 96)])
def test_a_nan_spoils_exactly_the_outputs_whose_window_holds_it(api, rot, D, T):
    n, at = 6 * T + 50, 2 * T + 7
    x, h = K.wide(n, 3), K.wide_taps(T, 6)
    h[h == 0] = 1.0
    clean = R.ddc(x, D, 99, h, *rot)
    x[at] = np.complex64(complex(np.nan, 1.0))          # the mixer spreads a NaN in one part over both
    m = np.arange(clean.size)
    spoiled = (m * D <= at) & (at < m * D + T)
    for y in (api.ddc_host(x, D, 99, h), R.ddc(x, D, 99, h, *rot)):
        assert np.array_equal(np.isnan(y.real), spoiled) and np.array_equal(np.isnan(y.imag), spoiled)
        assert np.array_equal(bits(y[~spoiled]), bits(clean[~spoiled]))


def test_out_len(api, lib):
    for D in DECIMS:
        for T in taps_of(D):
            for n in list(lengths(D, T)) + [10 ** 6 + 3]:
                assert api.ddc_out_len(n, D, T) == R.out_len(n, D, T) == len(range(0, n - T + 1, D))
    for bad in ((-1, 4, 96), (100, 0, 96), (100, 65, 96), (100, 4, 3), (100, 4, 4097)):
        assert lib.ofdm_ddc_out_len(*bad) == INVALID, bad


def gain(h, f):
    return abs(np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * f * np.arange(h.size))))


def test_the_design(api):
    """The table of DESIGN.md (EXT-16), for D = 4 (it is the same within 1 dB for D = 2 .. 64):
        taps a phase    8       16      24      32
        0.406 / D    -1.44   -0.08   +0.02   +0.02   dB   the passband's edge as the issue names it
        0.484 / D    -4.92   -3.95   -3.11   -2.41   dB   the modem's outermost carrier (tests/ddc_cases.py: the finding)
        stopband     -16.1   -39.2   -54.8   -59.7   dB   the worst gain beyond 0.594 / D (8 and 16 a phase: the transition ends behind it)"""
    for D in (1, 2, 3, 4, 8, 64):
        for tpp in (1, 8, 16, 24, 32, 64):
            h = api.ddc_design(D, tpp)
            want32, want = R.design(D, tpp)
            assert h.size == D * tpp and np.abs(h.astype(np.float64) - want).max() <= 1e-7 * np.abs(want).max(), (D, tpp)
            assert abs(float(h.astype(np.float64).sum()) - 1.0) <= h.size * 2.0 ** -25 * float(np.abs(h).max()) + 2.0 ** -23, (D, tpp)   # gain at 0
    assert np.array_equal(api.ddc_design(4), api.ddc_design(4, 24)) and api.DDC_TAPS_PER_PHASE == R.TAPS_PER_PHASE == 24
    assert api.ddc_design(1, 1).tolist() == [1.0]
    D = 4
    f_stop = np.linspace(0.594 / D, 0.5, 4000)
    rows = {}
    for tpp in (8, 16, 24, 32):
        h = api.ddc_design(D, tpp)
        db = lambda g: 20 * np.log10(g)
        rows[tpp] = (db(gain(h, 0.406 / D)), db(gain(h, 0.484 / D)), db(max(gain(h, f) for f in f_stop)), db(gain(h, 0.5 / D)))
        print("taps a phase %2d: droop at 0.406/D %.2f dB, at 0.484/D %.2f dB, worst stopband beyond 0.594/D %.1f dB, at 0.5/D %.2f dB" % ((tpp,) + rows[tpp]))
    droop, _, stop, mid = rows[24]
    assert stop < mid                                   # the default: its stopband lies below its transition band


# ---------------------------------------------------------------------------------------------------------- 4: errors and surface
def test_error_codes_without_a_gpu(api, lib):
    x, y, h = np.zeros(512, np.complex64), np.zeros(512, np.complex64), np.ones(96, np.float32)
    q = np.zeros((512, 2), np.int16)
    p = lambda a: a.ctypes.data
    n_out = C.c_int64(7)
    assert lib.ofdm_ddc(p(x), 512, 4, 0, p(h), 96, p(y), 512, C.byref(n_out)) == 0 and n_out.value == 105
    assert lib.ofdm_ddc(None, 0, 4, 0, p(h), 96, None, 0, C.byref(n_out)) == 0 and n_out.value == 0
    assert lib.ofdm_ddc(p(x), 95, 4, 0, p(h), 96, None, 0, None) == 0                        # no output: no buffer needed
    for D, T in ((0, 96), (-1, 96), (65, 96), (4, 3), (4, 4097), (4, 0)):
        assert lib.ofdm_ddc(p(x), 512, D, 0, p(h), T, p(y), 512, C.byref(n_out)) == INVALID, (D, T)
        assert lib.ofdm_ddc_sc16(p(q), 512, 1.0, D, 0, p(h), T, p(y), 512, C.byref(n_out)) == INVALID, (D, T)
    assert lib.ofdm_ddc(p(x), -1, 4, 0, p(h), 96, p(y), 512, None) == INVALID and lib.ofdm_ddc(None, 512, 4, 0, p(h), 96, p(y), 512, None) == INVALID
    assert lib.ofdm_ddc(p(x), 512, 4, 0, None, 96, p(y), 512, None) == INVALID and lib.ofdm_ddc(p(x), 512, 4, 0, p(h), 96, None, 512, None) == INVALID
    y[:] = 5
    assert lib.ofdm_ddc(p(x), 512, 4, 0, p(h), 96, p(y), 104, C.byref(n_out)) == INVALID and n_out.value == 105 and (y == 5).all()   # too small: nothing written
    assert lib.ofdm_ddc(p(x), 512, 4, 0, p(h), 96, p(y), -1, None) == INVALID
    assert lib.ofdm_ddc(p(x), 2 ** 40 + 1, 4, 0, p(h), 96, p(y), 512, None) == UNSUPPORTED
    assert lib.ofdm_ddc_sc16(p(q), 2 ** 40 + 1, 1.0, 4, 0, p(h), 96, p(y), 512, None) == UNSUPPORTED
    assert lib.ofdm_ddc_sc16(p(q), 512, 1.0, 4, 0, p(h), 96, p(y), 512, C.byref(n_out)) == 0 and n_out.value == 105
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.ofdm_ddc_sc16(p(q), 512, bad, 4, 0, p(h), 96, p(y), 512, None) == INVALID
    assert lib.ofdm_ddc_sc16(None, 512, 1.0, 4, 0, p(h), 96, p(y), 512, None) == INVALID
    inc = C.c_int32(7)
    for bad in (0.5000001, -0.51, float("nan"), float("inf"), -float("inf")):
        assert lib.ofdm_ddc_inc_for(bad, C.byref(inc)) == INVALID and inc.value == 7
    assert lib.ofdm_ddc_inc_for(0.1, None) == INVALID
    for bad in ((0, 24), (65, 24), (4, 0), (4, 65), (-4, 24)):
        assert lib.ofdm_ddc_design(bad[0], bad[1], p(h)) == INVALID, bad
    assert lib.ofdm_ddc_design(4, 24, None) == INVALID
    assert lib.ofdm_ddc_rotor_tables(None, p(x)) == INVALID and lib.ofdm_ddc_rotor_tables(p(x), None) == INVALID
    with pytest.raises(api.OfdmError):
        api.ddc_host(q, 4)                              # int16 without a scale
    with pytest.raises(api.OfdmError):
        api.ddc_host(x, 0)
    with pytest.raises(api.OfdmError):
        api.ddc_host(x, 4, taps=np.ones(3, np.float32))
    with pytest.raises(api.OfdmError):
        api.ddc_inc_for(0.6)
    with pytest.raises(api.OfdmError):
        api.ddc_design(4, 65)
    # NULL handles and contexts: invalid, never a crash
    hd, a, b = C.c_void_p(), C.c_int64(7), C.c_int64(7)
    assert lib.ofdm_ddc_create(None, None, 4, 0, p(h), 96, 4096) == INVALID
    assert lib.ofdm_ddc_create(C.byref(hd), None, 4, 0, p(h), 96, 4096) == INVALID and not hd.value
    assert lib.ofdm_ddc_destroy(None) == INVALID and lib.ofdm_ddc_reset(None) == INVALID
    assert lib.ofdm_ddc_push(None, p(x), 128, p(y), 512, C.byref(a)) == INVALID and a.value == 0
    assert lib.ofdm_ddc_push_sc16(None, p(q), 128, 1.0, p(y), 512, None) == INVALID
    assert lib.ofdm_ddc_state(None, C.byref(a), C.byref(b)) == INVALID
    d, i, t = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.ofdm_stream_set_ddc(None, 4, 0, None, 0) == INVALID and lib.ofdm_stream_get_ddc(None, C.byref(d), C.byref(i), C.byref(t)) == INVALID


def test_surface_in_every_layer():
    import ofdm_amd

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofdm_hip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ofdm_host.hpp")).read()
    api_src = open(os.path.join(ROOT, "ofdm_amd", "api.py")).read()
    for f in NEW:
        assert re.search(r"\b(int|int64_t) %s\(" % f, hdr), f
        assert f in ofdm_amd.SIGNATURES, f
        assert re.search(r"pub fn %s\s*\(" % f, rs), f
        assert re.search(r"\b%s\(" % f, hpp), f
        assert re.search(r"\b%s\(" % f, api_src), f
        # no new function is an `ofdm_ctx *ctx` entry point: the handle, or plain values, come first
        assert not re.search(r"\b%s\(\s*(const\s+)?ofdm_ctx\s*\*" % f, hdr), f
    assert "typedef struct ofdm_ddc_handle ofdm_ddc_handle;" in hdr and "class Ddc" in hpp and "struct Ddc" in rs
    assert "#define OFDM_DDC_TAPS_PER_PHASE 24" in hdr
    assert "set_ddc" in hpp and "set_ddc" in rs and "kernels_ddc.hip" in open(os.path.join(ROOT, "ofdm_amd", "build.py")).read()
    for name in ("def ddc_host", "def ddc_design", "def ddc_inc_for", "def ddc(", "class Ddc", "ddc=None", "def set_ddc"):
        assert name in api_src, name
    assert "ofdm_stream_set_ddc" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---------------------------------------------------------------------------------------------------------- 5: the reason to exist
@pytest.mark.parametrize("name", list(K.CASES))
def test_seeds_are_the_first_whose_narrow_band_frames_lock(orc, name):
    assert K.seed_of(orc, name) == K.SEEDS[name]


@pytest.mark.parametrize("D", K.DECIMS)
@pytest.mark.parametrize("name", list(K.CASES))
def test_plain_decimation_loses_the_frames_and_the_converter_brings_them_back(orc, rot, name, D):
    w = K.wideband(orc, name, K.SEEDS[name], D)
    cap = w.cap
    base = K.frames(orc, cap, cap.clean)                                    # the narrow-band capture itself
    assert all(K.timed(cap, base)) and all(e is not None for _, e in base)
    # raw[::D] carries the narrow-band samples K.PLAIN_DELAY late (the interpolator's delay): that is where its frames truly start
    plain = K.frames(orc, cap, w.raw[::D], K.PLAIN_DELAY)
    at = [s + K.PLAIN_DELAY for s in cap.starts]
    print(name, "D", D, "raw[::D]: offsets", [r["offset"] for r, _ in plain], "errors", [e for _, e in plain], "true starts", at,
          "timed", K.timed(cap, plain, K.PLAIN_DELAY))
    # 1: the first frame is lost to the noise lead (the DC term fires the detector there: EXT-15), and EVERY frame's bits are garbage,
    # also where the detector, searching from the end of the frame before, times the frame right: the neighbour and the DC term alias
    # onto the wanted band
    r0, _ = plain[0]
    assert not K.timed(cap, plain, K.PLAIN_DELAY)[0] and r0["offset"] < at[0] - cap.S, (name, D, r0["offset"], at[0])
    n_bits = 8 * (16 + len(cap.payloads[0]))
    assert all(e is None or e > n_bits // 4 for _, e in plain), (name, D, [e for _, e in plain])
    y = R.ddc(w.raw, D, w.inc, w.taps, *rot)
    assert w.taps.size == R.TAPS_PER_PHASE * D and w.delay * 2 * D == K.INTERP_TPP * D - w.taps.size
    conv = K.frames(orc, cap, y, w.delay)
    for k, ((r, e), (r0, e0)) in enumerate(zip(conv, base)):
        print(name, "D", D, "frame", k, "offset", r["offset"], "narrow-band", r0["offset"], "+ delay", w.delay, "errors", e, "narrow-band", e0)
        assert r["offset"] == r0["offset"] + w.delay, (name, D, k)          # 2: timed on the narrow-band capture's sample
        if name == "n64_qpsk":
            assert e == e0, (name, D, k, e, e0)                             # 3: the narrow-band capture's error count +- 0


def test_the_neighbour_finding(orc, rot):
    """What tests/ddc_cases.py's docstring reports, measured again (n64_qpsk; errors of the three frames)."""
    name, seed = "n64_qpsk", K.SEEDS["n64_qpsk"]
    cap = K.narrow(orc, name, seed)

    def errors(D, **kw):
        w = K.wideband(orc, name, seed, D, **kw)
        fr = K.frames(orc, cap, R.ddc(w.raw, D, w.inc, w.taps, *rot), w.delay)
        assert all(K.timed(cap, fr, w.delay))
        return [e for _, e in fr]

    base = [e for _, e in K.frames(orc, cap, cap.clean)]
    rows = {}
    for D in (2, 4):
        rows[D, "none"] = errors(D, neighbour=0.0)
        rows[D, "unfiltered"] = errors(D, neighbour_cut=0.5)
        rows[D, "unfiltered, noise-free"] = errors(D, neighbour_cut=0.5, neighbour_snr=300.0)
        rows[D, "chosen"] = errors(D)
    rows[4, "unfiltered, 0 dB"] = errors(4, neighbour_cut=0.5, neighbour=1.0)
    for k, v in rows.items():
        print("D = %d, neighbour %s: errors %s (narrow-band %s)" % (k + (v, base)))
    for D in (2, 4):
        assert rows[D, "none"] == base and rows[D, "chosen"] == base
    assert min(rows[4, "unfiltered"]) > 10 and min(rows[4, "unfiltered, noise-free"]) > 10    # not the neighbour's noise
    assert rows[2, "unfiltered"] == base                                                       # the artefact of the synchronous grid
    # the transmitter's carriers run up to bin 31 of 64: no guard band at the channel's edge
    tx = np.asarray(orc.encode(cap.payloads[0], guard=True, modulation=cap.mod, n_fft=64))
    used = np.abs(np.fft.fft(tx[12 * 80 + 16: 13 * 80])) > 1e-6
    assert used[6:32].all() and used[33:59].all() and not used[:6].any() and not used[59:].any() and not used[32]
