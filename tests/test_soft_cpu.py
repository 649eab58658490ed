"""CPU checks of the soft-decision extension (OFDM_ECC_HAMMING74_SOFT, ofdm_rx_llr_batch, ofdm_hamming74_decode_soft): the boundary
accepts the new ecc value and declares the two entry points, and the numpy restatement tests/soft_ref.py agrees with hand-worked
values and with the kernels' closed form, and the rule that holds the GPU's LLRs to the f64 oracle (soft_ref.llr_compare) accepts the
reference itself and rejects every listed way of getting an LLR wrong.  No kernel is launched here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import soft_ref as sr  # noqa: E402

NEW = ("ofdm_rx_llr_batch", "ofdm_hamming74_decode_soft")


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


def test_create_accepts_soft_hamming(lib):
    import torch

    assert _create(lib, 2) == (0 if torch.cuda.is_available() else -3)   # OFDM_ERR_NO_DEVICE without a GPU, never INVALID


def test_create_still_rejects_ecc_3_and_above(lib):
    assert [_create(lib, e) for e in (3, 4, -1, 100)] == [-1] * 4


def test_new_entry_points_are_on_every_surface(lib):
    import ofdm_amd
    from ofdm_amd import api

    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in ofdm_amd.SIGNATURES
        assert re.search(r"\bint " + n + r"\(", hdr) and ("pub fn " + n + "(") in rs
    assert re.search(r"OFDM_ECC_HAMMING74_SOFT = 2\b", hdr) and "pub const OFDM_ECC_HAMMING74_SOFT: i32 = 2;" in rs
    m = re.search(r"#define OFDM_SOFT_LLR_SCALE ([0-9.]+)f", hdr)
    assert m and float(m.group(1)) == api.SOFT_LLR_SCALE
    assert (ofdm_amd.ECC_HAMMING74_SOFT, ofdm_amd.SOFT_LLR_SCALE) == (2, api.SOFT_LLR_SCALE)


def test_soft_entry_points_reject_bad_arguments_without_a_context(lib):
    lib.ofdm_rx_llr_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_int64]
    lib.ofdm_hamming74_decode_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    assert lib.ofdm_rx_llr_batch(None, None, 1, 80, 80, 0, 1, None, None, None, 0, 16.0, None, 64) == -1
    assert lib.ofdm_hamming74_decode_soft(None, None, 56, None) == -1


def test_bpsk_and_qpsk_llr_is_v():
    v = np.array([-3.5, -1.0, -0.25, 0.0, 0.5, 1.0, 2.75])
    np.testing.assert_array_equal(sr.axis_llr(v, 1)[:, 0], v)
    np.testing.assert_array_equal(sr.point_llr(v + 0j, 1)[:, 0], v)
    z = np.array([0.3 - 0.7j, -1.2 + 0.1j])
    np.testing.assert_allclose(sr.point_llr(z, 2), [[0.3, -0.7], [-1.2, 0.1]], rtol=0, atol=1e-12)   # I bit, then Q bit


def test_16qam_closed_forms_by_hand():
    # M = 4: levels -3 -1 1 3, Gray 00 01 11 10.  MSB: v for |v| <= 2, 2v -+ 2 beyond; LSB: 2 - |v|
    for v, want in ((0.5, (0.5, 1.5)), (-0.5, (-0.5, 1.5)), (3.0, (4.0, -1.0)), (-2.5, (-3.0, -0.5)), (1.0, (1.0, 1.0)),
                    (-1.0, (-1.0, 1.0)), (2.0, (2.0, 0.0)), (5.0, (8.0, -3.0))):
        np.testing.assert_allclose(sr.axis_llr(np.array([v]), 2)[0], want, atol=1e-12)
    # a 16-QAM point at x = 1/3 (level 2, v = 1) on I and x = -1 (level 0, v = -3) on Q: bits I(1, 1), Q(0, 0)
    np.testing.assert_allclose(sr.point_llr(np.array([1 / 3 - 1j]), 4)[0], [1.0, 1.0, -4.0, -1.0], atol=1e-12)


def test_noiseless_weakest_bit_has_unit_magnitude():
    for m in (1, 2, 3, 4):
        M = 1 << m
        lam = sr.axis_llr(2.0 * np.arange(M) - (M - 1), m)
        assert np.abs(lam).min() == 1.0
        bits = np.stack([sr.gray_bit(np.arange(M), m, b) for b in range(m)], -1)
        assert ((lam > 0) == (bits == 1)).all()                    # positive means bit 1


def test_closed_form_is_the_brute_force_minimum():
    # every level and boundary, dense in between; out to three times the outermost level of the widest axis (15), so that the
    # lo < 0 / hi > M - 1 branches of llr_axis_bit are held far outside the constellation for every M
    v = np.concatenate([np.linspace(-48, 48, 96001), np.arange(-48, 49, 1.0)])
    for m in (1, 2, 3, 4):
        np.testing.assert_allclose(sr.axis_llr_closed(v, m), sr.axis_llr(v, m), rtol=0, atol=1e-9)


def test_quantise_and_weights():
    np.testing.assert_array_equal(sr.quantise([0.5, 1.5, -2.5, 200.0, -1e9, np.nan, np.inf, -np.inf]), [0, 2, -2, 127, -127, 0, 0, 0])
    hk = np.array([[1.0, 2.0, 0.0, 1j]])
    np.testing.assert_allclose(sr.channel_weights(hk, np.array([0, 1, 3])), [[0.5, 2.0, 0.5]])
    # what the seeded link of tools/link.py rests on (the GPU tests of this mode drew (n, p) directly before it): payloads drawn
    # max(p, 1) wide and cut to p are the payloads drawn p wide, and the generator stands where it stood, for p >= 1
    import torch

    for n, p in ((7, 400), (3, 1), (64, 560)):
        a, b = torch.Generator().manual_seed(77), torch.Generator().manual_seed(77)
        assert torch.equal(torch.randint(0, 256, (n, p), generator=a), torch.randint(0, 256, (n, max(p, 1)), generator=b)[:, :p])
        assert torch.equal(torch.randint(1, 33, (n,), generator=a), torch.randint(1, 33, (n,), generator=b))
        assert torch.equal(torch.rand((n,), dtype=torch.float64, generator=a), torch.rand((n,), dtype=torch.float64, generator=b))


def test_soft_hamming_restatement_by_hand():
    rng = np.random.default_rng(3)
    d = rng.integers(0, 16, 16)
    bits = np.array([(sr.ham_codeword(x) >> i) & 1 for x in d for i in range(7)])
    llr = (2 * bits - 1) * 20
    got = sr.ham_decode_soft(llr)
    np.testing.assert_array_equal(got, (d[0::2] | (d[1::2] << 4)).astype(np.uint8))
    assert (sr.ham_decode_soft(np.zeros(56, np.int8)) == 0).all()          # every codeword ties: the smallest nibble
    one = np.zeros(56, np.int64)
    one[3] = 5   # only d3 carries weight: every nibble with bit 3 set ties at +5, the smallest of them is 8
    assert sr.ham_decode_soft(one)[0] == 8
    assert sr.ham_decode_soft(np.zeros(55)).size == 0


# ---------------------------------------------------------------------------------------------------------- the comparison rule
SNRS = (30.0, 14.0, 6.0)


def _channels(orc, rng, n, n_frames):
    """None, one response per frame (1 + 0.3 randn) and the shared FFT of the reference's CHANNEL taps (|H| 0.29 .. 1.26), as fc32"""
    per_frame = (1.0 + 0.3 * (rng.standard_normal((n_frames, n)) + 1j * rng.standard_normal((n_frames, n)))).astype(np.complex64)
    return {"none": None, "per frame": per_frame, "taps": np.fft.fft(orc.channel_taps(), n).astype(np.complex64)}


def _case(orc, rng, n, guard, mod, snr, hk, n_frames=3, syms=None):
    from util import make_symbols_np

    syms = syms or (12 if n == 64 else 2)
    x, _ = make_symbols_np(orc, rng, n_frames * syms, n, guard, mod, snr_db=snr)
    x = x.reshape(n_frames, -1)
    if hk is not None:
        x = sr.through_h(x, n, hk.reshape(-1, n))
    return x, sr.oracle_llr_reference(orc, x, n, guard, mod, 32.0, hk)


@pytest.mark.parametrize("n,guard", [(64, True), (64, False), (1024, True)])
def test_rule_accepts_the_reference_and_excuses_at_most_one_percent(orc, n, guard):
    rng = np.random.default_rng(1000 + n + guard)
    worst = (0.0, None)
    for mod in (1, 2, 4, 6, 8):
        for snr in SNRS:
            for name, hk in _channels(orc, rng, n, 3).items():
                _, ref = _case(orc, rng, n, guard, mod, snr, hk)
                share = sr.llr_compare(sr.quantise(ref["y"]), ref["y"], ref["eps"], what=f"{n} {guard} {mod} {snr} {name}")
                sr.assert_signs(sr.quantise(ref["y"]), ref)
                print(f"reference alone: N {n} guard {guard} mod {mod} {snr} dB H {name}: excused {100 * share:.3f} % of {ref['y'].size}")
                assert share <= 0.01, (n, guard, mod, snr, name, share)
                worst = max(worst, (share, (mod, snr, name)))
    print("largest excused share", worst)


def _axis_llr_always_alo(v, m):
    """soft_ref.axis_llr_closed with the far level taken below l* whenever there is one"""
    v = np.asarray(v, np.float64)
    M = 1 << m
    ls = np.clip(np.floor(v / 2.0 + M / 2.0), 0, M - 1).astype(np.int64)
    a_s = 2.0 * ls - (M - 1)
    out = np.empty(v.shape + (m,))
    for b in range(m):
        h = 1 << (m - 1 - b)
        r = (ls + h) >> (m - b)
        lo, hi = (2 * r - 1) * h - 1, (2 * r + 1) * h
        ao = np.where(lo < 0, 2.0 * hi - (M - 1), 2.0 * lo - (M - 1))
        lam = 0.25 * (a_s - ao) * (2.0 * v - ao - a_s)
        out[..., b] = np.where(r & 1, lam, -lam)
    return out


def _mutants(ref, mod, hk, bins, n):
    """name -> a wrong LLR array for the case `ref` (int64, so that +-128 can be represented)"""
    y, pts, w = ref["y"], ref["points"], ref["weights"]
    q = sr.quantise(y).astype(np.int64)
    shape = y.shape
    out = {"off by one": q + 1, "off by minus one": q - 1, "sign flipped": -q,
           "truncated": np.clip(np.trunc(y), -127, 127).astype(np.int64), "clamp at 128": np.clip(np.rint(y), -128, 128).astype(np.int64)}
    m = mod // 2
    wb = 1.0 if w is None else w[:, None, :, None]
    if mod >= 2:
        out["I and Q swapped"] = sr.quantise(32.0 * wb * sr.point_llr(pts.imag + 1j * pts.real, mod)).reshape(shape).astype(np.int64)
    if mod >= 4:
        M = 1 << m
        lam = sr.point_llr(pts, mod)
        rev = np.concatenate([lam[..., :m][..., ::-1], lam[..., m:][..., ::-1]], axis=-1)
        out["Gray order reversed"] = sr.quantise(32.0 * wb * rev).reshape(shape).astype(np.int64)
        alo = np.concatenate([_axis_llr_always_alo(pts.real * (M - 1), m), _axis_llr_always_alo(pts.imag * (M - 1), m)], axis=-1)
        out["far level always alo"] = sr.quantise(32.0 * wb * alo).reshape(shape).astype(np.int64)
    if hk is not None:
        h2 = np.abs(hk.astype(np.complex128).reshape(-1, n)) ** 2
        lam = sr.point_llr(pts, mod)
        out["weights over all N bins"] = sr.quantise(32.0 * (h2[:, bins] / h2.mean(-1, keepdims=True))[:, None, :, None] * lam).reshape(shape).astype(np.int64)
        h1 = np.sqrt(h2[:, bins])
        out["w = |H|"] = sr.quantise(32.0 * (h1 / h1.mean(-1, keepdims=True))[:, None, :, None] * lam).reshape(shape).astype(np.int64)
    return out


@pytest.mark.parametrize("mod", [1, 2, 4, 6, 8])
def test_rule_rejects_every_mutation(orc, mod):
    n, guard = 64, True
    rng = np.random.default_rng(2000 + mod)
    bins = sr.data_bins(orc, n, guard)
    seen = set()
    for snr in SNRS:
        for name, hk in _channels(orc, rng, n, 3).items():
            _, ref = _case(orc, rng, n, guard, mod, snr, hk)
            for what, bad in _mutants(ref, mod, hk, bins, n).items():
                if what == "clamp at 128" and not (np.abs(ref["y"]) > 128.5 + ref["eps"]).any():
                    continue                                     # nothing saturates in this case (BPSK / QPSK at scale 32): no such mutant
                with pytest.raises(AssertionError):
                    sr.llr_compare(bad, ref["y"], ref["eps"])
                seen.add(what)
    want = {"off by one", "off by minus one", "sign flipped", "truncated", "weights over all N bins", "w = |H|"}
    want |= {"I and Q swapped"} if mod >= 2 else set()
    want |= {"Gray order reversed", "far level always alo", "clamp at 128"} if mod >= 4 else set()
    assert want <= seen, want - seen


def test_rule_edges_by_hand():
    y = np.array([0.2, 0.49, 0.51, 126.3, 127.3, 127.9, 500.0, -0.5, np.nan, np.inf])
    q = sr.quantise(y)
    np.testing.assert_array_equal(q, [0, 0, 1, 126, 127, 127, 127, 0, 0, 0])
    assert sr.llr_compare(q, y, 0.02) == 0.3                       # 0.49, 0.51 and -0.5 are within 0.02 of a boundary, the rest decided
    np.testing.assert_array_equal(sr.llr_decided(y, 0.02), [1, 0, 0, 1, 1, 1, 1, 0, 1, 1])
    sr.llr_compare([0, 1, 0, 126, 127, 127, 127, -1, 0, 0], y, 0.02)   # the undecided ones on the other side of their boundary
    for i, wrong in ((0, 1), (1, -1), (1, 2), (2, 2), (3, 127), (5, 126), (6, 126), (7, 1), (8, 1), (9, 127)):
        bad = q.astype(np.int64).copy()
        bad[i] = wrong
        with pytest.raises(AssertionError):
            sr.llr_compare(bad, y, 0.02)
    assert sr.llr_compare([1, 0], np.array([0.2, 0.9]), 0.6) == 1.0   # eps > 1/2: nothing is decided, one step across is allowed ...
    with pytest.raises(AssertionError):
        sr.llr_compare([2], np.array([0.2]), 0.6)                     # ... two are not
    with pytest.raises(AssertionError):
        sr.llr_compare([-1], np.array([0.2]), 0.6)                    # ... and -0.5 is 0.7 away


def test_slope_is_the_derivative_of_the_brute_force():
    rng = np.random.default_rng(5)
    for mod in (1, 2, 4, 6, 8):
        z = (rng.uniform(-1.6, 1.6, 4000) + 1j * rng.uniform(-1.6, 1.6, 4000))
        d = 1e-7
        num = (sr.point_llr(z + d * (1 + 1j), mod) - sr.point_llr(z - d * (1 + 1j), mod)) / (2 * d)
        sl = sr.llr_slope(z, mod)
        smooth = np.abs(np.abs(num) - sl) < 1e-3 * sl               # all but the points within d of a kink of Lambda
        assert smooth.mean() > 0.999 and sl.min() >= 1.0, (mod, smooth.mean())
