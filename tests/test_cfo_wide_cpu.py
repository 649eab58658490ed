"""CPU checks of EXT-8, wide CFO acquisition (include/ofdm_hip.h; definition: tests/cfo_wide_ref.py): with the f64 oracle alone the
definition picks the true multiple of 2 pi / S on every frame Schmidl-Cox detects, with a factor of at least 1.5 between the winner and
the runner-up, and the frame then decodes where it does not without it; the visiting order and the strict-greater rule, the dead-frame
rule and the scaling of the metric; the boundary takes cfo_mode 3 with Schmidl-Cox timing and nothing beyond it, and the new entry
point and constants are declared on every layer.  No kernel is launched here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfo_wide_ref as cw  # noqa: E402
from chest_ref import window_index  # noqa: E402
from util import through_channel, wide  # noqa: E402

BACKOFF = 4
RATIO = 1.5   # the issue's bound; the draws below give 2 and more


@pytest.fixture(scope="module")
def lib():
    from ofdm_amd import build

    return C.CDLL(build.build())


def _captures(orc, n, mod, guard, frames, snr_db, seed, payload=40, span=8):
    """frames of `payload` bytes through the FIR channel with a random delay, the offset frac + 2 pi m / S (m uniform over +-span, frac
    within +-0.95 pi / S) and noise -> [(samples f64, m, frac, payload bytes)]"""
    S = n + n // 4
    rng = np.random.default_rng([n, mod, seed])
    out = []
    for _ in range(frames):
        pay = bytes(rng.integers(0, 256, payload, dtype=np.uint8))
        tx = orc.encode(pay, guard, mod, n)
        m = int(rng.integers(-span, span + 1))
        frac = float((rng.random() * 1.9 - 0.95) * np.pi / S)
        delay = int(rng.integers(1, S))
        x = through_channel(orc, rng, tx, tx.size + S + 90, delay, frac + 2.0 * np.pi * m / S, snr_db, data_start=10 * S)
        out.append((wide(x), m, frac, pay))
    return out


def _sync(orc, x, S):
    d, _, _, f0 = orc.sc_sync(x, S)
    return d, max(d - S - BACKOFF, 0), f0


@pytest.mark.parametrize("n,mod,guard,snr_db,frames", [(64, 6, True, 6.0, 40), (64, 1, False, 4.0, 40), (256, 6, True, 8.0, 10)])
def test_the_definition_finds_the_offset(orc, n, mod, guard, snr_db, frames):
    S = n + n // 4
    trn = orc.default_training(n)
    ratios, detected = [], 0
    for x, m_true, frac, _ in _captures(orc, n, mod, guard, frames, snr_db, seed=1):
        d, o, f0 = _sync(orc, x, S)
        if d < 0 or o + 10 * S > x.size:
            continue
        detected += 1
        m, fd, metric = cw.cfo_wide(x, n, trn, [o], [f0])
        assert int(m[0]) == m_true, (m[0], m_true, metric)
        assert fd[0] == f0 + 2.0 * np.pi * m_true / S if m_true else fd[0] == f0
        assert abs(fd[0] - (frac + 2.0 * np.pi * m_true / S)) < 0.2 * np.pi / S        # the total offset, not its residue
        ratios.append(metric[0, 0] / metric[0, 1])
    print(f"N {n} mod {mod} {snr_db} dB: {detected} of {frames} detected, ratio min {min(ratios):.2f} median {np.median(ratios):.2f}")
    assert detected >= frames // 2 and min(ratios) >= RATIO


@pytest.mark.parametrize("n,mod,guard", [(64, 6, True), (128, 2, False)])
def test_the_total_offset_decodes_and_the_residue_does_not(orc, n, mod, guard):
    S = n + n // 4
    trn = orc.default_training(n)
    seen = set()
    for x, m_true, _, pay in _captures(orc, n, mod, guard, 12, 35.0, seed=2):
        d, o, f0 = _sync(orc, x, S)
        assert d >= 0
        m, fd, _ = cw.cfo_wide(x, n, trn, [o], [f0])
        assert int(m[0]) == m_true
        assert orc.decode_given(x, o, float(fd[0]), guard, mod, n)["bytes"] == pay
        if m_true:
            assert orc.decode_given(x, o, f0, guard, mod, n)["bytes"] != pay
        seen.add(m_true != 0)
    assert True in seen


def test_visiting_order_and_the_strict_greater_rule():
    assert cw.hypotheses(1) == [0, -1, 1] and cw.hypotheses(3) == [0, -1, 1, -2, 2, -3, 3]
    assert len(cw.hypotheses(cw.MAX_SPAN)) == 65
    assert cw.decide(np.ones(5), 2) == (0, 1.0, 1.0)                       # a tie keeps the first one visited
    assert cw.decide(np.array([1.0, 2.0, 2.0, 2.0, 1.0]), 2) == (-1, 2.0, 2.0)
    assert cw.decide(np.array([1.0, 2.0, 3.0, 0.0, 3.0]), 2) == (1, 3.0, 3.0)
    assert cw.decide(np.array([1.0, 0.0, 0.5, 0.0, 4.0]), 2) == (2, 4.0, 1.0)
    m, g, r = cw.decide(np.full(5, np.nan), 2)                              # nothing is greater than a NaN
    assert m == 0 and np.isnan(g) and np.isnan(r)
    # an all-zero capture: every G is 0
    n, S = 64, 80
    m, fd, metric = cw.cfo_wide(np.zeros((1, 12 * S)), n, np.ones(n), [3], [0.01])
    assert int(m[0]) == 0 and fd[0] == 0.01 and np.all(metric == 0)


def test_dead_frame_rule(orc):
    n, S = 64, 80
    trn = orc.default_training(n)
    x, m_true, _, _ = _captures(orc, n, 2, True, 1, 30.0, seed=3)[0]
    d, o, f0 = _sync(orc, x, S)
    rows = np.stack([x] * 5)
    frame_len = o + 10 * S                                                  # the training blocks end exactly at the capture's end
    off = np.array([o, o, o + 1, -1, o])
    status = np.array([0, -2, 0, 0, 0])
    f_in = np.array([f0, f0, f0, -0.0, f0])
    m, fd, metric = cw.cfo_wide(rows, n, trn, off, f_in, status=status, frame_len=frame_len)
    assert list(m) == [m_true, 0, 0, 0, m_true]
    assert np.all(metric[[1, 2, 3]] == 0) and np.all(metric[[0, 4]] > 0)
    assert fd[[1, 2, 3]].tobytes() == f_in[[1, 2, 3]].tobytes()            # untouched, bit for bit (the -0.0 included)
    assert metric[0].tobytes() == metric[4].tobytes()
    bad = rows.copy()
    bad[0, o + 7 * S + n // 4 + 5] = np.nan                                 # a training block of frame 0 only (behind its prefix)
    m2, fd2, metric2 = cw.cfo_wide(bad, n, trn, off, f_in, status=status, frame_len=frame_len)
    assert int(m2[0]) == 0 and fd2[0] == f0 and not np.isfinite(metric2[0]).any()
    assert np.array_equal(m2[1:], m[1:]) and np.array_equal(metric2[1:], metric[1:])


def test_the_metric_scales_with_the_square_of_the_capture_and_sums_the_window(orc):
    n, S = 128, 160
    trn = orc.default_training(n)
    x, m_true, _, _ = _captures(orc, n, 4, True, 1, 20.0, seed=4)[0]
    d, o, f0 = _sync(orc, x, S)
    m1, _, g1 = cw.cfo_wide(x, n, trn, [o], [f0])
    m4, _, g4 = cw.cfo_wide(4.0 * x, n, trn, [o], [f0])
    assert int(m1[0]) == int(m4[0]) == m_true
    np.testing.assert_allclose(g4, 16.0 * g1, rtol=1e-12)
    # the winner's metric, written out: the training blocks' sum, rotated, matched, and the cp_len delays of ofdm_chest_window
    cp = n // 4
    ybar = sum(x[o + (5 + b) * S + cp:o + (6 + b) * S] * np.exp(-1j * f0 * ((5 + b) * S + cp + np.arange(n))) for b in range(5))
    z = ybar * np.exp(-2j * np.pi * m_true * (cp + np.arange(n)) / S)
    g = np.fft.ifft(np.conj(trn) * np.fft.fft(z))
    idx = window_index(n)
    assert idx.size == cp and idx[0] == n - cp // 4
    np.testing.assert_allclose(g1[0, 0], np.sum(np.abs(g[idx]) ** 2), rtol=1e-9)
    assert np.sum(np.abs(g[idx]) ** 2) > 0.5 * np.sum(np.abs(g) ** 2)       # the right hypothesis puts the energy into the window


# ---------------------------------------------------------------------------------------------------------- the boundary
def _create(lib, cfo_mode, sync_mode=0):
    from ofdm_amd import Params

    p = Params()
    lib.ofdm_default_params(C.byref(p))
    p.cfo_mode, p.sync_mode = cfo_mode, sync_mode
    h = C.c_void_p()
    rc = lib.ofdm_create(C.byref(p), None, None, 0, None, C.byref(h))
    if rc == 0:
        lib.ofdm_destroy(h)
    return rc


def test_create_accepts_the_wide_mode_with_schmidl_cox_only(lib):
    """(before the mode existed cfo_mode = 3 was OFDM_ERR_INVALID)"""
    import torch
    from ofdm_amd import Params

    want = 0 if torch.cuda.is_available() else -3          # OFDM_ERR_NO_DEVICE without a GPU, as a valid context; never INVALID
    assert [_create(lib, m) for m in (0, 1, 2, 3)] == [want] * 4
    assert _create(lib, 3, sync_mode=1) == -1              # OFDM_SYNC_REFERENCE has no wide mode
    assert _create(lib, 2, sync_mode=1) == want
    assert [_create(lib, m) for m in (4, 5, -1)] == [-1] * 3
    p = Params()
    lib.ofdm_default_params(C.byref(p))
    assert p.cfo_mode == 1                                  # the default stays SIGNED
    assert C.sizeof(Params) == 64 and len(Params().reserved) == 4      # no span parameter: the layout did not move


def test_stage_rejects_a_null_context(lib):
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    lib.ofdm_cfo_wide_batch.argtypes = [vp, vp, i64, i64, i64, vp, vp, i32, vp, vp, vp]
    assert lib.ofdm_cfo_wide_batch(None, None, 1, 1200, 1200, None, None, 8, None, None, None) == -1
    assert lib.ofdm_cfo_wide_batch(None, None, 0, 1200, 1200, None, None, 8, None, None, None) == -1


def test_new_surface_is_on_every_layer(lib):
    import ofdm_amd
    from ofdm_amd import api

    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ofdm_host.hpp")).read()
    n = "ofdm_cfo_wide_batch"
    assert hasattr(lib, n) and n in ofdm_amd.SIGNATURES
    assert re.search(r"\bint " + n + r"\(", hdr) and ("pub fn " + n + "(") in rs and (n + "(") in hpp
    assert re.search(r"\bOFDM_CFO_WIDE = 3\b", hdr) and "pub const OFDM_CFO_WIDE: i32 = 3;" in rs
    assert re.search(r"#define OFDM_CFO_WIDE_SPAN 8\b", hdr) and "pub const OFDM_CFO_WIDE_SPAN: i32 = 8;" in rs
    assert re.search(r"#define OFDM_CFO_WIDE_MAX_SPAN 32\b", hdr) and "pub const OFDM_CFO_WIDE_MAX_SPAN: i32 = 32;" in rs
    assert (api.CFO_WIDE, api.CFO_WIDE_SPAN, api.CFO_WIDE_MAX_SPAN) == (3, 8, 32) == (ofdm_amd.CFO_WIDE, ofdm_amd.CFO_WIDE_SPAN, cw.MAX_SPAN)
    assert hasattr(api.Context, "cfo_wide")
    # the range the Schmidl-Cox estimate has always had is stated where it is returned, and the mode's range in the same words everywhere
    sc = hdr[hdr.index("/* Schmidl-Cox sliding autocorrelation"):hdr.index("int ofdm_sc_correlate_batch(")]
    assert "modulo 2 pi / L" in sc and "+-0.4 sub-carrier spacings" in sc
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        txt = open(os.path.join(ROOT, name)).read()
        assert "OFDM_CFO_WIDE" in txt and "±6.8 sub-carrier spacings" in txt and "±0.4" in txt, name
    assert "+-6.8 sub-carrier" in hdr and "+-6.8 sub-carrier" in rs
    src = open(os.path.join(ROOT, "ofdm_amd", "build.py")).read()
    assert '"kernels_cfowide.hip"' in src
