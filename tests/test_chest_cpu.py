"""CPU checks of EXT-5, channel-estimate denoising (include/ofdm_hip.h; definition: tests/chest_ref.py): the boundary takes
chest_mode 0 and 1 and nothing else, the new entry points and constants are declared on every layer, the host solver
ofdm_chest_matrix is numpy's inverse of R, the definition reproduces every channel inside its tap window and no tap outside it, and
-- with the f64 oracle alone -- the denoised estimate is closer to the noiseless one and costs fewer hard bit errors than the
reference's estimate on the captures of tests/chest_cases.py.  No kernel is launched here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chest_cases as cc  # noqa: E402
import chest_ref as cr  # noqa: E402

NEW = ("ofdm_chest_matrix", "ofdm_chest_smooth_batch", "ofdm_chest_window")
CONSTANTS = (("CHEST_LS", 0), ("CHEST_WLS", 1))


@pytest.fixture(scope="module")
def lib():
    from ofdm_amd import build

    lib = C.CDLL(build.build())
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    lib.ofdm_chest_matrix.argtypes = [i32, i32, vp, vp]
    lib.ofdm_chest_smooth_batch.argtypes = [vp, vp, i64, vp]
    lib.ofdm_chest_window.argtypes = [vp, vp, vp]
    lib.ofdm_default_pilots.argtypes = [i32, i32, vp, vp]
    return lib


def _create(lib, chest_mode=0, reserved=None):
    from ofdm_amd import Params

    p = Params()
    lib.ofdm_default_params(C.byref(p))
    p.chest_mode = chest_mode
    if reserved is not None:
        p.reserved[reserved] = 1
    h = C.c_void_p()
    rc = lib.ofdm_create(C.byref(p), None, None, 0, None, C.byref(h))
    if rc == 0:
        lib.ofdm_destroy(h)
    return rc


def test_create_accepts_the_two_chest_modes_and_nothing_else(lib):
    """(before the mode existed chest_mode = 1 was a non-zero reserved[0]: OFDM_ERR_INVALID)"""
    import torch
    from ofdm_amd import Params

    want = 0 if torch.cuda.is_available() else -3          # OFDM_ERR_NO_DEVICE without a GPU, never INVALID
    assert [_create(lib, m) for m in (0, 1)] == [want, want]
    assert [_create(lib, m) for m in (2, -1)] == [-1, -1]
    assert len(Params().reserved) == 4 and C.sizeof(Params) == 64          # the layout did not move
    assert Params.chest_mode.offset == 44 and Params.reserved.offset == 48
    assert [_create(lib, 0, r) for r in range(4)] == [-1] * 4              # the remaining words are still checked
    assert [_create(lib, 1, r) for r in range(4)] == [-1] * 4
    p = Params()
    lib.ofdm_default_params(C.byref(p))
    assert p.chest_mode == 0                                               # the default stays the reference's estimate


def test_new_surface_is_on_every_layer(lib):
    import ofdm_amd
    from ofdm_amd import api

    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ofdm_host.hpp")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in ofdm_amd.SIGNATURES
        assert re.search(r"\bint " + n + r"\(", hdr) and ("pub fn " + n + "(") in rs and (n + "(") in hpp
    assert hasattr(api.Context, "chest_smooth") and hasattr(api.Context, "chest_window")
    assert "chest_mode" in api.Context.__init__.__code__.co_varnames
    for name, value in CONSTANTS:
        assert re.search(r"\bOFDM_%s = %d\b" % (name, value), hdr), name
        assert ("pub const OFDM_%s: i32 = %d;" % (name, value)) in rs, name
        assert getattr(api, name) == value and getattr(ofdm_amd, name) == value
        assert ("OFDM_" + name) in hpp, name
    assert re.search(r"int32_t chest_mode;", hdr) and re.search(r"int32_t reserved\[4\];", hdr)
    assert "pub chest_mode: i32," in rs and "pub reserved: [i32; 4]," in rs
    assert "spoils the frame's WHOLE estimate" in hdr                      # the non-finite-sample caveat is stated
    assert lib.ofdm_abi_version() == 1


def test_entry_points_reject_null_arguments(lib):
    assert lib.ofdm_chest_smooth_batch(None, None, 1, None) == -1
    assert lib.ofdm_chest_smooth_batch(None, None, 0, None) == -1
    a, b = C.c_int32(), C.c_int32()
    assert lib.ofdm_chest_window(None, C.byref(a), C.byref(b)) == -1


def _tables():
    """(n_fft, training or None): the default tables and one custom table with a weak and a dead bin"""
    rng = np.random.default_rng(11)
    custom = rng.uniform(-1, 1, 128) + 1j * rng.uniform(-1, 1, 128)
    custom[5] *= 1e-3
    custom[77] = 0.0
    return [(64, None), (128, None), (1024, None), (128, custom)]


@pytest.mark.parametrize("n_fft,training", _tables(), ids=["64", "128", "1024", "128-custom"])
def test_chest_matrix_is_numpys_inverse(lib, n_fft, training):
    lh = n_fft // 4
    trn = np.zeros(n_fft, np.complex128)
    if training is None:
        assert lib.ofdm_default_pilots(n_fft, lh, None, trn.ctypes.data) == 0
    else:
        trn[:] = training
    got = np.zeros((lh, lh), np.complex128)
    assert lib.ofdm_chest_matrix(n_fft, lh, None if training is None else trn.ctypes.data, got.ctypes.data) == 0
    R = cr.rmatrix(trn, n_fft)
    assert np.allclose(R, R.conj().T, rtol=0, atol=1e-12) and np.linalg.eigvalsh(R).min() > 0
    cond = np.linalg.cond(R)
    want = np.linalg.inv(R)
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"n_fft {n_fft}: cond(R) {cond:.2f}, relative error {err:.2e}")
    assert err <= cond * 1e-13
    assert np.abs(got - got.conj().T).max() <= 1e-15 * np.abs(got).max()


def test_chest_matrix_rejects_bad_arguments(lib):
    out = np.zeros((16, 16), np.complex128)
    assert lib.ofdm_chest_matrix(64, 16, None, None) == -1
    assert lib.ofdm_chest_matrix(64, 8, None, out.ctypes.data) == -1       # cp_len must be n_fft / 4
    assert lib.ofdm_chest_matrix(96, 24, None, out.ctypes.data) == -1
    assert lib.ofdm_chest_matrix(32, 8, None, out.ctypes.data) == -1
    assert lib.ofdm_chest_matrix(8192, 2048, None, out.ctypes.data) == -1
    dead = np.zeros(64, np.complex128)
    dead[:10] = 1.0                                                        # 10 live bins cannot carry 16 taps: R is singular
    assert lib.ofdm_chest_matrix(64, 16, dead.ctypes.data, out.ctypes.data) == -1


@pytest.mark.parametrize("n_fft", [64, 1024])
def test_definition_keeps_what_lies_in_the_window_and_nothing_else(orc, n_fft):
    first, lh = cr.window(n_fft)
    assert (first, lh) == (-(n_fft // 16), n_fft // 4)
    trn = orc.default_training(n_fft)
    idx = cr.window_index(n_fft)
    rng = np.random.default_rng(5)
    taps = np.zeros((lh + 4, n_fft), np.complex128)
    taps[np.arange(lh), idx] = 1.0                                         # every unit tap of the window ...
    taps[lh:, idx] = rng.normal(size=(4, lh)) + 1j * rng.normal(size=(4, lh))   # ... and dense channels on it
    H = np.fft.fft(taps, axis=-1)
    err = np.abs(cr.smooth(H, trn, n_fft) - H).max(axis=-1) / np.abs(H).max(axis=-1)
    assert err.max() < 1e-12, err.max()
    # one tap just outside either end of the window, and one half a symbol away: exponentials at other delays are orthogonal to
    # the window's without weights and nearly so with them, so the fit keeps only a fraction of such a tap
    for d in (first - 1, first + lh, n_fft // 2):
        t = np.zeros(n_fft, np.complex128)
        t[d % n_fft] = 1.0
        H = np.fft.fft(t)
        left = np.linalg.norm(cr.smooth(H, trn, n_fft) - H) / np.linalg.norm(H)
        assert left > 0.5, (d, left)


@pytest.mark.parametrize("n_fft,snr_db", cc.WORTH)
def test_denoised_estimate_is_worth_it_on_the_oracle(orc, n_fft, snr_db):
    trn = orc.default_training(n_fft)
    m_ls, m_wls, e_ls, e_wls = 0.0, 0.0, 0, 0
    for cap in cc.captures(n_fft, snr_db):
        hs = cr.smooth(cap["h_ls"], trn, n_fft)
        d_ls = np.sum(np.abs(cap["h_ls"] - cap["h_clean"]) ** 2)
        d_wls = np.sum(np.abs(hs - cap["h_clean"]) ** 2)
        assert d_wls < d_ls
        m_ls, m_wls = m_ls + d_ls, m_wls + d_wls
        e_ls += cc.hard_errors(n_fft, cap, cap["h_ls"])
        e_wls += cc.hard_errors(n_fft, cap, hs)
    print(f"n_fft {n_fft} at {snr_db} dB: mean ||H - H0||^2 {m_ls / 6 / n_fft:.4f} -> {m_wls / 6 / n_fft:.4f} ({m_ls / m_wls:.1f}x), hard bit errors {e_ls} -> {e_wls}")
    # even an unweighted projection onto L_h of N dimensions removes all but L_h / N of white noise
    assert m_ls / m_wls >= n_fft / (n_fft // 4)
    assert e_wls < e_ls
