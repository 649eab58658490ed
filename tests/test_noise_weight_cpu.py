"""CPU checks of EXT-11, noise-aware LLR weights: the properties of the definition (tests/noise_weight_ref.py), the host-side surface
(setter / getter, header, ctypes table and Rust text), and the link experiment that shows why the rule exists -- the f64 oracle's
frames with a tone on top, LLRs and verdicts from the numpy definitions of the stages.  No kernel is launched here; the kernels are held
to noise_weight_ref in tests/test_gpu_noise_weight.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldpc_ref  # noqa: E402
import noise_weight_ref as nw  # noqa: E402
import quality_ref  # noqa: E402
import soft_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofdm_rx_noise_bins_batch", "ofdm_rx_llr_weighted_batch", "ofdm_set_llr_weight", "ofdm_get_llr_weight")


def _frames(rng, n, F, noise, fd=None):
    """F captures of five identical training blocks (and whatever else: random samples) + noise, the frame 11 samples in"""
    S = n + n // 4
    x = rng.normal(size=(F, 11 + 12 * S)) + 1j * rng.normal(size=(F, 11 + 12 * S))
    blk = rng.normal(size=(F, S)) + 1j * rng.normal(size=(F, S))
    for b in range(5, 10):
        x[:, 11 + b * S:11 + (b + 1) * S] = blk
    if fd is not None:
        x = x * np.exp(1j * np.asarray(fd)[:, None] * (np.arange(x.shape[1]) - 11))
    return x + noise * (rng.normal(size=x.shape) + 1j * rng.normal(size=x.shape))


# ---------------------------------------------------------------------------------------------------------- the definition's properties
@pytest.mark.parametrize("n", [64, 256])
def test_mean_of_the_bins_is_link_quality_noise_var(n):
    rng = np.random.default_rng(n)
    fd = rng.uniform(-0.01, 0.01, 6)
    x = _frames(rng, n, 6, 0.1, fd)
    x[2, 200] += 5.0                                             # one sample of one training block knocked out
    off = np.full(6, 11)
    trn = rng.normal(size=n) + 1j * rng.normal(size=n)
    s, q = nw.noise_bins(x, n, off, fd)
    rows = quality_ref.quality(x, n, True, 6, trn, offset=off, f_delta=fd)
    np.testing.assert_allclose(s.mean(axis=1), rows[:, quality_ref.Q_NOISE_VAR], rtol=1e-12)
    assert (s > 0).all() and (q >= 0).all() and (q <= 1).all()
    assert ((q == 1) == (s <= s.mean(axis=1, keepdims=True))).all() and (q < 1).any()


def test_noiseless_and_untested_frames_get_all_ones():
    rng = np.random.default_rng(3)
    n, S = 64, 80
    x = _frames(rng, n, 4, 0.05)
    x[0] = _frames(rng, n, 1, 0.0)[0]                            # noiseless: five identical blocks
    off = np.array([11, 11, 11, -1])                             # frame 3: a negative offset
    status = np.array([0, -2, 0, 0])                             # frame 1: no sync
    s, q = nw.noise_bins(x, n, off, None, status, frame_len=11 + 10 * S)
    assert (q[[0, 1, 3]] == 1).all() and (s[[1, 3]] == 0).all() and s[0].max() < 1e-25
    assert (q[2] < 1).any()
    s, q = nw.noise_bins(x, n, off, None, status, frame_len=11 + 10 * S - 1)   # the fifth block cut by one sample: nobody is tested
    assert (q == 1).all() and (s == 0).all()
    # NaN compares false; an infinite bin weighs 0 only against a finite mean, which a mean that includes it is not
    assert list(nw.weights_of([1.0, np.nan, 1.0, 1.0])) == [1.0] * 4
    assert list(nw.weights_of([1.0, 1.0, 1.0, 9.0])) == [1.0, 1.0, 1.0, 3.0 / 9.0]


@pytest.mark.parametrize("gain", [2.0 ** 20, 2.0 ** -20, -1.0])
def test_weights_do_not_depend_on_the_gain(gain):
    rng = np.random.default_rng(8)
    x = _frames(rng, 128, 3, 0.2)
    off = np.full(3, 11)
    s, q = nw.noise_bins(x, 128, off)
    sg, qg = nw.noise_bins(gain * x, 128, off)
    assert np.array_equal(q, qg) and np.array_equal(sg, s * gain * gain)


# ---------------------------------------------------------------------------------------------------------- the surface
def _header():
    txt = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    return txt, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_ctypes_and_rust_agree_on_the_new_functions():
    import ofdm_amd

    full, code = _header()
    assert "noise-aware LLR weights (EXT-11)" in full
    assert re.search(r"enum\s*\{\s*OFDM_LLRW_CHANNEL\s*=\s*0\s*,\s*OFDM_LLRW_NOISE\s*=\s*1\s*\}", code)
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    api_txt = open(os.path.join(ROOT, "ofdm_amd", "api.py")).read()
    for name in NEW:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert decl, name
        n_args = len([a for a in decl.group(1).split(",") if a.strip()])
        assert name in ofdm_amd.SIGNATURES and len(ofdm_amd.SIGNATURES[name][1]) == n_args, name
        rust = re.search(r"pub fn " + name + r"\s*\(([^;]*?)\)\s*->\s*c_int;", rs, flags=re.S)
        assert rust and len([a for a in rust.group(1).split(",") if a.strip()]) == n_args, name
        assert "lib." + name in api_txt, name
    assert "OFDM_LLRW_CHANNEL: i32 = 0" in rs and "OFDM_LLRW_NOISE: i32 = 1" in rs
    from ofdm_amd import api

    assert (api.LLRW_CHANNEL, api.LLRW_NOISE) == (0, 1)


def test_params_did_not_change():
    from ofdm_amd import Params

    assert C.sizeof(Params) == 64 and len(Params().reserved) == 4
    _, code = _header()
    body = re.search(r"typedef struct\s*\{([^{}]*?)\}\s*ofdm_params;", code, flags=re.S).group(1)
    assert "int32_t reserved[4];" in body and "llr" not in body


def test_setter_and_getter(ofdm):
    import torch

    lib = ofdm.load()
    mode = C.c_int32(7)
    assert lib.ofdm_set_llr_weight(None, 0) == -1 and lib.ofdm_get_llr_weight(None, C.byref(mode)) == -1 and mode.value == 7
    assert lib.ofdm_rx_noise_bins_batch(None, None, 0, 0, 100, None, None, None, None, None) == -1
    assert lib.ofdm_rx_llr_weighted_batch(None, None, 0, 0, 100, 0, 1, None, None, None, 0, 1.0, None, 0, None, 0) == -1
    if not torch.cuda.is_available():
        return                                                    # a context needs a device: tests/test_gpu_noise_weight.py goes on from here
    from ofdm_amd import api

    c = api.Context(n_fft=64, modulation=6, guard_bands=True, ecc=api.ECC_LDPC648)
    assert c.get_llr_weight() == 0
    assert lib.ofdm_set_llr_weight(c.h, 2) == -1 and lib.ofdm_set_llr_weight(c.h, -1) == -1 and c.get_llr_weight() == 0
    c.set_llr_weight(api.LLRW_NOISE)
    assert c.get_llr_weight() == 1
    assert lib.ofdm_set_llr_weight(c.h, 2) == -1 and c.get_llr_weight() == 1
    assert lib.ofdm_get_llr_weight(c.h, None) == -1
    assert api.Context(n_fft=64, llr_weight=api.LLRW_NOISE).get_llr_weight() == 1


# ---------------------------------------------------------------------------------------------------------- the link experiment
def _delivered(orc, snr_db, isr_db, frames, seed0, payload=560, n=64, mod=6):
    """per frame (unweighted whole?, weighted whole?) on the f64 definitions of every stage"""
    S, cp = n + n // 4, n // 4
    trn = orc.default_training(n)
    bins = soft_ref.data_bins(orc, n, True)
    nd = bins.size
    D = -(-8 * (16 + len(ldpc_ref.stream(bytes(payload)))) // (nd * mod))
    body = D * nd * mod // 8 - 16
    rng = np.random.default_rng(seed0)
    out = []
    for f in range(frames):
        pay = bytes(rng.integers(0, 256, payload, dtype=np.uint8))
        rx = nw.tone_capture(orc, ldpc_ref.stream(pay), snr_db, seed0 + f, isr_db, n=n, mod=mod)
        w = orc.decode_sc(rx, True, mod, n, cfo_off=True, want_soft=True, max_symbols=D)
        if w["status"] != 0 or w["n_symbols"] != D:
            out.append((False, False))
            continue
        off = w["offset"]
        H = np.fft.fft(rx[off + 5 * S:off + 10 * S].reshape(5, S)[:, cp:].mean(axis=0)) / trn
        wk = soft_ref.channel_weights(H[None], bins)
        _, q = nw.noise_bins(rx[None], n, [off])
        got = []
        for weights in (wk, wk * q[:, bins]):
            L = soft_ref.frame_llrs(w["soft"].reshape(1, D, nd), mod, 32.0, weights)[0]
            st, data = ldpc_ref.receive(L[128:], body)
            got.append(bool(st == 0 and data == pay))
        out.append(tuple(got))
    return out


def test_the_rule_earns_its_keep_on_the_definitions(orc):
    """N = 64, 64-QAM, guard bands, LDPC648, 560-byte payloads, 16 frames (seeds fixed here).  At 14 dB with a tone 10 dB under the
    frame on bin 11.3 the weighted LLRs deliver at least 12 of 16 frames whole and today's weights at most 4; at 8 dB without a tone
    both deliver the same frames.  Counts with these seeds: weighted 16 / 16 against 0 / 16 under the tone; 16 / 16 both without."""
    tone = _delivered(orc, 14.0, -10.0, 16, 4100)
    plain, weighted = sum(a for a, _ in tone), sum(b for _, b in tone)
    print(f"14 dB, tone -10 dB at bin 11.3: unweighted {plain} / 16, weighted {weighted} / 16")
    assert weighted >= 12 and plain <= 4
    clean = _delivered(orc, 8.0, None, 16, 4200)
    print(f"8 dB, no tone: unweighted {sum(a for a, _ in clean)} / 16, weighted {sum(b for _, b in clean)} / 16")
    assert all(a == b for a, b in clean) and sum(a for a, _ in clean) >= 12
