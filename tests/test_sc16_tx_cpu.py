"""EXT-10 without a GPU: the surface of the sc16 transmit output and the sc16 long-capture calls on every layer, the argument checks
they make before they touch a device, and the fact about normalize the GPU clipping cases rest on, restated on the f64 oracle alone."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ofdm_tx_encode_sc16_batch", "ofdm_tx_encode_sc16_host", "ofdm_rx_decode_long_sc16", "ofdm_rx_decode_long_sc16_host"]


@pytest.fixture(scope="module")
def lib(ofdm):
    return ofdm.load()


def test_the_surface_is_on_every_layer(ofdm):
    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ofdm_host.hpp")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in ofdm.SIGNATURES, n
        assert re.search(r"pub fn %s\s*\(" % n, rs), n
    for n in ("ofdm_tx_encode_sc16_host", "ofdm_rx_decode_long_sc16_host", "encode_sc16", "decode_capture_sc16"):
        assert n in hpp, n
    from ofdm_amd import api, build

    for m in ("encode_batch_sc16", "encode_host_sc16", "decode_long_sc16", "decode_long_host_sc16"):
        assert callable(getattr(api.Context, m)), m
    assert "kernels_n64_tx_sc16.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "ofdm_amd", "csrc", "kernels_n64_tx_sc16.hip"))
    # the header states the signed-maximum fact and what the count is for
    doc = hdr[hdr.index("sc16 transmit output"):hdr.index("int ofdm_tx_encode_sc16_batch(")]
    assert "SIGNED maximum" in doc and "clipped_dev" in doc and "scale is too large" in doc
    tool = open(os.path.join(ROOT, "tools", "ofdm_loopback.cpp")).read()
    assert "encode_sc16" in tool and "decode_sc16" in tool and "normalised to a peak of 1" not in tool


def test_the_new_laboratory_key_is_private_and_described():
    priv = open(os.path.join(ROOT, "ofdm_amd", "csrc", "ofdm_hip_tuning.h")).read()
    assert 'OFDM_TUNE_KEY("no_txframe64_sc16", no_txframe64_sc16, false)' in priv
    comment = priv[: priv.index("#ifndef OFDM_TUNE_KEY")]
    assert "no_txframe64_sc16" in comment and "ofdm_tx_encode_sc16_batch's two-pass path" in comment   # sc16_chunk_frames says so
    assert "no_txframe64_sc16" not in open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()


def test_null_context_is_invalid_on_all_four(lib):
    s = 12000.0
    assert lib.ofdm_tx_encode_sc16_batch(None, None, 1, 8, None, 8, s, None, 1600, None) == -1
    assert lib.ofdm_tx_encode_sc16_host(None, None, 1, 8, None, 8, s, None, 1600, None, 0) == -1
    assert lib.ofdm_rx_decode_long_sc16(None, None, 2000, s, 0, 0, -1, 8, None, 64, None, None, None, None, None) == -1
    assert lib.ofdm_rx_decode_long_sc16_host(None, None, 2000, s, 8, None, 64, None, None, None, None, None) == -1


def _clips_at_full_scale(x):
    """does a frame of the f64 oracle have a component whose rint(x * 32767) lies below -32767?  (its positive peak is exactly 1)"""
    comp = np.concatenate([x.real, x.imag])
    assert comp.max() == 1.0
    return bool((np.rint(comp * 32767.0) < -32767.0).any()), float(comp.min())


def test_normalize_divides_by_the_signed_maximum(orc):
    """normalize (src/transmitter.rs:183-194) makes the POSITIVE peak 1; the negative peak is whatever it is.  The reference's default
    shape (BPSK, no guard bands) clips at scale 32767 in every frame; 64-QAM with guard bands never does."""
    lows = []
    for seed in range(40):
        pay = bytes(np.random.default_rng(seed).integers(0, 256, 20, dtype=np.uint8))
        clips, low = _clips_at_full_scale(orc.encode(pay, guard=False, modulation=orc.BPSK))
        assert clips, (seed, low)
        lows.append(low)
    assert min(lows) < -1.5
    for seed in range(40):
        pay = bytes(np.random.default_rng(seed).integers(0, 256, 100, dtype=np.uint8))
        clips, low = _clips_at_full_scale(orc.encode(pay, guard=True, modulation=orc.QAM64))
        assert not clips, (seed, low)
