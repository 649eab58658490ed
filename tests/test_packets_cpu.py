"""EXT-13 without a GPU: tests/packets_ref.py -- the definition of ofdm_rx_decode_packets -- held to a literal loop over the oracle on the
captures of scan_ref.CAPTURES, the integer rules of the row geometry on their own, and the surface of the two new entry points on
every layer."""
import inspect
import os
import re

import numpy as np
import pytest

import packets_ref as P
import scan_ref as R
from util import wide

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ofdm_rx_decode_packets", "ofdm_rx_decode_all_long_host"]
BACKOFF, MOD, GUARD = 4, 4, True                      # scan_ref's captures: 16-QAM with guard bands; the default sync_backoff
# name -> the detections of scan(holdoff = shortest frame - W) whose trimmed start is not in front of lo_k: for them "the packet found from
# lo_k" (orc.decode_sc on capture[lo_k:]) and "the packet at d_hat_k" are the same samples.  Every detection but a frame that follows its
# predecessor by less than the holdoff's slack qualifies; which do is a property of the captures, asserted below.
LOOP_CASES = {"n64_a": (0, 1, 2, 3, 4, 5, 6), "n64_a_cut6": (0, 1, 2, 3, 4, 5, 6), "n64_b": (0, 1, 2, 3, 4, 5), "n256": (0, 1, 2, 3, 4, 5)}


def scanned(orc, name):
    """-> (Built, Scan) of a capture of scan_ref.CAPTURES; name + "_cut6": the capture less its first 6 samples (packets_ref.cut6)"""
    b = P.built(orc, name)
    s = R.scan(orc, b.x, b.L, R.REPS, R.THRESHOLD, min(b.frame_samples) - b.W, 10 ** 6, sums=b.sums)
    return b, s


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_ref_is_the_loop_over_the_oracle(orc, name):
    b, s = scanned(orc, name)
    Dk = P.CASES[name]
    n, bps = len(b.x), (48 * (b.n_fft // 64)) * MOD // 8
    assert R.certified(b.x, b.L, b.W, R.THRESHOLD, b.sums)
    assert len(s.d_hat) == len(b.frame_samples)
    R_row = P.row_samples(n, b.S, Dk)
    assert R_row % 2 == 0 and R_row == (10 + Dk) * b.S + 2
    held = []
    for k, (lo, d, fd, m) in enumerate(zip(s.lo, s.d_hat, s.f_delta, s.metric)):
        g = P.geometry(n, b.S, BACKOFF, d, Dk)
        off = max(d - b.S - BACKOFF, 0)                                        # the trimmed start in the capture
        assert g.r == off & ~1 and g.r % 2 == 0 and 0 <= off - g.r <= 1 and g.d_rel == d - g.r and g.row_len == min(R_row, n - g.r)
        assert P.row_rule_is_length_rule(n, b.S, BACKOFF, d, Dk, bps), (name, k)
        got = P.packet(orc, b.x, d, fd, m, b.n_fft, GUARD, MOD, Dk, BACKOFF)
        assert got["offset"] == off and got["f_delta"] == fd and got["metric"] == np.float32(m)
        if off < lo:
            continue
        held.append(k)
        # the literal loop: the packet found from lo_k by the oracle's own search ...
        w = orc.decode_sc(wide(b.x[lo:]), GUARD, MOD, b.n_fft, threshold=R.THRESHOLD, backoff=BACKOFF, max_symbols=Dk)
        assert (w["status"], lo + w["offset"], w["f_delta"]) == (got["status"], got["offset"], got["f_delta"]), (name, k, w["status"], got["status"])
        assert w["bytes"] == got["bytes"] and len(w["bytes"]) == got["len"], (name, k)
        # ... and the same given the scan's timing on the row's sub-capture
        w = orc.decode_given(wide(b.x[g.r:]), off - g.r, fd, GUARD, MOD, b.n_fft, max_symbols=Dk)
        assert (w["status"], len(w["bytes"]), w["bytes"]) == (got["status"], got["len"], got["bytes"]), (name, k)
    assert tuple(held) == LOOP_CASES[name], (name, held)
    # What the GPU tests count on.  The frame at sample 0: the channel's delay puts its trimmed start 5 samples in, so the rule's clamp
    # max(., 0) is at work only in the capture cut by 6 samples (peak 83 < L + b).  The last frame is cut by the capture's end.
    first, last = (P.packet(orc, b.x, s.d_hat[k], s.f_delta[k], s.metric[k], b.n_fft, GUARD, MOD, Dk, BACKOFF) for k in (0, -1))
    assert P.first_is_clamped(b, s.d_hat, BACKOFF) == name.endswith("_cut6"), (name, s.d_hat[0])
    assert first["offset"] == (0 if name.endswith("_cut6") else 5) and first["status"] == 0
    assert P.last_is_cut(b, last), (name, last["status"], last["ns"])


def test_prepare_and_geometry_rules():
    S, b = 80, 4
    # FRAME_SHORT below 10 L behind the trimmed start; then no data symbol; 16 bytes need ceil(16 / bps) symbols
    assert P.prepare(10 * S - 1, 0, S, b, 8, 24) == (P.FRAME_SHORT, 0, 0)
    assert P.prepare(10 * S, 0, S, b, 8, 24) == (P.FRAME_NODATA, 0, 0)
    assert P.prepare(10 * S + 1, 0, S, b, 8, 24) == (P.FRAME_OK, 0, 1)
    assert P.prepare(10 * S + 1, 0, S, b, 8, 6) == (P.FRAME_NODATA, 0, 0) and P.prepare(12 * S + 1, 0, S, b, 8, 6) == (P.FRAME_OK, 0, 3)
    assert P.prepare(10 ** 6, 85, S, b, 8, 24) == (P.FRAME_OK, 1, 8) and P.prepare(10 ** 6, 84, S, b, 8, 24).off == 0
    assert P.prepare(10 * S + 84, 85 + 84, S, b, 8, 24) == (P.FRAME_SHORT, 85, 0) and P.prepare(11 * S + 85, 85 + 84, S, b, 8, 24) == (P.FRAME_OK, 85, 1)
    # rows: even starts, the clamp at sample 0, R capped by a short capture (rounded up to even), len_k at the capture's end
    assert P.geometry(10 ** 5, S, b, 50, 8) == (0, 50, 10 ** 5, 18 * S + 2)
    assert P.geometry(10 ** 5, S, b, 84 + 1001, 8) == (1000, 85, 99_000, 18 * S + 2)
    assert P.geometry(10 ** 5, S, b, 84 + 1000, 8).r == 1000 and P.geometry(10 ** 5, S, b, 84 + 1002, 8).r == 1002
    assert P.row_samples(1001, S, 8) == 1002 and P.row_samples(1000, S, 8) == 1000 and P.row_samples(18 * S + 2, S, 8) == 18 * S + 2
    assert P.geometry(10 ** 5, S, b, 10 ** 5 - 1, 8) == (10 ** 5 - 86, 85, 86, 86)
    for n in (1441, 1442, 3001, 10 ** 5):              # the cut at R never changes the timing fields, for any peak and either parity
        for d in list(range(0, 200)) + list(range(n - 1700, n)):
            if 0 <= d < n:
                assert P.row_rule_is_length_rule(n, S, b, d, 8, 24), (n, d)
                assert P.row_rule_is_length_rule(n, S, b, d, 1, 6), (n, d)
    assert P.cfo_through(-0.01, P.CFO_OFF) == 0.0 and P.cfo_through(-0.01, P.CFO_ABS) == 0.01 and P.cfo_through(-0.01, P.CFO_SIGNED) == -0.01


def test_the_two_entry_points_are_declared_on_every_layer(ofdm):
    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "ofdm_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ofdm_host.hpp")).read()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in ofdm.SIGNATURES, name
        assert re.search(r"pub fn %s\s*\(" % name, rs), name
    assert "ofdm_rx_decode_packets" in hpp and "decode_packets(" in hpp and "bool batched" in hpp
    assert "#define OFDM_HIP_ABI_VERSION 1" in hdr                                  # entry points were added, nothing changed
    from ofdm_amd import api, build

    for m in ("decode_packets", "decode_all_host"):
        assert callable(getattr(api.Context, m)), m
    sig = inspect.signature(api.decode_all)
    assert sig.parameters["batched"].default is False
    assert "kernels_packets.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "ofdm_amd", "csrc", "kernels_packets.hip"))
    priv = open(os.path.join(ROOT, "ofdm_amd", "csrc", "ofdm_hip_tuning.h")).read()
    assert 'OFDM_TUNE_KEY("packets_chunk_rows", packets_chunk_rows, false)' in priv and "packets_chunk_rows" not in hdr


def test_argument_checks_that_need_no_device(ofdm):
    lib = ofdm.load()
    assert lib.ofdm_rx_decode_packets(None, None, 1000, 0, None, None, None, 8, None, 64, None, None, None, None, None) == -1
    assert lib.ofdm_rx_decode_all_long_host(None, None, 1000, 0, 0, 1, 4, 8, None, 64, None, None, None, None, None, None, None, None, None) == -1
    from ofdm_amd import api

    with pytest.raises(api.OfdmError):                 # before any context is made
        api.decode_all(np.zeros(4000, np.complex64), True, api.QAM16, batched=True)
