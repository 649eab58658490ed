"""CPU checks of the holdoff scan's definition (tests/scan_ref.py; include/ofdm_hip.h, "every packet of one long capture"): no GPU.

  * scan_ref.scan against a LITERAL loop over the oracle on hand-built captures: d1 from the oracle's own per-lag metric and confirmed by
    two bounded orc.sc_sync searches (one that ends at d1 finds it, one that ends in front of it finds nothing), the peak from
    orc.sc_sync(capture[lo:]);
  * every capture tests/test_gpu_scan.py uses is certified (no summation order can change a decision) and has the properties the GPU
    cases rely on;
  * k_sc_walk's rule on the packed bitmap, stepped as the kernel steps, against the rule on plain lags."""
import numpy as np
import pytest

import scan_ref as R
from util import through_channel, wide


def _hand_capture(orc, seed, starts, span, nbytes=8, snr_db=15.0):
    rng = np.random.default_rng(seed)
    cap = np.zeros(span, np.complex128)
    for st in starts:
        tx = orc.encode(bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)), True, orc.QAM16, 64)
        seg = wide(through_channel(orc, rng, tx, tx.size + 64, 0, (rng.random() * 1.8 - 0.9) * np.pi / 80, snr_db=None, data_start=800))
        k = max(0, min(seg.size, span - st))
        cap[st: st + k] += seg[:k]
    sigma = np.sqrt(float(np.mean(np.abs(tx[800:]) ** 2)) / 10 ** (snr_db / 10) / 2)
    return (cap + sigma * (rng.standard_normal(span) + 1j * rng.standard_normal(span))).astype(np.complex64)


def _oracle_loop(orc, x32, L, reps, thr, holdoff, max_det, lag_lo, lag_hi):
    """the rule as a loop over the oracle alone"""
    W = reps * L
    x = wide(x32)
    valid, lo, hi = R.lag_range(x.size, L, W, lag_lo, lag_hi)
    out = []
    if valid <= 0:
        return out, False
    m = orc.sc_metric(x, L, reps)[0]
    while lo < hi:
        at = np.nonzero(m[lo:hi] >= thr)[0]
        if at.size == 0:
            break
        d1 = lo + int(at[0])
        assert orc.sc_sync(x[lo:], L, reps, d1 - lo + 1, thr)[0] == d1 - lo          # a search that ends at d1 finds it ...
        assert d1 == lo or orc.sc_sync(x[lo:], L, reps, d1 - lo, thr)[0] == -1       # ... one that ends in front of it finds nothing
        if len(out) == max_det:
            return out, True
        d, _, metric, fd = orc.sc_sync(x[lo:], L, reps, 0, thr)
        out.append((lo, d1, lo + d, fd, metric))
        lo = d1 + holdoff
    return out, False


HAND = (("three short frames", 11, (0, 1000, 2300), 4000), ("two frames, the second cut by the end", 12, (150, 3300), 3900),
        ("back to back", 13, (40, 40 + 880 + 64), 2600))


@pytest.mark.parametrize("what,seed,starts,span", HAND)
def test_ref_is_the_loop_over_the_oracle(orc, what, seed, starts, span):
    x = _hand_capture(orc, seed, starts, span)
    L, W = 80, 240
    sums = R.lag_sums(x, L, W)
    assert R.certified(x, L, W, 0.5, sums), R.certify(x, L, W, 0.5, sums)
    total = len(R.scan(orc, x, L, 3, 0.5, 640, 10 ** 6, sums=sums).d1)
    assert total >= len(starts)
    plateau = R.scan(orc, x, L, 3, 0.5, 640, 1, sums=sums).d1[0] + 20               # a lag_lo inside the first plateau
    for holdoff, lag_lo, lag_hi in ((1, 0, 600), (1, plateau, plateau + 300), (W, 0, 0), (640, 0, 0), (640, plateau, 0), (640, 7, starts[-1] + 20),
                                    (span + 9, 0, 0), (100, 0, starts[-1] + 60)):
        count = len(R.scan(orc, x, L, 3, 0.5, holdoff, 10 ** 6, lag_lo, lag_hi, sums).d1)
        for max_det in (0, 1, count, count + 3):
            got = R.scan(orc, x, L, 3, 0.5, holdoff, max_det, lag_lo, lag_hi, sums)
            want, more = _oracle_loop(orc, x, L, 3, 0.5, holdoff, max_det, lag_lo, lag_hi)
            assert (list(zip(got.lo, got.d1, got.d_hat, got.f_delta, got.metric)), got.more) == (want, more), (what, holdoff, lag_lo, lag_hi, max_det)
            assert got.more == (max_det < count)


def test_ref_on_captures_without_a_detection(orc):
    noise = R.noise_capture(3000)
    assert R.scan(orc, noise, 80, 3, 0.5, 1, 5).d1 == [] and R.certified(noise, 80, 240, 0.5)
    short = R.noise_capture(80 + 240 - 1)           # one sample short of a single lag
    got = R.scan(orc, short, 80, 3, 0.5, 1, 5)
    assert got.d1 == [] and not got.more
    assert R.scan(orc, R.noise_capture(320), 80, 3, 0.5, 1, 5).d1 == []     # exactly one lag, no crossing


@pytest.mark.parametrize("name", sorted(R.CAPTURES))
def test_gpu_captures_are_certified_and_have_their_properties(orc, name):
    b = R.build_capture(orc, name)
    c = R.CAPTURES[name]
    margin, lead = R.certify(b.x, b.L, b.W, R.THRESHOLD, b.sums)
    print(f"{name}: smallest |num - thr den| / den = {margin:.3g}, smallest peak lead = {lead:.3g}")
    assert margin > R.CERT_THR and lead > R.CERT_PEAK, (name, margin, lead)
    starts = [st for st, _ in c.frames]
    ends = [st + n for st, n in zip(starts, b.frame_samples)]
    assert starts[0] == 0 and ends[-1] > c.samples and len(set(b.frame_samples)) == 2 and 5 <= len(starts) <= 7
    gaps = [s - e for s, e in zip(starts[1:], ends[:-1])]
    assert min(gaps) > 0 and min(gaps) < b.W and len(set(gaps)) == len(gaps)
    holdoff = min(b.frame_samples) - b.W
    s = R.scan(orc, b.x, b.L, R.REPS, R.THRESHOLD, holdoff, 10 ** 6, sums=b.sums)
    assert len(s.d1) == len(starts)                                   # one detection a frame at the real frame size
    assert all(0 <= d - st < b.L for d, st in zip(s.d1, starts))
    k = R.WORD_EDGE[name]
    assert (s.d1[k + 1] - s.d1[k]) % 64 == 1                          # lag_lo = d1[k] - 63: bits 63 and 0 of two bitmap words
    assert s.d1[k] - 63 > s.d1[k - 1] + b.W                           # and that lag_lo lies behind the previous frame's plateaus


def test_walk_on_synthetic_bitmaps():
    rng = np.random.default_rng(5)
    for n_bits, density in ((1, 1.0), (63, 0.5), (64, 0.02), (65, 0.02), (4096, 0.001), (4097, 0.3), (9000, 0.002), (20_000, 0.0005), (5000, 0.0)):
        flags = rng.random(n_bits) < density
        if n_bits == 9000:
            flags[[63, 64, 4095, 4096, 8191, 8192, 8999]] = True      # word edges, edges of the 64-word step, the last bit
        words = R.pack_bits(flags)
        assert words.size == (n_bits + 63) // 64
        for holdoff in (1, 7, 64, 100, 4096, 5000, n_bits + 1):
            count = len(R.walk_lags(flags, 0, n_bits, holdoff, 10 ** 9)[0])
            for max_det in (0, 1, count, count + 3):
                got = R.walk_words(words, n_bits, holdoff, max_det)
                assert got == R.walk_lags(flags, 0, n_bits, holdoff, max_det), (n_bits, density, holdoff, max_det)
                assert got[1] == (max_det < count)


def test_bindings_mirror_the_scan():
    """api.decode_all / Context.sc_scan_long exist with the documented arguments (nothing is launched)"""
    import inspect

    from ofdm_amd import api

    sig = inspect.signature(api.decode_all)
    assert sig.parameters["holdoff"].default is None and "max_packets" in sig.parameters
    assert "frame_samples(payload_bytes) - W" in api.decode_all.__doc__
    for name in ("sc_scan_long", "sc_scan_long_host", "default_holdoff"):
        assert hasattr(api.Context, name), name
