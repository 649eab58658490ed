"""The holdoff scan of ofdm_sc_scan_long (include/ofdm_hip.h, "every packet of one long capture") in numpy f64 plus the oracle, shared by
tests/test_scan_cpu.py and tests/test_gpu_scan.py.

Notation as oracle/ofdm_oracle.c: L = S, W = reps L, num = |P|^2, den = E R, valid = n - W - L + 1.

    lo_0 = lag_lo
    detection k:  d1_k = the first lag d in [lo_k, lag_hi) with den(d) > 0 and num(d) >= thr den(d)        (none: the scan ends)
                  d_hat_k, f_delta_k, M_k = orc.sc_sync(capture[lo_k:]) re-based by lo_k
    lo_{k+1} = d1_k + holdoff
    the scan ends after max_det detections; more = a further detection exists

  * lag_sums: per-lag num / den by direct window sums (numpy adds a window pairwise, the oracle and the kernels in order: the two agree
    to a few ulp, which is why a case must be CERTIFIED before anything is compared with it);
  * scan: the rule above.  d1 comes from lag_sums, the peak from the oracle;
  * certify: every lag's |num - thr den| exceeds 1e-9 den and, for every lag that crosses (any of them can become a d1 under some
    holdoff or lag_lo), the peak of its window leads the runner-up by more than 1e-9: no summation order can change a decision.  A lag
    whose windows are all zeros has num = den = 0 exactly in any order and decides "no crossing" without a margin.  A case that fails
    certification is a broken test;
  * pack_bits / walk_words / walk_lags: the bitmap k_sc_mark writes (bit j of word j >> 6, LSB first) and k_sc_walk's rule on it, stepped
    as the kernel steps (64 words at a time), against the rule on plain lags;
  * CAPTURES / build_capture: the seeded captures of the GPU tests.
"""
import functools
from collections import namedtuple

import numpy as np

from util import through_channel, wide

CERT_THR, CERT_PEAK = 1e-9, 1e-9


def lag_sums(x32, L, W):
    """(num, den) at every valid lag of the capture: f64, direct sums over each lag's own window"""
    x = wide(x32)
    valid = x.size - W - L + 1
    if valid <= 0:
        return np.zeros(0), np.zeros(0)
    q = np.conj(x[:-L]) * x[L:]
    e = x.real ** 2 + x.imag ** 2
    win = np.lib.stride_tricks.sliding_window_view
    P = win(q, W)[:valid].sum(axis=1)
    E = win(e, W)[:valid].sum(axis=1)
    R = win(e[L:], W)[:valid].sum(axis=1)
    return P.real ** 2 + P.imag ** 2, E * R


def crossings(num, den, thr):
    return (den > 0.0) & (num >= thr * den)


def lag_range(n, L, W, lag_lo, lag_hi):
    valid = n - W - L + 1
    hi = valid if (lag_hi <= 0 or lag_hi > valid) else lag_hi
    return valid, max(lag_lo, 0), hi


def walk_lags(cross, lo, hi, holdoff, max_det):
    """The rule on a boolean array over lags -> (d1 list, more)"""
    d1, pos = [], lo
    while pos < hi:
        nz = np.nonzero(cross[pos:hi])[0]
        if nz.size == 0:
            break
        if len(d1) == max_det:
            return d1, True
        d1.append(pos + int(nz[0]))
        pos = d1[-1] + holdoff
    return d1, False


def pack_bits(flags):
    """bool[n] -> uint64 words, bit j in word j >> 6 at position j & 63; the last word's spare bits are zero"""
    n = len(flags)
    pad = np.zeros(((n + 63) // 64) * 64, np.uint8)
    pad[:n] = np.asarray(flags, np.uint8)
    return np.packbits(pad.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)


def _ctz(v):
    return (int(v) & -int(v)).bit_length() - 1


def walk_words(words, n_bits, holdoff, max_det):
    """k_sc_walk on the packed bitmap, in its own steps: 64 words are looked at together, the first non-zero one (after the bits below
    `pos` are masked off) gives the detection; the 64 words are kept while the next start lies inside them.  -> (bit indices, more)"""
    words = [int(w) for w in words]
    out, pos = [], 0
    while pos < n_bits:
        base = pos >> 6
        held = [words[i] if i < len(words) else 0 for i in range(base, base + 64)]
        end = (base + 64) << 6
        while pos < end and pos < n_bits:
            pw = pos >> 6
            v = [0 if base + i < pw else (w & ~((1 << (pos & 63)) - 1) if base + i == pw else w) for i, w in enumerate(held)]
            first = next((i for i, w in enumerate(v) if w), None)
            if first is None:
                pos = end
                break
            d = ((base + first) << 6) + _ctz(v[first])
            if len(out) == max_det:
                return out, True
            out.append(d)
            pos = d + holdoff
    return out, False


Scan = namedtuple("Scan", "lo d1 d_hat f_delta metric more")


def scan(orc, x32, L, reps, thr, holdoff, max_det, lag_lo=0, lag_hi=0, sums=None):
    """The definition.  sums: lag_sums(x32, L, W) if the caller has them already."""
    W = reps * L
    valid, lo, hi = lag_range(len(x32), L, W, lag_lo, lag_hi)
    if valid <= 0 or lo >= hi:
        return Scan([], [], [], [], [], False)
    num, den = lag_sums(x32, L, W) if sums is None else sums
    d1, more = walk_lags(crossings(num, den, thr), lo, hi, holdoff, max_det)
    x = wide(x32)
    los, dh, fd, m = [], [], [], []
    for k, d in enumerate(d1):
        lo_k = lo if k == 0 else d1[k - 1] + holdoff
        od, _, om, ofd = orc.sc_sync(x[lo_k:], L, reps, 0, thr)
        assert d <= lo_k + od <= min(d + W, valid - 1), (k, d, lo_k + od)      # the oracle crossed at d1_k too
        los.append(lo_k); dh.append(lo_k + od); fd.append(ofd); m.append(om)
    return Scan(los, d1, dh, fd, m, more)


def certify(x32, L, W, thr, sums=None):
    """-> (smallest |num - thr den| / den over the lags with den > 0, smallest lead of a window's peak over its runner-up among the windows
    of every crossing lag); the case is certified when the first exceeds CERT_THR and the second CERT_PEAK"""
    num, den = lag_sums(x32, L, W) if sums is None else sums
    live = den > 0.0
    assert np.all(num[~live] == 0.0)
    margin = float(np.min(np.abs(num[live] - thr * den[live]) / den[live])) if live.any() else np.inf
    M = np.where(live, num / np.where(live, den, 1.0), 0.0)
    lead = np.inf
    for d in np.nonzero(crossings(num, den, thr))[0]:
        w = M[d: min(d + W, M.size - 1) + 1]
        if w.size > 1:
            top = np.partition(w, -2)[-2:]
            lead = min(lead, float(top[1] - top[0]))
    return margin, lead


def certified(x32, L, W, thr, sums=None):
    margin, lead = certify(x32, L, W, thr, sums)
    return margin > CERT_THR and lead > CERT_PEAK


# ---------------------------------------------------------------- the captures of the GPU tests
# name -> n_fft, samples, seed, frames (start, payload bytes); 16-QAM with guard bands at 15 dB, every frame with its own CFO.  Each has
# a frame at sample 0, a gap shorter than W between two frames, unequal gaps, two frame lengths and a last frame cut by the capture's
# end.  WORD_EDGE names two consecutive detections (at the holdoff given) whose first crossings are 1 apart modulo 64: a lag_lo that
# puts the first on bit 63 of a bitmap word puts the second on bit 0 of a later one.  tests/test_scan_cpu.py asserts all of it.
Capture = namedtuple("Capture", "n_fft samples seed frames")
CAPTURES = {
    "n64_a": Capture(64, 40_000, 6401, ((0, 200), (1750, 560), (9000, 200), (10_800, 560), (21_037, 200), (29_999, 560), (38_900, 560))),
    "n64_b": Capture(64, 39_000, 6402, ((0, 560), (2900, 200), (8121, 560), (19_002, 200), (27_500, 560), (37_300, 560))),
    "n256": Capture(256, 60_000, 25601, ((0, 300), (5300, 1400), (20_000, 300), (31_009, 1400), (46_001, 300), (57_000, 1400))),
}
SNR_DB, THRESHOLD, REPS = 15.0, 0.5, 3
WORD_EDGE = {"n64_a": 4, "n64_b": 2, "n256": 2}   # k: detections k and k + 1 of scan(holdoff = shortest frame - W, lag_lo = 0)
Built = namedtuple("Built", "name n_fft S L W x payloads frame_samples sums")


@functools.lru_cache(maxsize=None)
def build_capture(orc, name):
    """-> Built: the capture as complex64, the payloads sent, the frames' sizes in samples, lag_sums of the capture"""
    c = CAPTURES[name]
    rng = np.random.default_rng(c.seed)
    S = c.n_fft + c.n_fft // 4
    cap = np.zeros(c.samples, np.complex128)
    pays, sizes, sigma = [], [], None
    for st, nbytes in c.frames:
        pay = bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))
        tx = orc.encode(pay, True, orc.QAM16, c.n_fft)
        fd = (rng.random() * 1.8 - 0.9) * np.pi / S
        seg = wide(through_channel(orc, rng, tx, tx.size + 64, 0, fd, snr_db=None, data_start=10 * S))
        k = max(0, min(seg.size, c.samples - st))
        cap[st: st + k] += seg[:k]
        if sigma is None:
            sigma = np.sqrt(float(np.mean(np.abs(tx[10 * S:]) ** 2)) / 10 ** (SNR_DB / 10) / 2)
        pays.append(pay); sizes.append(tx.size)
    cap += sigma * (rng.standard_normal(c.samples) + 1j * rng.standard_normal(c.samples))
    x = cap.astype(np.complex64)
    return Built(name, c.n_fft, S, S, REPS * S, x, pays, sizes, lag_sums(x, S, REPS * S))


def noise_capture(n, seed=77):
    rng = np.random.default_rng(seed)
    return (0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
