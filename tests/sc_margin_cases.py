"""Razor-thin Schmidl-Cox decisions, shared by tests/test_sc_margins_cpu.py and tests/test_gpu_sc_margins.py.

The packet-detect threshold is a context parameter, so ANY lag of ANY capture becomes a close `num >= thr * den` decision when
the threshold is set next to that lag's own metric: thr = M(d_k) (1 + sign eps).  That is the situation the detectors' prefix
differences, slid window sums and f32 / upper-bound filters exist for, and which thresholds on the steep edge of the metric
(0.5, 0.37, 0.81: margins of percent) never produce.

Per period N (S = 5 N / 4, L = S, W = 3 S), seeded:
  * four captures of 14 S samples (2 176 at N = 64): an ordinary one (a frame through the FIR channel with CFO at 30 dB, delay below one period)
    and the same capture behind a 12-sample burst in its first 14 samples, scaled so that the smallest window energy over the
    record lags is 2^-9, 2^-15 and 2^-17 of the capture's total energy (f64 sums, asserted within one octave).  Prefix
    differences lose that many bits; direct sums lose none, and every lag from 14 on has the same windows in all four captures.
    (The amplitudes are solved from the capture's own energies; for an N = 64 capture they come out near 40, 400 and 700.)
  * record lags: d >= 20 with M(d) in (0.1, 0.95) that exceeds every earlier M by a factor of more than 1 + 1e-6 (M from
    orc.sc_metric); six of them spread evenly over that range at N = 64, two at every larger N.
  * a case is (capture, record lag d_k, eps, sign): threshold M(d_k) (1 + sign eps) as a double, eps in {1e-6, 1e-9, eps_min(N)},
    search bounded to n_lags = d_k + W + 64.  1e-6 is where the f32 and upper-bound filters have their slack, 1e-9 is k_sc80's
    documented trust level, eps_min(N) = max(1e-12, 100 x the oracle's own relative error of M(d_k) against exact arithmetic).
    The expected d_hat, f_delta and metric are orc.sc_sync's for that threshold and that n_lags.
  * a case is kept only if the oracle's verdict is unambiguous for reasons the test controls: no lag up to the oracle's crossing
    other than d_k has |M - thr| / thr < 1e-6, and the oracle's peak beats every other lag of its window by more than 1e-9
    relative.  At most 10 % of the cases of any (N, capture) may be dropped.
  * every case is certified by exact arithmetic: P, E, R at d_k as exact sums of exact products of the f32 samples
    (fractions.Fraction), num >= Fraction(thr) * den; the oracle's verdict at the razor lag must be that one.

All four captures of a size share the thresholds (every capture's cases at a threshold are rows of one batch), so a threshold is
one detector call over the batch; `rows` of a Threshold says which rows are unambiguous there and what the oracle answers.

Only d_hat and the peak's CFO and metric leave a detector, and over d_k + W + 64 lags a crossing found one lag late returns the same
peak: that search alone cannot show a wrong decision at the razor lag.  Every threshold therefore carries a second search over
d_k + 1 lags (`razor`), whose answer is the decision itself: d_k, or -1 for nothing found.  A case is kept when both are unambiguous.

Measured (tests/test_sc_margins_cpu.py prints them): the oracle's largest relative error of M(d_k) against exact arithmetic, and
the resulting eps_min.

    N      oracle error   eps_min
    64     2.1e-15        1e-12
    256    4.8e-15        1e-12
    1024   5.1e-15        1e-12
    2048   6.2e-15        1e-12
"""
import functools
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np

from util import fc32, through_channel, wide

SIZES = ((64, False), (256, False), (1024, False), (2048, False), (64, True))       # (N, late)
CAPTURES = ("ordinary", "burst 2^-9", "burst 2^-15", "burst 2^-17")
RATIO_LOG2 = (None, -9.0, -15.0, -17.0)       # smallest window energy / total energy of the burst captures
EPS_FIXED = (1e-6, 1e-9)
EPS_FLOOR, EPS_FACTOR = 1e-12, 100.0          # eps_min(N) = max(EPS_FLOOR, EPS_FACTOR x oracle error)
AMBIGUOUS_THR, AMBIGUOUS_PEAK = 1e-6, 1e-9
MAX_DROP_SHARE = 0.10
BURST = slice(2, 14)
# 6400 + N + 1000 k, the first k for which the detector on plain prefix differences (prefix_detector) gets a case of the 2^-9 burst wrong
# at eps_min: its error there is about eps_min itself, and with two record lags a size has only four such cases (k = 1 at N = 64, 256;
# the late set of N = 64 takes k = 0 as it comes)
SEEDS = {(64, False): 7464, (256, False): 7656, (1024, False): 7424, (2048, False): 8448, (64, True): 6464}
LATE_DELAY = 1000

# a case: capture index, razor lag, eps, sign, threshold, n_lags, kept, exact verdict and the oracle's at the razor lag
Case = namedtuple("Case", "cap d eps sign thr n_lags kept exact_crosses oracle_crosses")
# a threshold: (d, eps, sign) -> thr, n_lags and per row of the batch None (ambiguous there) or orc.sc_sync's (d_hat, P, metric, f_delta):
# `rows` for the search over n_lags lags, `razor` for the search that ends at the razor lag (n_lags = d + 1)
Threshold = namedtuple("Threshold", "d eps sign thr n_lags rows razor")
Size = namedtuple("Size", "n S W caps ratios records metric exact_m oracle_err eps_min cases thresholds")


def record_lags(m):
    """lags d >= 20 with M in (0.1, 0.95) and M > (1 + 1e-6) x every earlier M"""
    before = np.concatenate([[0.0], np.maximum.accumulate(m)[:-1]])
    ok = (m > 0.1) & (m < 0.95) & (m > before * (1.0 + 1e-6)) & (np.arange(m.size) >= 20)
    return np.nonzero(ok)[0]


def pick_evenly(lags, count):
    if len(lags) <= count:
        return [int(d) for d in lags]
    return [int(lags[i]) for i in np.unique(np.round(np.linspace(0, len(lags) - 1, count)).astype(int))]


def exact_sums(row, d, L, W):
    """(|P|^2, E R) at lag d as Fractions: exact sums of exact products of the f32 samples"""
    seg = row[d: d + W + L]
    re = [Fraction(float(v)) for v in seg.real]
    im = [Fraction(float(v)) for v in seg.imag]
    e = sum(re[m] * re[m] + im[m] * im[m] for m in range(W))
    r = sum(re[m] * re[m] + im[m] * im[m] for m in range(L, L + W))
    pr = sum(re[m] * re[m + L] + im[m] * im[m + L] for m in range(W))         # conj(a) b
    pi = sum(re[m] * im[m + L] - im[m] * re[m + L] for m in range(W))
    return pr * pr + pi * pi, e * r


def prefix_detector(row, L, W, n_lags, thr):
    """The oracle's detector on f64 PREFIX DIFFERENCES (np.cumsum; the products of f32 samples are exact in f64): what a streaming
    kernel computes when it takes no further care.  -> d_hat"""
    x = wide(row)
    se = np.concatenate([[0.0], np.cumsum(x.real ** 2 + x.imag ** 2)])
    q = np.conj(x[:-L]) * x[L:]
    sqr = np.concatenate([[0.0], np.cumsum(q.real)])
    sqi = np.concatenate([[0.0], np.cumsum(q.imag)])
    d = np.arange(n_lags)
    e, r = se[d + W] - se[d], se[d + L + W] - se[d + L]
    pr, pi = sqr[d + W] - sqr[d], sqi[d + W] - sqi[d]
    num, den = pr * pr + pi * pi, e * r
    cross = np.nonzero((den > 0.0) & (num >= thr * den))[0]
    if cross.size == 0:
        return -1
    best = int(cross[0])
    for j in range(best + 1, min(best + W, n_lags - 1) + 1):
        if den[j] > 0.0 and num[j] * den[best] > num[best] * den[j]:
            best = j
    return best


def _captures(orc, n, late):
    rng = np.random.default_rng(SEEDS[n, late])
    S = n + n // 4
    W, span = 3 * S, max(14 * S, 2176)       # (N = 64: the one-launch f32 filter k_sc_cf<256> is reached by searches over more than 960 lags)
    tx = orc.encode(bytes(rng.integers(0, 256, 40 * (n // 64), dtype=np.uint8)), True, orc.QAM16, n)
    delay = int(rng.integers(S // 16, S // 4)) + (LATE_DELAY if late else 0)
    fd = float((rng.random() * 1.8 - 0.9) * np.pi / S)
    ordinary = through_channel(orc, rng, tx, span, delay, fd, 30.0, data_start=10 * S)
    m = orc.sc_metric(wide(ordinary), S, 3, delay + S + S // 4 + W + 64)[0]
    records = record_lags(m)
    assert records.size >= 2
    x = wide(ordinary)
    se = np.concatenate([[0.0], np.cumsum(np.abs(x[14:]) ** 2)])                   # from sample 14 on: the same in all four captures
    win = lambda d: se[d - 14 + W] - se[d - 14]
    e_min = min(min(win(int(d)), win(int(d) + S)) for d in records)
    shape = rng.standard_normal(12) + 1j * rng.standard_normal(12)
    caps = [ordinary]
    for lg in RATIO_LOG2[1:]:
        # total = quiet + |x[2:14] + a shape|^2 ~ quiet + a^2 |shape|^2: the amplitude that puts e_min / total at 2^lg
        quiet = float(np.sum(np.abs(x) ** 2))
        a = np.sqrt((e_min / 2.0 ** lg - quiet) / float(np.sum(np.abs(shape) ** 2)))
        y = x.copy()
        y[BURST] += a * shape
        caps.append(fc32(y))
    return S, W, np.stack(caps), m


@functools.lru_cache(maxsize=None)
def build(orc, n, late=False):
    """Everything the margin tests need for period n, computed once per process -> Size.  late (N = 64 only): the same construction with
    the packet LATE_DELAY samples further into the capture, so that the record lags lie beyond the 960 lags a 128-chunk tile of
    k_sc_cf holds and a search that ends at the razor lag is served by k_sc_cf<256>, one launch or two."""
    assert n == 64 or not late
    S, W, caps, m0 = _captures(orc, n, late)
    L = S
    max_lags = caps.shape[1] - W - L + 1
    # every lag from 14 on has the same windows in all four captures: only the first 20 values of M are the burst captures' own
    assert all(np.array_equal(c[14:], caps[0][14:]) for c in caps)
    metric = [m0] + [np.concatenate([orc.sc_metric(wide(c), L, 3, 20)[0], m0[20:]]) for c in caps[1:]]
    records = [pick_evenly(record_lags(m), 6 if n == 64 else 2) for m in metric]
    ratios = []
    for c, m in zip(caps, metric):
        e = np.abs(wide(c)) ** 2
        win = lambda d: float(np.sum(e[d: d + W]))
        ratios.append(min(min(win(int(d)), win(int(d) + L)) for d in record_lags(m)) / float(np.sum(e)))
    # the oracle's error of M(d_k) against exact arithmetic -> eps_min
    exact_m, err = {}, 0.0
    for ci, lags in enumerate(records):
        for d in lags:
            if ci and (0, d) in exact_m:
                exact_m[ci, d] = exact_m[0, d]                    # (the same samples)
                continue
            num, den = exact_sums(caps[ci], d, L, W)
            exact_m[ci, d] = (num, den)
            err = max(err, float(abs(Fraction(float(metric[ci][d])) - num / den) / (num / den)))
    eps_min = max(EPS_FLOOR, EPS_FACTOR * err)
    wcaps = [wide(c) for c in caps]

    @functools.lru_cache(maxsize=None)
    def crosses_at(ci, d, thr):                # the oracle's own decision at lag d alone: the same sums in the same order
        return orc.sc_sync(wcaps[ci][d: d + W + L], L, 3, 1, thr)[0] == 0

    def read_off(ci, d, thr, n_lags):
        """None if the oracle's verdict on capture ci is ambiguous at this threshold, else the d_hat that M shows"""
        m = metric[ci][:n_lags]
        ge = m >= thr
        ge[d] = crosses_at(ci, d, thr)
        cross = np.nonzero(ge)[0]
        d1 = int(cross[0]) if cross.size else -1
        front = np.arange(n_lags) <= (d1 if d1 >= 0 else n_lags)
        front[d] = False
        if np.any(front & (np.abs(m - thr) < AMBIGUOUS_THR * thr)):
            return None
        if d1 < 0:
            return -1
        hi = min(d1 + W, n_lags - 1)
        best = d1 + int(np.argmax(m[d1: hi + 1]))
        others = np.delete(m[d1: hi + 1], best - d1)
        if others.size and m[best] <= others.max() * (1.0 + AMBIGUOUS_PEAK):
            return None
        return best

    keys, jobs = [], []
    for d in sorted({d for lags in records for d in lags}):
        owners = [ci for ci, lags in enumerate(records) if d in lags]
        assert all(float(metric[ci][d]) == float(metric[owners[0]][d]) for ci in owners)
        for eps in EPS_FIXED + (eps_min,):
            for sign in (-1, 1):
                thr = float(metric[owners[0]][d]) * (1.0 + sign * eps)
                n_lags = d + W + 64
                assert n_lags <= max_lags and n_lags <= metric[0].size
                keys.append((d, eps, sign, thr, n_lags, owners))
                for lags in (n_lags, d + 1):
                    for ci in range(len(caps)):
                        guess = read_off(ci, d, thr, lags)
                        if guess is not None:
                            jobs.append((ci, d, thr, lags, guess))
    # the expected values are orc.sc_sync's own (a few threads: the oracle is plain C behind ctypes)
    with ThreadPoolExecutor(4) as pool:
        wants = list(pool.map(lambda j: orc.sc_sync(wcaps[j[0]], L, 3, j[3], j[2]), jobs))
    verdict = {}
    for (ci, d, thr, lags, guess), want in zip(jobs, wants):
        assert want[0] == guess, (n, ci, d, thr, lags, guess, want[0])      # the crossing and the peak read off M are the oracle's
        verdict[ci, thr, lags] = want
    thresholds, cases = [], []
    for d, eps, sign, thr, n_lags, owners in keys:
        rows = [verdict.get((ci, thr, n_lags)) for ci in range(len(caps))]
        razor = [verdict.get((ci, thr, d + 1)) for ci in range(len(caps))]
        thresholds.append(Threshold(d, eps, sign, thr, n_lags, rows, razor))
        for ci in owners:
            num, den = exact_m[ci, d]
            cases.append(Case(ci, d, eps, sign, thr, n_lags, rows[ci] is not None and razor[ci] is not None,
                              num >= Fraction(thr) * den, crosses_at(ci, d, thr)))
    return Size(n, S, W, caps, ratios, records, metric, exact_m, err, eps_min, cases, thresholds)
