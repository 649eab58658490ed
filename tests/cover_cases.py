"""The options of the decode chain as a pairwise cover ("The options meet"): the factors, the constraints, the
committed rows, and per row the payload, the channel and the captures -- shared by tests/test_cover_cpu.py and tests/test_gpu_cover.py.
What a row must deliver is tests/receiver_ref.py.

Every allowed pair of values of every two factors occurs in some row of ROWS.  The table is a literal: tools/cover_rows.py grew it and
grows it again when a factor or a value is added; nothing is generated at import.

The captures are made on the CPU, so that the reference and the device consume the same samples: orc.encode of the mode's coded
stream, then `channel` below -- the test bench of ofdm_channel_batch restated in numpy (the 64 FIR taps, the frame placed at its delay
in a slot 160 samples longer than the frame, the CFO, noise on every sample of the slot scaled by the pseudo-variance of the channel
output), the noise drawn from numpy's generator instead of SplitMix64.  The delays are 1 .. 32 and the CFOs within +-1 / S, drawn in
the order tools/link.py draws them.  Three things are fitted to what a row's options can acquire, because a chain that cannot lock
delivers nothing and then checks nothing behind its front end:
  * cfo_mode OFF gets no CFO, ABS and every row under SYNC_REFERENCE (whose frequency_correction drops the sign) get |CFO|;
  * cfo_mode WIDE adds a whole multiple m of 2 pi / S, m = -8, 0, 8 in the three frames;
  * a Schmidl-Cox row with sync_window_reps = r < 3 is sent with the last 3 - r of the four preamble copies blanked.  The frame
    carries four copies, so a window of r periods sees a plateau of M = 1 that is (3 - r) S lags long, and "the first maximum" falls
    anywhere on it: timing is then late by up to that much and no seed gives a frame start inside the cyclic prefix (a finding about
    the link, measured in tests/test_cover_cpu.py).  With r + 1 copies the peak is one lag wide again.

A row's seed is the first of 1000 + 8 row .. + 7 whose three frames lock on the reference alone (seed_of): status 0 and a frame start
within [true delay - backoff - 2, true delay], and for a hard inner mode, where the f64 reference needs nothing from the device, two
payloads of three delivered.  The kernel's rows are never looked at to pick it.  Rows the link cannot carry at all are not grown
(`carried`): two more findings about the link, stated there.
"""
import functools
import itertools
from collections import namedtuple

import numpy as np

SC, REFERENCE = 0, 1
CFO_OFF, CFO_SIGNED, CFO_ABS, CFO_WIDE = 0, 1, 2, 3
LS, WLS = 0, 1
LLRW_CHANNEL, LLRW_NOISE = 0, 1
OUTER_NONE, OUTER_RS, OUTER_FCS, OUTER_BOTH = 0, 20, 64, 84
BACKOFF_CP = -1                 # sync_backoff = cp_len, whatever n_fft is
LAGS_ALL, LAGS_BOUNDED = 0, 1   # n_lags = 0 (every lag) or 40 + S

FACTORS = (
    ("n_fft", (64, 128, 256, 512, 1024, 2048, 4096)),
    ("modulation", (1, 2, 4, 6, 8)),
    ("guard_bands", (0, 1)),
    ("inner", (0, 1, 2, 5, 10, 11, 12, 16, 41, 42, 43)),
    ("outer", (OUTER_NONE, OUTER_RS, OUTER_FCS, OUTER_BOTH)),
    ("sync_mode", (SC, REFERENCE)),
    ("cfo_mode", (CFO_OFF, CFO_SIGNED, CFO_ABS, CFO_WIDE)),
    ("chest_mode", (LS, WLS)),
    ("llr_weight", (LLRW_CHANNEL, LLRW_NOISE)),
    ("sync_window_reps", (1, 2, 3)),
    ("sync_backoff", (0, 1, 4, BACKOFF_CP)),
    ("sync_threshold", (0.5, 0.37)),
    ("n_lags", (LAGS_ALL, LAGS_BOUNDED)),
)
NAMES = tuple(name for name, _ in FACTORS)
CONSTRAINED = ("inner", "outer", "sync_mode", "cfo_mode", "chest_mode", "sync_backoff")
RS_INNER = (0, 10, 11, 12)

Row = namedtuple("Row", NAMES)


def allowed(row):
    """the library's own constraints (ofdm_create refuses the rest):
      * RS only around ECC_NONE and the framed convolutional modes;
      * no wide CFO acquisition under the reference's detector;
      * under Schmidl-Cox no CHEST_WLS and no CFO_WIDE with sync_backoff >= 3 cp_len / 4 (of the values here: cp_len).  Both model the
        channel's taps at delays [-cp / 4, 3 cp / 4) behind the frame start, and the back-off puts the first tap at delay
        sync_backoff -- this cover found it: the first table had such rows, and their REFERENCE (f64) delivered nothing, BER 0.3 - 0.5
        (include/ofdm_hip.h, "The window and sync_backoff").  SYNC_REFERENCE does not use the back-off and takes any."""
    r = Row(*row)
    if r.outer in (OUTER_RS, OUTER_BOTH) and r.inner not in RS_INNER:
        return False
    if r.cfo_mode == CFO_WIDE and r.sync_mode == REFERENCE:
        return False
    return not (r.sync_mode == SC and r.sync_backoff == BACKOFF_CP and (r.chest_mode == WLS or r.cfo_mode == CFO_WIDE))


LINK_FACTORS = ("n_fft", "modulation")      # what `carried` reads beyond CONSTRAINED


def carried(row):
    """rules of the link, not of the library: rows the generator does not grow, because the f64 reference itself delivers nothing
    there and a dead row checks nothing behind its front end.  Every pair of such a row is also held by rows the link does carry
    (SYNC_REFERENCE uses no back-off: its frame start is one sample early whatever sync_backoff says).  Both rules come from the
    channel's 64 taps: the main tap is the tenth, the one before it has 4 % of its energy, the nine behind it 15 %.
      * under Schmidl-Cox, no back-off at all with 64-QAM or more.  The frame start is then the main tap's, the tap before it lies in
        front of the FFT window, and every symbol takes one sample of the next.  Rows of the first tables: n_fft 128, 64-QAM under
        RS: 60 bit errors in every frame of 271 bytes, none with a back-off of 1 or 4; n_fft 4096, 256-QAM with no code: 1 - 3 bit
        errors in 8 frames of 9, none with a back-off of 1.  No seed of their eight delivered two payloads of three.
      * under Schmidl-Cox, a back-off of the whole cyclic prefix with 16-QAM or more at n_fft <= 256.  The FFT window then starts
        where the prefix does, and the taps behind the main one put the tail of the symbol before into it: 1.3 % raw bit errors at
        n_fft = 64 with 16-QAM, which the rate-3/4 code of that row did not survive (0 of 3)."""
    r = Row(*row)
    if r.sync_mode != SC:
        return True
    if r.sync_backoff == 0 and r.modulation >= 6:
        return False
    return not (r.sync_backoff == BACKOFF_CP and r.n_fft <= 256 and r.modulation >= 4)


def _constrained_rows():
    """every allowed setting of the constrained factors, the others at their first value"""
    idx = [NAMES.index(n) for n in CONSTRAINED]
    base = [vals[0] for _, vals in FACTORS]
    out = []
    for combo in itertools.product(*[FACTORS[i][1] for i in idx]):
        row = list(base)
        for i, v in zip(idx, combo):
            row[i] = v
        if allowed(row):
            out.append(tuple(row))
    return out


def allowed_pairs():
    """every ((i, value), (j, value)), i < j, that some allowed row holds -- from the factor lists and `allowed` alone (the
    constraints read the CONSTRAINED factors only, so the others are free)"""
    held = set()
    free = [i for i in range(len(FACTORS)) if NAMES[i] not in CONSTRAINED]
    for row in _constrained_rows():
        cons = [(i, row[i]) for i in range(len(FACTORS)) if i not in free]
        held |= set(itertools.combinations(cons, 2))
        held |= {tuple(sorted((c, (i, v)))) for c in cons for i in free for v in FACTORS[i][1]}
    for i, j in itertools.combinations(free, 2):
        held |= {((i, v), (j, w)) for v in FACTORS[i][1] for w in FACTORS[j][1]}
    return sorted(held)


def excluded_pairs():
    """[((factor, value), (factor, value))] no allowed row holds"""
    held = set(allowed_pairs())
    out = []
    for i, j in itertools.combinations(range(len(FACTORS)), 2):
        out += [((NAMES[i], v), (NAMES[j], w)) for v in FACTORS[i][1] for w in FACTORS[j][1] if ((i, v), (j, w)) not in held]
    return out


def pairs_of(row):
    return {((i, row[i]), (j, row[j])) for i, j in itertools.combinations(range(len(row)), 2)}


# (n_fft, modulation, guard_bands, inner, outer, sync_mode, cfo_mode, chest_mode, llr_weight, sync_window_reps, sync_backoff,
#  sync_threshold, n_lags)
ROWS = (
    (64, 1, 1, 5, 0, 1, 2, 0, 0, 3, -1, 0.37, 1),
    (64, 1, 1, 11, 0, 1, 0, 0, 0, 3, 0, 0.37, 1),
    (64, 2, 0, 42, 64, 1, 0, 0, 0, 2, 4, 0.37, 0),
    (64, 4, 0, 2, 0, 0, 3, 1, 1, 2, 4, 0.5, 0),
    (64, 4, 0, 12, 64, 0, 3, 0, 1, 3, 0, 0.37, 0),
    (64, 6, 0, 0, 20, 0, 1, 1, 1, 1, 4, 0.5, 1),
    (64, 6, 0, 43, 0, 0, 3, 1, 1, 2, 1, 0.5, 0),
    (64, 8, 0, 10, 84, 0, 0, 1, 0, 2, 1, 0.37, 1),
    (64, 8, 0, 16, 64, 0, 3, 1, 0, 1, 1, 0.37, 0),
    (64, 8, 1, 1, 0, 1, 0, 0, 1, 3, -1, 0.37, 1),
    (64, 8, 1, 41, 0, 1, 1, 0, 1, 3, -1, 0.37, 1),
    (128, 1, 0, 2, 0, 0, 1, 0, 1, 1, 1, 0.5, 1),
    (128, 1, 1, 10, 20, 0, 0, 0, 0, 1, 0, 0.5, 1),
    (128, 1, 1, 42, 64, 0, 0, 1, 1, 3, 4, 0.37, 1),
    (128, 2, 0, 12, 84, 1, 0, 1, 0, 2, -1, 0.5, 1),
    (128, 2, 0, 16, 0, 1, 2, 1, 1, 2, 1, 0.5, 1),
    (128, 2, 0, 41, 0, 0, 3, 1, 0, 1, 1, 0.5, 1),
    (128, 2, 1, 0, 20, 0, 2, 0, 0, 2, 0, 0.37, 0),
    (128, 4, 0, 11, 0, 0, 3, 0, 0, 2, 1, 0.37, 1),
    (128, 4, 1, 5, 0, 1, 0, 1, 1, 2, 4, 0.37, 1),
    (128, 6, 1, 1, 64, 1, 2, 1, 1, 3, 4, 0.5, 0),
    (128, 8, 0, 43, 64, 1, 0, 0, 1, 3, -1, 0.5, 1),
    (256, 1, 0, 1, 64, 0, 3, 1, 0, 2, 1, 0.37, 0),
    (256, 1, 1, 0, 0, 0, 3, 0, 1, 1, 1, 0.5, 1),
    (256, 1, 1, 41, 0, 0, 3, 1, 1, 3, 1, 0.37, 0),
    (256, 2, 0, 43, 0, 0, 1, 0, 0, 1, 0, 0.37, 0),
    (256, 4, 0, 11, 20, 1, 0, 1, 1, 3, 1, 0.5, 1),
    (256, 6, 0, 5, 64, 1, 2, 0, 0, 1, 0, 0.5, 1),
    (256, 6, 0, 10, 84, 0, 3, 0, 1, 3, 4, 0.5, 0),
    (256, 6, 0, 16, 64, 1, 1, 1, 1, 2, -1, 0.5, 0),
    (256, 8, 0, 2, 0, 1, 0, 1, 1, 3, 4, 0.37, 1),
    (256, 8, 0, 42, 0, 1, 2, 0, 0, 1, -1, 0.37, 0),
    (256, 8, 1, 12, 0, 0, 1, 1, 0, 2, 4, 0.37, 0),
    (512, 1, 0, 41, 0, 0, 0, 1, 1, 2, 4, 0.5, 0),
    (512, 1, 1, 11, 84, 1, 0, 0, 0, 1, 0, 0.37, 0),
    (512, 2, 1, 2, 64, 0, 3, 1, 0, 3, 4, 0.5, 0),
    (512, 2, 1, 10, 84, 1, 1, 1, 0, 2, -1, 0.37, 1),
    (512, 4, 0, 16, 0, 0, 1, 0, 1, 1, -1, 0.5, 1),
    (512, 4, 1, 1, 64, 0, 3, 0, 0, 1, 4, 0.37, 0),
    (512, 4, 1, 5, 64, 0, 3, 0, 0, 3, 4, 0.5, 1),
    (512, 4, 1, 43, 64, 1, 2, 1, 1, 3, 4, 0.5, 1),
    (512, 6, 0, 42, 0, 1, 1, 1, 1, 3, 0, 0.37, 1),
    (512, 8, 0, 0, 20, 0, 1, 1, 0, 3, 4, 0.37, 0),
    (512, 8, 0, 12, 84, 1, 2, 1, 1, 1, 1, 0.5, 1),
    (1024, 1, 0, 0, 64, 0, 3, 1, 1, 1, 1, 0.5, 1),
    (1024, 1, 0, 1, 0, 0, 3, 1, 1, 2, 0, 0.5, 1),
    (1024, 1, 0, 5, 64, 1, 1, 1, 0, 2, 1, 0.5, 1),
    (1024, 1, 0, 16, 64, 0, 0, 1, 1, 2, 4, 0.37, 0),
    (1024, 2, 1, 11, 64, 1, 1, 1, 1, 2, -1, 0.37, 0),
    (1024, 2, 1, 43, 0, 0, 1, 1, 0, 1, 1, 0.37, 0),
    (1024, 4, 0, 12, 20, 0, 0, 0, 1, 1, -1, 0.37, 1),
    (1024, 4, 0, 42, 0, 0, 3, 1, 1, 3, 1, 0.37, 1),
    (1024, 4, 1, 10, 64, 0, 3, 0, 0, 3, 1, 0.5, 1),
    (1024, 6, 0, 0, 84, 1, 0, 1, 1, 3, 0, 0.5, 1),
    (1024, 6, 1, 2, 64, 1, 2, 1, 0, 3, -1, 0.37, 0),
    (1024, 8, 1, 41, 0, 1, 2, 0, 0, 1, 4, 0.37, 0),
    (2048, 1, 1, 10, 84, 1, 2, 0, 0, 2, -1, 0.5, 1),
    (2048, 1, 1, 12, 84, 1, 2, 1, 0, 2, 4, 0.5, 1),
    (2048, 2, 0, 42, 0, 1, 0, 0, 1, 1, -1, 0.37, 1),
    (2048, 2, 0, 43, 0, 0, 0, 1, 1, 3, 1, 0.5, 0),
    (2048, 2, 1, 5, 64, 0, 3, 1, 1, 3, 1, 0.37, 0),
    (2048, 2, 1, 16, 0, 1, 1, 0, 0, 1, -1, 0.5, 1),
    (2048, 4, 1, 0, 84, 1, 0, 1, 0, 3, -1, 0.37, 1),
    (2048, 6, 0, 11, 20, 0, 2, 0, 1, 1, -1, 0.5, 0),
    (2048, 6, 0, 41, 0, 0, 0, 0, 0, 2, -1, 0.5, 1),
    (2048, 8, 0, 1, 0, 0, 1, 0, 1, 1, 1, 0.37, 0),
    (2048, 8, 0, 2, 0, 1, 0, 1, 0, 2, 0, 0.37, 1),
    (4096, 1, 0, 43, 64, 1, 0, 1, 1, 3, 4, 0.5, 0),
    (4096, 1, 1, 16, 0, 0, 2, 1, 1, 3, 0, 0.5, 0),
    (4096, 2, 0, 2, 64, 0, 0, 1, 0, 3, 1, 0.37, 1),
    (4096, 2, 1, 1, 64, 1, 0, 0, 0, 3, -1, 0.37, 0),
    (4096, 4, 0, 10, 0, 1, 2, 0, 0, 2, 1, 0.5, 1),
    (4096, 4, 1, 41, 64, 0, 1, 1, 1, 3, 0, 0.37, 0),
    (4096, 6, 0, 12, 84, 0, 2, 0, 0, 3, 4, 0.5, 0),
    (4096, 6, 1, 42, 0, 0, 3, 1, 1, 1, 1, 0.5, 1),
    (4096, 8, 0, 0, 20, 0, 0, 0, 1, 3, 1, 0.37, 0),
    (4096, 8, 0, 5, 64, 0, 1, 0, 1, 3, 1, 0.37, 1),
    (4096, 8, 1, 11, 20, 0, 3, 1, 0, 2, 4, 0.5, 0),
)

FRAMES = 3
# the channel's snr_db behind tools.link.data_snr(n, .), per modulation: what the mode tests that run every modulation give it
# (tests/test_gpu_soft.py, _conv, _framed: 30 dB, 38 dB for 256-QAM)
SNR_DB = {1: 30.0, 2: 30.0, 4: 30.0, 6: 30.0, 8: 38.0}
SEEDS_PER_ROW = 8


class Case:
    """one row with what follows from it"""

    def __init__(self, index):
        self.index = index
        self.row = r = Row(*ROWS[index])
        self.n, self.mod, self.guard = r.n_fft, r.modulation, bool(r.guard_bands)
        self.S = r.n_fft + r.n_fft // 4
        self.inner, self.outer, self.ecc = r.inner, r.outer, r.inner + r.outer
        self.sync_mode, self.cfo_mode, self.chest_mode, self.llr_weight = r.sync_mode, r.cfo_mode, r.chest_mode, r.llr_weight
        self.reps, self.threshold = r.sync_window_reps, r.sync_threshold
        self.backoff = r.n_fft // 4 if r.sync_backoff == BACKOFF_CP else r.sync_backoff
        self.n_lags = 40 + self.S if r.n_lags == LAGS_BOUNDED else 0
        self.payload = 100 if r.n_fft <= 256 else 300
        self.snr_db = float(SNR_DB[r.modulation] + 10.0 * np.log10(r.n_fft / 64))      # tools.link.data_snr
        self.carriers = 48 * (r.n_fft // 64) if r.guard_bands else r.n_fft
        self.bytes_per_symbol = self.carriers * r.modulation // 8
        self.first_seed = 1000 + 8 * index
        self.id = "-".join(f"{v}" for v in r)

    def context_kw(self):
        """the keywords of api.Context"""
        return dict(n_fft=self.n, modulation=self.mod, guard_bands=self.guard, ecc=self.ecc, sync_mode=self.sync_mode, cfo_mode=self.cfo_mode,
                    chest_mode=self.chest_mode, llr_weight=self.llr_weight, sync_window_reps=self.reps, sync_backoff=self.backoff,
                    sync_threshold=self.threshold)

    def data_symbols(self, coded_len):
        return -(-(-(-(16 + coded_len) * 8 // self.mod)) // self.carriers)

    def blanked_copies(self):
        """preamble copies the capture is sent without (the module's text)"""
        return 3 - self.reps if self.sync_mode == SC else 0


def cases():
    return [Case(i) for i in range(len(ROWS))]


def channel(orc, tx, snr_db, rng, delay, f_delta, span):
    """ofdm_channel_batch's test bench for one frame, in numpy (the module's text) -> complex64 [span]"""
    y = np.convolve(tx, orc.channel_taps())
    assert y.size == tx.size + 63 and delay + y.size <= span
    y = y * np.exp(1j * f_delta * np.arange(1, y.size + 1))
    var = orc.variance(y)
    scale = np.sqrt(0.5 * var / 10.0 ** (snr_db / 10.0))
    out = scale * (rng.uniform(-1.0, 1.0, span) + 1j * rng.uniform(-1.0, 1.0, span))
    out[delay:delay + y.size] += y
    return out.astype(np.complex64)


Link = namedtuple("Link", "pay tx rx delay f_delta m D")


@functools.lru_cache(maxsize=4)
def link(orc, index, seed):
    """the three frames of row `index` under `seed` -> Link(payloads uint8 [3, p], sent frames complex128 [3, frame], captures
    complex64 [3, frame + 160], delays, CFOs, the wide multiples, data symbols of a frame)"""
    import receiver_ref as rr

    k = Case(index)
    rng = np.random.default_rng(seed)
    pay = rng.integers(0, 256, (FRAMES, k.payload), dtype=np.uint8)
    delay = rng.integers(1, 33, FRAMES)
    fd = (rng.random(FRAMES) - 0.5) * (2.0 / k.S)
    if k.cfo_mode == CFO_OFF:
        fd[:] = 0.0
    elif k.cfo_mode == CFO_ABS or k.sync_mode == REFERENCE:
        fd = np.abs(fd)
    m = np.array([-8, 0, 8]) if k.cfo_mode == CFO_WIDE else np.zeros(FRAMES, np.int64)
    fd = fd + 2.0 * np.pi * m / k.S
    tx = np.stack([orc.encode(rr.mode_encode(k.ecc, bytes(p)), k.guard, k.mod, k.n) for p in pay])
    sent = tx.copy()
    blank = k.blanked_copies()
    if blank:
        sent[:, (5 - blank) * k.S:5 * k.S] = 0.0
    span = tx.shape[1] + 160
    rx = np.stack([channel(orc, sent[f], k.snr_db, rng, int(delay[f]), float(fd[f]), span) for f in range(FRAMES)])
    return Link(pay, tx, rx, delay, fd, m, (tx.shape[1] - 10 * k.S) // k.S)


# data-symbol SNR of the stressed captures, per modulation: where an uncoded link has some 5 % bit errors, so that every soft decoder
# works at its edge and every LLR bears on what it delivers
STRESS_SNR_DB = {1: 3.0, 2: 6.0, 4: 12.0, 6: 18.0, 8: 24.0}


def stressed(orc, index, seed):
    """the row's captures under white Gaussian noise at STRESS_SNR_DB below the power of the sent data symbols -> complex64 [3, span].
    Nothing is asked of such a capture but that the chain and the composition of the stages agree on it to the byte."""
    k = Case(index)
    ln = link(orc, index, seed)
    rng = np.random.default_rng(1_000_000 + seed)
    power = np.mean(np.abs(ln.tx[:, 10 * k.S:]) ** 2, axis=1) * np.sum(orc.channel_taps() ** 2)
    sigma = np.sqrt(power / 10.0 ** (STRESS_SNR_DB[k.mod] / 10.0) / 2.0)[:, None]
    noise = sigma * (rng.standard_normal(ln.rx.shape) + 1j * rng.standard_normal(ln.rx.shape))
    return (ln.rx.astype(np.complex128) + noise).astype(np.complex64)


@functools.lru_cache(maxsize=4)
def reference_front(orc, index, seed):
    """receiver_ref.front_end of the row's captures under `seed` (kept: the seed's condition and the GPU test both read it)"""
    import receiver_ref as rr

    ln = link(orc, index, seed)
    return tuple(rr.front_end(orc, ln.rx, Case(index), ln.D))


def locks(orc, index, seed):
    """the liveness condition of the seed, on the reference alone: every frame's status 0 and its frame start within
    [true delay - backoff - 2, true delay]; the true delay is the slot's delay plus that of the channel's main tap (9 samples)"""
    k = Case(index)
    ln = link(orc, index, seed)
    true = ln.delay + int(np.argmax(np.abs(orc.channel_taps())))
    return all(w.status == 0 and true[f] - k.backoff - 2 <= w.offset <= true[f] for f, w in enumerate(reference_front(orc, index, seed)))


def delivered_by_reference(orc, index, seed):
    """frames of a hard inner mode (0, 1) whose payload the f64 reference delivers, outer layers by the CPU rule; None for a soft mode,
    whose reference needs the device's LLRs"""
    import receiver_ref as rr

    k = Case(index)
    if k.inner not in rr.HARD_INNER:
        return None
    ln = link(orc, index, seed)
    good = 0
    for f, w in enumerate(reference_front(orc, index, seed)):
        body, _ = rr.hard_reference(orc, ln.rx[f], k, w.offset, w.f_delta, ln.D)
        st, data = rr.outer_layers(k.ecc, 0, rr.hard_finish(orc, k.inner, body))
        good += st == 0 and data[:k.payload] == bytes(ln.pay[f])
    return good


@functools.lru_cache(maxsize=None)
def seed_of(orc, index):
    """the first of the row's eight seeds whose captures lock and, where the reference alone can tell (a hard inner mode), deliver two
    payloads of the three; None if none does.  The kernel's rows are never looked at."""
    first = Case(index).first_seed
    for seed in range(first, first + SEEDS_PER_ROW):
        if not locks(orc, index, seed):
            continue
        good = delivered_by_reference(orc, index, seed)
        if good is None or good >= 2:
            return seed
    return None
