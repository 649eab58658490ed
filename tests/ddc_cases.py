"""The inputs behind the down-converter's tests (EXT-16), shared by tests/test_ddc_cpu.py, tests/test_gpu_ddc.py and tools/bench_ddc.py.

1. wide / wide_taps: samples and taps on which the ORDER of a filter's additions shows in the f32 result (the bit-for-bit comparisons
   could not tell a wrong kernel apart otherwise).

2. Wide-band captures, on the f64 oracle alone.  A narrow-band capture is tests/dcblock_cases.stream_capture without its DC term: three
   frames through the oracle's channel, noise in front, between and behind.  wideband() makes of it what a radio hands over that runs at
   D times the modem's rate, tuned off-centre, with a neighbour in the band:
       interpolation   zero-stuffed by D, filtered by D * a Blackman-windowed sinc of T_I = INTERP_TPP D taps with the cutoff 0.5 / D;
       shift           times exp(2 pi i f0 n), f0 = k / D cycles per sample (so that raw DC, mixed to -f0, aliases onto output bin 0, a
                       null carrier, and lies in the filter's stopband; at D = 2, f0 = 0.25 it would land on the output's Nyquist
                       frequency, the filter's -6 dB point, and the prototype lost a frame to it);
       neighbour       a second capture (its own payloads and noise seed), interpolated with the cutoff NEIGHBOUR_TX_CUT / D (below),
                       NEIGHBOUR_AMP times the amplitude, one channel away: at f0 + 1 / D;
       DC              1 x the rms of the wanted frames at the input rate, phase 0.6 rad;
       complex64.
   ddc(raw) with the default design (T = 24 D) then carries narrow-band sample j at output j + delay(D), delay = (T_I - T) / (2 D):
   both filters are symmetric, the cascade peaks (T_I - 1) / 2 - (T - 1) / 2 input samples behind the narrow sample's own place.

   THE FINDING the issue left open (D = 4 / 8 with a +6 dB neighbour one channel away: 19 - 47 hard-bit errors a frame at QPSK / 8 dB;
   D = 2 and the neighbour-free D = 4 capture: 0).  Settled on the oracle; test_ddc_cpu.py::test_the_neighbour_finding repeats the
   measurements and prints them (n64_qpsk, seed 1600, errors of the three frames):
     - reproduced with an unfiltered neighbour (neighbour_cut = 0.5): D = 3: 34 / 22 / 31, D = 4: 33 / 22 / 26, D = 8: 22 / 14 / 16, D = 2: 0;
       neighbour below instead of above: the same; at half the amplitude (0 dB): 5 / 1 / 4.
     - it is NOT noise: the neighbour made at 300 dB leaves 29 / 23 / 32 at D = 4.  It is not timing and not the CFO estimate: every frame
       is timed on the narrow-band capture's sample, and decoding with the CFO estimate switched off leaves the same counts.
     - it is NOT the interpolator's passband edge on the wanted signal: without the neighbour every D has 0 errors.
     - the issue's premise was wrong.  With guard bands the oracle's transmitter uses FFT bins 6 .. 31 and 33 .. 58: the nulls are the
       eleven bins around DC and the Nyquist bin, and the DATA runs up to +-31 / 64 = 0.484 of the band, not 0.406 -- there is no guard
       band at the channel's edge.  So the outermost carriers of an adjacent channel of the same modem lie at 0.516 / D .. 0.56 / D from the
       wanted centre, inside the transition band of any filter whose cutoff is 0.5 / D (the default design: -10 dB at 0.516 / D, -16 dB
       at 0.531 / D, -40 dB at 0.5625 / D), and fold onto the wanted signal's own outermost carriers, which the same filter (-3.1 dB at
       0.484 / D) and the oracle's channel (-8 dB at bin 31) have already weakened.  Measured at D = 4: the neighbour alone leaves -19 dB
       (relative to the wanted signal's strongest bin) on output bins 29 .. 35 and less than -37 dB from bin 26 inwards; every bit error
       sits on the carriers of bins 28 and 36.  More taps a phase narrow the transition and help; no number of taps removes it while
       both channels carry data up to their common boundary.
     - D = 2 was clean through an artefact of the capture, not through the filter: there the neighbour lies on the Nyquist frequency, both
       its edges border the wanted channel, and a carrier at 0.5 / D + e and its zero-stuffing image at -0.5 / D + e fold onto the SAME
       output bin with opposite signs, because the decimator keeps exactly the samples of the interpolator's own grid (the delay
       (T_I - T) / 2 is a multiple of D).  Decimating the same filtered samples one input sample later leaves the neighbour 30 dB
       stronger on output bins 29 .. 35.  A neighbour that is not sample-synchronous with the wanted signal gets no such help.
   WHAT WAS CHOSEN.  The test captures' neighbour is a signal WITH a guard band at its channel edge: the same kind of capture, +6 dB, one
   channel away at f0 + 1 / D, but interpolated with the cutoff NEIGHBOUR_TX_CUT = 0.42 / D, the way a transmit filter bounds an
   emission, so that it ends in front of the wanted channel's transition band.  With it the QPSK case has the narrow-band capture's
   error count +- 0 (0 / 0 / 0) at D = 2, 4 and 8 with no noise added at the input rate; with the cutoff 0.46 / D at D = 4 as well.
   An adjacent channel of this very modem, unfiltered, is NOT covered by the default design and is said so in DESIGN.md (EXT-16).
"""
import functools

import numpy as np

import dcblock_cases as K
import ddc_ref as R

INTERP_TPP = 32             # the interpolator's taps per phase: T_I = 32 D, so that delay(D) = (32 D - 24 D) / (2 D) = 4 for every D
NEIGHBOUR_AMP = 2.0         # +6 dB
NEIGHBOUR_TX_CUT = 0.42     # the neighbour's own transmit filter: cutoff in units of 1 / D
DC_FACTOR = 1.0
BACKOFF = 4

# name -> (n_fft, modulation bits, snr_db, frames, payload bytes); D and k are parameters of wideband()
# n64_qpsk_stream: the QPSK case as the GPU stream test runs it -- 14 dB and 300 bytes, so that an UNCODED payload of the one-shot path
# has no bit error to lose (at 8 dB the f64 oracle has none in these frames, with nothing to spare)
CASES = {"n64_qpsk": (64, 2, 8.0, 3, 560), "n64_qam64": (64, 6, 25.0, 3, 560), "n256": (256, 6, 30.0, 3, 560), "n1024": (1024, 6, 34.0, 2, 560),
         "n64_qpsk_stream": (64, 2, 14.0, 3, 300)}
SEEDS_PER_CASE = 8
SEEDS = {"n64_qpsk": 1600, "n64_qam64": 1608, "n256": 1616, "n1024": 1624, "n64_qpsk_stream": 1632}
DECIMS = (2, 4)


def first_seed(name):
    return 1600 + 8 * list(CASES).index(name)


PLAIN_DELAY = INTERP_TPP // 2    # raw[::D] carries narrow-band sample j at j + ((32 D - 1) / 2) / D = j + 16 - 1 / (2 D): 16 samples late


def delay(D, taps_per_phase=R.TAPS_PER_PHASE):
    d, r = divmod((INTERP_TPP - taps_per_phase) * D, 2 * D)
    assert r == 0
    return d


# ---------------------------------------------------------------------------------------------------------- 1
def wide(n, seed):
    """samples whose magnitudes span 2^-40 .. 2^40 (dcblock_cases.wide: large values that cancel, small ones between them)"""
    return K.wide(n, seed)


def wide_taps(T, seed):
    """T taps of magnitudes 2^-12 .. 2^12 that cancel: a value, somewhere else its negative, small ones between them"""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(T // 3 + 1) * np.exp2(rng.integers(0, 13, T // 3 + 1))).astype(np.float32)
    s = (rng.standard_normal(T) * np.exp2(rng.integers(-12, 1, T))).astype(np.float32)
    h = np.concatenate([a, -a, s])[:max(T, 1)]
    return np.ascontiguousarray(rng.permutation(h)[:T]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- 2
def interpolator(D, cut=0.5, tpp=INTERP_TPP):
    """D * a Blackman-windowed sinc of tpp D taps, cutoff `cut` / D, unit gain at 0 per phase"""
    T = tpp * D
    k = np.arange(T, dtype=np.float64)
    g = np.sinc(2.0 * cut * (k - (T - 1) / 2.0) / D) * np.blackman(T)
    return g * (D / g.sum())


def interpolate(z, D, cut=0.5):
    """narrow-band z -> len(z) D + T_I - 1 input-rate samples; narrow sample j lies at j D + (T_I - 1) / 2"""
    up = np.zeros(len(z) * D, np.complex128)
    up[::D] = z
    return np.convolve(up, interpolator(D, cut))


class Wide:
    pass


def narrow(orc, name, seed, snr=None):
    n_fft, mod, snr0, frames, payload = CASES[name]
    return K.stream_capture(orc, n_fft, mod, snr0 if snr is None else snr, frames, payload, seed, 0.0)


@functools.lru_cache(maxsize=None)
def wideband(orc, name, seed, D, k=1, neighbour=NEIGHBOUR_AMP, neighbour_at=1.0, neighbour_cut=NEIGHBOUR_TX_CUT, neighbour_snr=None,
             dc=DC_FACTOR):
    """-> Wide: raw (complex64, the input-rate capture), cap (the narrow-band Capture: clean, payloads, starts, D, S, frame), f0, inc,
    taps (the default design), delay"""
    w = Wide()
    w.cap = narrow(orc, name, seed)
    other = narrow(orc, name, seed + 100, neighbour_snr).clean if neighbour else None
    w.D, w.f0 = D, k / D
    w.raw = widen_capture(w.cap.clean, w.cap.rms, D, k, other, neighbour, neighbour_at, neighbour_cut, dc)
    w.inc = R.inc_for(w.f0)
    w.taps = R.design(D)[0]
    w.delay = delay(D)
    return w


def widen_capture(z, rms, D, k=1, other=None, neighbour=NEIGHBOUR_AMP, neighbour_at=1.0, neighbour_cut=NEIGHBOUR_TX_CUT, dc=DC_FACTOR):
    """any narrow-band capture z (and a neighbour's, `other`) -> the input-rate capture, complex64; rms: the wanted frames' rms"""
    f0 = k / D
    x = interpolate(np.asarray(z).astype(np.complex128), D)
    n = np.arange(len(x), dtype=np.float64)
    x = x * np.exp(2j * np.pi * f0 * n)
    if other is not None and neighbour:
        zn = interpolate(np.asarray(other).astype(np.complex128), D, neighbour_cut)[: len(x)]
        x[: len(zn)] += neighbour * zn * np.exp(2j * np.pi * (f0 + neighbour_at / D) * n[: len(zn)])
    return (x + dc * rms * K.DC_PHASE).astype(np.complex64)                 # interpolation keeps the amplitude


def frames(orc, cap, x, shift=0):
    """decode_sc of every frame of a capture (x: any array laid out as the narrow-band capture, `shift` samples late) -> [(result,
    hard-bit errors of the header + payload stream or None)]; offsets are relative to x"""
    out = []
    lag = int(np.argmax(np.abs(orc.channel_taps())))               # a frame's search starts where the channel's output of the one before ends
    cuts = [0] + [cap.starts[i] - lag - K.GAPS[(i - 1) % len(K.GAPS)] * (cap.S // 80) + shift for i in range(1, len(cap.starts))]
    coded = [len(p).to_bytes(16, "little") + p for p in cap.payloads]
    for i, cut in enumerate(cuts):
        end = cap.starts[i] + shift + cap.frame + 2 * cap.S
        r = orc.decode_sc(x[cut:end], guard=True, modulation=cap.mod, n_fft=cap.n_fft, backoff=BACKOFF, max_symbols=cap.D, want_soft=True)
        if r["status"] in (-1, -2, -3):
            out.append((r, None))
            continue
        r["offset"] += cut
        hard = np.frombuffer(orc.demodulate(r["soft"], cap.mod), np.uint8)
        want = np.frombuffer(coded[i], np.uint8)
        m = min(len(hard), len(want))
        out.append((r, int(np.unpackbits(hard[:m] ^ want[:m]).sum()) + 8 * (len(want) - m)))
    return out


def timed(cap, fr, shift=0):
    """which frames are timed within the back-off of their true start"""
    return [r["status"] not in (-1, -2, -3) and cap.starts[i] + shift - BACKOFF - 2 <= r["offset"] <= cap.starts[i] + shift
            for i, (r, _) in enumerate(fr)]


def seed_of(orc, name):
    """the first of the case's eight seeds whose narrow-band frames all lock"""
    for seed in range(first_seed(name), first_seed(name) + SEEDS_PER_CASE):
        cap = narrow(orc, name, seed)
        if all(timed(cap, frames(orc, cap, cap.clean))):
            return seed
    return None
