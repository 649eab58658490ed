"""The captures behind the DC blocker's reason to exist (EXT-15), on the f64 oracle alone, shared by tests/test_dcblock_cpu.py,
tests/test_gpu_dcblock.py and tools/bench_dcblock.py.

A capture is lead_of(n_fft) samples of noise, then two frames of the oracle's transmitter through the oracle's channel (orc.channel: the 64 taps and
the noise of the case's SNR), GAP samples of noise apart, then TAIL samples of noise; the noise outside the frames is complex Gaussian of
the variance the channel added inside them (measured: the capture less the same capture at 300 dB).  A DC term is a complex constant of
`factor` times the rms of the received frames, added to every sample.  The seed of a case is the first of its eight whose DC-FREE frames
lock on the oracle (status 0 is not asked: an uncoded 64-QAM header at 14 dB seldom survives; the frame start within the back-off of
the truth is), as tests/cover_cases.py picks its seeds; SEEDS commits them and test_dcblock_cpu.py recomputes them.
"""
import functools

import numpy as np

import dcblock_ref as D

GAP, TAIL, PAYLOAD, BACKOFF = 37, 300, 560, 4


def lead_of(n_fft):
    """the noise in front of the first frame: 2000 samples, and at least six symbols -- the detector takes its peak from the window W = 3 S
    behind the first crossing, so with a lead shorter than W + S a crossing at lag 0 would still find the frame's peak"""
    return max(2000, 6 * (n_fft + n_fft // 4))

DC_FACTORS = (0.3, 1.0, 10.0)
DC_PHASE = np.exp(0.6j)
RHO_FIRES = 2.41          # |c|^2 / sigma^2 from which (rho / (1 + rho))^2 >= 0.5: the detector fires on noise plus DC alone
BAND = (0.5, 1, 2, 3, 4, 8)  # windows r S of the band map
SEEDS_PER_CASE = 8

# name -> (n_fft, modulation bits, snr_db)
CASES = {"n64_qam64": (64, 6, 14.0), "n64_qpsk": (64, 2, 8.0), "n256_qam64": (256, 6, 24.0), "n1024_qam64": (1024, 6, 34.0)}
SEEDS = {"n64_qam64": 1500, "n64_qpsk": 1508, "n256_qam64": 1516, "n1024_qam64": 1524}


def first_seed(name):
    return 1500 + 8 * list(CASES).index(name)


class Capture:
    pass


@functools.lru_cache(maxsize=None)
def capture(orc, name, seed):
    """the DC-free capture of a case under a seed, complex128, with everything the checks need"""
    n_fft, mod, snr = CASES[name]
    rng = np.random.default_rng(seed)
    c = Capture()
    c.name, c.n_fft, c.mod, c.snr, c.S = name, n_fft, mod, snr, n_fft + n_fft // 4
    c.payloads = [bytes(rng.integers(0, 256, PAYLOAD, dtype=np.uint8)) for _ in range(2)]
    rx, noise = [], []
    for k, p in enumerate(c.payloads):
        tx = orc.encode(p, guard=True, modulation=mod, n_fft=n_fft)
        y = orc.channel(tx, snr, False, seed * 2 + k)[0]
        rx.append(y)
        noise.append(y - orc.channel(tx, 300.0, False, seed * 2 + k)[0])
    c.sigma2 = float(np.mean(np.abs(np.concatenate(noise)) ** 2))
    c.rms = float(np.sqrt(np.mean(np.abs(np.concatenate(rx)) ** 2)))
    g = lambda n: np.sqrt(c.sigma2 / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    delay = int(np.argmax(np.abs(orc.channel_taps())))  # the channel's main tap: where a frame's first sample arrives
    c.lead = lead_of(n_fft)
    c.at = [c.lead, c.lead + len(rx[0]) + GAP]              # where the channel's output of frame k begins
    c.starts = [a + delay for a in c.at]                # the true frame starts
    c.x = np.concatenate([g(c.lead), rx[0], g(GAP), rx[1], g(TAIL)])
    c.cuts = [0, c.at[1] - GAP]                         # where the search for frame k starts
    c.D = (len(rx[0]) - 63) // c.S - 10                 # data symbols of a frame
    c.coded = [len(p).to_bytes(16, "little") + p for p in c.payloads]   # the byte stream of a frame: the length header, the payload
    return c


def with_dc(c, factor):
    """the capture with the DC term, as the radio hands it over: complex64"""
    return (c.x + factor * c.rms * DC_PHASE).astype(np.complex64)


def rho(c, factor):
    return (factor * c.rms) ** 2 / c.sigma2


def frames(orc, c, x):
    """decode_sc of both frames of a capture (any array of the capture's length): [(result dict with soft symbols, bit errors)]; the offset
    is capture-relative"""
    out = []
    for k, cut in enumerate(c.cuts):
        r = orc.decode_sc(x[cut:], guard=True, modulation=c.mod, n_fft=c.n_fft, backoff=BACKOFF, max_symbols=c.D, want_soft=True)
        if r["status"] in (-2, -3, -1):
            out.append((r, None))
            continue
        r["offset"] += cut
        hard = np.frombuffer(orc.demodulate(r["soft"], c.mod), np.uint8)
        want = np.frombuffer(c.coded[k], np.uint8)
        n = min(len(hard), len(want))
        errs = int(np.unpackbits(hard[:n] ^ want[:n]).sum()) + 8 * (len(want) - n)
        out.append((r, errs))
    return out


def locks(orc, c, x):
    """every frame timed within the back-off of its true start"""
    return all(r["status"] not in (-1, -2, -3) and c.starts[k] - BACKOFF - 2 <= r["offset"] <= c.starts[k] for k, (r, _) in enumerate(frames(orc, c, x)))


def seed_of(orc, name):
    for seed in range(first_seed(name), first_seed(name) + SEEDS_PER_CASE):
        c = capture(orc, name, seed)
        if locks(orc, c, c.x.astype(np.complex64)):
            return seed
    return None


def blocks_of(c, r):
    """the window of r symbols, in blocks: ceil(r S / 64)"""
    return max(int(-(-r * c.S // D.BLOCK)), 1)


def wide(n, seed):
    """samples whose magnitudes span 2^-40 .. 2^40 and whose large values cancel inside every block of 64: 24 values of up to 2^40, their
    negatives in another order, 16 values of 2^-40 .. 1, all shuffled.  A block's sum is then small, and what rounding leaves of the large
    values depends on the order of the additions and shows in the f32 mean"""
    rng = np.random.default_rng(seed)
    nb = -(-n // 64)
    big = (rng.standard_normal((nb, 24)) + 1j * rng.standard_normal((nb, 24))) * np.exp2(rng.integers(0, 41, (nb, 24)))
    small = (rng.standard_normal((nb, 16)) + 1j * rng.standard_normal((nb, 16))) * np.exp2(rng.integers(-40, 1, (nb, 16)))
    big = big.astype(np.complex64)
    x = np.concatenate([big, -rng.permuted(big, axis=1), small.astype(np.complex64)], axis=1)
    return np.ascontiguousarray(rng.permuted(x, axis=1)).reshape(-1)[:n].astype(np.complex64)


# ---- a stream a radio with LO leakage hands over (tests/test_gpu_dcblock.py, tools/bench_dcblock.py)
GAPS = (37, 211, 90, 402)


@functools.lru_cache(maxsize=None)
def stream_capture(orc, n_fft, mod, snr, n_frames, payload, seed, factor=1.0):
    """lead_of(n_fft) samples of noise, n_frames frames GAPS apart through the oracle's channel, TAIL samples of noise, the whole on a
    DC term of `factor` times the frames' rms -> Capture with x (complex64, DC included), clean (complex64, DC-free), payloads, starts (the
    true frame starts), D (data symbols of a frame), frame (samples of a sent frame), S"""
    rng = np.random.default_rng(seed)
    c = Capture()
    c.n_fft, c.mod, c.S = n_fft, mod, n_fft + n_fft // 4
    c.payloads = [bytes(rng.integers(0, 256, payload, dtype=np.uint8)) for _ in range(n_frames)]
    rx, noise = [], []
    for k, p in enumerate(c.payloads):
        tx = orc.encode(p, guard=True, modulation=mod, n_fft=n_fft)
        y = orc.channel(tx, snr, False, seed * 16 + k)[0]
        rx.append(y)
        noise.append(y - orc.channel(tx, 300.0, False, seed * 16 + k)[0])
        c.frame = len(tx)
    c.sigma2 = float(np.mean(np.abs(np.concatenate(noise)) ** 2))
    c.rms = float(np.sqrt(np.mean(np.abs(np.concatenate(rx)) ** 2)))
    g = lambda n: np.sqrt(c.sigma2 / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    delay = int(np.argmax(np.abs(orc.channel_taps())))
    parts, c.starts, at = [g(lead_of(n_fft))], [], lead_of(n_fft)
    for k, y in enumerate(rx):
        c.starts.append(at + delay)
        gap = g(GAPS[k % len(GAPS)] * (c.S // 80) if k + 1 < n_frames else TAIL)
        parts += [y, gap]
        at += len(y) + len(gap)
    z = np.concatenate(parts)
    c.clean = z.astype(np.complex64)
    c.x = (z + factor * c.rms * DC_PHASE).astype(np.complex64)
    c.D = c.frame // c.S - 10
    return c
