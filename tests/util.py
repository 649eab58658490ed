"""Shared helpers for the parity tests: seeded synthetic inputs and comparison rules.

Inputs handed to the GPU are fc32 (the wire format, src/utils.rs:228-254); the oracle is fed the SAME
f32-rounded samples widened to f64 (bytes_to_sig), so both sides see identical data.
"""
import numpy as np

TAPS = None


def fc32(x):
    """Round complex128 to the fc32 wire format and widen back (what both GPU and oracle consume)."""
    return np.asarray(x).astype(np.complex64)


def wide(x32):
    return np.asarray(x32).astype(np.complex128)


def rel_err(a, b):
    """norm-relative error (per-bin relative error is unbounded at null carriers)."""
    a = np.asarray(a).astype(np.complex128).ravel()
    b = np.asarray(b).astype(np.complex128).ravel()
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (n if n > 0 else 1.0))


def awgn(rng, shape, sigma):
    return sigma * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


def make_symbols(orc, rng, n_sym, n_fft, guard, mod, snr_db=30.0):
    """Config-2 style input: n_sym OFDM symbols (CP + N) carrying random points, AWGN, H == 1.
    Returns (samples complex64 [n_sym*S], payload bytes)."""
    nd = orc.data_carriers(n_fft, guard)
    nbytes = n_sym * nd * mod // 8
    data = bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))
    pts = orc.modulate(data, mod)
    out = []
    for s in range(n_sym):
        blk, used = orc.encode_block(pts[s * nd:(s + 1) * nd], n_fft, guard)
        out.append(orc.prefix_block(blk))
    x = np.concatenate(out)
    p = np.mean(np.abs(x) ** 2)
    x = x + awgn(rng, x.shape, np.sqrt(p / 10 ** (snr_db / 10) / 2))
    return fc32(x), data


def make_symbols_np(orc, rng, n_sym, n_fft, guard, mod, snr_db=30.0):
    """make_symbols for large batches: the same construction (modulate -> encode_block -> prefix_block -> AWGN) with the
    per-symbol oracle calls replaced by numpy array operations (the carrier map comes from the oracle's carrier_class,
    the points from the oracle's modulate).  Only an INPUT generator: expected outputs always come from the oracle."""
    nd = orc.data_carriers(n_fft, guard)
    nbytes = n_sym * nd * mod // 8
    data = bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))
    pts = np.asarray(orc.modulate(data, mod)).reshape(n_sym, nd)
    cls = np.array([orc.carrier_class(i, n_fft, guard) for i in range(n_fft)])
    bins = np.zeros((n_sym, n_fft), np.complex128)
    bins[:, cls == 0] = pts
    bins[:, cls == 2] = 1.0
    t = np.fft.ifft(bins, axis=1)
    cp = n_fft // 4
    x = np.concatenate([t[:, n_fft - cp:], t], axis=1).reshape(-1)
    p = np.mean(np.abs(x) ** 2)
    x = x + awgn(rng, x.shape, np.sqrt(p / 10 ** (snr_db / 10) / 2))
    return fc32(x), data


def _raw_data_symbols(orc, stream, n_fft, guard, mod):
    """prefix_block(encode_block(modulate(stream))) of a whole byte stream, unscaled, as orc.encode builds its data symbols"""
    pts = orc.modulate(bytes(stream), mod)
    out, used = [], 0
    while used < pts.size:
        blk, c = orc.encode_block(pts[used:], n_fft, guard)
        used += c
        out.append(orc.prefix_block(blk))
    return np.concatenate(out)


def forge_frame(orc, stream: bytes, n_fft, guard, mod, allow_louder=False):
    """A frame whose 16-byte length header is whatever `stream` starts with: `stream` is the WHOLE byte stream of the data symbols,
    header included.  The ten header blocks and the frame's scale come from orc.encode of a seeded random payload of the same
    length (an honest frame that is no louder than its header): scale = honest sample / raw sample at the largest raw sample of
    the honest data symbols, which normalize (src/transmitter.rs:183-194) makes one real constant per frame.
    Returns complex128 [(10 + D) S].
    Only for streams that are no louder than the header blocks (the normalisation then does not depend on the data symbols): asserted.
    allow_louder: a stream that is louder (a run of equal bits that fills a symbol with equal points: a header of ones in BPSK, a
    code word of zeros in 64-QAM) is passed through the oracle's normalize instead, which divides the whole frame by the new
    maximum as orc.encode would have."""
    stream = bytes(stream)
    assert len(stream) >= 16
    S = n_fft + n_fft // 4
    n_body = len(stream) - 16
    peak = lambda x: max(x.real.max(), x.imag.max())          # normalize's maximum: signed, over re and im
    for seed in range(8):                                     # the first filler whose frame is no louder than its header
        filler = bytes(np.random.default_rng([n_body, seed]).integers(0, 256, n_body, dtype=np.uint8))
        honest = orc.encode(filler, guard, mod, n_fft)
        if peak(honest[:10 * S]) == 1.0:
            break
    assert peak(honest[:10 * S]) == peak(honest) == 1.0, "no honest frame of this length with full scale in its header"
    raw_honest = _raw_data_symbols(orc, n_body.to_bytes(16, "little") + filler, n_fft, guard, mod)
    raw = _raw_data_symbols(orc, stream, n_fft, guard, mod)
    assert honest.size == 10 * S + raw_honest.size and raw.size == raw_honest.size
    k = int(np.argmax(np.abs(raw_honest)))
    ratio = honest[10 * S + k] / raw_honest[k]
    assert abs(ratio.imag) <= 1e-12 * abs(ratio), ratio
    frame = np.concatenate([honest[:10 * S], ratio.real * raw])
    if allow_louder:
        return orc.normalize(frame)
    assert peak(frame[10 * S:]) <= 1.0, "a forged frame louder than its header is not handled"
    return frame


def header_values(B, extra_lo=()):
    """The (lo, hi) halves of the forged u128 length headers, for a decoder that sees a body of B bytes: 26 pairs, then (lo, 0) for
    every extra_lo.  Small lengths, lengths around B, lengths around the 32-bit and 64-bit edges, and a high half that is not 0."""
    los = [0, 1, 2, 3, 4, 6, 7, 8, 13, 14, B - 8, B - 7, B - 1, B, B + 1,
           2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 32 + B - 1, 2 ** 63, 2 ** 64 - 1]
    pairs = [(lo, 0) for lo in los] + [(5, 1), (0, 2 ** 63), (2 ** 64 - 1, 2 ** 64 - 1)] + [(lo, 0) for lo in extra_lo]
    assert all(0 <= lo < 2 ** 64 and 0 <= hi < 2 ** 64 for lo, hi in pairs)
    return pairs


def header_bytes(lo, hi):
    return int(lo).to_bytes(8, "little") + int(hi).to_bytes(8, "little")


def header_rule(lo, hi, body):
    """src/receiver.rs:85-95 in plain integers: the bytes kept of a body of `body` bytes"""
    return lo if (hi == 0 and lo < body) else body


def through_channel(orc, rng, tx, span, delay, f_delta, snr_db=30.0, taps=True, data_start=None):
    """Config-3 style capture: `delay` leading zeros, FIR CHANNEL (src/channel.rs:26-31), CFO
    exp(+j f (i+1)) (channel.rs:58-62), AWGN, cut/padded to `span` samples.
    The SNR is set against the power of the DATA symbols (tx[data_start:]): the lock / preamble blocks are
    time-domain constants while IFFT output shrinks as 1/N, so for large N the header would dominate."""
    y = np.convolve(tx, orc.channel_taps())[: tx.size + 24] if taps else tx.copy()
    buf = np.zeros(span, np.complex128)
    n = min(span - delay, y.size)
    buf[delay:delay + n] = y[:n]
    buf *= np.exp(1j * f_delta * np.arange(1, span + 1))
    p = np.mean(np.abs(y[data_start or 0:]) ** 2)
    if snr_db is not None:
        buf += awgn(rng, span, np.sqrt(p / 10 ** (snr_db / 10) / 2))
    return fc32(buf)


def decision_margin(soft, mod):
    """Distance of every soft point to its nearest hard-decision boundary, per axis (in the same units as the
    points).  Used to excuse a differing decision ONLY where the oracle's own value sits within the
    floating-point tolerance of a boundary."""
    soft = np.asarray(soft)
    if mod == 1:
        return np.abs(soft.real)
    m = mod // 2
    M = 1 << m
    def axis(x):
        u = x * (M - 1) / 2.0          # boundaries at integers (inner ones only matter up to the clamp)
        d = np.abs(u - np.round(u))
        outer = np.abs(u) > (M / 2 - 0.5)  # beyond the outermost boundary: clamped, no boundary nearby
        return np.where(outer, np.inf, d) * 2.0 / (M - 1)
    return np.minimum(axis(soft.real), axis(soft.imag))


def assert_bytes_match(got: bytes, want: bytes, soft, mod, nd_per_byte_group=None, tol=1e-5, what=""):
    """Bit-exact byte equality, excusing only decisions whose oracle soft value lies within `tol` (relative to
    the constellation scale 1.0) of a boundary.  Returns the number of excused points (normally 0)."""
    assert len(got) == len(want), f"{what}: length {len(got)} != {len(want)}"
    if got == want:
        return 0
    g = np.unpackbits(np.frombuffer(got, np.uint8), bitorder="little")
    w = np.unpackbits(np.frombuffer(want, np.uint8), bitorder="little")
    bad_pts = np.unique(np.nonzero(g != w)[0] // mod)
    margin = decision_margin(np.asarray(soft)[bad_pts], mod)
    assert np.all(margin < tol), f"{what}: {np.sum(margin >= tol)} decisions differ away from any boundary"
    return int(bad_pts.size)
