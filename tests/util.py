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


def make_capture(orc, rng, mod, guard, payload, span, delay, fd, snr_db=30.0, n_fft=64):
    tx = orc.encode(payload, guard, mod, n_fft)
    return through_channel(orc, rng, tx, span, delay, fd, snr_db), tx


# the (threshold, n_lags, frame_len) searches k_sc80's corner-case captures are put through: other thresholds, bounded searches,
# captures barely longer than one window
SC80_SPAN = 2176
SC80_SEARCHES = ((0.5, 0, SC80_SPAN), (0.37, 0, SC80_SPAN), (0.81, 300, SC80_SPAN), (0.5, 0, 400), (0.5, 0, 322), (0.5, 45, 2000))


def sc80_corner_captures(orc):
    """The N = 64 captures k_sc80 is tested on (seeded): -> (13 ordinary captures of SC80_SPAN samples, packets at delays 1 .. 79 through
    the FIR channel with CFO at 30 dB; the five dynamic-range captures [zeros then a noiseless frame, a burst then EXACT zeros then
    the frame, a burst then a packet 75 dB down, a burst 50 dB up in front of a packet, an ordinary capture])."""
    rng = np.random.default_rng(80)
    span = SC80_SPAN
    tx = orc.encode(bytes(rng.integers(0, 256, 560, dtype=np.uint8)), True, orc.QAM64)
    ordinary = [through_channel(orc, rng, tx, span, int(d), float(fd), 30.0) for d, fd in
                zip(rng.integers(1, 80, 13), (rng.random(13) * 1.9 - 0.95) * np.pi / 80)]
    clean = np.zeros(span, complex); clean[500:500 + 1600] = tx[:1600]            # zeros, then a noiseless frame: exact, stays on the fast path
    lead = fc32(clean)
    gap = clean.copy(); gap[3:40] += 30.0 * (rng.standard_normal(37) + 1j * rng.standard_normal(37))      # burst, EXACT zeros, frame
    quiet = 1e-3 * wide(ordinary[0]); quiet[5:25] += 3.0 * (rng.standard_normal(20) + 1j * rng.standard_normal(20))     # burst, then a packet 75 dB down
    hot = wide(ordinary[1]).copy(); hot[2:14] += 40.0 * (rng.standard_normal(12) + 1j * rng.standard_normal(12))       # burst 50 dB up: trusted
    return ordinary, np.stack([lead, fc32(gap), fc32(quiet), fc32(hot), ordinary[2]])


def long_period_captures(orc, rng, n, mod, nbytes, nf, span):
    """nf frames of nbytes through the FIR channel (delay below one period, CFO, 32 dB), a noise-only capture and the first capture cut
    inside its preamble: [nf + 2, span] complex64"""
    S = n + n // 4
    caps = []
    for f in range(nf):
        tx = orc.encode(bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)), True, mod, n)
        d = int(rng.integers(1, S))
        fd = (rng.random() * 1.8 - 0.9) * np.pi / S
        caps.append(through_channel(orc, rng, tx, span, d, fd, 32.0, data_start=10 * S))
    caps.append(fc32(0.05 * (rng.standard_normal(span) + 1j * rng.standard_normal(span))))     # noise only
    cut = caps[0].copy(); cut[int(3.5 * S):] = 0                                               # ends inside the preamble
    caps.append(cut)
    return np.stack(caps)


def loud_payload(orc, n, mod, nbytes, sym=1, seed=0):
    """A payload whose data symbol `sym` has a time sample far above the header blocks' full scale (without guard bands every bin is a
    data carrier: each carrier gets the constellation point whose contribution to sample 1 of the symbol is largest)."""
    rng = np.random.default_rng(seed)
    sym_bytes = n * mod // 8
    pts = []
    for pat in range(1 << mod):                       # the point of every bit pattern (LSB-first stream bits)
        bits = np.array([(pat >> b) & 1 for b in range(8)], np.uint8)
        pts.append(orc.modulate(bytes(np.packbits(bits, bitorder="little")), mod)[0])
    pts = np.array(pts)
    freq, used = orc.encode_block(np.arange(1, n + 1, dtype=np.float64) + 0j, n, False)
    assert used == n
    pos_of = {int(round(freq[p].real)) - 1: p for p in range(n)}     # where stream point i lands in the frequency vector
    resp = np.empty(n, np.complex128)
    for p in range(n):                                # what a unit at bin position p contributes to time sample 1
        e = np.zeros(n, np.complex128)
        e[p] = 1.0
        resp[p] = orc.prefix_block(e)[n // 4 + 1]
    pat = np.array([int(np.argmax((pts * resp[pos_of[i]]).real)) for i in range(n)])
    bits = ((pat[:, None] >> np.arange(mod)[None, :]) & 1).astype(np.uint8).reshape(-1)
    loud = np.packbits(bits, bitorder="little")
    pay = rng.integers(0, 256, nbytes, dtype=np.uint8)
    lo = sym * sym_bytes - 16
    assert loud.size == sym_bytes and lo >= 0 and lo + sym_bytes <= nbytes
    pay[lo: lo + sym_bytes] = loud
    return pay
