"""EXT-6 link quality (include/ofdm_hip.h): the definition, in numpy f64.  The reference measures nothing of the
kind, so this file is what ofdm_rx_quality_batch (k_linkq) and Context.link_quality are held to.

Per frame f, with o = offset[f], fd = f_delta[f], S = N + cp, samples at or beyond frame_len reading as zero, and the derotation of
estimate_channel (sample id n counted from o: y[n] = x[o + n] exp(-j fd n)):

  training part -- counted only if o >= 0 and o + 10 S <= frame_len, else valid = 0 and every field of the row is 0
    y_b[n]     derotated sample (5 + b) S + cp + n, b < 5, n < N;  ybar = mean_b y_b;  Ybar = FFT(ybar), unnormalised
    noise_var  (1/4) sum_b sum_n |y_b[n] - ybar[n]|^2  ==  (1 / (4 N)) sum_k sum_b |Y_b[k] - Ybar[k]|^2      (Parseval)
    gain       sum_{k in D} (|Ybar[k]|^2 - noise_var / 5) / sum_{k in D} |t_k|^2,  D = the data carriers, t = the training table
    snr        max(gain, 0) Es / noise_var, linear; +inf if noise_var == 0
    llr_unit   4 mean_{k in D} |hk[k]|^2 / ((M - 1)^2 noise_var), M = levels per axis (2 for BPSK and QPSK); the mean is 1 without hk
  data part -- point j (rx_demod's stream order from data symbol first_symbol, nd = |D| points per symbol) is counted iff
    j < n_points[f], j // nd < syms_per_frame and o + (first_symbol + j // nd + 1) S <= frame_len
    x          the equalised (Y / hk), pilot-phase-corrected point: what rx_demod delivers as `soft`
    evm2       sum |x - xh|^2 / sum |xh|^2 over the counted points, xh = map(demap(x)); 0 when nothing is counted
    points     the number counted

quality(..., f32=True) restates the same quantities in the device's precision and ORDER of operations -- complex64 samples, the
radix-8 / radix-4 Stockham passes of device_common.hpp with their twiddle chains, the one-pass (Welford) noise sum, per-thread serial
sums followed by the butterfly tree of symbol_sum -- so that its distance from the f64 definition sets the tolerance the kernel gets."""
import numpy as np

Q_VALID, Q_NOISE_VAR, Q_GAIN, Q_SNR, Q_LLR_UNIT, Q_EVM2, Q_POINTS = range(7)
FIELDS = 8
NAMES = ("valid", "noise_var", "gain", "snr", "llr_unit", "evm2", "points")


def levels(mod):
    return 2 if mod <= 2 else 1 << (mod // 2)


def es(mod):
    """mean |point|^2 of the constellation (EXT-1: axis levels (2 l - (M - 1)) / (M - 1))"""
    if mod <= 2:
        return float(mod)
    M = levels(mod)
    return 2.0 * (M + 1) / (3.0 * (M - 1))


def carrier_masks(n_fft, guard):
    """(data, pilot) masks over the bins: the reference's 64-bin map tiled K = n_fft / 64 times (EXT-4)"""
    c = np.arange(n_fft) // (n_fft // 64)
    if not guard:
        return np.ones(n_fft, bool), np.zeros(n_fft, bool)
    null = (c >= 59) | (c <= 5) | (c == 32)
    pilot = (c == 6) | (c == 25) | (c == 39) | (c == 58)
    return ~null & ~pilot, pilot


def slice_points(x, mod):
    """xh = map(demap(x)): the constellation point of the hard decision (src/receiver.rs:147-190, EXT-1), NaN decided as level 0"""
    x = np.asarray(x)
    if mod == 1:
        return np.where(x.real > 0, 1.0, -1.0) + 0j
    if mod == 2:
        re, im = x.real, x.imag
        i = np.where(re >= 0, 1.0, -1.0)
        q = np.where((re >= 0) & (im >= 0), 1.0, np.where((re >= 0) & (im <= 0), -1.0, np.where((re < 0) & (im > 0), 1.0, -1.0)))
        return i + 1j * q
    M = levels(mod)

    def axis(v):
        with np.errstate(invalid="ignore"):
            lvl = np.clip(np.floor(v * (M - 1) * 0.5) + M // 2, 0, M - 1)
        lvl = np.where(np.isnan(v), 0, lvl)
        return (2 * lvl - (M - 1)) / (M - 1)
    return axis(x.real) + 1j * axis(x.imag)


# ------------------------------------------------------------------------------------------------ the device's FFT, restated
def _plan(n):
    log2 = n.bit_length() - 1
    b4 = 0 if log2 % 3 == 0 else (1 if log2 % 3 == 2 else 2)
    a8 = (log2 - 2 * b4) // 3
    return a8, b4


def _mul_mj(a):
    return (a.imag - 1j * a.real).astype(np.complex64)


def _bfly8(v):
    h = np.float32(0.70710678118654752440)
    a0, a4 = v[0] + v[4], v[0] - v[4]
    a1, a5 = v[1] + v[5], v[1] - v[5]
    a2, a6 = v[2] + v[6], v[2] - v[6]
    a3, a7 = v[3] + v[7], v[3] - v[7]
    a5 = ((a5.real + a5.imag) * h + 1j * ((a5.imag - a5.real) * h)).astype(np.complex64)
    a6 = _mul_mj(a6)
    a7 = ((a7.imag - a7.real) * h + 1j * ((-a7.real - a7.imag) * h)).astype(np.complex64)
    b0, b2 = a0 + a2, a0 - a2
    b1, b3 = a1 + a3, _mul_mj(a1 - a3)
    b4, b6 = a4 + a6, a4 - a6
    b5, b7 = a5 + a7, _mul_mj(a5 - a7)
    return [b0 + b1, b4 + b5, b2 + b3, b6 + b7, b0 - b1, b4 - b5, b2 - b3, b6 - b7]


def _bfly4(v, o):
    s0, d0 = v[o] + v[o + 4], v[o] - v[o + 4]
    s1, d1 = v[o + 2] + v[o + 6], _mul_mj(v[o + 2] - v[o + 6])
    v[o], v[o + 4], v[o + 2], v[o + 6] = s0 + s1, s0 - s1, d0 + d1, d0 - d1


def fft_c64(x):
    """fft_symbol<N, false> of device_common.hpp over the last axis, in complex64: the same passes, butterflies and twiddle chains"""
    x = np.asarray(x, np.complex64)
    n = x.shape[-1]
    T = n // 8
    a8, b4 = _plan(n)
    passes = a8 + b4
    tw = np.exp(-2j * np.pi * np.arange(n) / n).astype(np.complex64)
    t = np.arange(T)
    v = [x[..., m * T:(m + 1) * T].copy() for m in range(8)]
    buf = np.zeros(x.shape, np.complex64)
    ns = 1
    for p in range(passes):
        if p > 0:
            v = [buf[..., t + m * T] for m in range(8)]
        if p < a8:
            if p > 0:
                w1 = tw[(t % ns) * (n // (ns * 8))]
                wr = w1
                for r in range(1, 8):
                    v[r] = v[r] * wr
                    if r < 7:
                        wr = wr * w1
            v = _bfly8(v)
            if p < passes - 1:
                base = (t // ns) * ns * 8 + t % ns
                for r in range(8):
                    buf[..., base + r * ns] = v[r]
            ns *= 8
        else:
            step = n // (ns * 4)
            wa1, wb1 = tw[(t % ns) * step], tw[((t + T) % ns) * step]
            wa, wb = wa1, wb1
            for r in range(1, 4):
                v[2 * r] = v[2 * r] * wa
                v[2 * r + 1] = v[2 * r + 1] * wb
                if r < 3:
                    wa, wb = wa * wa1, wb * wb1
            _bfly4(v, 0)
            _bfly4(v, 1)
            if p < passes - 1:
                ja, jb = t, t + T
                basea, baseb = (ja // ns) * ns * 4 + ja % ns, (jb // ns) * ns * 4 + jb % ns
                for r in range(4):
                    buf[..., basea + r * ns] = v[2 * r]
                    buf[..., baseb + r * ns] = v[2 * r + 1]
            ns *= 4
    return np.concatenate(v, axis=-1)


def _symbol_sum32(part):
    """symbol_sum: part [..., T] float32 per-thread sums -> [...]: xor butterfly over the wavefront's lanes, then the wavefronts in order"""
    part = np.asarray(part, np.float32)
    T = part.shape[-1]
    W = min(T, 64)
    x = part.reshape(part.shape[:-1] + (T // W, W))
    lane = np.arange(W)
    m = W // 2
    while m >= 1:
        x = x + x[..., lane ^ m]
        m >>= 1
    s = np.zeros(x.shape[:-2], np.float32)
    for i in range(T // W):
        s = s + x[..., i, 0]
    return s


def _threads(a, T):
    """[..., N] -> [..., 8, T]: element [m, t] is bin / sample t + m T, the eight a thread holds"""
    return a.reshape(a.shape[:-1] + (8, T))


def _phasor(turns, n, f32):
    ph = turns * n
    ph = ph - np.rint(ph)
    z = np.exp(-2j * np.pi * ph)
    return z.astype(np.complex64) if f32 else z


# ------------------------------------------------------------------------------------------------ the definition
def quality(rx, n_fft, guard, mod, training, syms_per_frame=0, first_symbol=10, n_points=None, offset=None, f_delta=None, hk=None,
            status=None, frame_len=None, f32=False, detail=False):
    """rows [n_frames, FIELDS] (float64 values; with f32 the device-precision restatement).  rx: [n_frames, stride] complex; hk: None,
    [N] shared or [n_frames, N].  detail: also a dict with `noise_var_bins` (the bin-domain form of noise_var), `soft` (per frame the
    counted points x, f64 path) and `sum_ref` (per frame sum |xh|^2)."""
    rx = np.asarray(rx)
    F, stride = rx.shape
    N, cp = n_fft, n_fft // 4
    S, T = N + cp, N // 8
    frame_len = stride if frame_len is None else frame_len
    data, pilot = carrier_masks(N, guard)
    nd = int(data.sum())
    K = N // 64
    M = levels(mod)
    cdt, fdt = (np.complex64, np.float32) if f32 else (np.complex128, np.float64)
    t2 = float(np.sum(np.abs(np.asarray(training, np.complex128)[data]) ** 2))
    off = np.zeros(F, np.int64) if offset is None else np.asarray(offset, np.int64)
    fd = None if f_delta is None else np.asarray(f_delta, np.float64)
    npts = np.zeros(F, np.int64) if n_points is None else np.broadcast_to(np.asarray(n_points, np.int64), (F,))
    npts = np.clip(npts, 0, syms_per_frame * nd)
    alive = np.ones(F, bool) if status is None else (np.asarray(status) == 0)
    trained = alive & (off >= 0) & (off + 10 * S <= frame_len)
    whole = np.maximum((frame_len - off) // S - first_symbol, 0)
    nsym = np.where(trained, np.minimum(-(-npts // nd), whole), 0)

    def window(f, sym):  # the derotated N samples of symbol `sym` of frame f (all inside the capture when asked for)
        a = off[f] + sym * S + cp
        y = rx[f, a:a + N].astype(cdt)
        if fd is not None:
            turns = fd[f] * 0.15915494309189533577
            if f32:  # the device's chain: one phasor per thread, stepped T samples at a time
                ph, st = _phasor(turns, sym * S + cp + np.arange(T), True), _phasor(turns, T, True)
                y = y.reshape(8, T).copy()
                for m in range(8):
                    y[m] = y[m] * ph
                    ph = ph * st
                y = y.reshape(N)
            else:
                y = y * _phasor(turns, sym * S + cp + np.arange(N), False)
        return y

    rows = np.zeros((F, FIELDS), np.float64)
    extra = {"noise_var_bins": np.zeros(F), "soft": [np.zeros(0, complex)] * F, "sum_ref": np.zeros(F)}
    with np.errstate(all="ignore"):
        for f in range(F):
            if not trained[f]:
                continue
            Y = np.stack([window(f, 5 + b) for b in range(5)])
            if f32:
                acc = np.zeros(N, np.complex64)
                part = np.zeros(T, np.float32)
                for b in range(5):  # Welford: deviations against the running mean before and after the block
                    ro = np.float32(0.0 if b == 0 else 1.0 / b)
                    rn = np.float32(1.0 / (b + 1))
                    old = Y[b] - ro * acc
                    acc = acc + Y[b]
                    new = Y[b] - rn * acc
                    term = _threads(old.real * new.real + old.imag * new.imag, T).astype(np.float32)
                    for m in range(8):
                        part = part + term[m]
                noise = _symbol_sum32(part) * np.float32(0.25)
                A = fft_c64(acc)
                pw = _threads(np.where(data, A.real * A.real + A.imag * A.imag, np.float32(0)).astype(np.float32), T)
                part = np.zeros(T, np.float32)
                for m in range(8):
                    part = part + pw[m]
                sig = _symbol_sum32(part)
                gain = (sig * np.float32(0.04) - np.float32(nd) * (noise * np.float32(0.2))) * np.float32(1.0 / t2)
            else:
                ybar = Y.mean(axis=0)
                noise = np.sum(np.abs(Y - ybar) ** 2) / 4.0
                Yb = np.fft.fft(Y, axis=-1)
                Ybar = np.fft.fft(ybar)
                extra["noise_var_bins"][f] = np.sum(np.abs(Yb - Ybar) ** 2) / (4.0 * N)
                gain = np.sum(np.abs(Ybar[data]) ** 2 - noise / 5.0) / t2
            h = None if hk is None else np.asarray(hk if np.ndim(hk) == 1 else hk[f]).astype(cdt)
            if h is None:
                h2 = fdt(1.0)
            elif f32:
                n2 = (h.real * h.real + h.imag * h.imag).astype(np.float32)
                pw = _threads(np.where(data, n2, np.float32(0)), T)
                part = np.zeros(T, np.float32)
                for m in range(8):
                    part = part + pw[m]
                h2 = _symbol_sum32(part) / np.float32(nd)
            else:
                h2 = np.mean(np.abs(h[data]) ** 2)
            # ---- data part
            e_part, r_part, cnt = np.zeros(T, fdt), np.zeros(T, fdt), 0
            soft = []
            q_of_bin = np.cumsum(data) - 1  # stream position of a data bin inside its symbol
            for k in range(int(nsym[f])):
                X = fft_c64(window(f, first_symbol + k)) if f32 else np.fft.fft(window(f, first_symbol + k))
                if h is not None:
                    if f32:
                        q = X * np.conj(h)
                        X = (q * (np.float32(1.0) / n2)).astype(np.complex64)
                    else:
                        X = X / h
                if guard:
                    ang = np.arctan2(X.imag, X.real).astype(fdt) / fdt(np.pi)  # in units of pi, as the device sums them
                    if f32:
                        pa = _threads(np.where(pilot, ang, np.float32(0)).astype(np.float32), T)
                        part = np.zeros(T, np.float32)
                        for m in range(8):
                            part = part + pa[m]
                        phase = _symbol_sum32(part) / np.float32(4.0 * K)
                    else:
                        phase = np.sum(ang[pilot]) / (4.0 * K)
                    rot = np.exp(-1j * np.pi * np.float64(phase)).astype(cdt)
                    X = (X * rot).astype(cdt)
                counted = data & (k * nd + q_of_bin < npts[f])
                xh = slice_points(X, mod).astype(cdt)
                d = X - xh
                e = np.where(counted, (d.real * d.real + d.imag * d.imag).astype(fdt), fdt(0))
                r = np.where(counted, (xh.real * xh.real + xh.imag * xh.imag).astype(fdt), fdt(0))
                e, r = _threads(e, T), _threads(r, T)
                for m in range(8):
                    e_part = e_part + e[m]
                    r_part = r_part + r[m]
                cnt += int(counted.sum())
                soft.append(X[counted])
            if f32:
                err, ref = _symbol_sum32(e_part), _symbol_sum32(r_part)
            else:
                err, ref = np.sum(e_part), np.sum(r_part)
            if soft:
                extra["soft"][f] = np.concatenate(soft)
            extra["sum_ref"][f] = float(ref)
            noise = fdt(noise)
            rows[f, Q_VALID] = 1.0
            rows[f, Q_NOISE_VAR] = noise
            rows[f, Q_GAIN] = gain
            rows[f, Q_SNR] = np.inf if noise == 0 else fdt(np.fmax(gain, 0)) * fdt(es(mod)) / noise
            rows[f, Q_LLR_UNIT] = fdt(4.0) * fdt(h2) / (fdt((M - 1) ** 2) * noise)
            rows[f, Q_EVM2] = err / ref if cnt else 0.0
            rows[f, Q_POINTS] = cnt
    return (rows, extra) if detail else rows
