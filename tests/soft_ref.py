"""numpy restatement of the soft-decision contract (include/ofdm_hip.h, "soft decisions").

Brute force on purpose: the LLR is a minimum over all M levels of an axis, the soft Hamming(7,4) decoder a maximum over all 16
codewords.  The kernels use closed forms (ofdm_amd/csrc/device_common.hpp); `axis_llr_closed` restates that form here so that a
CPU test can hold it against the brute force.

Comparing int8 LLRs with an f64 reference (`llr_compare`).  With points, channel and weights from the f64 oracle the unrounded
product y = scale * w_k * Lambda is known to better than any f32 kernel can compute it, so an LLR is held to `quantise(y)` EXACTLY
unless y lies within eps of a rounding boundary (a half-integer k + 0.5, |k + 0.5| <= 127.5), where it may be the integer on the
other side of that boundary instead.  eps is not fitted to any kernel: it is the project's point tolerance, 1e-5 of the
constellation scale (tests/util.py assert_bytes_match `tol`, the parity tests' TOL), carried through the exact derivative

    eps = |dLambda/dx| * scale * w_k * 1e-5 / min(1, |H_k|) + |y| * 1e-5

|dLambda/dx| = (M - 1) |a_0 - a_1| / 2 with a_0, a_1 the nearest levels of bit value 0 and 1 (`llr_slope`; 1 for BPSK).  The
1 / |H_k| is there because equalisation divides the FFT's rounding error by |H_k|; the second term covers the f32 weight
nd |H_k|^2 / sum |H|^2.  Nothing in this module takes a value from the GPU.
"""
import numpy as np


def gray_bit(level, m, b):
    """axis bit b (b = 0: the Gray MSB) of level index `level` on an axis of 2^m levels"""
    g = np.asarray(level) ^ (np.asarray(level) >> 1)
    return (g >> (m - 1 - b)) & 1


def axis_llr(v, m):
    """Lambda_b(v) for b = 0 .. m-1 (last axis), v = x (M - 1): (min over bit-0 levels - min over bit-1 levels of (v - a)^2) / 4."""
    v = np.asarray(v, np.float64)
    M = 1 << m
    lv = np.arange(M)
    a = 2.0 * lv - (M - 1)
    d2 = (v[..., None] - a) ** 2
    out = np.empty(v.shape + (m,))
    for b in range(m):
        bit = gray_bit(lv, m, b)
        out[..., b] = (d2[..., bit == 0].min(-1) - d2[..., bit == 1].min(-1)) / 4.0
    return out


def axis_llr_closed(v, m):
    """The kernels' closed form (device_common.hpp llr_axis_bit): the nearest level l*, and the nearest level of the other bit value
    just across one of the two bit boundaries around l*."""
    v = np.asarray(v, np.float64)
    M = 1 << m
    ls = np.clip(np.floor(v / 2.0 + M / 2.0), 0, M - 1).astype(np.int64)
    a_s = 2.0 * ls - (M - 1)
    out = np.empty(v.shape + (m,))
    for b in range(m):
        j = m - 1 - b
        h = 1 << j
        r = (ls + h) >> (j + 1)
        lo, hi = (2 * r - 1) * h - 1, (2 * r + 1) * h
        alo, ahi = 2.0 * lo - (M - 1), 2.0 * hi - (M - 1)
        ao = np.where(lo < 0, ahi, np.where(hi > M - 1, alo, np.where(v - alo <= ahi - v, alo, ahi)))
        lam = 0.25 * (a_s - ao) * (2.0 * v - ao - a_s)
        out[..., b] = np.where(r & 1, lam, -lam)
    return out


def point_llr(z, bps):
    """Lambda of every bit of the points z (complex, any shape) in the demapper's stream order -> shape z.shape + (bps,)"""
    z = np.asarray(z, np.complex128)
    if bps == 1:
        return z.real[..., None].copy()
    m = bps // 2
    M = 1 << m
    return np.concatenate([axis_llr(z.real * (M - 1), m), axis_llr(z.imag * (M - 1), m)], axis=-1)


def quantise(y):
    """int8 L = clamp(rint(y), -127, 127); 0 where y is not finite"""
    y = np.asarray(y, np.float64)
    fin = np.isfinite(y)
    q = np.clip(np.rint(np.where(fin, y, 0.0)), -127, 127)
    return q.astype(np.int8)


def channel_weights(hk, data_bins):
    """w_k = |H_k|^2 / mean over the data carriers of |H|^2, at the data carriers in ordinal order; hk [..., N] -> [..., nd]"""
    hn = np.abs(np.asarray(hk, np.complex128)[..., data_bins]) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return hn / hn.mean(-1, keepdims=True)


def frame_llrs_unrounded(points, bps, scale, weights=None):
    """points [n_frames, syms, nd], weights [n_frames or 1, nd] or None -> the f64 products y = scale * w_k * Lambda before
    `quantise`, [n_frames, syms * nd * bps] in frame_llrs' order"""
    with np.errstate(invalid="ignore", over="ignore"):
        lam = point_llr(points, bps)                              # [F, S, nd, bps]
        w = 1.0 if weights is None else np.asarray(weights)[:, None, :, None]
        y = scale * w * lam
    return y.reshape(lam.shape[0], -1)


def frame_llrs(points, bps, scale, weights=None):
    """points [n_frames, syms, nd] (rx_demod's soft output, reshaped), weights [n_frames or 1, nd] or None -> int8
    [n_frames, syms * nd * bps], LLR j = bit j of the stream rx_demod packs LSB-first"""
    return quantise(frame_llrs_unrounded(points, bps, scale, weights))


def axis_slope(v, m):
    """|dLambda_b/dv| for b = 0 .. m-1 (last axis) from the brute force: |a_0 - a_1| / 2, a_0 / a_1 the nearest levels of bit 0 / 1"""
    v = np.asarray(v, np.float64)
    M = 1 << m
    lv = np.arange(M)
    a = 2.0 * lv - (M - 1)
    d2 = (v[..., None] - a) ** 2
    out = np.empty(v.shape + (m,))
    for b in range(m):
        bit = gray_bit(lv, m, b)
        a0 = a[bit == 0][np.argmin(d2[..., bit == 0], -1)]
        a1 = a[bit == 1][np.argmin(d2[..., bit == 1], -1)]
        out[..., b] = np.abs(a0 - a1) / 2.0
    return out


def llr_slope(points, bps):
    """|dLambda/dx| of every bit of the points (x = the coordinate of the bit's axis) -> shape points.shape + (bps,); non-finite points
    give whatever the brute force picks: their y is not finite either and `llr_compare` expects 0 there whatever eps is"""
    z = np.asarray(points, np.complex128)
    if bps == 1:
        return np.ones(z.shape + (1,))
    m = bps // 2
    M = 1 << m
    with np.errstate(invalid="ignore", over="ignore"):
        return (M - 1) * np.concatenate([axis_slope(z.real * (M - 1), m), axis_slope(z.imag * (M - 1), m)], axis=-1)


POINT_TOL = 1e-5   # of the constellation scale: tests/util.py assert_bytes_match `tol`, the parity tests' TOL


def llr_eps(points, bps, scale, weights=None, habs=None):
    """eps of the module docstring, in frame_llrs' order; weights / habs [n_frames or 1, nd] (|H_k| at the data carriers) or None"""
    sl = llr_slope(points, bps)
    w = 1.0 if weights is None else np.asarray(weights)[:, None, :, None]
    g = 1.0 if habs is None else np.minimum(1.0, np.asarray(habs))[:, None, :, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        y = scale * w * point_llr(points, bps)
        eps = sl * scale * w * POINT_TOL / g + np.abs(y) * POINT_TOL
    return eps.reshape(sl.shape[0], -1)


def llr_decided(y, eps):
    """True where y is farther than eps from every int8 rounding boundary k + 0.5, |k + 0.5| <= 127.5 (beyond 127.5 + eps the clamp
    decides), and where y is not finite (L = 0 by contract)"""
    y = np.asarray(y, np.float64)
    fin = np.isfinite(y)
    yc = np.where(fin, y, 0.0)
    nearest = np.clip(np.floor(yc) + 0.5, -127.5, 127.5)
    with np.errstate(invalid="ignore"):
        return ~fin | (np.abs(yc - nearest) > np.where(fin, eps, 0.0))


def llr_compare(got, y, eps, what=""):
    """The rule of the module docstring: decided elements equal quantise(y); an undecided element may instead be the integer across
    the boundary (q + 0.5 or q - 0.5) that y is within eps of, never more than 1 away and never beyond +-127.  Raises AssertionError
    with the count and the first offender; returns the excused (= undecided) share of the elements."""
    got = np.asarray(got).astype(np.int64)
    y = np.asarray(y, np.float64)
    eps = np.broadcast_to(np.asarray(eps, np.float64), y.shape)
    assert got.shape == y.shape, f"{what}: shape {got.shape} != {y.shape}"
    fin = np.isfinite(y)
    yc = np.where(fin, y, 0.0)
    e = np.where(fin & np.isfinite(eps), eps, 0.0)
    q = quantise(y).astype(np.int64)
    decided = llr_decided(y, eps)
    up = (got == q + 1) & (q < 127) & (q + 0.5 - yc <= e)
    down = (got == q - 1) & (q > -127) & (yc - (q - 0.5) <= e)
    ok = (got == q) | (~decided & (up | down))
    if not ok.all():
        i = np.unravel_index(int(np.argmax(~ok)), ok.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} LLRs outside the rule ({int((~ok & decided).sum())} of them decided); "
                             f"first at {i}: got {got[i]}, y = {y[i]!r}, eps = {eps[i]:.3g}")
    return float((~decided).mean()) if decided.size else 0.0


def ham_codeword(d):
    """ham_enc: data bits 0..3, parities d0^d1^d3, d0^d2^d3, d1^d2^d3 at bits 4..6"""
    d0, d1, d2, d3 = d & 1, (d >> 1) & 1, (d >> 2) & 1, (d >> 3) & 1
    return d | ((d0 ^ d1 ^ d3) << 4) | ((d0 ^ d2 ^ d3) << 5) | ((d1 ^ d2 ^ d3) << 6)


CODE_SIGNS = np.array([[2 * ((ham_codeword(d) >> i) & 1) - 1 for i in range(7)] for d in range(16)], np.int64)  # [16, 7]


def ham_decode_soft(llr):
    """ML decode: floor(n / 56) blocks of 8 codewords (7 LLRs each, low nibble first) -> 4 bytes per block; per codeword the d
    maximising sum_i (2 c_i - 1) L_i, ties to the smallest d"""
    llr = np.asarray(llr, np.int64).ravel()
    nb = llr.size // 56
    cw = llr[: nb * 56].reshape(nb * 8, 7)
    corr = cw @ CODE_SIGNS.T                                      # [n_cw, 16]
    d = np.argmax(corr, axis=1).astype(np.uint8)                  # first maximum = smallest nibble
    d = d.reshape(nb * 4, 2)
    return (d[:, 0] | (d[:, 1] << 4)).astype(np.uint8)


def unpack_bits(b):
    """bytes -> bits LSB-first (the stream order of the demapper's packing)"""
    return np.unpackbits(np.asarray(b, np.uint8), axis=-1, bitorder="little")


# ---------------------------------------------------------------------------------------------- oracle-anchored cases
def data_bins(orc, n, guard):
    return np.array([i for i in range(n) if orc.carrier_class(i, n, guard) == 0])


def through_h(x, n, h):
    """Symbols x [n_frames, syms * (n + n/4)] (fc32) through the per-frame or shared frequency response h ([n_frames or 1, n]) as a
    circular convolution per symbol, cyclic prefix rebuilt, rounded to fc32 again"""
    F = x.shape[0]
    cp = n // 4
    t = np.asarray(x, np.complex128).reshape(F, -1, n + cp)[:, :, cp:]
    t = np.fft.ifft(np.fft.fft(t, axis=-1) * np.asarray(h)[:, None, :], axis=-1)
    return np.concatenate([t[..., n - cp:], t], axis=-1).reshape(F, -1).astype(np.complex64)


def oracle_llr_reference(orc, x, n, guard, mod, scale, hk=None):
    """The f64 side of one rx_llr call on symbol streams: x [n_frames, syms * (n + n/4)] fc32 (the GPU's input), hk None, [n] (shared) or
    [n_frames, n] fc32 (the GPU's channel).  Everything is computed by the oracle and numpy from the widened inputs ->
    dict(y, eps [n_frames, syms * nd * mod], bits: the oracle's hard bits in the same order)"""
    F = x.shape[0]
    bins = data_bins(orc, n, guard)
    h = None if hk is None else np.asarray(hk).astype(np.complex128).reshape(-1, n)
    pts, bits = [], []
    for f in range(F):
        hf = None if h is None else h[f if h.shape[0] > 1 else 0]
        with np.errstate(all="ignore"):
            by, soft = orc.rx_demod(np.asarray(x[f]).astype(np.complex128), n, guard, mod, hk=hf, want_soft=True)
        pts.append(soft.reshape(-1, len(bins)))
        bits.append(unpack_bits(np.frombuffer(by, np.uint8)))
    pts = np.stack(pts)
    w = None if h is None else channel_weights(h, bins)
    ha = None if h is None else np.abs(h[:, bins])
    return {"y": frame_llrs_unrounded(pts, mod, scale, w), "eps": llr_eps(pts, mod, scale, w, ha), "bits": np.stack(bits), "points": pts,
            "weights": w}


def assert_signs(got, ref, what=""):
    """every decided element with |y| >= 0.5 + eps carries the sign of the ORACLE's hard bit (positive = bit 1)"""
    y, eps = ref["y"], ref["eps"]
    with np.errstate(invalid="ignore"):
        sure = llr_decided(y, eps) & np.isfinite(y) & (np.abs(y) >= 0.5 + eps)
    got = np.asarray(got)
    assert ((got > 0) == (ref["bits"] == 1))[sure].all() and (got != 0)[sure].all(), what
