"""numpy restatement of the soft-decision contract (include/ofdm_hip.h, "soft decisions").

Brute force on purpose: the LLR is a minimum over all M levels of an axis, the soft Hamming(7,4) decoder a maximum over all 16
codewords.  The kernels use closed forms (ofdm_amd/csrc/device_common.hpp); `axis_llr_closed` restates that form here so that a
CPU test can hold it against the brute force.
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


def frame_llrs(points, bps, scale, weights=None):
    """points [n_frames, syms, nd] (rx_demod's soft output, reshaped), weights [n_frames or 1, nd] or None -> int8
    [n_frames, syms * nd * bps], LLR j = bit j of the stream rx_demod packs LSB-first"""
    lam = point_llr(points, bps)                                  # [F, S, nd, bps]
    w = 1.0 if weights is None else np.asarray(weights)[:, None, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        y = scale * w * lam
    return quantise(y).reshape(lam.shape[0], -1)


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
