"""The digital down-converter of EXT-16 (include/ofdm_hip.h, "a digital down-converter") in numpy: THE definition the host functions
ofdm_ddc / ofdm_ddc_sc16 and the device handle ofdm_ddc_* are held to, bit for bit (tests/test_ddc_cpu.py, tests/test_gpu_ddc.py), and
a stateful mirror of the handle that shows the rule does not care how a stream is cut.

    rotors   C[i] = f32(cos, sin)(2 pi i / 1024), F[i] = f32(cos, sin)(2 pi i / 2^20), i < 1024: an INPUT here (the library hands out its
             own bytes, ofdm_ddc_rotor_tables; tables() is numpy's f64 value of them, which the CPU test holds the library's to)
    a (x) b  re = fma(a.re, b.re, -(a.im * b.im)), im = fma(a.re, b.im, a.im * b.re), the inner product one rounded f32 multiply
    mixer    p = (n * inc) mod 2^20 in integers, n the absolute index; r = C[p >> 10] (x) F[p & 1023]; v[n] = x[n] (x) r
    filter   y[m] = sum_k h[k] v[m D + k], 0 <= m < M(n), each part from +0.0 in ascending k as acc = fma(h[k], v.part, acc);
             M(n) = 0 for n < T, else (n - T) // D + 1

numpy has no f32 fma.  fma32 is exact: the product of two f32 is exact in f64 (24 + 24 bits); TwoSum with c gives s + e exactly; s is
rounded to odd (if e != 0 and the last mantissa bit of s is even, s moves one f64 step towards e), and rounding an f64 that was rounded to
odd to f32 is the single rounding of the exact value (53 >= 2 * 24 + 2).
"""
import numpy as np

PHASE_BITS = 20
PHASE_MOD = 1 << PHASE_BITS
MAX_DECIM, MAX_TAPS = 64, 4096
TAPS_PER_PHASE = 24


def tables():
    """numpy's own rotor tables: f64 cos / sin rounded to f32, complex64 [1024] each (coarse, fine)"""
    i = np.arange(1024, dtype=np.float64)
    a, b = 2.0 * np.pi * i / 1024.0, 2.0 * np.pi * i / float(PHASE_MOD)
    mk = lambda t: (np.cos(t).astype(np.float32) + 1j * np.sin(t).astype(np.float32)).astype(np.complex64)
    return mk(a), mk(b)


def out_len(n, D, T):
    return 0 if n < T else (n - T) // D + 1


def inc_for(f0):
    """(-rint(f0 2^20)) mod 2^20"""
    return int(-np.rint(f0 * PHASE_MOD)) % PHASE_MOD


def design(D, taps_per_phase=TAPS_PER_PHASE):
    """the Hamming-windowed sinc of T = taps_per_phase D taps, cutoff 0.5 / D, f64, normalised to sum 1 -> (float32 taps, the f64 ones)"""
    T = D * taps_per_phase
    if T == 1:
        return np.ones(1, np.float32), np.ones(1)
    k = np.arange(T, dtype=np.float64)
    h = np.sinc((k - (T - 1) / 2.0) / D) * (0.54 - 0.46 * np.cos(2.0 * np.pi * k / (T - 1)))
    h = h / h.sum()
    return h.astype(np.float32), h


def widen(q, scale):
    """EXT-9's rule: (float)v * scale, one rounded f32 product per component; q int16 [n, 2] -> complex64 [n]"""
    q = np.asarray(q, np.int16).reshape(-1, 2)
    return np.ascontiguousarray(q.astype(np.float32) * np.float32(scale)).view(np.complex64).reshape(-1)


def fma32(a, b, c):
    """f32 fma(a, b, c) of float32 arrays (broadcast), exactly as IEEE defines it"""
    a, b, c = (np.asarray(t, np.float32).astype(np.float64) for t in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                   # exact
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)               # s + e = p + c exactly
        odd = (s.view(np.int64) & 1) != 0
        move = np.isfinite(s) & np.isfinite(e) & (e != 0) & ~odd
        s = np.where(move, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def cmul(a, b):
    """a (x) b of complex64 arrays"""
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    ar, ai, br, bi = a.real, a.imag, b.real, b.imag
    with np.errstate(invalid="ignore", over="ignore"):
        re = fma32(ar, br, -(ai * bi))              # float32 * float32 in numpy: one rounded f32 product
        im = fma32(ar, bi, ai * br)
    out = np.empty(np.broadcast(a, b).shape, np.complex64)
    out.real, out.imag = re, im
    return out


def phases(n0, n, inc):
    """(n * inc) mod 2^20 for the absolute indices n0 .. n0 + n - 1, in exact integers"""
    inc = int(inc) % PHASE_MOD
    idx = (np.arange(n, dtype=np.int64) + (int(n0) % PHASE_MOD)) % PHASE_MOD        # < 2^20, so the product stays below 2^40
    return (idx * inc) % PHASE_MOD


def mix(x, n0, inc, C, F):
    x = np.ascontiguousarray(x, np.complex64).reshape(-1)
    p = phases(n0, x.size, inc)
    return cmul(x, cmul(C[p >> 10], F[p & 1023]))


def fir(v, D, h, M):
    """y[m] = sum_k h[k] v[m D + k], m < M, ascending k, fma"""
    h = np.asarray(h, np.float32)
    re, im = np.zeros(M, np.float32), np.zeros(M, np.float32)
    if M == 0:
        return np.zeros(0, np.complex64)
    vr, vi = np.ascontiguousarray(v.real), np.ascontiguousarray(v.imag)
    last = (M - 1) * D
    for k in range(h.size):
        re = fma32(h[k], vr[k: k + last + 1: D], re)
        im = fma32(h[k], vi[k: k + last + 1: D], im)
    out = np.empty(M, np.complex64)
    out.real, out.imag = re, im
    return out


def ddc(x, D, inc, h, C, F, n0=0):
    """the definition on one whole stream: complex64 [n] -> complex64 [M(n)]; n0: the absolute index of x[0]"""
    h = np.asarray(h, np.float32).reshape(-1)
    assert 1 <= D <= MAX_DECIM and D <= h.size <= MAX_TAPS
    x = np.ascontiguousarray(x, np.complex64).reshape(-1)
    return fir(mix(x, n0, inc, C, F), D, h, out_len(x.size, D, h.size))


def ddc_sc16(q, scale, D, inc, h, C, F):
    return ddc(widen(q, scale), D, inc, h, C, F)


class Handle:
    """ofdm_ddc_handle in numpy: what the device handle carries from push to push -- the raw samples behind the last output (at most
    T - 1) and the absolute index -- and nothing else"""

    def __init__(self, D, inc, h, C, F):
        self.D, self.inc, self.h, self.C, self.F = D, inc, np.asarray(h, np.float32).reshape(-1), C, F
        self.T = self.h.size
        self.reset()

    def reset(self):
        self.total_in = 0
        self.carry = np.zeros(0, np.complex64)          # the samples D M(total_in) .. total_in - 1

    @property
    def total_out(self):
        return out_len(self.total_in, self.D, self.T)

    def push(self, x):
        x = np.ascontiguousarray(x, np.complex64).reshape(-1)
        if x.size == 0:
            return x.copy()
        m0 = self.total_out
        m1 = out_len(self.total_in + x.size, self.D, self.T)
        z = np.concatenate([self.carry, x])             # from sample D m0 on
        y = fir(mix(z, self.D * m0, self.inc, self.C, self.F), self.D, self.h, m1 - m0)
        self.total_in += x.size
        self.carry = z[self.D * (m1 - m0):].copy()
        assert self.carry.size <= self.T - 1 or self.T == 1 and self.carry.size == 0
        return y
