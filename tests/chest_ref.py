"""EXT-5 channel-estimate denoising (include/ofdm_hip.h): the definition, in numpy f64.  The reference has no
such stage, so this file is what ofdm_chest_matrix, k_chest_solve and the OFDM_CHEST_WLS receive mode are held to.

    W_k = |t_k|^2                          t = the context's training table
    window: L_h = N / 4 taps at delays n in [-pre, L_h - pre) mod N, pre = L_h / 4
    h^ = argmin_h sum_k W_k |H^_k - sum_n h_n e^{-2 pi i k n / N}|^2
       = R^-1 g,   g_n = sum_k W_k H^_k e^{+2 pi i k n / N},   R[n, m] = r[n - m],   r[d] = sum_k W_k e^{+2 pi i k d / N}
    H'_k = sum_n h^_n e^{-2 pi i k n / N}
W_k H^_k counts as 0 where t_k = 0."""
import numpy as np


def window(n_fft):
    """(first_tap, n_taps) = (-pre, L_h)"""
    lh = n_fft // 4
    return -(lh // 4), lh


def window_index(n_fft):
    """the window's delays as indices into a row of n_fft taps"""
    first, lh = window(n_fft)
    return (np.arange(lh) + first) % n_fft


def weights(training):
    return np.abs(np.asarray(training, np.complex128)) ** 2


def rmatrix(training, n_fft):
    """R: Hermitian, Toeplitz, positive definite; independent of the window's offset"""
    lh = n_fft // 4
    r = n_fft * np.fft.ifft(weights(training))
    d = np.arange(lh)[:, None] - np.arange(lh)[None, :]
    return r[d % n_fft]


def rinv(training, n_fft):
    return np.linalg.inv(rmatrix(training, n_fft))


def smooth(h_ls, training, n_fft):
    """rows of n_fft bins -> rows of n_fft bins, f64"""
    h_ls = np.asarray(h_ls, np.complex128)
    rows = h_ls.reshape(-1, n_fft)
    w = weights(training)
    a = np.where(w == 0, 0, w * np.where(w == 0, 0, rows))
    idx = window_index(n_fft)
    g = n_fft * np.fft.ifft(a, axis=-1)[:, idx]
    h = g @ rinv(training, n_fft).T
    full = np.zeros_like(rows)
    full[:, idx] = h
    return np.fft.fft(full, axis=-1).reshape(h_ls.shape)


def smooth_c64(h_ls, training, n_fft):
    """The same steps with every stage's result rounded to complex64 and the contraction carried out in complex64: the precision the
    device path works at (f32 tables, f32 FFTs, f32 accumulation), in one particular summation order.  Its distance from smooth()
    sets the tolerance the kernel is given."""
    c64 = np.complex64
    rows = np.asarray(h_ls).astype(c64).reshape(-1, n_fft)
    w = weights(training).astype(np.float32)
    a = np.where(w == 0, 0, w * np.where(w == 0, 0, rows)).astype(c64)
    idx = window_index(n_fft)
    g = np.fft.ifft(a.astype(np.complex128), axis=-1).astype(c64)[:, idx]          # the device's inverse FFT carries the 1 / N
    m = (n_fft * rinv(training, n_fft)).astype(c64)                                  # ... so the table carries the N
    h = np.matmul(g, np.ascontiguousarray(m.T))
    assert h.dtype == c64
    full = np.zeros_like(rows)
    full[:, idx] = h
    return np.fft.fft(full.astype(np.complex128), axis=-1).astype(c64).reshape(np.shape(h_ls))
