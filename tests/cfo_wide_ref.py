"""EXT-8 wide CFO acquisition (include/ofdm_hip.h): the definition, in numpy f64.  The reference has no such stage
(its frequency_correction has the same 2 pi / S ambiguity as the Schmidl-Cox phase and drops the sign as well), so this file is what
k_cfo_wide, ofdm_cfo_wide_batch and the OFDM_CFO_WIDE receive mode are held to.

Per frame, o = offset[f], f0 = f_delta[f] (the Schmidl-Cox value, defined modulo 2 pi / S), S = N + cp, samples at or beyond frame_len
reading as zero, derotation as ofdm_estimate_channel_batch (sample id counted from o):

    tested       iff status == 0, o >= 0 and o + 10 S <= frame_len; otherwise m = 0, both metrics 0, f_delta untouched
    ybar[n]      sum_{b < 5} x[o + (5 + b) S + cp + n] e^{-i f0 ((5 + b) S + cp + n)}, n < N: the SUM of the five training blocks
    z_m[n]       ybar[n] e^{-2 pi i m (cp + n) / S}
    g_m          IFFT_N(conj(t) o FFT_N(z_m)), the inverse transform carrying the 1 / N (numpy's convention); t = the training table
    G_m          sum over the delays [-pre, L_h - pre) mod N of |g_m|^2, L_h = cp, pre = cp / 4 (chest_ref.window_index)
    decision     hypotheses in the order 0, -1, +1, -2, +2, ..., -span, +span; one is kept only if its G is strictly greater than the
                 best so far; m = the kept one, metric[0] = G_m, metric[1] = the largest G among the others
    result       f_delta = f0 + 2 pi m / S in f64 (m = 0: f0 itself, bit for bit)
A non-finite sample in a training block makes every G non-finite: nothing is ever strictly greater, m = 0, both metrics non-finite."""
import numpy as np

from chest_ref import window_index

MAX_SPAN = 32


def hypotheses(span):
    """0, -1, +1, ..., -span, +span: the visiting order"""
    out = [0]
    for k in range(1, span + 1):
        out += [-k, k]
    return out


def tested(offset, status, S, frame_len):
    return status == 0 and offset >= 0 and offset + 10 * S <= frame_len


def training_sum(x, o, f0, n_fft, dtype=np.complex128):
    """ybar of one frame; x: the capture's samples (all of them inside frame_len)"""
    cp = n_fft // 4
    S = n_fft + cp
    acc = np.zeros(n_fft, dtype)
    for b in range(5):
        j = (5 + b) * S + cp + np.arange(n_fft)
        acc = (acc + (x[o + j] * np.exp(-1j * ((f0 * j) % (2.0 * np.pi)))).astype(dtype)).astype(dtype)
    return acc


def metrics(ybar, training, n_fft, span, dtype=np.complex128):
    """G_m for every hypothesis in visiting order -> f64 array of 2 span + 1.  dtype = complex64: every stage's result rounded to
    complex64 (a restatement at the device's precision; its distance from the f64 values sets the kernel's tolerance)."""
    cp = n_fft // 4
    S = n_fft + cp
    idx = window_index(n_fft)
    ct = np.conj(np.asarray(training, np.complex128)).astype(dtype)
    j = cp + np.arange(n_fft)
    out = []
    with np.errstate(all="ignore"):
        for m in hypotheses(span):
            z = (ybar * np.exp(-2j * np.pi * ((m * j) % S) / S).astype(dtype)).astype(dtype)
            Z = np.fft.fft(z.astype(np.complex128)).astype(dtype)
            g = np.fft.ifft((ct * Z).astype(dtype).astype(np.complex128)).astype(dtype)[idx]
            real = np.float32 if dtype == np.complex64 else np.float64
            p = (g.real.astype(np.float64) ** 2 + g.imag.astype(np.float64) ** 2).astype(real)
            out.append(float(np.sum(p, dtype=real)))
    return np.array(out, np.float64)


def decide(G, span):
    """(m, G_m, largest G among the others) from the metrics in visiting order"""
    hyp = hypotheses(span)
    best = 0
    for i in range(1, len(hyp)):
        if G[i] > G[best]:
            best = i
    others = np.delete(G, best)
    with np.errstate(all="ignore"):
        return hyp[best], float(G[best]), float(np.max(others))


def cfo_wide(x, n_fft, training, offset, f_delta, span=8, status=None, frame_len=None, dtype=np.complex128):
    """x [frames, len] -> (m int32 [frames], f_delta f64 [frames], metric f64 [frames, 2])"""
    assert 1 <= span <= MAX_SPAN
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[None, :]
    frames = x.shape[0]
    frame_len = x.shape[1] if frame_len is None else frame_len
    S = n_fft + n_fft // 4
    offset = np.asarray(offset).reshape(frames)
    f0 = np.asarray(f_delta, np.float64).reshape(frames)
    status = np.zeros(frames, np.int32) if status is None else np.asarray(status).reshape(frames)
    m = np.zeros(frames, np.int32)
    fd = f0.copy()
    metric = np.zeros((frames, 2), np.float64)
    for f in range(frames):
        o = int(offset[f])
        if not tested(o, int(status[f]), S, frame_len):
            continue
        row = x[f, :frame_len].astype(dtype)
        with np.errstate(all="ignore"):
            ybar = training_sum(row, o, float(f0[f]), n_fft, dtype)
        G = metrics(ybar, training, n_fft, span, dtype)
        m[f], metric[f, 0], metric[f, 1] = decide(G, span)
        if m[f] != 0:
            fd[f] = f0[f] + 2.0 * np.pi * int(m[f]) / S
    return m, fd, metric
