"""EXT-11 noise-aware LLR weights (include/ofdm_hip.h): the definition, in numpy f64.  The reference has nothing of
the kind, so this file is what ofdm_rx_noise_bins_batch (k_noise_bins), ofdm_rx_llr_weighted_batch (k_sym<llrw>) and the decode chains
under OFDM_LLRW_NOISE are held to.

Per frame f, with o = offset[f], fd = f_delta[f], S = N + cp, samples at or beyond frame_len reading as zero, and the derotation of
estimate_channel / quality_ref (sample id n counted from o: y[n] = x[o + n] exp(-j fd n)):

  tested   iff status[f] == 0 (or no status), o >= 0 and o + 10 S <= frame_len; a frame that is not tested gets s_k = 0, q_k = 1
  y_b[n]   derotated sample (5 + b) S + cp + n, b < 5, n < N, exactly quality_ref's;  ybar = mean_b y_b;  d_b = y_b - ybar (time domain),
           evaluated as (1/5) sum_c (y_b - y_c), so that five identical blocks give exactly 0
  s_k      (1/4) sum_b |FFT_N(d_b)[k]|^2, unnormalised FFT: the unbiased noise variance of received bin k; mean_k s_k over all N bins
           is quality_ref's noise_var (Parseval)
  sbar     mean_k s_k over all N bins
  q_k      sbar / s_k if s_k > sbar else 1 (the comparison is false for NaN); in [0, 1]; all ones for a noiseless frame
  LLR      L = clamp(rint(scale w_k q_k Lambda), +-127), w_k soft_ref.channel_weights; 0 when the product is not finite

q is homogeneous of degree 0 in the capture and s of degree 2.  What the scatter cannot see: a tone whose phase advances a whole
number of turns per symbol (bin x with x S / N an integer) is the same in all five blocks and counts as signal."""
import numpy as np


def noise_bins(rx, n_fft, offset=None, f_delta=None, status=None, frame_len=None):
    """(s, q), float64 [n_frames, n_fft] each.  rx: [n_frames, stride] complex."""
    rx = np.asarray(rx)
    F, stride = rx.shape
    N, cp = n_fft, n_fft // 4
    S = N + cp
    frame_len = stride if frame_len is None else frame_len
    off = np.zeros(F, np.int64) if offset is None else np.asarray(offset, np.int64)
    fd = None if f_delta is None else np.asarray(f_delta, np.float64)
    alive = np.ones(F, bool) if status is None else (np.asarray(status) == 0)
    tested = alive & (off >= 0) & (off + 10 * S <= frame_len)
    s = np.zeros((F, N))
    q = np.ones((F, N))
    with np.errstate(all="ignore"):
        for f in np.flatnonzero(tested):
            Y = np.empty((5, N), np.complex128)
            for b in range(5):
                n0 = (5 + b) * S + cp
                y = rx[f, off[f] + n0:off[f] + n0 + N].astype(np.complex128)
                if fd is not None:
                    ph = fd[f] * 0.15915494309189533577 * (n0 + np.arange(N))  # in turns, reduced before the exponential
                    y = y * np.exp(-2j * np.pi * (ph - np.rint(ph)))
                Y[b] = y
            dev = (Y[:, None, :] - Y[None, :, :]).sum(axis=1) / 5.0   # y_b - ybar as the mean of y_b - y_c: identical blocks give exactly 0
            D = np.fft.fft(dev, axis=-1)
            s[f] = np.sum(D.real ** 2 + D.imag ** 2, axis=0) / 4.0
            q[f] = weights_of(s[f])
    return s, q


def tone_capture(orc, stream, snr_db, seed, isr_db=None, tone_bin=11.3, n=64, mod=6):
    """The link of the experiments (tests/test_noise_weight_cpu.py, tests/test_gpu_noise_weight.py): one frame of the f64 oracle
    carrying the coded bytes `stream`, guard bands on, through the oracle's channel at snr_db, 37 samples into its slot, with a complex
    tone at the fractional bin `tone_bin` of power isr_db relative to the frame's mean power on top (None: no tone) -> the capture"""
    tx = orc.encode(bytes(stream), True, mod, n)
    y, _ = orc.channel(tx, snr_db=snr_db, timing_error=False, seed=seed)
    rx = np.concatenate([np.zeros(37), y, np.zeros(160)])
    if isr_db is not None:
        amp = np.sqrt(np.mean(np.abs(y) ** 2) * 10.0 ** (isr_db / 10.0))
        rx = rx + amp * np.exp(2j * np.pi * tone_bin * np.arange(rx.size) / n)
    return rx


def weights_of(s):
    """q of one row s_k (all n_fft bins)"""
    s = np.asarray(s, np.float64)
    with np.errstate(all="ignore"):
        sbar = np.mean(s)
        big = s > sbar                                             # false for NaN
        return np.where(big, sbar / np.where(big, s, 1.0), 1.0)
