"""Input gains for the receive side (tests/test_gain_cpu.py, tests/test_gpu_gain.py): the gains, the one exact way a capture is scaled,
the bit-for-bit comparisons, and the CPU captures the f64 definitions are shown homogeneous on.

Multiplying an fc32 capture by +-2^k is exact, and every f32 / f64 operation downstream is then the same operation on scaled
operands as long as nothing overflows or goes subnormal: a receiver whose constants are all relative to the energy it sees returns
THE SAME BITS at every gain.  Nothing here knows a tolerance."""
import functools

import numpy as np

# 2^15 is the raw-count sc16 scale (int16 * 1.0); 2^-10 is a signal of 30 LSB at the default sc16 scale; -1 turns every sample round
GAINS = (2.0 ** -20, 2.0 ** -10, 2.0 ** 10, 2.0 ** 15, 2.0 ** 20, -1.0)
F32_TINY = float(np.finfo(np.float32).tiny)


def bits(a):
    """the bit patterns of a numpy array or a torch tensor (moved to the host), complex ones as their (re, im) pairs"""
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    a = np.ascontiguousarray(a)
    size = a.dtype.itemsize // (2 if a.dtype.kind == "c" else 1)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[size])


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def scaled(x, g):
    """complex64 (numpy array or torch tensor, any shape) times the real gain g as ONE f32 multiplication per component -- after
    asserting that the product is exact (x g / g == x bit for bit) and that every scaled sample is normal or zero"""
    if hasattr(x, "detach"):
        import torch

        assert x.dtype == torch.complex64
        r = torch.view_as_real(x)
        y = r * float(np.float32(g))
        assert y.dtype == torch.float32 and torch.equal((y / float(np.float32(g))).view(torch.int32), r.contiguous().view(torch.int32)), g
        assert bool(((y.abs() >= F32_TINY) | (y == 0)).all()) and bool(torch.isfinite(y).all()), g
        return torch.view_as_complex(y.contiguous())
    x = np.ascontiguousarray(x, np.complex64)
    r = x.view(np.float32)
    y = r * np.float32(g)
    assert y.dtype == np.float32 and np.array_equal((y / np.float32(g)).view(np.uint32), r.view(np.uint32)), g
    assert np.all((np.abs(y) >= F32_TINY) | (y == 0)) and np.all(np.isfinite(y)), g
    return y.view(np.complex64)


def times(a, factor):
    """a (real or complex floating point, numpy or torch) times a power of two in a's own precision: what an output that scales with
    the input must equal bit for bit"""
    a = np.atleast_1d(a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a))
    real = a.view(a.real.dtype) if a.dtype.kind == "c" else a
    with np.errstate(over="raise", under="raise"):
        out = real * real.dtype.type(factor)
    return out.view(a.dtype)


# ---------------------------------------------------------------------------------------------------------------- CPU captures
CPU_SHAPES = ((64, 6, 100), (256, 4, 300), (1024, 2, 300))      # (n_fft, bits per point, payload bytes), guard bands on
CPU_SNR_DB = 40.0     # uncoded 64-QAM through the FIR channel's fades needs it for "the payload back", which the baseline must give


@functools.lru_cache(maxsize=None)
def cpu_case(n, mod, nbytes):
    """One frame through the FIR channel at CPU_SNR_DB with a delay and a CFO, as complex64, with what the f64 oracle makes of it:
    dict(rx, pay, delay, sync = orc.sc_sync, dec = orc.decode_sc, S, D, trn, hk = the oracle's channel estimate at its own offset of the
    capture derotated by its own CFO)"""
    from oracle import oracle as orc
    from util import through_channel, wide

    orc.lib()
    rng = np.random.default_rng([n, mod, nbytes, 7])
    S = n + n // 4
    pay = bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))
    tx = orc.encode(pay, True, mod, n)
    delay = int(rng.integers(1, 33))
    fd = float((rng.random() * 1.8 - 0.9) * np.pi / S)
    rx = through_channel(orc, rng, tx, tx.size + 160 + 1, delay, fd, CPU_SNR_DB, data_start=10 * S)     # (an odd length)
    sync = orc.sc_sync(wide(rx), S, 3, 0, 0.5)
    dec = orc.decode_sc(wide(rx), True, mod, n)
    trn = orc.default_training(n)
    return dict(rx=rx, pay=pay, delay=delay, f_delta=fd, sync=sync, dec=dec, S=S, D=tx.size // S - 10, trn=trn,
                hk=channel_estimate(orc, wide(rx), dec["offset"], dec["f_delta"], trn, n))


def channel_estimate(orc, x, offset, f_delta, trn, n):
    """the oracle's estimate_channel on training blocks 5 .. 9 of the frame at `offset`, derotated from the frame's first sample"""
    S = n + n // 4
    y = orc.cfo_rotate(x[offset:offset + 10 * S], f_delta, 0)
    return orc.estimate_channel(y[5 * S:10 * S], trn, n)
