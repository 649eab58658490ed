"""EXT-9, sc16 <-> fc32: the numpy restatement of the definition in include/ofdm_hip.h ("sc16 receive input").

sc16 is interleaved little-endian int16 I and Q: arrays of shape [..., 2] here.  Every function works component by component in f32;
numpy's f32 `*` is one IEEE multiplication rounded to nearest even, which is what the definition asks of the library.
"""
import numpy as np

DEFAULT_SCALE = np.float32(1.0 / 32768.0)


def widen_f32(i16, scale=DEFAULT_SCALE):
    """int16 [...] -> float32 [...]: x = (float)v * scale (the conversion is exact, the product rounded once)"""
    return np.asarray(i16, np.int16).astype(np.float32) * np.float32(scale)


def widen(i16, scale=DEFAULT_SCALE):
    """int16 [..., 2] -> complex64 [...]"""
    w = np.ascontiguousarray(widen_f32(i16, scale))
    assert w.shape[-1] == 2
    return w.view(np.complex64)[..., 0]


def narrow_f32(x, scale):
    """float32 [...] -> (int16 [...], clipped): y = x * scale (one rounded f32 product), q = rint(y) ties to even, clamped to
    [-32767, 32767], NaN -> 0; a component counts as clipped when y is not finite or rint(y) lies outside [-32767, 32767]"""
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.asarray(x, np.float32) * np.float32(scale)
        r = np.rint(y)                                   # float32, ties to even; inf and NaN stay
        clipped = ~(np.abs(r) <= np.float32(32767.0))    # True for NaN and +-inf
        q = np.where(np.isnan(r), np.float32(0.0), np.clip(r, np.float32(-32767.0), np.float32(32767.0)))
    return q.astype(np.int16), int(np.count_nonzero(clipped))


def narrow(z, scale):
    """complex64 [...] -> (int16 [..., 2], clipped components)"""
    z = np.ascontiguousarray(z, np.complex64)
    q, clipped = narrow_f32(z.view(np.float32).reshape(z.shape + (2,)), scale)
    return q, clipped


def quantise(z, peak_fraction=0.9):
    """complex [...] -> (int16 [..., 2], scale): the capture quantised so that its largest component sits at peak_fraction of full scale;
    widen(q, scale) is the capture as a receiver behind a 16-bit ADC sees it (scale = a power of two times nothing: any f32)"""
    z = np.asarray(z, np.complex64)
    peak = float(max(np.abs(z.real).max(), np.abs(z.imag).max()))
    gain = np.float32(peak_fraction * 32767.0 / peak)
    q, _ = narrow(z, gain)
    return q, np.float32(1.0) / gain
