"""Pilot tables other than the library's default, and captures made with them.  The preamble and the training table are INPUTS of a
context (ofdm_create; include/ofdm_hip.h), so every kernel and host routine that reads one is held to its definition under tables it
was not written around -- tests/test_pilots_cpu.py certifies the families below on the CPU, tests/test_gpu_pilots.py runs them.

    stdrng     the reference's own tables: rand 0.8 StdRng, seeds 100 / 50 (orc.stdrng_preamble / orc.stdrng_training)
    unit_loud  training exp(2 pi i u_k), |t_k| = 1; preamble 0.9 (U(-1, 1) + i U(-1, 1)) with one sample set to -0.99 + 0.2i and another
               to 0.1 + 0.95i: the header's signed maximum over re and im (normalize, src/transmitter.rs:183-194) is 0.95, in the
               IMAGINARY part of a PREAMBLE sample, while its largest magnitude, 0.99, is negative -- abs would be wrong, and the
               locking signal (just under 0.5) is not the peak
    holes      training a_k exp(2 pi i u_k), a_k in U(0.5, 1), with max(3, N / 32) bins exactly 0, drawn without replacement from the
               bins that are not pilot-class (data and null bins; a dead pilot bin would turn whole symbols into NaN on both sides and
               show nothing); the default preamble
    default    the library's SplitMix64 stand-ins, for comparison

Every draw is seeded by [n_fft, family, SEED]; the order of the draws is part of the definition."""
import functools

import numpy as np

from util import through_channel

FAMILIES = ("stdrng", "unit_loud", "holes")
SEED = 0                                  # (test_pilots_cpu.py holds cond(R) of `holes` under 10 at every N: another seed if it does not)
SIZES = (64, 128, 256, 1024, 4096)
LOUD_NEG, LOUD_POS = -0.99 + 0.2j, 0.1 + 0.95j


def _orc():
    from oracle import oracle as orc

    orc.lib()
    return orc


def _family_id(name):
    return FAMILIES.index(name) if name in FAMILIES else len(FAMILIES)       # ("default" seeds its captures with 3)


def _rng(n_fft, name):
    return np.random.default_rng([n_fft, _family_id(name), SEED])


@functools.lru_cache(maxsize=None)
def _tables(name, n_fft):
    orc = _orc()
    S = n_fft + n_fft // 4
    if name == "default":
        return orc.default_preamble(S), orc.default_training(n_fft)
    if name == "stdrng":
        return orc.stdrng_preamble(S), orc.stdrng_training(n_fft)
    rng = _rng(n_fft, name)
    if name == "unit_loud":
        pre = 0.9 * (rng.uniform(-1, 1, S) + 1j * rng.uniform(-1, 1, S))
        neg, pos = rng.choice(S, 2, replace=False)
        pre[neg], pre[pos] = LOUD_NEG, LOUD_POS
        return pre, np.exp(2j * np.pi * rng.random(n_fft))
    if name == "holes":
        trn = rng.uniform(0.5, 1.0, n_fft) * np.exp(2j * np.pi * rng.random(n_fft))
        free = np.array([k for k in range(n_fft) if orc.carrier_class(k, n_fft, True) != 2])
        trn[rng.choice(free, max(3, n_fft // 32), replace=False)] = 0.0
        return orc.default_preamble(S), trn
    raise KeyError(name)


def tables(name, n_fft):
    """(preamble[S], training[N]) complex128 of a family (or "default"); fresh copies"""
    pre, trn = _tables(name, n_fft)
    return pre.copy(), trn.copy()


def loud_positions(n_fft):
    """(sample of -0.99 + 0.2i, sample of 0.1 + 0.95i) inside unit_loud's preamble"""
    pre = _tables("unit_loud", n_fft)[0]
    return int(np.nonzero(pre == LOUD_NEG)[0][0]), int(np.nonzero(pre == LOUD_POS)[0][0])


def dead_bins(training):
    return np.nonzero(np.asarray(training) == 0)[0]


def band_nulled(n_fft):
    """the 802.11-style training table: holes' live values, zero on every null-class bin of carrier_class(guard = True).  A table that
    is zero on a whole band makes the WLS matrix R singular to rounding: outside the stage's domain (include/ofdm_hip.h)"""
    orc = _orc()
    rng = np.random.default_rng([n_fft, 9, SEED])
    trn = rng.uniform(0.5, 1.0, n_fft) * np.exp(2j * np.pi * rng.random(n_fft))
    trn[[k for k in range(n_fft) if orc.carrier_class(k, n_fft, True) == 1]] = 0.0
    return trn


def signed_peak(x):
    """(value, sample, "re" / "im") of normalize's maximum: signed, over the real and imaginary parts"""
    x = np.asarray(x)
    r, i = int(np.argmax(x.real)), int(np.argmax(x.imag))
    return (float(x.real[r]), r, "re") if x.real[r] >= x.imag[i] else (float(x.imag[i]), i, "im")


def captures(name, n_fft, mod, guard, payloads, snr_db=30.0, seed=0):
    """One capture per payload: orc.encode under the family's tables through util.through_channel (FIR channel, noise at snr_db against
    the data symbols) with a delay below S and a CFO inside +-0.9 pi / S; the capture is S + 160 samples longer than the frame.
    -> dict(rx complex64 [F, span], tx [list of complex128], delay, f_delta, pre, trn)"""
    orc = _orc()
    S = n_fft + n_fft // 4
    pre, trn = tables(name, n_fft)
    rng = np.random.default_rng([n_fft, mod, int(guard), _family_id(name), seed])
    tx = [orc.encode(bytes(p), guard, mod, n_fft, preamble=pre, training=trn) for p in payloads]
    span = max(t.size for t in tx) + S + 160
    span += span % 2
    F = len(tx)
    delay = rng.integers(1, S, F)
    fd = (rng.random(F) * 1.8 - 0.9) * np.pi / S
    rx = np.stack([through_channel(orc, rng, tx[f], span, int(delay[f]), float(fd[f]), snr_db, data_start=10 * S) for f in range(F)])
    return dict(rx=rx, tx=tx, delay=delay, f_delta=fd, pre=pre, trn=trn)


# ---------------------------------------------------------------------------------------------------------- cases (CPU only, computed once)
@functools.lru_cache(maxsize=None)
def rx_hard_case(name, n_fft, mod, guard, nbytes, frames=6, seed=0):
    """`frames` captures of one family at 30 dB and what orc.decode_sc(..., training=) makes of each (soft points included)
    -> dict(captures()' fields, pay [frames, nbytes] uint8, D, want [the oracle's dicts])"""
    orc = _orc()
    rng = np.random.default_rng([n_fft, mod, nbytes, seed])
    pay = rng.integers(0, 256, (frames, nbytes), dtype=np.uint8)
    k = captures(name, n_fft, mod, guard, [bytes(p) for p in pay], 30.0, seed)
    S = n_fft + n_fft // 4
    D = k["tx"][0].size // S - 10
    with np.errstate(all="ignore"):
        want = [orc.decode_sc(np.asarray(c).astype(np.complex128), guard, mod, n_fft, training=k["trn"], max_symbols=D, want_soft=True)
                for c in k["rx"]]
    k.update(pay=pay, D=D, want=want)
    return k


CHEST_ROWS = 67


@functools.lru_cache(maxsize=None)
def chest_stage_case(name, n_fft):
    """The rows of tests/test_gpu_chest.py's stage test under a family's tables: 33 oracle LS estimates of a frame through orc.channel at
    30 dB and 33 at 14 dB (NaN in the table's dead bins, as LS leaves them) and the bare H = 1 -> (rows complex64 [67, n_fft], the f64
    definition of the same rows, the complex64 restatement's error against it, the tolerance max(4 x that, 1e-5))"""
    import chest_ref as cr
    from util import rel_err, wide

    orc = _orc()
    S = n_fft + n_fft // 4
    pre, trn = tables(name, n_fft)
    tx = orc.encode(b"EXT-5", guard=True, modulation=6, n_fft=n_fft, preamble=pre, training=trn)
    off, rows = None, []
    with np.errstate(all="ignore"):
        for i in range(CHEST_ROWS - 1):
            rx, _ = orc.channel(tx, 30.0 if i % 2 == 0 else 14.0, False, 500 + i)
            if off is None:
                off = orc.decode_sc(rx, guard=True, modulation=6, n_fft=n_fft, training=trn)["offset"]
            rows.append(orc.estimate_channel(rx[off + 5 * S:off + 10 * S], trn, n_fft))
        rows.append(np.ones(n_fft, np.complex128))
        rows = np.asarray(rows).astype(np.complex64)
        want = cr.smooth(wide(rows), trn, n_fft)
        c64 = cr.smooth_c64(rows, trn, n_fft)
    measured = max(rel_err(c64[r], want[r]) for r in range(CHEST_ROWS))
    return rows, want, measured, max(4.0 * measured, 1e-5)


WIDE_M = (-8, -3, 0, 5, 8)
WIDE_SNR = {64: 30.0, 1024: 35.0}


@functools.lru_cache(maxsize=None)
def cfo_wide_case(name, n_fft, mod=6, guard=True, span=8):
    """Five short frames of a family turned by frac + 2 pi m / S, m = WIDE_M, through the FIR channel (N = 64 at 30 dB, N = 1024 at 35 dB;
    odd row stride), the trimmed start and the estimate of frac a search would hand over (tests/test_gpu_cfo_wide.py's construction),
    and the f64 definition under the family's training table -> dict(rx, m, off, f0, trn, ref = (m, f_delta, metric [5, 2]), tol, dist):
    dist = the complex64 restatement's relative distance from the f64 metrics, tol = max(4 dist, 1e-5)"""
    import cfo_wide_ref as cw
    from util import wide

    orc = _orc()
    S = n_fft + n_fft // 4
    pre, trn = tables(name, n_fft)
    F = len(WIDE_M)
    D = -(-8 * (16 + 8) // mod // orc.data_carriers(n_fft, guard))
    length = (10 + D) * S + n_fft // 4 + 61
    length += 1 - length % 2
    rng = np.random.default_rng([n_fft, _family_id(name), 8])
    m = np.array(WIDE_M, np.int32)
    frac = (rng.random(F) * 1.9 - 0.95) * np.pi / S
    delay = rng.integers(0, n_fft // 4, F)
    rx = np.zeros((F, length), np.complex64)
    for f in range(F):
        tx = orc.encode(bytes(rng.integers(0, 256, 8, dtype=np.uint8)), guard, mod, n_fft, preamble=pre, training=trn)
        rx[f] = through_channel(orc, rng, tx, length, int(delay[f]), float(frac[f] + 2.0 * np.pi * m[f] / S), WIDE_SNR[n_fft], data_start=10 * S)
    off = (delay + 5 + rng.integers(-2, 3, F)).astype(np.int32)
    f0 = frac + rng.standard_normal(F) * 1e-3 / S
    with np.errstate(all="ignore"):
        ref = cw.cfo_wide(wide(rx), n_fft, trn, off, f0, span)
        g32 = cw.cfo_wide(rx, n_fft, trn, off, f0, span, dtype=np.complex64)[2]
    dist = float(np.max(np.abs(g32 - ref[2]) / ref[2]))
    return dict(rx=rx, m=m, off=off, f0=f0, trn=trn, pre=pre, ref=ref, dist=dist, tol=max(4.0 * dist, 1e-5))
