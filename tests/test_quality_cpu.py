"""EXT-6 link quality, the definition on its own (tests/quality_ref.py; no GPU): what it estimates, checked against frames whose
noise variance and channel are known.  Frames come from the oracle's encode over a flat channel (offset 0, no CFO); complex white
noise of per-sample variance s2 is added, so a received bin carries noise of variance N s2; 256 frames are drawn per case and every
mean is held to 5 standard errors taken from the sample."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as qr  # noqa: E402
from util import awgn  # noqa: E402

FRAMES = 256
PAYLOAD = 40


def _mean_se(v):
    v = np.asarray(v, np.float64)
    return float(v.mean()), float(v.std(ddof=1) / np.sqrt(v.size))


@functools.lru_cache(maxsize=None)
def _case(n_fft, mod, snr_db, seed=0):
    """One noiseless frame, its row and H, and FRAMES noisy copies at a per-bin training SNR of snr_db.  Computed once."""
    from oracle import oracle as orc

    orc.lib()
    rng = np.random.default_rng([n_fft, mod, seed])
    trn = orc.default_training(n_fft)
    tx = orc.encode(bytes(rng.integers(0, 256, PAYLOAD, dtype=np.uint8)), True, mod, n_fft)
    nd = orc.data_carriers(n_fft, True)
    n_points = -(-8 * (16 + PAYLOAD) // mod)
    syms = -(-n_points // nd)
    data, _ = qr.carrier_masks(n_fft, True)
    S = n_fft + n_fft // 4
    hk = np.fft.fft(tx[5 * S + n_fft // 4:6 * S]) / trn             # the noiseless frame's H (flat: the frame's scale in every bin)
    clean, extra0 = qr.quality(tx[None, :], n_fft, True, mod, trn, syms, 10, n_points, hk=hk, detail=True)
    gain0 = float(clean[0, qr.Q_GAIN])
    t2_mean = float(np.mean(np.abs(trn[data]) ** 2))
    s2 = gain0 * t2_mean / 10 ** (snr_db / 10) / n_fft              # N s2 = gain mean|t|^2 / snr
    rx = tx[None, :] + awgn(rng, (FRAMES, tx.size), np.sqrt(s2 / 2))
    rows, extra = qr.quality(rx, n_fft, True, mod, trn, syms, 10, n_points, hk=hk, detail=True)
    return dict(tx=tx, trn=trn, rx=rx, rows=rows, extra=extra, clean=clean, soft0=extra0["soft"][0], hk=hk, s2=s2, gain0=gain0, nd=nd,
                n_points=n_points, syms=syms, data=data, S=S)


@pytest.mark.parametrize("n_fft", [64, 256])
def test_parseval_the_two_forms_of_noise_var_agree(n_fft):
    c = _case(n_fft, 4, 10.0)
    t, b = c["rows"][:, qr.Q_NOISE_VAR], c["extra"]["noise_var_bins"]
    assert np.all(c["rows"][:, qr.Q_VALID] == 1) and np.all(t > 0)
    assert np.max(np.abs(t - b) / t) <= 1e-12


@pytest.mark.parametrize("n_fft,snr_db", [(64, 0.0), (64, 20.0), (256, 10.0)])
def test_noise_var_is_unbiased(n_fft, snr_db):
    c = _case(n_fft, 4, snr_db)
    mean, se = _mean_se(c["rows"][:, qr.Q_NOISE_VAR])
    want = n_fft * c["s2"]
    print(f"N {n_fft}: noise_var mean {mean:.6g} want {want:.6g}, relative standard error {se / want:.4%} (expected {1 / np.sqrt(4 * n_fft * FRAMES):.4%})")
    assert abs(mean - want) <= 5 * se
    assert 0.7 / np.sqrt(4 * n_fft * FRAMES) < se / want < 1.4 / np.sqrt(4 * n_fft * FRAMES)     # chi-square with 8 N degrees of freedom


def test_gain_is_unbiased_and_the_bias_term_is_what_makes_it_so():
    """At 0 dB the uncorrected sum |Ybar|^2 / sum |t|^2 overshoots by noise_var / (5 mean_D |t|^2), 20 % of the gain: far outside five
    standard errors, so the test pins the - noise_var / 5 term."""
    c = _case(64, 4, 0.0)
    rows, nd = c["rows"], c["nd"]
    t2 = float(np.sum(np.abs(c["trn"][c["data"]]) ** 2))
    mean, se = _mean_se(rows[:, qr.Q_GAIN])
    unc_mean, unc_se = _mean_se(rows[:, qr.Q_GAIN] + nd * rows[:, qr.Q_NOISE_VAR] / 5.0 / t2)
    print(f"gain {c['gain0']:.6g}: corrected mean {mean:.6g} +- {se:.2g}, uncorrected {unc_mean:.6g} +- {unc_se:.2g}")
    assert abs(unc_mean - c["gain0"]) > 5 * max(se, unc_se)          # the chosen point separates the two estimates
    assert abs(mean - c["gain0"]) <= 5 * se


def test_evm_is_the_inverse_snr_when_no_decision_fails():
    c = _case(64, 4, 26.0)
    rows = c["rows"]
    want = qr.slice_points(c["soft0"], 4)
    for f in range(FRAMES):                                           # no decision error anywhere in the case
        assert np.array_equal(qr.slice_points(c["extra"]["soft"][f], 4), want), f
    assert np.all(rows[:, qr.Q_POINTS] == c["n_points"]) and c["n_points"] % c["nd"] != 0
    mean, se = _mean_se(rows[:, qr.Q_EVM2] * rows[:, qr.Q_SNR])
    print(f"evm2 * snr: mean {mean:.5f} +- {se:.5f}; snr {10 * np.log10(rows[:, qr.Q_SNR].mean()):.2f} dB")
    assert abs(mean - 1.0) <= 5 * se


@pytest.mark.parametrize("mod", [2, 4, 6])
def test_llr_unit_is_the_headers_formula(mod):
    """llr_unit = 4 mean|H|^2 / ((M - 1)^2 sigma^2) with sigma^2 = N s2.  The estimate is proportional to 1 / noise_var, whose mean is
    not 1 / mean: the comparison is made on 1 / llr_unit, which is unbiased."""
    c = _case(64, mod, 15.0)
    M = qr.levels(mod)
    want = 4.0 * np.mean(np.abs(c["hk"][c["data"]]) ** 2) / ((M - 1) ** 2 * 64 * c["s2"])
    mean, se = _mean_se(1.0 / c["rows"][:, qr.Q_LLR_UNIT])
    assert abs(mean - 1.0 / want) <= 5 * se
    assert abs(c["rows"][:, qr.Q_LLR_UNIT].mean() / want - 1.0) < 0.03


def test_edge_rows():
    c = _case(64, 4, 26.0)
    rx, trn, S, nd, npts, syms = c["rx"][:4], c["trn"], c["S"], c["nd"], c["n_points"], c["syms"]
    full = c["rows"][:4]
    q = lambda **kw: qr.quality(rx, 64, True, 4, trn, kw.pop("syms", syms), 10, kw.pop("n_points", npts), hk=c["hk"], **kw)
    # cut inside the training blocks: nothing is counted, the row is zero
    assert np.all(q(frame_len=10 * S - 1) == 0)
    assert np.all(q(offset=np.full(4, rx.shape[1] - 10 * S + 1)) == 0)
    assert np.all(q(offset=np.full(4, -1)) == 0)
    # cut inside the second data symbol: the training fields stand, one whole symbol is counted
    cut = q(frame_len=11 * S + S // 2)
    assert np.array_equal(cut[:, :qr.Q_EVM2], full[:, :qr.Q_EVM2]) and np.all(cut[:, qr.Q_POINTS] == nd)
    assert np.all(cut[:, qr.Q_EVM2] > 0) and not np.array_equal(cut[:, qr.Q_EVM2], full[:, qr.Q_EVM2])
    assert np.array_equal(q(frame_len=12 * S - 1), q(frame_len=11 * S))
    # the caller's count decides: not a multiple of nd, more than the symbols hold, none
    assert npts % nd and np.all(full[:, qr.Q_POINTS] == npts)
    assert np.all(q(n_points=nd + 5)[:, qr.Q_POINTS] == nd + 5)
    assert np.all(q(n_points=10 ** 6)[:, qr.Q_POINTS] == syms * nd)
    assert np.all(q(n_points=npts, syms=1)[:, qr.Q_POINTS] == nd)
    none = q(n_points=0)
    assert np.array_equal(none[:, :qr.Q_EVM2], full[:, :qr.Q_EVM2]) and np.all(none[:, qr.Q_EVM2:] == 0)
    per_frame = q(n_points=np.array([0, 7, nd, npts]))
    assert list(per_frame[:, qr.Q_POINTS]) == [0, 7, nd, npts] and np.array_equal(per_frame[3], full[3])
    # padding points (zeros behind the last data point) are what the count keeps out: counting them moves evm2
    assert np.all(q(n_points=syms * nd)[:, qr.Q_EVM2] > 1.5 * full[:, qr.Q_EVM2])
    # a frame whose status is not 0 is not measured
    st = q(status=np.array([0, -2, 0, -4]))
    assert np.array_equal(st[[0, 2]], full[[0, 2]]) and np.all(st[[1, 3]] == 0)
    assert np.all(full[:, 7] == 0)


def test_non_finite_samples_reach_only_their_fields():
    c = _case(64, 4, 26.0)
    S = c["S"]
    rx = c["rx"][:3].copy()
    rx[1, 7 * S + 30] = np.nan                  # a training block of frame 1
    rx[2, 11 * S + 40] = np.nan                 # the second data symbol of frame 2
    rows = qr.quality(rx, 64, True, 4, c["trn"], c["syms"], 10, c["n_points"], hk=c["hk"])
    assert np.array_equal(rows[0], c["rows"][0])
    t = [qr.Q_NOISE_VAR, qr.Q_GAIN, qr.Q_SNR, qr.Q_LLR_UNIT]
    assert np.all(np.isnan(rows[1, t])) and rows[1, qr.Q_VALID] == 1 and np.isfinite(rows[1, qr.Q_EVM2]) and rows[1, qr.Q_POINTS] == c["n_points"]
    assert np.array_equal(rows[2, :qr.Q_EVM2], c["rows"][2, :qr.Q_EVM2]) and np.isnan(rows[2, qr.Q_EVM2]) and rows[2, qr.Q_POINTS] == c["n_points"]


@pytest.mark.parametrize("n_fft,mod", [(64, 4), (128, 1), (1024, 6)])
def test_device_precision_restatement_stays_close(n_fft, mod):
    """the complex64 restatement (the device's order of operations) against the definition, with CFO and an offset: what sets the
    tolerance of tests/test_gpu_quality.py must itself be a faithful restatement"""
    c = _case(n_fft, mod, 18.0)
    rng = np.random.default_rng(n_fft)
    rx = np.zeros((5, c["tx"].size + 40), np.complex64)
    off = rng.integers(0, 30, 5)
    fd = (rng.random(5) - 0.5) * 2.0 / c["S"]
    for f in range(5):
        rx[f, off[f]:off[f] + c["tx"].size] = c["rx"][f] * np.exp(1j * fd[f] * np.arange(c["tx"].size))
    kw = dict(offset=off, f_delta=fd, hk=c["hk"].astype(np.complex64))
    want = qr.quality(rx, n_fft, True, mod, c["trn"], c["syms"], 10, c["n_points"], **kw)
    got = qr.quality(rx, n_fft, True, mod, c["trn"], c["syms"], 10, c["n_points"], f32=True, **kw)
    assert np.all(want[:, qr.Q_VALID] == 1) and np.array_equal(got[:, qr.Q_POINTS], want[:, qr.Q_POINTS])
    assert np.max(np.abs(want[:, qr.Q_NOISE_VAR] / (n_fft * c["s2"]) - 1)) < 0.5        # (the derotation undid the CFO)
    rel = np.abs(got - want)[:, 1:6] / np.abs(want[:, 1:6])
    print("restatement, largest relative distance per field:", dict(zip(qr.NAMES[1:6], rel.max(axis=0))))
    assert rel.max() < 1e-4
