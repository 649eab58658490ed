"""GPU checks of EXT-6, link quality (include/ofdm_hip.h; definition: tests/quality_ref.py): ofdm_rx_quality_batch (k_linkq) against the
f64 definition on THE SAME fc32 samples, offsets, CFOs and hk, so that the comparison isolates the kernel, and Context.link_quality on
the seeded link of tools/link.py.

Tolerance (the precedent is tests/test_gpu_chest.py): quality_ref restates the computation in complex64 with the device's order of
operations; its distance from the f64 definition is measured on the case's own rows, per field, and the kernel is allowed 4x that or
1e-5 relative, whichever is larger.  valid and points must be equal.

Decision boundaries: a point within 1e-5 (util.decision_margin, the scale of util.assert_bytes_match) of a decision boundary of the f64
reference may slice the other way on the device.  |x - xh|^2 itself is continuous there (the boundary is equidistant: within 1e-5 of
it the two values differ by at most 2 d 1e-5, d = the level spacing), but the re-sliced xh moves sum |xh|^2 by up to d (2 - d) (two
neighbouring levels of one axis; 0 for BPSK / QPSK), so a frame holding c such points is compared with its bound widened by
c (2 d 1e-5 + evm2 d (2 - d)) / sum |xh|^2: the largest change of the frame's evm2 when c points slice the other way.  At most 2 % of a
case's frames may be excused this way; the cases' seeds and SNRs are such that the reference alone stays within that (a seed is
skipped on the CPU if it does not), and the largest share seen is printed."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as qr  # noqa: E402
from chain_checks import ofdm_api as _api  # noqa: E402
from tools.link import link  # noqa: E402
from util import decision_margin, through_channel, wide  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-5
FIELDS = (qr.Q_NOISE_VAR, qr.Q_GAIN, qr.Q_SNR, qr.Q_LLR_UNIT, qr.Q_EVM2)
# the SNR a modulation's cases are drawn at: high enough that a decision boundary is several sigma from the points, so that next to
# no point of the reference lies within 1e-5 of one
SNR = {1: 8.0, 2: 11.0, 4: 22.0, 6: 30.0, 8: 37.0}


def _widening(mod, evm2, sum_ref, count):
    d = 2.0 if mod <= 2 else 2.0 / (qr.levels(mod) - 1)
    jump_r = 0.0 if mod <= 2 else d * (2.0 - d)
    return np.where(count > 0, count * (2.0 * d * TOL + evm2 * jump_r) / np.maximum(sum_ref, 1e-300), 0.0)


def _reference(rx, n, guard, mod, trn, syms, n_points, **kw):
    """(want rows, per-field tolerance, per-frame count of points at a decision boundary, evm2 widening per frame, restatement distance)"""
    want, extra = qr.quality(wide(rx), n, guard, mod, trn, syms, 10, n_points, detail=True, **{k: (wide(v) if k == "hk" and v is not None else v) for k, v in kw.items()})
    r32 = qr.quality(rx, n, guard, mod, trn, syms, 10, n_points, f32=True, **kw)
    near = np.array([int((decision_margin(s, mod) < TOL).sum()) if s.size else 0 for s in extra["soft"]])
    ok = want[:, qr.Q_VALID] == 1
    dist = {}
    for fld in FIELDS:
        use = ok & (want[:, fld] != 0) & np.isfinite(want[:, fld])
        if fld == qr.Q_EVM2:
            use &= near == 0
        dist[fld] = float(np.max(np.abs(r32[use, fld] - want[use, fld]) / np.abs(want[use, fld]))) if use.any() else 0.0
    tol = {fld: max(4.0 * dist[fld], TOL) for fld in FIELDS}
    return want, tol, near, _widening(mod, want[:, qr.Q_EVM2], extra["sum_ref"], near), dist


def _assert_rows(got, want, tol, near, widen, what):
    assert np.array_equal(got[:, qr.Q_VALID], want[:, qr.Q_VALID]) and np.array_equal(got[:, qr.Q_POINTS], want[:, qr.Q_POINTS]), what
    assert np.all(got[:, 7] == 0), what
    worst = {}
    for fld in FIELDS:
        err = np.abs(got[:, fld].astype(np.float64) - want[:, fld])
        bound = tol[fld] * np.abs(want[:, fld]) + (widen if fld == qr.Q_EVM2 else 0.0)
        scale = np.where(want[:, fld] != 0, np.abs(want[:, fld]), 1.0)
        worst[qr.NAMES[fld]] = float(np.max(err / scale))
        assert np.all(err <= bound), (what, qr.NAMES[fld], int(np.argmax(err - bound)), float(np.max(err / scale)), tol[fld])
    return worst


# ---------------------------------------------------------------------------------------------------------- 1. the kernel
CASES = [  # n_fft, modulation, guard bands, frames, data symbols, hk ("frame" / "shared" / None)
    (64, 1, True, 3, 4, "frame"),
    (64, 6, False, 70, 6, "shared"),
    (64, 8, True, 70, 4, None),
    (128, 2, True, 70, 5, "frame"),
    (128, 6, False, 3, 3, None),
    (1024, 6, True, 70, 3, "frame"),
    (1024, 2, False, 3, 4, "shared"),
    (4096, 8, True, 3, 3, "frame"),
    (4096, 1, False, 70, 3, "shared"),
]


@functools.lru_cache(maxsize=None)
def _kernel_case(n, mod, guard, frames, D, hk_mode):
    """Captures of `frames` frames of D data symbols through the FIR channel with a delay and a CFO each (odd row stride), the offsets,
    CFOs and hk the call is given, and the reference rows.  Computed once; the first seed whose reference excuses at most 2 % of the
    frames is the case's."""
    from oracle import oracle as orc

    orc.lib()
    S = n + n // 4
    nd = orc.data_carriers(n, guard)
    trn = orc.default_training(n)
    payload = D * nd * mod // 8 - 16 - 3                         # D data symbols, the last one not full
    n_points = -(-8 * (16 + payload) // mod)
    assert -(-n_points // nd) == D and n_points % nd
    span = (10 + D) * S + 2 * n // 4 + 61
    span += 1 - span % 2                                          # an odd row stride
    for seed in range(8):
        rng = np.random.default_rng([n, mod, int(guard), frames, seed])
        rx = np.zeros((frames, span), np.complex64)
        off = rng.integers(0, n // 4, frames).astype(np.int32)
        fd = (rng.random(frames) - 0.5) * 2.0 / S
        for f in range(frames):
            tx = orc.encode(bytes(rng.integers(0, 256, payload, dtype=np.uint8)), guard, mod, n)
            if hk_mode is None:                                   # no estimate is passed: the frame arrives with H = 1 (encode's scale undone)
                tx = tx / np.mean(np.fft.fft(tx[5 * S + n // 4:6 * S]) / trn)
            rx[f] = through_channel(orc, rng, tx, span, int(off[f]), float(fd[f]), SNR[mod], taps=hk_mode is not None, data_start=10 * S)
        fd = fd + rng.standard_normal(frames) * 1e-3 / S          # what a search would hand over: not the channel's exact value
        hk = None
        if hk_mode is not None:
            rows = []
            for f in range(frames if hk_mode == "frame" else 1):
                x = orc.cfo_rotate(wide(rx[f, off[f]:off[f] + 10 * S]), float(fd[f]), 0)
                rows.append(orc.estimate_channel(x[5 * S:], trn, n))
            hk = np.asarray(rows if hk_mode == "frame" else rows[0]).astype(np.complex64)
        ref = _reference(rx, n, guard, mod, trn, D, n_points, offset=off, f_delta=fd, hk=hk)
        share = float(np.mean(ref[2] > 0))
        if share <= 0.02:
            break
    assert share <= 0.02, share
    return dict(rx=rx, off=off, fd=fd, hk=hk, n_points=n_points, ref=ref, share=share, seed=seed, trn=trn, nd=nd, S=S)


def _dev(c, a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=c.device, dtype=dtype)


@pytest.mark.parametrize("n,mod,guard,frames,D,hk_mode", CASES)
def test_kernel_matches_the_definition(n, mod, guard, frames, D, hk_mode):
    api = _api()
    k = _kernel_case(n, mod, guard, frames, D, hk_mode)
    want, tol, near, widen, dist = k["ref"]
    assert np.all(want[:, qr.Q_VALID] == 1) and np.all(want[:, qr.Q_POINTS] == k["n_points"])
    c = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    rx = c.to_device(k["rx"])
    assert rx.shape[1] % 2 == 1
    args = dict(n_points=k["n_points"], offset=_dev(c, k["off"], torch.int32), f_delta=_dev(c, k["fd"], torch.float64),
                hk=None if k["hk"] is None else c.to_device(k["hk"]))
    got = c.rx_quality(rx, D, **args)
    c.synchronize()
    assert c.last_dispatch() == "k_linkq"
    worst = _assert_rows(got.cpu().numpy(), want, tol, near, widen, (n, mod))
    print(f"N {n} mod {mod}: restatement {({qr.NAMES[f]: f'{v:.1e}' for f, v in dist.items()})}, kernel {({a: f'{v:.1e}' for a, v in worst.items()})}, "
          f"frames with a point at a boundary {k['share']:.1%} (seed {k['seed']})")
    for cap in (1, 3):                                            # many frames per slot: the same bits
        c.set_tuning("grid_cap", cap)
        assert torch.equal(c.rx_quality(rx, D, **args), got), cap
    c.set_tuning("grid_cap", 0)
    out = torch.full_like(got, 7.0)
    assert c.rx_quality(rx, D, out=out, **args) is out and torch.equal(out, got)
    # more symbols offered than the points fill: the count decides
    assert torch.equal(c.rx_quality(rx, D + 2, **args), got)


# ---------------------------------------------------------------------------------------------------------- 2. ragged batches
@pytest.mark.parametrize("n,mod", [(64, 6), (128, 4), (1024, 2)])
def test_ragged_batch_rows_are_the_rows_of_the_frames_alone(n, mod):
    """Frames of different n_points side by side in one wavefront (N = 1024: one workgroup), a dead frame first (status != 0, then one
    with n_points = 0), frames cut inside the training blocks and inside the third data symbol: every row equals the reference's and,
    bit for bit, the row of the frame run alone."""
    api = _api()
    from oracle import oracle as orc

    orc.lib()
    S, D, frames = n + n // 4, 4, 12
    nd = orc.data_carriers(n, True)
    trn = orc.default_training(n)
    payload = D * nd * mod // 8 - 16 - 3
    full = -(-8 * (16 + payload) // mod)
    rng = np.random.default_rng([n, mod, 5])
    span = (10 + D) * S + 41
    #         dead  none  live  7     cut in training        live   cut in 3rd symbol      nd    nd + 1      live  2 nd  live
    delay = [3, 0, 5, 1, span - 10 * S + 1, 2, span - 13 * S + S // 3, 7, 0, span - (10 + D) * S, 4, 6]
    n_points = np.array([full, 0, full, 7, full, full, full, nd, nd + 1, full, 2 * nd, full], np.int32)
    status = np.array([-2] + [0] * 11, np.int32)
    rx = np.zeros((frames, span), np.complex64)
    fd = (rng.random(frames) - 0.5) * 2.0 / S
    for f in range(frames):
        tx = orc.encode(bytes(rng.integers(0, 256, payload, dtype=np.uint8)), True, mod, n)
        rx[f] = through_channel(orc, rng, tx, span, delay[f], float(fd[f]), SNR[mod], data_start=10 * S)
    off = np.array(delay, np.int32)
    hk = np.stack([orc.estimate_channel(orc.cfo_rotate(np.concatenate([wide(rx[f, off[f]:]), np.zeros(10 * S)])[:10 * S], float(fd[f]), 0)[5 * S:], trn, n)
                   for f in range(frames)]).astype(np.complex64)
    want, tol, near, widen, _ = _reference(rx, n, True, mod, trn, D, n_points, offset=off, f_delta=fd, hk=hk, status=status)
    assert list(want[:, qr.Q_VALID]) == [0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1]
    assert list(want[:, qr.Q_POINTS]) == [0, 0, full, 7, 0, full, 2 * nd, nd, nd + 1, full, 2 * nd, full]
    assert np.all(want[[0, 4]] == 0) and int(near.sum()) == 0
    c = api.Context(n_fft=n, modulation=mod, guard_bands=True)
    t = dict(rx=c.to_device(rx), n_points=_dev(c, n_points, torch.int32), offset=_dev(c, off, torch.int32), f_delta=_dev(c, fd, torch.float64),
             hk=c.to_device(hk), status=_dev(c, status, torch.int32))
    got = c.rx_quality(t["rx"], D, n_points=t["n_points"], offset=t["offset"], f_delta=t["f_delta"], hk=t["hk"], status=t["status"])
    _assert_rows(got.cpu().numpy(), want, tol, near, widen, n)
    for f in range(frames):
        one = c.rx_quality(t["rx"][f:f + 1], D, n_points=t["n_points"][f:f + 1], offset=t["offset"][f:f + 1], f_delta=t["f_delta"][f:f + 1],
                           hk=t["hk"][f:f + 1], status=t["status"][f:f + 1])
        assert torch.equal(one[0], got[f]), f
    for cap in (1, 3):
        c.set_tuning("grid_cap", cap)
        assert torch.equal(c.rx_quality(t["rx"], D, n_points=t["n_points"], offset=t["offset"], f_delta=t["f_delta"], hk=t["hk"], status=t["status"]), got)


# ---------------------------------------------------------------------------------------------------------- 3. non-finite samples
@pytest.mark.parametrize("n", [64, 1024])
def test_a_nan_reaches_exactly_the_fields_of_the_definition(n):
    api = _api()
    k = _kernel_case(n, 6, False, 70, 6, "shared") if n == 64 else _kernel_case(n, 6, True, 70, 3, "frame")
    D = 6 if n == 64 else 3
    S = k["S"]
    c = api.Context(n_fft=n, modulation=6, guard_bands=n != 64)
    rx = k["rx"][:4].copy()
    hk = k["hk"] if k["hk"].ndim == 1 else k["hk"][:4]
    args = dict(n_points=k["n_points"], offset=_dev(c, k["off"][:4], torch.int32), f_delta=_dev(c, k["fd"][:4], torch.float64), hk=c.to_device(hk))
    clean = c.rx_quality(c.to_device(rx), D, **args).cpu().numpy()
    rx[1, k["off"][1] + 7 * S + n // 3] = np.nan                 # a training block of frame 1
    rx[2, k["off"][2] + 11 * S + n // 2] = complex(0.0, np.nan)  # the second data symbol of frame 2
    got = c.rx_quality(c.to_device(rx), D, **args).cpu().numpy()
    want = qr.quality(wide(rx), n, n != 64, 6, k["trn"], D, 10, k["n_points"], offset=k["off"][:4], f_delta=k["fd"][:4], hk=wide(hk))
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    assert np.array_equal(got[[0, 3]], clean[[0, 3]])
    t = [qr.Q_NOISE_VAR, qr.Q_GAIN, qr.Q_SNR, qr.Q_LLR_UNIT]
    assert not np.isfinite(got[1, t]).any() and np.array_equal(got[1, [0, 5, 6, 7]], clean[1, [0, 5, 6, 7]])
    assert not np.isfinite(got[2, qr.Q_EVM2]) and np.array_equal(np.delete(got[2], qr.Q_EVM2), np.delete(clean[2], qr.Q_EVM2))


# ---------------------------------------------------------------------------------------------------------- 4. the Python method on the link
@pytest.mark.parametrize("chest", ["CHEST_LS", "CHEST_WLS"])
@pytest.mark.parametrize("ecc_name,fcs", [("ECC_NONE", False), ("ECC_LDPC648", False), ("ECC_CONV_K7F_R34", True)])
def test_link_quality_on_the_seeded_link(orc, ecc_name, fcs, chest):
    api = _api()
    ecc = getattr(api, ecc_name) + (api.ECC_FCS if fcs else 0)
    n, mod, payload, frames = 64, api.QAM64, 100, 24
    shares = []
    for seed in range(600, 608):      # the first seed whose REFERENCE excuses at most 2 % of the frames (the kernel's rows are not looked at)
        c, pay, rx, D = link(ecc, n, mod, frames, payload, 12.0, seed, chest_mode=getattr(api, chest))
        g = torch.Generator(device=c.device)
        g.manual_seed(1)
        rx[0] = 1e-3 * torch.randn(rx.shape[1], dtype=torch.complex64, device=c.device, generator=g)    # a slot without a packet
        r = c.decode_batch(rx, max_symbols=D)
        status = r["status"].cpu().numpy()
        n_points = c.frame_points(payload)
        # the reference, fed with the decode's outputs and the device's channel estimate for them
        offs = torch.where(r["status"] == 0, r["offset"], torch.zeros_like(r["offset"]))
        hk = c.estimate_channel(rx, offs, r["f_delta"])
        assert ("k_chest_solve" in c.last_dispatch()) == (chest == "CHEST_WLS")
        want, tol, near, widen, _ = _reference(rx.cpu().numpy(), n, True, mod, orc.default_training(n), D, n_points, offset=offs.cpu().numpy(),
                                               f_delta=r["f_delta"].cpu().numpy(), hk=hk.cpu().numpy(), status=status)
        shares.append(float(np.mean(near > 0)))
        if shares[-1] <= 0.02:
            break
    print(f"{ecc_name} {chest}: seed {seed}, frames with a point at a boundary per seed tried {[f'{v:.1%}' for v in shares]}")
    assert shares[-1] <= 0.02
    before = {k: v.clone() for k, v in r.items()}
    q = c.link_quality(rx, r, payload_bytes=payload)
    c.synchronize()
    assert c.last_dispatch() == "k_linkq"
    assert all(torch.equal(r[k], before[k]) for k in r)
    assert status[0] != 0 and int((status == 0).sum()) >= frames // 2
    assert n_points == -(-8 * (16 + c.coded_len(payload)) // mod) and D == -(-n_points // c.data_carriers)
    got = np.zeros((frames, qr.FIELDS))
    got[:, qr.Q_VALID] = q["valid"].cpu().numpy()
    for name, fld in (("noise_var", qr.Q_NOISE_VAR), ("gain", qr.Q_GAIN), ("llr_unit", qr.Q_LLR_UNIT), ("points", qr.Q_POINTS)):
        got[:, fld] = q[name].cpu().numpy()
    got[:, qr.Q_SNR] = 10.0 ** (q["snr_db"].cpu().numpy().astype(np.float64) / 10.0)
    got[:, qr.Q_EVM2] = 10.0 ** (q["evm_db"].cpu().numpy().astype(np.float64) / 10.0)
    dead = status != 0
    assert np.all(want[dead] == 0) and not q["valid"].cpu().numpy()[dead].any()
    for name in ("noise_var", "gain", "llr_unit", "points"):
        assert np.all(q[name].cpu().numpy()[dead] == 0), name
    assert np.isnan(q["snr_db"].cpu().numpy()[dead]).all() and np.isnan(q["evm_db"].cpu().numpy()[dead]).all()
    got[dead] = 0
    _assert_rows(got, want, tol, near, widen, ecc_name)
    live = ~dead
    assert np.all(want[live, qr.Q_POINTS] == n_points)
    # without a payload size or a count only the training fields are measured
    t_only = c.link_quality(rx, r)
    assert torch.equal(t_only["noise_var"], q["noise_var"]) and torch.equal(t_only["gain"], q["gain"]) and float(t_only["points"].sum()) == 0
    assert torch.isnan(t_only["evm_db"]).all()
    # a per-frame count
    counts = torch.full((frames,), n_points, dtype=torch.int32, device=c.device)
    per = c.link_quality(rx, r, n_points=counts)
    assert all(torch.equal(per[k2][live], q[k2][live]) for k2 in q)


# ---------------------------------------------------------------------------------------------------------- 5. arguments
def test_invalid_arguments_launch_nothing():
    api = _api()
    c = api.Context(n_fft=64, modulation=4, guard_bands=True)
    x = c.to_device(np.ones((2, 1200), np.complex64))
    out = torch.full((2, 8), 7.0, dtype=torch.float32, device=c.device)
    hk = c.to_device(np.ones((2, 64), np.complex64))
    assert c.rx_quality(x, 2, out=out) is out and c.last_dispatch() == "k_linkq"
    assert bool((out[:, 0] == 1).all())
    c.fft(c.to_device(np.ones((1, 64), np.complex64)))
    assert c.last_dispatch() == "k_sym<fft>"
    out.fill_(7.0)
    f = c.lib.ofdm_rx_quality_batch
    X, O, H = x.data_ptr(), out.data_ptr(), hk.data_ptr()
    bad = [f(None, X, 2, 1200, 1200, 10, 2, None, None, None, None, 0, None, O),
           f(c.h, None, 2, 1200, 1200, 10, 2, None, None, None, None, 0, None, O),
           f(c.h, X, 2, 1200, 1200, 10, 2, None, None, None, None, 0, None, None),
           f(c.h, X, -1, 1200, 1200, 10, 2, None, None, None, None, 0, None, O),
           f(c.h, X, 2, -1, 1200, 10, 2, None, None, None, None, 0, None, O),
           f(c.h, X, 2, 1200, 0, 10, 2, None, None, None, None, 0, None, O),
           f(c.h, X, 2, 1200, 1200, -1, 2, None, None, None, None, 0, None, O),
           f(c.h, X, 2, 1200, 1200, 10, -1, None, None, None, None, 0, None, O),
           f(c.h, X, 2, 1200, 1200, 10, 2, None, None, None, H, 5, None, O),
           f(c.h, X, 2, 1200, 1200, 10, (1 << 24) // 48 + 1, None, None, None, None, 0, None, O)]
    assert bad == [-1] * len(bad), bad
    assert f(c.h, None, 0, 0, 1200, 10, 2, None, None, None, None, 0, None, None) == 0
    c.synchronize()
    assert c.last_dispatch() == "k_sym<fft>" and bool((out == 7.0).all())
    assert f(c.h, X, 2, 1200, 1200, 10, (1 << 24) // 48, None, None, None, H, 64, None, O) == 0 and c.last_dispatch() == "k_linkq"
    with pytest.raises(api.OfdmError):
        c.rx_quality(x, 2, n_points=torch.zeros(3, dtype=torch.int32, device=c.device))
