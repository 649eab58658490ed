"""GPU checks of EXT-8, wide CFO acquisition (include/ofdm_hip.h; definition: tests/cfo_wide_ref.py): ofdm_cfo_wide_batch (k_cfo_wide)
against the f64 definition on THE SAME fc32 samples, offsets and Schmidl-Cox estimates, so that the comparison isolates the kernel, and
the OFDM_CFO_WIDE receive mode through every decode entry point on the seeded wide link of tools/link.py.

The decision: the test first asserts ON THE F64 DEFINITION that every live frame's winner holds at least 1.5 times the runner-up's
window energy (the draws give 2 and more); a decision with that margin is one an f32 kernel takes exactly as f64 does, so m must be
EQUAL and f_delta must be f0 + 2 pi m / S bit for bit.
The metrics (the precedent is tests/test_gpu_chest.py and tests/test_gpu_quality.py): cfo_wide_ref restates the computation with every
stage rounded to complex64; its distance from the f64 definition is measured on the case's own rows, and the kernel is allowed 4x
that or 1e-5 relative, whichever is larger.  The measured values are printed.

The chain's f_delta: the Schmidl-Cox estimate carries its own noise (about 1e-5 rad/sample at these SNRs), so no receiver returns the
channel's offset to 1e-9.  What the mode adds is exact, and that is what is held to 1e-9: f_delta equals the CFO_SIGNED decode's
f_delta of the same capture plus 2 pi m / S with the TRUE m; against the channel's own value it must lie within 5 % of one ambiguity
step 2 pi / S -- modulo nothing."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfo_wide_ref as cw  # noqa: E402
from chain_checks import ofdm_api as _api  # noqa: E402
from tools.link import data_snr, generator, wide_channel, wide_link_on  # noqa: E402
from util import through_channel, wide  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-5
RATIO = 1.5
# the SNR (against the data symbols) a modulation's stage cases are drawn at, as in tests/test_gpu_quality.py
SNR = {1: 8.0, 2: 11.0, 4: 22.0, 6: 30.0, 8: 37.0}
PAYLOAD = 8


def _dev(c, a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=c.device, dtype=dtype)


def _frames(n, mod, guard, frames, span, seed, delays=None):
    """Captures of `frames` short frames through the FIR channel, each with a delay, the offset frac + 2 pi m / S and noise (odd row
    stride); the trimmed start a search would hand over (CHANNEL at delays 1 .. 15 of it) and its estimate of frac"""
    from oracle import oracle as orc

    orc.lib()
    S = n + n // 4
    D = -(-8 * (16 + PAYLOAD) // mod // orc.data_carriers(n, guard))
    length = (10 + D) * S + n // 4 + 61
    length += 1 - length % 2
    rng = np.random.default_rng([n, mod, int(guard), frames, span, seed])
    rx = np.zeros((frames, length), np.complex64)
    m = rng.integers(-span, span + 1, frames).astype(np.int32)
    frac = (rng.random(frames) * 1.9 - 0.95) * np.pi / S
    delay = rng.integers(0, n // 4, frames) if delays is None else np.asarray(delays)
    for f in range(frames):
        tx = orc.encode(bytes(rng.integers(0, 256, PAYLOAD, dtype=np.uint8)), guard, mod, n)
        rx[f] = through_channel(orc, rng, tx, length, int(delay[f]), float(frac[f] + 2.0 * np.pi * m[f] / S), SNR[mod], data_start=10 * S)
    off = (delay + 5 + rng.integers(-2, 3, frames)).astype(np.int32)
    f0 = frac + rng.standard_normal(frames) * 1e-3 / S
    return dict(rx=rx, m=m, off=off, f0=f0, S=S, trn=orc.default_training(n))


def _reference(k, n, span, status=None, frame_len=None):
    """(m, f_delta, metric) of the f64 definition, the metric tolerance and the restatement's distance"""
    with np.errstate(all="ignore"):
        m, fd, g = cw.cfo_wide(wide(k["rx"]), n, k["trn"], k["off"], k["f0"], span, status, frame_len)
        _, _, g32 = cw.cfo_wide(k["rx"], n, k["trn"], k["off"], k["f0"], span, status, frame_len, dtype=np.complex64)
    live = np.isfinite(g).all(axis=1) & (g[:, 0] > 0)
    dist = float(np.max(np.abs(g32[live] - g[live]) / g[live])) if live.any() else 0.0
    return m, fd, g, max(4.0 * dist, TOL), dist, live


def _assert_rows(r, m, fd, g, tol, what):
    """r: Context.cfo_wide's dict -> the largest relative metric error"""
    assert np.array_equal(r["m"].cpu().numpy(), m), what
    assert r["f_delta"].cpu().numpy().tobytes() == fd.tobytes(), what      # f0 + 2 pi m / S in f64, bit for bit (m = 0: f0 itself)
    got = r["metric"].cpu().numpy().astype(np.float64)
    err = np.abs(got - g)
    assert np.all(err <= tol * np.abs(g)), (what, float(np.max(err / np.maximum(np.abs(g), 1e-300))), tol)
    return float(np.max(err[g != 0] / np.abs(g[g != 0]))) if (g != 0).any() else 0.0


# ---------------------------------------------------------------------------------------------------------- 1. the kernel
CASES = [  # n_fft, modulation, guard bands, frames, span
    (64, 1, True, 70, 8),          # eight frames share a wavefront
    (64, 6, False, 3, 8),
    (64, 8, True, 70, 32),
    (128, 2, True, 70, 8),         # shuffle exchange
    (128, 4, False, 3, 8),
    (512, 4, False, 70, 8),
    (512, 6, True, 3, 8),
    (1024, 6, True, 70, 8),        # workgroup path
    (1024, 2, False, 3, 8),
    (4096, 8, True, 3, 8),
    (4096, 1, False, 70, 8),
]


@functools.lru_cache(maxsize=None)
def _kernel_case(n, mod, guard, frames, span):
    k = _frames(n, mod, guard, frames, span, 0)
    k["ref"] = _reference(k, n, span)
    return k


@pytest.mark.parametrize("n,mod,guard,frames,span", CASES)
def test_kernel_matches_the_definition(n, mod, guard, frames, span):
    api = _api()
    k = _kernel_case(n, mod, guard, frames, span)
    m, fd, g, tol, dist, live = k["ref"]
    # the definition itself: every frame is live, finds the true m, and by a factor of at least 1.5
    assert live.all() and np.array_equal(m, k["m"])
    ratio = g[:, 0] / g[:, 1]
    assert ratio.min() >= RATIO, ratio.min()
    c = api.Context(n_fft=n, modulation=mod, guard_bands=guard)
    rx = c.to_device(k["rx"])
    assert rx.shape[1] % 2 == 1
    off, f0 = _dev(c, k["off"], torch.int32), _dev(c, k["f0"], torch.float64)
    r = c.cfo_wide(rx, off, f0, span)
    c.synchronize()
    assert c.last_dispatch() == "k_cfo_wide"
    assert f0.cpu().numpy().tobytes() == k["f0"].tobytes()                  # the caller's estimate is left as it was
    worst = _assert_rows(r, m, fd, g, tol, (n, mod))
    print(f"N {n} mod {mod} span {span}: ratio min {ratio.min():.2f} median {np.median(ratio):.2f}, restatement {dist:.1e}, kernel {worst:.1e}, tol {tol:.1e}")
    for cap in (1, 3):                                                      # many frames per slot: the same bits
        c.set_tuning("grid_cap", cap)
        r2 = c.cfo_wide(rx, off, f0, span)
        assert all(torch.equal(r2[key], r[key]) for key in r), cap
    c.set_tuning("grid_cap", 0)
    # m_dev and metric_dev are optional; f_delta_dev is updated in place
    fd_io = f0.clone()
    assert c.lib.ofdm_cfo_wide_batch(c.h, rx.data_ptr(), frames, rx.shape[1], rx.shape[1], off.data_ptr(), None, span, fd_io.data_ptr(), None, None) == 0
    c.synchronize()
    assert torch.equal(fd_io, r["f_delta"])
    # a smaller span that still holds every frame's m gives the same decision; one that does not cannot return it
    if span == 8:
        r4 = c.cfo_wide(rx, off, f0, 4)
        inside = torch.from_numpy(np.abs(k["m"]) <= 4).to(c.device)
        assert torch.equal(r4["m"][inside], r["m"][inside]) and bool((r4["m"].abs() <= 4).all())


# ---------------------------------------------------------------------------------------------------------- 2. ragged batches
@pytest.mark.parametrize("n,mod", [(64, 6), (128, 4), (512, 2), (1024, 2)])
def test_ragged_batch_rows_are_the_rows_of_the_frames_alone(n, mod):
    """Live and dead frames side by side in one wavefront (N = 1024: one workgroup): a frame whose status is not 0, one whose training
    blocks end one sample behind the capture, one that ends exactly with it, a negative offset.  Every row equals the definition's
    and, bit for bit, the row of the frame run alone and the rows under a grid of 1 and of 3 workgroups."""
    api = _api()
    S, frames = n + n // 4, 12
    k = _frames(n, mod, True, frames, 8, 5)
    length = k["rx"].shape[1]
    status = np.array([-2, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0], np.int32)
    off = k["off"].copy()
    off[2] = length - 10 * S + 1                                             # the training blocks reach past the capture
    off[4] = -1
    off[7] = -(2 ** 31)
    k["off"] = off
    m, fd, g, tol, dist, live = _reference(k, n, 8, status)
    dead = [0, 2, 4, 5, 7]
    assert list(np.nonzero(~live)[0]) == dead and np.all(m[dead] == 0) and np.all(g[dead] == 0)
    assert fd[dead].tobytes() == k["f0"][dead].tobytes()
    assert np.array_equal(m[live], k["m"][live]) and (g[live, 0] / g[live, 1]).min() >= RATIO
    c = api.Context(n_fft=n, modulation=mod, guard_bands=True)
    rx, o, f0, st = c.to_device(k["rx"]), _dev(c, off, torch.int32), _dev(c, k["f0"], torch.float64), _dev(c, status, torch.int32)
    r = c.cfo_wide(rx, o, f0, 8, status=st)
    _assert_rows(r, m, fd, g, tol, n)
    for f in range(frames):
        one = c.cfo_wide(rx[f:f + 1], o[f:f + 1], f0[f:f + 1], 8, status=st[f:f + 1])
        assert all(torch.equal(one[key][0], r[key][f]) for key in r), f
    for cap in (1, 3):
        c.set_tuning("grid_cap", cap)
        r2 = c.cfo_wide(rx, o, f0, 8, status=st)
        assert all(torch.equal(r2[key], r[key]) for key in r), cap
    c.set_tuning("grid_cap", 0)
    # a capture that ends exactly behind the training blocks is tested; one sample shorter it is not
    f = 1
    edge = int(off[f]) + 10 * S
    a = c.cfo_wide(rx[f:f + 1], o[f:f + 1], f0[f:f + 1], 8, frame_len=edge)
    b = c.cfo_wide(rx[f:f + 1], o[f:f + 1], f0[f:f + 1], 8, frame_len=edge - 1)
    assert all(torch.equal(a[key][0], r[key][f]) for key in r)
    assert int(b["m"][0]) == 0 and bool((b["metric"] == 0).all()) and torch.equal(b["f_delta"], f0[f:f + 1])


# ---------------------------------------------------------------------------------------------------------- 3. non-finite samples
@pytest.mark.parametrize("n", [64, 1024])
def test_a_nan_spoils_its_own_frame_only(n):
    api = _api()
    k = _kernel_case(n, 1, True, 70, 8) if n == 64 else _kernel_case(n, 6, True, 70, 8)
    S = k["S"]
    c = api.Context(n_fft=n, modulation=1 if n == 64 else 6, guard_bands=True)
    rx = k["rx"][:9].copy()
    off, f0 = _dev(c, k["off"][:9], torch.int32), _dev(c, k["f0"][:9], torch.float64)
    clean = c.cfo_wide(c.to_device(rx), off, f0)
    rx[1, k["off"][1] + 7 * S + n // 4 + n // 3] = np.nan                    # a training block of frame 1, behind its prefix
    rx[4, k["off"][4] + 9 * S + n // 4] = complex(0.0, np.inf)
    rx[6, k["off"][6] + 10 * S + n // 4 + 3] = np.nan                        # a data symbol: not read
    got = c.cfo_wide(c.to_device(rx), off, f0)
    for f in (1, 4):
        assert int(got["m"][f]) == 0 and not bool(torch.isfinite(got["metric"][f]).any())
        assert torch.equal(got["f_delta"][f], f0[f])
    keep = [0, 2, 3, 5, 6, 7, 8]
    assert all(torch.equal(got[key][keep], clean[key][keep]) for key in got)


# ---------------------------------------------------------------------------------------------------------- 4. the chain
CHAIN = [  # n_fft, ecc, modulation, channel snr_db at N = 64, payload, the kernel behind the front end
    (64, "ECC_NONE", 4, 35.0, 100, "k_rxframe64"),                           # the fused frame kernels
    (1024, "ECC_NONE", 4, 35.0, 300, "k_rxframe1024"),
    (64, "ECC_LDPC648", 6, 30.0, 100, "k_sym<llr>"),                         # the soft branch
    (64, "ECC_CONV_K7F_R34", 6, 30.0, 100, "k_sym<llr>"),
    (256, "ECC_NONE", 4, 35.0, 200, "k_sym<chest>"),                         # the generic pair
]


def _payload_rows(r, n_frames):
    status, ln, by = r["status"].cpu().numpy(), r["len"].cpu().numpy(), r["bytes"].cpu().numpy()
    return status, [bytes(by[f, :ln[f]]) for f in range(n_frames)]


@pytest.mark.parametrize("n,ecc_name,mod,snr,payload,behind", CHAIN)
def test_decode_batch_under_cfo_wide(orc, n, ecc_name, mod, snr, payload, behind):
    api = _api()
    ecc, frames, S = getattr(api, ecc_name), 64, n + n // 4
    c = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=ecc, cfo_mode=api.CFO_WIDE)
    s = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=ecc, cfo_mode=api.CFO_SIGNED)
    m = np.random.default_rng(800 + n).integers(-8, 9, frames)              # uniform over +-8, the ends and the middle in any case
    m[:3] = (0, -8, 8)
    pay, rx, m, fd_true = wide_link_on(c, frames, payload, data_snr(n, snr), 800 + n, m=torch.from_numpy(m.astype(np.int32)).to(c.device))
    D = c.data_symbols(payload)
    r = c.decode_batch(rx, max_symbols=D)
    c.synchronize()
    trace = c.last_dispatch()
    assert "k_rx_prepare+k_cfo_wide+" in trace and behind in trace, trace
    ctl = s.decode_batch(rx, max_symbols=D)
    s.synchronize()
    assert "k_cfo_wide" not in s.last_dispatch()
    m, fd_true, want = m.cpu().numpy(), fd_true.cpu().numpy(), pay.cpu().numpy()
    assert len(set(m)) >= 10 and (m == 0).any() and m.min() == -8 and m.max() == 8
    status, rows = _payload_rows(r, frames)
    assert np.all(status == 0), status
    offset, fd = r["offset"].cpu().numpy(), r["f_delta"].cpu().numpy()
    host = wide(rx.cpu().numpy())
    for f in range(frames):
        assert rows[f] == bytes(want[f]), f
        if ecc == api.ECC_NONE:                                             # the oracle's chain at the offset and the total CFO the device found
            ref = orc.decode_given(host[f], int(offset[f]), float(fd[f]), True, mod, n, max_symbols=D)
            assert ref["status"] == 0 and ref["bytes"] == rows[f], f
    # the total offset: the Schmidl-Cox residue plus the TRUE multiple, exactly; and near the channel's own value, modulo nothing
    fd_ctl = ctl["f_delta"].cpu().numpy()
    assert np.max(np.abs(fd - (fd_ctl + 2.0 * np.pi * m / S))) <= 1e-9
    assert np.max(np.abs(fd - fd_true)) <= 0.05 * 2.0 * np.pi / S
    assert np.array_equal(offset, ctl["offset"].cpu().numpy()) and torch.equal(r["metric"], ctl["metric"])
    # the control: without the mode every frame with m != 0 is lost, every frame with m = 0 is the same frame
    cst, crows = _payload_rows(ctl, frames)
    lost = np.array([cst[f] != 0 or crows[f] != bytes(want[f]) for f in range(frames)])
    assert np.array_equal(lost, m != 0), (np.nonzero(lost != (m != 0))[0], m)
    zero = torch.from_numpy(m == 0).to(c.device)
    for key in ("len", "status", "offset", "f_delta"):                        # (the rows: compared above, out_len bytes each)
        assert torch.equal(r[key][zero], ctl[key][zero]), key


@pytest.mark.parametrize("n,ecc_name,mod,snr,payload", [(64, "ECC_NONE", 4, 35.0, 100), (1024, "ECC_NONE", 4, 35.0, 300), (64, "ECC_LDPC648", 6, 30.0, 100)])
def test_inside_the_old_range_the_mode_changes_nothing(n, ecc_name, mod, snr, payload):
    """offsets all within +-0.95 pi / S: CFO_WIDE and CFO_SIGNED return bit-identical rows"""
    api = _api()
    ecc, frames = getattr(api, ecc_name), 64
    c = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=ecc, cfo_mode=api.CFO_WIDE)
    s = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=ecc)
    pay, rx, m, fd_true = wide_link_on(c, frames, payload, data_snr(n, snr), 900 + n, m=torch.zeros(frames, dtype=torch.int32, device=c.device))
    assert float(fd_true.abs().max()) <= 0.95 * math.pi / c.S
    rx[5] = 1e-3 * torch.randn(rx.shape[1], dtype=torch.complex64, device=c.device, generator=generator(c, 3))     # a slot without a packet
    D = c.data_symbols(payload)
    a, b = c.decode_batch(rx, max_symbols=D), s.decode_batch(rx, max_symbols=D)
    c.synchronize()
    assert "k_cfo_wide" in c.last_dispatch() and "k_cfo_wide" not in s.last_dispatch()
    for key in ("len", "status", "offset", "f_delta", "metric"):
        assert torch.equal(a[key], b[key]), key
    ln = a["len"].cpu().numpy()
    ba, bb = a["bytes"].cpu().numpy(), b["bytes"].cpu().numpy()
    assert all(bytes(ba[f, :ln[f]]) == bytes(bb[f, :ln[f]]) for f in range(frames))
    status = a["status"].cpu().numpy()
    assert status[5] != 0 and int((status == 0).sum()) == frames - 1


# ---------------------------------------------------------------------------------------------------------- 5. the other entry points
def test_decode_long_finds_a_packet_with_a_wide_offset():
    """one packet 300 samples into a capture, m = -5: the searched branch, and the branch that is handed its timing (lag_lo > 0)"""
    api = _api()
    n, mod, payload = 64, api.QAM16, 100
    c = api.Context(n_fft=n, modulation=mod, guard_bands=True, cfo_mode=api.CFO_WIDE)
    s = api.Context(n_fft=n, modulation=mod, guard_bands=True)
    g = generator(c, 77)
    pay = torch.randint(0, 256, (1, payload), dtype=torch.uint8, device=c.device, generator=g)
    tx = c.encode_batch(pay)
    fd_true = 0.3 * math.pi / c.S - 5 * 2.0 * math.pi / c.S
    cap = c.channel_batch(tx, snr_db=35.0, seed=77, delay=torch.tensor([300], dtype=torch.int32, device=c.device),
                          f_delta=torch.tensor([fd_true], dtype=torch.float64, device=c.device), span=tx.shape[1] + 460)[0].contiguous()
    D = c.data_symbols(payload)
    want = bytes(pay[0].cpu().numpy())
    ctl = s.decode_long(cap, D)
    assert ctl["status"] != 0 or bytes(ctl["bytes"][:ctl["len"]].cpu().numpy()) != want
    for kw, front in ((dict(), "k_rx_prepare+k_cfo_wide"), (dict(lag_lo=200), "k_set_sync+k_rx_prepare+k_cfo_wide")):
        r = c.decode_long(cap, D, **kw)
        assert front in c.last_dispatch(), c.last_dispatch()
        assert r["status"] == 0 and bytes(r["bytes"][:r["len"]].cpu().numpy()) == want, kw
        assert r["offset"] == ctl["offset"] and 280 <= r["offset"] <= 330
        assert abs(r["f_delta"] - (ctl["f_delta"] - 5 * 2.0 * np.pi / c.S)) <= 1e-9
        assert abs(r["f_delta"] - fd_true) <= 0.05 * 2.0 * np.pi / c.S
    h = c.decode_long_host(cap.cpu().numpy(), D)
    assert h["status"] == 0 and bytes(h["bytes"][:h["len"]]) == want and abs(h["f_delta"] - r["f_delta"]) <= 1e-9


def test_decode_combine_with_a_different_multiple_on_each_capture():
    api = _api()
    n, mod, payload, frames, R = 64, api.QAM64, 100, 8, 2
    c = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=api.ECC_LDPC648, cfo_mode=api.CFO_WIDE)
    s = api.Context(n_fft=n, modulation=mod, guard_bands=True, ecc=api.ECC_LDPC648)
    g = generator(c, 31)
    pay = torch.randint(0, 256, (frames, payload), dtype=torch.uint8, device=c.device, generator=g)
    tx = c.encode_batch(pay)
    ms = [torch.tensor([3, -8, 0, 5, -1, 8, 2, -4], dtype=torch.int32, device=c.device),
          torch.tensor([-2, 7, 4, 0, 6, -8, -3, 1], dtype=torch.int32, device=c.device)]
    rows, truth = [], []
    for r_, m in enumerate(ms):
        rx, _, fd = wide_channel(c, tx, 30.0, 31 + r_, g, m=m)
        rows.append(rx)
        truth.append(fd)
    rx = torch.stack(rows, dim=1).contiguous()
    D = c.data_symbols(payload)
    r = c.decode_combine(rx, max_symbols=D)
    c.synchronize()
    assert "k_rx_prepare+k_cfo_wide+" in c.last_dispatch() and "k_llr_combine" in c.last_dispatch()
    assert bool((r["status"] == 0).all()) and bool((r["branch_status"] == 0).all())
    assert bool((r["len"] == payload).all()) and torch.equal(r["bytes"][:, :payload], pay)
    assert float((r["f_delta"] - torch.stack(truth, dim=1)).abs().max()) <= 0.05 * 2.0 * math.pi / c.S
    assert bool((r["weight"] > 0).all())                                    # both captures of every frame count
    ctl = s.decode_combine(rx, max_symbols=D)
    lost = (ctl["status"] != 0) | (ctl["len"] != payload) | (ctl["bytes"][:, :payload] != pay).any(dim=1)
    both = torch.from_numpy((ms[0].cpu().numpy() != 0) & (ms[1].cpu().numpy() != 0)).to(c.device)
    assert bool(lost[both].all())                                           # without the mode a frame with no capture inside the old range is lost


# ---------------------------------------------------------------------------------------------------------- 6. arguments
def test_invalid_arguments_launch_nothing():
    api = _api()
    c = api.Context(n_fft=64, modulation=4, guard_bands=True, cfo_mode=api.CFO_ABS)      # the stage works whatever the context's mode
    x = c.to_device(np.ones((2, 1200), np.complex64))
    off = torch.zeros(2, dtype=torch.int32, device=c.device)
    fd = torch.full((2,), 0.01, dtype=torch.float64, device=c.device)
    r = c.cfo_wide(x, off, fd, api.CFO_WIDE_MAX_SPAN)
    assert c.last_dispatch() == "k_cfo_wide" and r["m"].shape == (2,) and r["metric"].shape == (2, 2)
    c.fft(c.to_device(np.ones((1, 64), np.complex64)))
    assert c.last_dispatch() == "k_sym<fft>"
    f = c.lib.ofdm_cfo_wide_batch
    X, O, F = x.data_ptr(), off.data_ptr(), fd.data_ptr()
    bad = [f(None, X, 2, 1200, 1200, O, None, 8, F, None, None),
           f(c.h, None, 2, 1200, 1200, O, None, 8, F, None, None),
           f(c.h, X, 2, 1200, 1200, None, None, 8, F, None, None),
           f(c.h, X, 2, 1200, 1200, O, None, 8, None, None, None),
           f(c.h, X, -1, 1200, 1200, O, None, 8, F, None, None),
           f(c.h, X, 2, -1, 1200, O, None, 8, F, None, None),
           f(c.h, X, 2, 1200, 0, O, None, 8, F, None, None),
           f(c.h, X, 2, 1200, 1200, O, None, 0, F, None, None),
           f(c.h, X, 2, 1200, 1200, O, None, -1, F, None, None),
           f(c.h, X, 2, 1200, 1200, O, None, api.CFO_WIDE_MAX_SPAN + 1, F, None, None)]
    assert bad == [-1] * len(bad), bad
    assert f(c.h, None, 0, 0, 1200, None, None, 8, None, None, None) == 0
    c.synchronize()
    assert c.last_dispatch() == "k_sym<fft>" and bool((fd == 0.01).all())
    with pytest.raises(api.OfdmError):
        c.cfo_wide(x, off[:1], fd)
    with pytest.raises(api.OfdmError):
        api.Context(n_fft=64, cfo_mode=api.CFO_WIDE, sync_mode=api.SYNC_REFERENCE)
    with pytest.raises(api.OfdmError):
        api.Context(n_fft=64, cfo_mode=4)
